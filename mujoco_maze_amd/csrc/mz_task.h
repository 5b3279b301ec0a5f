// mz_task.h — the task of a maze (MazeTask, maze_task.py): its float64 constants (TaskDev), their derivation from the
// compiled `mz_model` (include/mazestep.h), and task_eval_dev, the reward / termination predicate that every step kernel
// and the host emulation run.  Also mz_refuse, the way every *_dev_from_model turns a model down.
//
// Plain C++ (no HIP): shared by the kernel translation units and the CPU emulation in tests/emu/.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "../../include/mazestep.h"
#include "mz_lanes.h"

// Task constants.  Everything a flag depends on is float64, exactly the reference's values (maze_task.py:26-47): the
// goal predicate `np.linalg.norm(obs[:dim] - pos) <= threshold` is evaluated in fp64 on the returned observation.
// thr_sq[g] = the largest double s with sqrt(s) <= threshold (sqrt correctly rounded, as numpy's): `s <= thr_sq` is
// then the same predicate without a square root, so no floating-point build flag can change a flag.
struct TaskDev {
  int ngoal, reward_kind, reward_slot, reward_binary, term_slot, max_steps;
  int goal_dim[MZ_MAX_GOAL];
  double goal_pos[MZ_MAX_GOAL][3], thr[MZ_MAX_GOAL], thr_sq[MZ_MAX_GOAL], rscale[MZ_MAX_GOAL];
  double penalty, task_scale, inner_scale, fwd_w, ctrl_w;
  // per-env goal POSITIONS (mz_bind_env_goals; device pointer, [N][MZ_MAX_GOAL][3] float64, or NULL: the batch shares goal_pos).  The
  // reference resamples a task's goals at EVERY episode reset (maze_env.py:374-376: one task object per env); thresholds, reward
  // scales and dims stay the task class's
  const double* env_goals;
};

// how a *_dev_from_model turns a model down: the reason into the caller's buffer, MZ_ERR_UNSUPPORTED back
static inline int mz_refuse(char* err, int n, const char* msg) {
  if (err && n > 0) { strncpy(err, msg, (size_t)n - 1); err[n - 1] = 0; }
  return MZ_ERR_UNSUPPORTED;
}

// largest double s with sqrt(s) <= thr (host libm sqrt is correctly rounded); -1 for a negative threshold (never matches)
static inline double mz_sqrt_le_bound(double thr) {
  if (!(thr >= 0.0)) return -1.0;
  if (isinf(thr)) return thr;
  double s = thr * thr;
  while (sqrt(s) > thr) s = nextafter(s, 0.0);
  while (sqrt(nextafter(s, INFINITY)) <= thr) s = nextafter(s, INFINITY);
  return s;
}

static inline void task_dev_from_model(TaskDev* t, const mz_model* m) {
  memset(t, 0, sizeof(*t));
  t->ngoal = m->ngoal; t->reward_kind = m->reward_kind; t->reward_slot = m->reward_slot;
  t->reward_binary = m->reward_binary; t->term_slot = m->term_slot; t->max_steps = m->max_episode_steps;
  for (int g = 0; g < m->ngoal; g++) {
    t->goal_dim[g] = m->goal_dim[g];
    for (int k = 0; k < 3; k++) t->goal_pos[g][k] = m->goal_pos[g][k];
    t->thr[g] = m->goal_threshold[g];
    t->thr_sq[g] = mz_sqrt_le_bound(m->goal_threshold[g]);
    t->rscale[g] = m->goal_reward_scale[g];
  }
  t->penalty = m->penalty; t->task_scale = m->task_scale; t->inner_scale = m->inner_reward_scaling;
  t->fwd_w = m->forward_reward_weight; t->ctrl_w = m->ctrl_cost_weight;
}

// ------------------------------------------------------------------ MazeTask reward / termination on the fp32 observation
// that is returned to the caller (obs[0:3] agent slot, obs[3:6] object slot).  Flags and goal index are the reference's
// float64 predicate (maze_task.py:43-44 `np.linalg.norm(obs[:dim] - pos) <= threshold`, :77-81 any goal, :403-407 first
// match) evaluated on float64(obs): differences and squares in fp64, summed in index order without contraction, compared
// with the squared-threshold bound of TaskDev (bit-exact whatever the build flags of the translation unit).
// `env`: the env slot whose row of TaskDev::env_goals holds its own goal positions (per-episode resampling); -1 or no table bound:
// the batch's shared goal table.
MZ_HD void task_eval_dev(const TaskDev& T, const float* obs, float* reward, int* term, int* goal_idx, int env = -1) {
#pragma clang fp contract(off) reciprocal(off) reassociate(off)
  // (two loads, not one pointer select: the shared table stays a scalar load of the constant block)
  const double* eg = (T.env_goals && env >= 0) ? T.env_goals + (size_t)env * (3 * MZ_MAX_GOAL) : nullptr;
  const double slot_a[3] = {(double)obs[0], (double)obs[1], (double)obs[2]}, slot_o[3] = {(double)obs[3], (double)obs[4], (double)obs[5]};
  int tm = 0, first = -1, first_t = -1;
  for (int g = 0; g < T.ngoal; g++) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < 3; k++)
      if (k < T.goal_dim[g]) {
        const double gk = eg ? eg[3 * g + k] : T.goal_pos[g][k];
        double e = (T.term_slot == MZ_SLOT_OBJECT ? slot_o[k] : slot_a[k]) - gk; a += e * e;
        double f = (T.reward_slot == MZ_SLOT_OBJECT ? slot_o[k] : slot_a[k]) - gk; b += f * f;
      }
    if (!tm && a <= T.thr_sq[g]) { tm = 1; first_t = g; }
    if (first < 0 && b <= T.thr_sq[g]) first = g;
  }
  double r = 0.0;
  if (T.reward_kind == MZ_REWARD_FIRST_MATCH) r = T.reward_binary ? (tm ? 1.0 : T.penalty) : (first >= 0 ? T.rscale[first] : T.penalty);
  else if (T.reward_kind == MZ_REWARD_NEG_DIST && T.ngoal > 0) {
    double a = 0.0;
    for (int k = 0; k < 3; k++)
      if (k < T.goal_dim[0]) { double e = (T.reward_slot == MZ_SLOT_OBJECT ? slot_o[k] : slot_a[k]) - (eg ? eg[k] : T.goal_pos[0][k]); a += e * e; }
    r = -sqrt(a) / T.task_scale;
  }
  // goal index: the goal that set the reward where the reward is a goal's (first match on the reward's slot, maze_task.py:403-407);
  // for the other reward kinds (zero, distance) the first goal that ends the episode (termination's slot, maze_task.py:77-81,599,653)
  *reward = (float)r; *term = tm; *goal_idx = T.reward_kind == MZ_REWARD_FIRST_MATCH ? first : first_t;
}
