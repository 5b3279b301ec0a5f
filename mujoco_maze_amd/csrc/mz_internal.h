// mz_internal.h — what the five translation units of libmazestep.so share on the HOST side:
//   mazestep.hip        the C-ABI of include/mazestep.h (handle life cycle, options, argument checks, dispatch)
//   ant_kernels.hip     Ant kernels (fp32, built with the relaxed floating-point flags of csrc/Makefile)
//   planar_kernels.hip  Point / Swimmer / Reacher kernels (fp64, built with strict IEEE flags: the Point's manual wall
//                       detector and every task predicate must reproduce the reference's float64 decisions bit for bit)
//   generic_kernels.hip the general engine: any compiled model (fp64, no relaxed flags at all: generic_dyn.h)
//   render_kernels.hip  the top view of render.py for a batch of env states (fp64, no relaxed flags: mz_render.h)
// Kernels never call across translation units, so no relocatable device code is needed.
// mz_handle embeds the three specialised robots' constant blocks by value, hence their MODEL headers below; no engine's dynamics
// header (ant_dyn.h, planar_dyn.h, generic_dyn.h) is included here, and none includes another engine's — what they all need
// lives in mz_lanes.h (programming model), mz_task.h (TaskDev, task_eval_dev) and mz_maze.h (MazeDev, grid-aligned boxes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ant_model.h"
#include "mz_view.h"
#include "point_dyn.h"
#include "swimmer_dyn.h"

struct RenderDev;  // mz_render.h (only mazestep.hip and render_kernels.hip see the renderer)
struct GenDev;  // generic_dyn.h (the generic-robot path keeps its float64 constant block out of the other translation units)

struct AntLayout { int nq, nv, rec, rec_t, obs_dim, nblock3, ostride; };  // record layout of the instantiated block count; obs_dim: without the
                                                                          // top-down view, ostride: floats between observation rows

struct mz_handle {
  mz_model model;
  int n, device, robot;
  AntDev ant;
  AntDev* ant_dev;  // device copy read by the step kernel (refreshed when an option changes it)
  int ant_dirty;
  AntLayout lay;
  PointDev* point_dev;  // device copy
  PointDev point;
  SwimmerDev* swimmer_dev;
  SwimmerDev swimmer;
  GenDev* gen_dev;      // generic robot (MZ_ROBOT_GENERIC): device copy of the constant block (mz_model + pair tables)
  float* state;         // ant: [n][REC]; point / swimmer: SoA [2 NV][n]
  int* pt_t;
  uint32_t* pt_ep;
  int pt_rec;           // Point: floats per env-major state record (planar_kernels.hip PointState); 0: SoA
  int* status;
  ViewDev view;         // MazeTask.TOP_DOWN_VIEW: the maze bitmasks the view kernel reads (passed by value)
  int base_obs;         // observation width without the view; rows are model.obs_dim = base_obs (+ MZ_VIEW_DIM) floats apart
  float* final_obs;     // caller's buffer for terminal observations under auto-reset (mz_bind_final_obs), or NULL
  float* record;        // caller's [n, obs_dim + 2] buffer for the packed record obs | reward | done (mz_bind_record), or NULL
  unsigned long long* prof;  // 16 phase-cycle accumulators (option "profile_phases")
  int auto_reset, lanes, waves_per_block, wpb_set;
  int waves_per_simd;  // option "waves_per_simd": 0 = chosen by the launch's wave count, 1 / 2 = the plain ant's one- / two-wave kernel (ant_kernels.hip)
  uint64_t seed, env0;  // env0: global slot of local env 0 (sharded runs)
  char err[256];
  int lanes_set;  // lanes_per_env chosen by the caller (else the per-robot default)
  const double* env_goals;  // caller's per-env goal positions (mz_bind_env_goals), or NULL: carried into every TaskDev copy
  int simds;      // 4 x the device's compute units, read once in mz_create: the batch-size rules of the launch shapes compare wave counts with it
  // kernel timing ring (option "time_kernels")
  int ntime, itime;
  int time_stride, time_phase;  // option "time_kernels_stride": every k-th launch carries the event pair
  hipEvent_t* ev;  // 2 * ntime
  long nsteps;
  float* render_qpos;  // [n][nq] scratch of mz_render without a caller's qpos (allocated on first use, freed by mz_destroy)
  float* policy_act;   // [n][nu] actions of mz_rollout_policy's launch-by-launch loop without a caller's actions_seq (allocated on first use, freed by mz_destroy)
  // the caller's observation normaliser (mz_bind_obs_norm): [obs_dim] device arrays read by every network evaluation, or NULL both
  const float* nrm_mean;
  const float* nrm_inv_std;
  float nrm_clip;
  // context inputs (mz_context): the identity normaliser [2][obs_dim] (zeros, then ones) of a call with a context and no bound
  // normaliser, and the [n][MZ_MAX_CONTEXT] old columns of the relative transition; both allocated on first use, freed by mz_destroy
  float* ctx_ident;
  float* ctx_old;
  // option "wide_nets" (include/mazestep.h): 0 = widths up to MZ_POLICY_MAX_HIDDEN on the group kernels; 1 = mz_net widths up to
  // MZ_NET_MAX_WIDTH, a network with a layer wider than 64 on the tiled kernels (mz_net_tile.h); 2 = every mz_net network tiled
  int wide_nets;
};

// ---- ant_kernels.hip
hipError_t mzk_ant_step(mz_handle* h, hipStream_t st, const float* actions, float* obs, float* reward, uint8_t* done, int* goal_idx, float* info);
hipError_t mzk_ant_forward(mz_handle* h, hipStream_t st, const float* actions, float* qacc, int* counts);
hipError_t mzk_ant_reset(mz_handle* h, hipStream_t st, const uint8_t* mask, uint64_t seed, float* obs);
hipError_t mzk_ant_set_state(mz_handle* h, hipStream_t st, const float* qpos, const float* qvel, const float* warm, const int* t);
hipError_t mzk_ant_get_state(mz_handle* h, hipStream_t st, float* qpos, float* qvel, float* warm, int* t);
hipError_t mzk_ant_task_eval(mz_handle* h, hipStream_t st, int n, const float* obs, float* reward, uint8_t* done, int* goal_idx);

// launch shape the next mz_step takes (mz_get_info): lanes per env, and for the plain ant at 16 lanes which instantiation (1 / 2 waves per SIMD)
void mzk_ant_shape(const mz_handle* h, int* lanes, int* waves_per_simd);
int mzk_ant_lanes_ok(const mz_handle* h, int lanes);  // 1: the Ant ladder has a step instantiation of that lane count for the handle's movable bodies
int mzk_planar_lanes(const mz_handle* h);

// ---- planar_kernels.hip (Point, Swimmer, Reacher)
hipError_t mzk_planar_step(mz_handle* h, hipStream_t st, const float* actions, float* obs, float* reward, uint8_t* done, int* goal_idx, float* info);
hipError_t mzk_planar_reset(mz_handle* h, hipStream_t st, const uint8_t* mask, uint64_t seed, float* obs);
hipError_t mzk_planar_set_state(mz_handle* h, hipStream_t st, const float* qpos, const float* qvel, const int* t);
hipError_t mzk_planar_get_state(mz_handle* h, hipStream_t st, float* qpos, float* qvel, float* warm, int* t);
hipError_t mzk_planar_task_eval(mz_handle* h, hipStream_t st, int n, const float* obs, float* reward, uint8_t* done, int* goal_idx);
hipError_t mzk_point_detect(mz_handle* h, hipStream_t st, int n, const double* old_xy, const double* new_xy, int* hit, double* point,
                            double* final_xy);
// MazeEnv.get_top_down_view into the rows the step / reset kernel just wrote (no-op unless the task has TOP_DOWN_VIEW):
// every row of obs, and the rows of final_obs of envs that finished (done != NULL: the step under auto-reset)
hipError_t mzk_view_fill(mz_handle* h, hipStream_t st, float* obs, float* final_obs, const uint8_t* done);
// mz_rollout on the fused kernels (Point / Swimmer / Reacher without a top-down view): no launch advances more than
// MZ_ROLLOUT_CHUNK steps, which bounds a kernel's duration
constexpr int MZ_ROLLOUT_CHUNK = 256;
int mzk_planar_rollout_fused(const mz_handle* h);

// One rollout call, whichever entry of include/mazestep.h it came through (mz_rollout, mz_rollout_policy, mz_rollout_policy_sample,
// mz_rollout_actor_critic, mz_rollout_net, mz_rollout_ex).  The entry checks its arguments and fills a plan; rollout_run (mazestep.hip)
// is the one driver that executes it, and mzk_planar_rollout below the one launcher of the fused kernels.  Arrays as in mz_rollout_io.
struct RolloutPlan {
  const char* who;  // the entry the call stands for: the name in the messages of a refusal
  int n_steps;
  // the action source: a tensor ..
  const float* actions_dev;
  long action_step_stride;
  // .. or an actor (sample: drawn from its Gaussian with the noise of (noise_seed, noise_step + k), formed in noise_mode = MZ_NOISE_*)
  const mz_net* actor;
  int sample;
  uint64_t noise_seed, noise_step;
  int noise_mode;
  // an optional critic beside the actor; the two sequences are not read without one
  const mz_net* critic;
  float *value_seq_dev, *next_value_seq_dev;
  // the call came through an entry that takes an int `hidden` (the networks are then legacy_net's, mazestep.hip)
  int legacy;
  // outputs: obs, reward, done required; logp_seq is not read unless sample
  float *obs_dev, *reward_dev;
  uint8_t* done_dev;
  int32_t* goal_idx_dev;
  float *info_dev, *obs_seq_dev, *actions_seq_dev, *logp_seq_dev, *next_obs_seq_dev;
  // a state-dependent log-std head on the actor (mz_rollout_head; NULL: none) and logf((float)actor->action_scale), computed once by the
  // entry
  const mz_head* head;
  float head_logA;
  // a context behind the observation (mz_rollout_ctx; NULL: none): such a plan runs the launch-by-launch loop on every handle
  const mz_context* ctx;
};

// The kernels a closed-loop plan runs: what every entry launched before there was a plan, and what it must go on launching.
//
//   call                                               | launch-by-launch loop                     | fused (Point / Swimmer without view)
//   ---------------------------------------------------+-------------------------------------------+-------------------------------------
//   legacy entry, no normaliser bound                  | policy_act_kernel / policy_sample_kernel  | non-DEEP instantiations
//                                                      |   / value_kernel              (one_layer) |
//   mz_rollout_net / mz_rollout_ex, both nets at most  | net_act_kernel<false>                     | non-DEEP instantiations
//     one tanh hidden layer, no normaliser             |   / net_value_kernel<false>               |
//   any other shape, no normaliser                     | the same net kernels                      | DEEP
//   normaliser bound (any entry)                       | net_*_kernel<true>                        | DEEP + NRM
//   a head on the actor (mz_rollout_head)              | net_sample_head_kernel<NRM>               | SMP + DEEP + EXT (+ NRM)
//
// EXT exactly when next_obs_seq is given, a sampled call uses MZ_NOISE_ACTION or the actor has a head (whose fields travel beside the
// noise mode and are read by the SMP + DEEP + EXT instantiations alone); an open-loop plan reads `ext` alone.
struct RolloutKernels { bool one_layer, deep, nrm, ext; };
inline RolloutKernels mzk_rollout_kernels(const mz_handle* h, const RolloutPlan& p) {
  auto shallow = [](const mz_net* net) { return !net || (net->n_hidden <= 1 && net->activation == MZ_ACT_TANH); };
  const bool nrm = h->nrm_mean != nullptr;
  return RolloutKernels{p.legacy && !nrm, nrm || p.head || !shallow(p.actor) || !shallow(p.critic), nrm,
                        p.next_obs_seq_dev || p.head || (p.sample && p.noise_mode != MZ_NOISE_PRE_SQUASH)};
}
// the plan on the fused kernels: launches of at most MZ_ROLLOUT_CHUNK steps with the launch geometry and the instantiation of the step
// kernel they stand for — the open-loop kernels for a tensor of actions, else the policy kernels' SMP / CRT / DEEP / NRM / EXT
// instantiation of mzk_rollout_kernels; every launch writes obs at its last step.  The caller has checked the plan.
hipError_t mzk_planar_rollout(mz_handle* h, hipStream_t st, const RolloutPlan& p);
int mzk_planar_state_width(const mz_handle* h);  // coordinates per env of the state (NV)
int mzk_planar_record_width(const mz_handle* h); // Point: floats per env-major record; 0 for the chains (SoA)

// ---- generic_kernels.hip (a user robot of any tree topology, csrc/generic_dyn.h)
int mzk_generic_needed(const mz_model* m);  // no specialised kernel steps this model, or the caller asked for the general engine (mz_model.engine)
int mzk_generic_create(mz_handle* h, char* err, int errlen);  // builds + uploads the constant block; MZ_OK or MZ_ERR_*
void mzk_generic_destroy(mz_handle* h);
hipError_t mzk_generic_step(mz_handle* h, hipStream_t st, const float* actions, float* obs, float* reward, uint8_t* done, int* goal_idx, float* info);
hipError_t mzk_generic_reset(mz_handle* h, hipStream_t st, const uint8_t* mask, uint64_t seed, float* obs);
hipError_t mzk_generic_set_state(mz_handle* h, hipStream_t st, const float* qpos, const float* qvel, const float* warm, const int* t);
hipError_t mzk_generic_get_state(mz_handle* h, hipStream_t st, float* qpos, float* qvel, float* warm, int* t);
hipError_t mzk_generic_set_task(mz_handle* h, const TaskDev* task);  // replaces the task block of the device constants (mz_set_goals)
hipError_t mzk_generic_task_eval(mz_handle* h, hipStream_t st, int n, const float* obs, float* reward, uint8_t* done, int* goal_idx);

// ---- render_kernels.hip (render.render_top_down for a batch: mz_render)
// images i < count of R's model: qpos row i (qpos_by_env = 0) or row env_idx[i] (qpos_by_env = 1) of qpos, [nq] floats each;
// env_idx NULL = 0 .. count - 1; an env index outside 0 .. n - 1 gives an all-zero image.  rgb: uint8 [count][height][width][3]
hipError_t mzk_render(mz_handle* h, hipStream_t st, const RenderDev* R, const float* qpos, int qpos_by_env, const int* env_idx, int count,
                      int width, int height, uint8_t* rgb);
