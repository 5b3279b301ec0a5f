// planar_kernels.hip — HIP kernels (gfx950 / CDNA4) of the Point, Swimmer and Reacher paths and their launchers.
//
//   planar_step_kernel<NB,NS,G>  one MazeEnv.step for the Point (+ NB movable blocks or NS object balls): lane group
//                                per env, PlanarScratch in LDS, fp64.
//   swimmer_step_kernel<NL,NB,G> one MazeEnv.step for the Swimmer (NL = 3) / Reacher (NL = 2): G = 4 lanes per env (lane b = link b), fp64.
//   planar_rollout_kernel / swimmer_rollout_kernel  up to MZ_ROLLOUT_CHUNK steps of the same on a state that stays on chip (mz_rollout).
//   planar_policy_rollout_kernel / swimmer_policy_rollout_kernel  the same with the actions of every step computed on chip by the policy
//                                of mz_policy.h from the step's observation row (mz_rollout_policy), or sampled from its Gaussian
//                                (SMP instantiations: mz_rollout_policy_sample); CRT instantiations also evaluate a critic on the rows
//                                (mz_rollout_actor_critic).
//   reset / state copy kernels; debug kernels for the parity tests (task predicates, the Point's wall detector).
//
// HBM layout: SoA  q_0..q_{NV-1} | v_0..v_{NV-1}, each [N] fp32; t[N], episode[N] i32.  API arrays are row-major [N, k].
//
// This translation unit is built without -fapprox-func / -fno-signed-zeros (csrc/Makefile); the dynamics may use
// reciprocal division, but the Point's manual wall detector (point_dyn.h: point_detect / point_bounce) and the task
// predicates reproduce the reference's float64 decisions bit for bit — inside those functions contraction, reciprocal
// division and reassociation are switched off (#pragma clang fp ...), and sqrt is correctly rounded.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "mz_task.h"
#include "point_dyn.h"
#include "planar_dyn.h"
#include "swimmer_dyn.h"
#include "mz_device.h"
#include "mz_internal.h"
#include "mz_policy.h"

// ------------------------------------------------------------------ state in HBM
// Chains (Swimmer / Reacher: 64 envs per workgroup): SoA qv[2 NV][n] + t[n] + episode[n] — a wave's loads of one coordinate are one line.
// Point (`rec` > 0; round 4): env-major records qv[n][rec] = q[NV] | v[NV] | t | episode (| pad to a multiple of 4 floats).  A Point
// workgroup is ONE wave = 2 envs (32 lanes each): in SoA it touched 8 bytes of eight different 128-byte lines per array pass, and
// every such partial store left the L2 as a transaction of its own (PMC, round 4: WRITE_SIZE 1.9 MB per launch against 0.3 MB of
// algorithmic writes, FETCH_SIZE 1.1 MB against 0.2); its two records are 64 contiguous bytes.
struct PointState { float* qv; int* t; uint32_t* ep; int rec; };
// The bare Point's record (no movable bodies) carries the solver's warm start behind t | episode: qacc - qacc_smooth of the step's last
// forward evaluation, the first guess of the next step's first solve (round 6; reset and set_state clear it)
constexpr int PT_WARM_OFF = 8;
__device__ __forceinline__ float& st_q(const PointState& S, int n, int nv, int k, int env) { return S.rec ? S.qv[(size_t)env * S.rec + k] : S.qv[(size_t)k * n + env]; }
__device__ __forceinline__ float& st_v(const PointState& S, int n, int nv, int k, int env) { return S.rec ? S.qv[(size_t)env * S.rec + nv + k] : S.qv[(size_t)(nv + k) * n + env]; }
__device__ __forceinline__ int& st_t(const PointState& S, int nv, int env) { return S.rec ? reinterpret_cast<int*>(S.qv)[(size_t)env * S.rec + 2 * nv] : S.t[env]; }
__device__ __forceinline__ uint32_t& st_ep(const PointState& S, int nv, int env) { return S.rec ? reinterpret_cast<uint32_t*>(S.qv)[(size_t)env * S.rec + 2 * nv + 1] : S.ep[env]; }

// One MazeEnv.step of the Point (+ NB movable blocks or NS object balls): G lanes per env, PlanarScratch in LDS, SoA state in HBM
// (q_0..q_{NV-1} | v_0..v_{NV-1}, each [n]).
// The bare Point at 32 lanes per env runs two waves per SIMD (4096 envs = 2048 waves on 1024 SIMDs): its register budget is pinned
// to 256 so that a few registers more do not silently halve the occupancy and send half the waves into a second round.
template <int NB, int NS, int G>
__device__ __forceinline__ void planar_step_body(const PointDev& P, PlanarScratch<NB, NS>& s, float* o, const DevCtx<G>& cx, int n, const PointState& S,
                                                 int env, bool live, const float* __restrict__ actions, float* __restrict__ obs,
                                                 float* __restrict__ reward, uint8_t* __restrict__ done, int* __restrict__ goal_idx,
                                                 float* __restrict__ info, int* __restrict__ status, int auto_reset, uint64_t seed, uint64_t env0,
                                                 float* __restrict__ final_obs, int ostride) {
  using D = PlanarDims<NB, NS>;
  constexpr int NV = D::NV, NOBS = D::NOBS;
  for (int k = cx.l; k < NV; k += G) { s.q[k] = (double)st_q(S, n, NV, k, env); s.v[k] = (double)st_v(S, n, NV, k, env); }
  if constexpr (NB == 0 && NS == 0) { for (int k = cx.l; k < 3; k += G) s.wds[k] = (double)S.qv[(size_t)env * S.rec + PT_WARM_OFF + k]; }  // the bare Point's warm start
  double a[2] = {(double)actions[(size_t)env * 2], (double)actions[(size_t)env * 2 + 1]};
  cx.sync();
  planar_env_step<NB, NS>(cx, P, s, a);
  const int t_new = st_t(S, NV, env) + 1;  // (read here, behind the step: one register less carried through it)
  for (int i = cx.l; i < NOBS; i += G) o[i] = planar_obs_elem<NB, NS>(P, s, i, t_new);
  cx.sync();
  float outer; int tm, gi;
  task_eval_dev(P.task, o, &outer, &tm, &gi, env);  // flags from the fp32 observation that is returned
  const uint8_t d = (uint8_t)((tm ? 1 : 0) | (t_new >= P.task.max_steps ? 2 : 0));
  const bool rst = auto_reset && d;  // vector-env convention: obs <- first observation of the new episode, terminal one -> final_obs
  if (live) {
    // rows are `ostride` floats apart: NOBS, or NOBS + MZ_VIEW_DIM with the time entry behind the view (mz_device.h obs_slot)
    float* orow = ((rst && final_obs) ? final_obs : obs) + (size_t)env * ostride;
    if (!rst || final_obs) {
      for (int i = cx.l; i < NOBS; i += G) orow[obs_slot(i, NOBS, ostride)] = o[i];
      if (ostride != NOBS) for (int i = cx.l; i < 2 * NB; i += G) orow[NOBS - 1 + i] = planar_block_coord<NB, NS>(P, s, i >> 1, i & 1);
    }
    if (cx.l == 0) {
      reward[env] = outer;  // Point inner reward is 0.0 (point.py:61)
      done[env] = d;
      if (goal_idx) goal_idx[env] = gi;
      if (info) { info[(size_t)env * 4] = o[0]; info[(size_t)env * 4 + 1] = o[1]; info[(size_t)env * 4 + 2] = 0.f; info[(size_t)env * 4 + 3] = 0.f; }
      int st = s.status;
      bool badv = false;
      for (int k = 0; k < NV; k++) badv = badv || !(fabs(s.q[k]) < 1e10) || !(fabs(s.v[k]) < 1e10);
      if (badv) st |= MZ_STATUS_BAD_STATE;
      if (st) atomicOr(&status[env], st);
    }
  }
  uint32_t ep = st_ep(S, NV, env);
  if (rst) {  // point.py:71-81: noise on the robot, blocks / ball back to their spawn state
    ep += 1;
    const uint64_t es = episode_seed(seed, ep);
    cx.sync();
    for (int k = cx.l; k < NV; k += G) {
      s.q[k] = k < 3 ? (double)reset_qpos((float)P.qpos0[k], es, env0 + (uint64_t)env, k) : 0.0;
      s.v[k] = k < 3 ? (double)reset_qvel(P.reset_kind, NV, es, env0 + (uint64_t)env, k) : 0.0;
    }
    cx.sync();
    if (live) {
      float* orow = obs + (size_t)env * ostride;
      for (int i = cx.l; i < NOBS; i += G) orow[obs_slot(i, NOBS, ostride)] = planar_obs_elem<NB, NS>(P, s, i, 0);
      if (ostride != NOBS) for (int i = cx.l; i < 2 * NB; i += G) orow[NOBS - 1 + i] = planar_block_coord<NB, NS>(P, s, i >> 1, i & 1);
    }
  }
  if (live) {
    for (int k = cx.l; k < NV; k += G) {
      st_q(S, n, NV, k, env) = (float)s.q[k];
      st_v(S, n, NV, k, env) = (float)s.v[k];
    }
    if (cx.l == 0) { st_t(S, NV, env) = rst ? 0 : t_new; st_ep(S, NV, env) = ep; }
    if constexpr (NB == 0 && NS == 0) { for (int k = cx.l; k < 3; k += G) S.qv[(size_t)env * S.rec + PT_WARM_OFF + k] = rst ? 0.f : (float)s.wds[k]; }
  }
}

template <int NB, int NS, int G>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((NB == 0 && NS == 0 && G == 32) ? 2 : 1))) void planar_step_kernel(const PointDev* __restrict__ Pp, int n, PointState S,
                                                          const float* __restrict__ actions, float* __restrict__ obs,
                                                          float* __restrict__ reward, uint8_t* __restrict__ done,
                                                          int* __restrict__ goal_idx, float* __restrict__ info,
                                                          int* __restrict__ status, int auto_reset, uint64_t seed, uint64_t env0,
                                                          float* __restrict__ final_obs, int ostride) {
  constexpr int EPW = 64 / G;
  __shared__ PointDev P;  // segment table + task shared by the block (L2-resident source)
  __shared__ PlanarScratch<NB, NS> scr[EPW];
  __shared__ float obuf[EPW][MZ_MAX_OBS];
  for (int i = threadIdx.x; i < (int)(sizeof(PointDev) / 4); i += blockDim.x) ((uint32_t*)&P)[i] = ((const uint32_t*)Pp)[i];
  __syncthreads();
  DevCtx<G> cx{(int)threadIdx.x % G};
  const int grp = threadIdx.x / G;
  int env = xcd_block(blockIdx.x, gridDim.x) * EPW + grp;
  const bool live = env < n;
  if (!live) env = n - 1;  // idle groups shadow the last env (no stores) so that every lane reaches the wave-level votes
  planar_step_body<NB, NS, G>(P, scr[grp], obuf[grp], cx, n, S, env, live, actions, obs, reward, done, goal_idx, info, status, auto_reset, seed, env0, final_obs,
                              ostride);
}

// `nsteps` (<= MZ_ROLLOUT_CHUNK) successive planar_step_kernel launches in one (mz_rollout): PointDev and the env's state are loaded
// once, the steps run on the state in LDS, the state is stored once.  Between two steps the state takes exactly the values the HBM
// round trip of separate launches gives it — q, v and the bare Point's warm start rounded to fp32 and widened again, t and the episode
// counter carried as ints — so the outputs equal those of sequential stepping bit for bit.  Step k reads its actions at
// actions + k * astride and writes row k of reward / done / goal_idx / info / obs_seq ([nsteps][n][..]; obs_seq nullable); `obs` gets
// the row of step last_obs_step only (-1: none — a later launch of the same rollout writes it).  No top-down view: rows are NOBS floats apart.
// EXT (mz_rollout_ex with next_obs_seq_dev): every step also stores the row it produced, before any auto-reset, to row k of
// next_obs_seq — from `o`, inside the `if (live)` block, before the reset rewrites it.  A template flag, not a nullable argument alone:
// the extra pointer cost the existing instantiations registers or scratch (profiles/rollout/transitions.md).  EXT == false compiles
// the source as it was and never reads next_obs_seq.
template <int NB, int NS, int G, bool EXT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((NB == 0 && NS == 0 && G == 32) ? 2 : 1))) void planar_rollout_kernel(
    const PointDev* __restrict__ Pp, int n, PointState S, int nsteps, const float* __restrict__ actions, long astride, float* __restrict__ obs,
    int last_obs_step, float* __restrict__ reward, uint8_t* __restrict__ done, int* __restrict__ goal_idx, float* __restrict__ info,
    float* __restrict__ obs_seq, int* __restrict__ status, int auto_reset, uint64_t seed, uint64_t env0, float* __restrict__ final_obs,
    float* __restrict__ next_obs_seq) {
  using D = PlanarDims<NB, NS>;
  constexpr int NV = D::NV, NOBS = D::NOBS, EPW = 64 / G;
  constexpr bool BARE = NB == 0 && NS == 0;
  __shared__ PointDev P;
  __shared__ PlanarScratch<NB, NS> scr[EPW];
  __shared__ float obuf[EPW][MZ_MAX_OBS];
  for (int i = threadIdx.x; i < (int)(sizeof(PointDev) / 4); i += blockDim.x) ((uint32_t*)&P)[i] = ((const uint32_t*)Pp)[i];
  __syncthreads();
  DevCtx<G> cx{(int)threadIdx.x % G};
  const int grp = threadIdx.x / G;
  int env = xcd_block(blockIdx.x, gridDim.x) * EPW + grp;
  const bool live = env < n;
  if (!live) env = n - 1;  // idle groups shadow the last env (no stores), as in planar_step_kernel
  PlanarScratch<NB, NS>& s = scr[grp];
  float* o = obuf[grp];
  for (int k = cx.l; k < NV; k += G) { s.q[k] = (double)st_q(S, n, NV, k, env); s.v[k] = (double)st_v(S, n, NV, k, env); }
  if constexpr (BARE) { for (int k = cx.l; k < 3; k += G) s.wds[k] = (double)S.qv[(size_t)env * S.rec + PT_WARM_OFF + k]; }
  int t = st_t(S, NV, env), stacc = 0;
  uint32_t ep = st_ep(S, NV, env);
  for (int step = 0; step < nsteps; step++) {
    const float* act = actions + (size_t)step * astride + (size_t)env * 2;
    double a[2] = {(double)act[0], (double)act[1]};
    cx.sync();
    planar_env_step<NB, NS>(cx, P, s, a);
    const int t_new = t + 1;
    for (int i = cx.l; i < NOBS; i += G) o[i] = planar_obs_elem<NB, NS>(P, s, i, t_new);
    cx.sync();
    float outer; int tm, gi;
    task_eval_dev(P.task, o, &outer, &tm, &gi, env);
    const uint8_t d = (uint8_t)((tm ? 1 : 0) | (t_new >= P.task.max_steps ? 2 : 0));
    const bool rst = auto_reset && d;
    const size_t row = (size_t)step * n + env;
    float* oseq = obs_seq ? obs_seq + row * NOBS : nullptr;
    float* olast = step == last_obs_step ? obs + (size_t)env * NOBS : nullptr;
    if (live) {
      if constexpr (EXT) {  // the row this step produced, before a reset rewrites o
        if (next_obs_seq) for (int i = cx.l; i < NOBS; i += G) next_obs_seq[row * NOBS + i] = o[i];
      }
      if (rst) {
        if (final_obs) for (int i = cx.l; i < NOBS; i += G) final_obs[(size_t)env * NOBS + i] = o[i];
      } else {
        if (oseq) for (int i = cx.l; i < NOBS; i += G) oseq[i] = o[i];
        if (olast) for (int i = cx.l; i < NOBS; i += G) olast[i] = o[i];
      }
      if (cx.l == 0) {
        reward[row] = outer;
        done[row] = d;
        if (goal_idx) goal_idx[row] = gi;
        if (info) { info[row * 4] = o[0]; info[row * 4 + 1] = o[1]; info[row * 4 + 2] = 0.f; info[row * 4 + 3] = 0.f; }
        int st = s.status;
        bool badv = false;
        for (int k = 0; k < NV; k++) badv = badv || !(fabs(s.q[k]) < 1e10) || !(fabs(s.v[k]) < 1e10);
        if (badv) st |= MZ_STATUS_BAD_STATE;
        stacc |= st;
      }
    }
    cx.sync();  // lane 0 has read the whole state
    if (rst) {
      ep += 1;
      const uint64_t es = episode_seed(seed, ep);
      for (int k = cx.l; k < NV; k += G) {
        s.q[k] = k < 3 ? (double)reset_qpos((float)P.qpos0[k], es, env0 + (uint64_t)env, k) : 0.0;
        s.v[k] = k < 3 ? (double)reset_qvel(P.reset_kind, NV, es, env0 + (uint64_t)env, k) : 0.0;
      }
      cx.sync();
      if (live) {
        if (oseq) for (int i = cx.l; i < NOBS; i += G) oseq[i] = planar_obs_elem<NB, NS>(P, s, i, 0);
        if (olast) for (int i = cx.l; i < NOBS; i += G) olast[i] = planar_obs_elem<NB, NS>(P, s, i, 0);
      }
      cx.sync();
    }
    t = rst ? 0 : t_new;
    // the state as the next launch of planar_step_kernel would load it
    for (int k = cx.l; k < NV; k += G) { s.q[k] = (double)(float)s.q[k]; s.v[k] = (double)(float)s.v[k]; }
    if constexpr (BARE) { for (int k = cx.l; k < 3; k += G) s.wds[k] = rst ? 0.0 : (double)(float)s.wds[k]; }
  }
  cx.sync();
  if (live) {
    for (int k = cx.l; k < NV; k += G) {
      st_q(S, n, NV, k, env) = (float)s.q[k];
      st_v(S, n, NV, k, env) = (float)s.v[k];
    }
    if (cx.l == 0) {
      st_t(S, NV, env) = t; st_ep(S, NV, env) = ep;
      if (stacc) atomicOr(&status[env], stacc);
    }
    if constexpr (BARE) { for (int k = cx.l; k < 3; k += G) S.qv[(size_t)env * S.rec + PT_WARM_OFF + k] = (float)s.wds[k]; }
  }
}

// mzp_group_net_sample_head for the fused kernels, NOT inlined: inlined, the second sampling path cost every SMP + DEEP + EXT
// instantiation about 25 AGPRs (the bare Point at 32 lanes: 100 bytes of scratch per lane) and the calls without a head 3 % on the
// Point; behind a call the callers keep their registers to within a few AGPRs (profiles/rollout/sac_head.md).  The pointers arrive
// as generic ones (hid, hid2 and act are LDS, x is LDS or global memory), which only the head path pays for; the arithmetic is the
// header's, so the bits are those of net_sample_head_kernel (mazestep.hip).  Every lane of the wavefront makes the call (ns.head is
// uniform), act is always stored.
__device__ __attribute__((noinline)) void planar_head_act(int l, int G, const float* par, int obs_dim, int nu, mzp_shape s, int squash, float action_scale,
                                                          mzp_head hd, uint64_t key, uint64_t slot, const float* x, float* hid, float* hid2, float* act,
                                                          float* logp) {
  mzp_group_net_sample_head(l, G, par, obs_dim, nu, s, squash, action_scale, hd, key, slot, x, hid, hid2, act, true, logp);
}

// planar_rollout_kernel with the actions computed on chip (mz_rollout_policy): before every step the group evaluates the policy of
// mz_policy.h on the fp32 observation row in `o` — for the launch's first step the row of `obs` (what the previous launch, mz_step or
// mz_reset wrote there), afterwards the row the step before computed, after an in-kernel auto-reset the new episode's t = 0 row — with
// the unit functions policy_act_kernel (mazestep.hip) runs on the same row, so a_k and everything after it equal the loop of
// mz_policy_act and mz_step bit for bit.  Lanes l, l + G, .. own hidden units (phid), lanes 0 and 1 the two outputs (pact); `obs` is
// written at the launch's last step, always: the next launch of the same rollout reads its first row there.  Idle groups shadow the
// last env through every hand-off and store nothing.  A kernel of its own beside planar_rollout_kernel, whose code stays what it was.
// SMP (mz_rollout_policy_sample): the policy is the diagonal Gaussian of mz_policy.h — the lane that owns output u draws eps_u for
// (ns.seed, ns.step + step, env0 + env, u) and forms the action, the group's first lane writes the row of ns.logp_seq, actions_seq
// gets the sampled actions — with the unit functions policy_sample_kernel (mazestep.hip) runs: equal to the loop of mz_policy_sample
// and mz_step bit for bit.  SMP == false compiles the deterministic kernel's source unchanged and never reads `ns`.
struct PolicyNoise {
  uint64_t seed, step;  // noise_seed; noise_step of the launch's first step
  float* logp_seq;      // [nsteps][n] rows of the launch (nullable)
  int mode;             // MZ_NOISE_* (mz_policy.h mzp_sample_unit), read by the EXT instantiations alone
  int head;             // 1: the actor has the state-dependent log-std head `hd` (mz_rollout_head; mz_policy.h mzp_group_net_sample_head), its
  mzp_head hd;          //    output layer 2 nu units wide; both read by the SMP + DEEP + EXT instantiations alone, where every head plan goes
};
// CRT (mz_rollout_actor_critic with a critic): the group also evaluates the critic of mz_policy.h (mzp_group_value: the unit functions
// value_kernel, mazestep.hip, runs) on the rows in `o` — at the launch's start on its first row; after every step on the row the step
// produced, which is the terminal row when the env is about to reset (next_value_seq[k]); if the env did not reset that same number
// is value_seq[k + 1] (one evaluation, stored twice), if it did the new episode's first row is valued once more.  The hidden units go
// through phid, which is free between the hand-over of the actor's outputs and the next evaluation of the actor; the group's first
// lane holds the value.  CRT == false compiles the source without it and never reads `cr`.
struct PolicyCritic {
  const float* params;    // [nvpar], or [n][nvpar] with stride = nvpar
  long stride;
  int hidden;
  float* value_seq;       // [nsteps][n] rows of the launch (nullable)
  float* next_value_seq;  // [nsteps][n] rows of the launch (nullable)
};
// DEEP (mz_rollout_net where a network has two hidden layers or ReLU units): actor and critic are networks of the shapes in `sh`
// (mzp_group_net_act / mzp_group_net_value: the unit functions net_act_kernel and net_value_kernel, mazestep.hip, run), and every
// group has a second hidden row (phid[grp][1]) for the second hidden vector; `hidden` and cr.hidden are not read.  The hand-offs are
// those of the one-layer kernel — the critic takes both hidden rows only after the actor's outputs have been handed over — plus the
// phase boundary behind each hidden layer inside the group functions.  A template parameter, not a run-time depth: DEEP == false
// compiles the source as it was, never reads `sh`, and its instantiations keep their registers and their LDS.
struct PolicyShapes {
  mzp_shape actor, critic;
};
// NRM (a normaliser bound with mz_bind_obs_norm; instantiated for DEEP alone — bound handles route every shape there): the networks
// read the normalised row of mz_policy.h, staged in a second LDS row per group (pnrm) beside the raw row `o`.  Every lane writes the
// elements of pnrm it owns where it writes those of `o` — at the launch's start, after a step, after an in-kernel reset: the three
// places after which a network reads the row — from the raw value it has just stored, so pnrm is rewritten exactly where `o` is and
// the hand-offs that keep `o` from being rewritten under a reader keep pnrm.  Only the actor and the critic read pnrm; the task
// predicate, every observation store and info read `o`.  NRM == false compiles the source as it was and never reads `nm`.
// EXT (mz_rollout_ex with next_obs_seq_dev or MZ_NOISE_ACTION): as in planar_rollout_kernel, and the sampled actions are formed in
// the mode ns.mode.  EXT == false compiles the source as it was: it never reads next_obs_seq, and samples in MZ_NOISE_PRE_SQUASH.
// A head actor (mz_rollout_head: ns.head) is a run-time branch of the SMP + DEEP + EXT instantiations — planar_head_act above:
// mzp_group_net_sample_head, the unit functions net_sample_head_kernel (mazestep.hip) runs, in place of mzp_group_net_act; the
// log-prob terms go to the group's first lane through the hidden row the output layer does not read, which nothing rewrites before
// the hand-over of pact.
template <int NB, int NS, int G, bool SMP = false, bool CRT = false, bool DEEP = false, bool NRM = false, bool EXT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((NB == 0 && NS == 0 && G == 32) ? 2 : 1))) void planar_policy_rollout_kernel(
    const PointDev* __restrict__ Pp, int n, PointState S, int nsteps, const float* __restrict__ params, long pstride, int hidden, int squash,
    float action_scale, float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ done, int* __restrict__ goal_idx,
    float* __restrict__ info, float* __restrict__ obs_seq, float* __restrict__ actions_seq, int* __restrict__ status, int auto_reset,
    uint64_t seed, uint64_t env0, float* __restrict__ final_obs, PolicyNoise ns, PolicyCritic cr, PolicyShapes sh, mzp_norm nm,
    float* __restrict__ next_obs_seq) {
  static_assert(!NRM || DEEP, "the normalised row is staged in the DEEP instantiations only");
  using D = PlanarDims<NB, NS>;
  constexpr int NV = D::NV, NOBS = D::NOBS, EPW = 64 / G;
  constexpr bool BARE = NB == 0 && NS == 0;
  __shared__ PointDev P;
  __shared__ PlanarScratch<NB, NS> scr[EPW];
  __shared__ float obuf[EPW][MZ_MAX_OBS];
  __shared__ float phid[EPW][DEEP ? 2 : 1][MZ_POLICY_MAX_HIDDEN];
  __shared__ float pact[EPW][2];
  __shared__ float pnrm[NRM ? EPW : 1][NRM ? MZ_MAX_OBS : 1];  // (never referenced without NRM: no LDS is allocated for it)
  for (int i = threadIdx.x; i < (int)(sizeof(PointDev) / 4); i += blockDim.x) ((uint32_t*)&P)[i] = ((const uint32_t*)Pp)[i];
  __syncthreads();
  DevCtx<G> cx{(int)threadIdx.x % G};
  const int grp = threadIdx.x / G;
  int env = xcd_block(blockIdx.x, gridDim.x) * EPW + grp;
  const bool live = env < n;
  if (!live) env = n - 1;  // idle groups shadow the last env (no stores), as in planar_step_kernel
  PlanarScratch<NB, NS>& s = scr[grp];
  float* o = obuf[grp];
  auto stage = [&](int i) {  // element i of the normalised row from the raw element this lane has just written
    if constexpr (NRM) pnrm[grp][i] = mzp_norm_elem(o[i], nm.mean[i], nm.inv_std[i], nm.clip);
  };
  const float* par = params + (size_t)env * pstride;
  for (int k = cx.l; k < NV; k += G) { s.q[k] = (double)st_q(S, n, NV, k, env); s.v[k] = (double)st_v(S, n, NV, k, env); }
  if constexpr (BARE) { for (int k = cx.l; k < 3; k += G) s.wds[k] = (double)S.qv[(size_t)env * S.rec + PT_WARM_OFF + k]; }
  for (int i = cx.l; i < NOBS; i += G) { o[i] = obs[(size_t)env * NOBS + i]; stage(i); }  // the observation the policy acts on first
  int t = st_t(S, NV, env), stacc = 0;
  uint32_t ep = st_ep(S, NV, env);
  const float* vpar = nullptr;
  float vcur = 0.0f;  // the group's first lane: V(the row in o)
  auto value_of_row = [&]() -> float {  // every lane of the group; phid must be free (mzp_group_value)
    if constexpr (NRM) return mzp_group_net_value(cx.l, G, vpar, NOBS, sh.critic, pnrm[grp], phid[grp][0], phid[grp][DEEP ? 1 : 0]);
    else if constexpr (DEEP) return mzp_group_net_value(cx.l, G, vpar, NOBS, sh.critic, o, phid[grp][0], phid[grp][DEEP ? 1 : 0]);
    else return mzp_group_value(cx.l, G, vpar, NOBS, cr.hidden, o, phid[grp][0]);
  };
  if constexpr (CRT) {
    vpar = cr.params + (size_t)env * cr.stride;
    cx.sync();  // the row in o is complete
    vcur = value_of_row();
  }
  for (int step = 0; step < nsteps; step++) {
    const size_t row = (size_t)step * n + env;
    cx.sync();  // the row in o is complete (CRT: and the critic is done with phid)
    if constexpr (CRT) { if (live && cx.l == 0 && cr.value_seq) cr.value_seq[row] = vcur; }
    bool head = false;  // (a run-time branch of the SMP + DEEP + EXT instantiations: no instantiation of its own)
    if constexpr (SMP && DEEP && EXT) head = ns.head != 0;
    if (head) {
      if constexpr (SMP && DEEP && EXT) {
        const float* xin;
        if constexpr (NRM) xin = pnrm[grp]; else xin = o;
        planar_head_act(cx.l, G, par, NOBS, 2, sh.actor, squash, action_scale, ns.hd, mzp_noise_key(ns.seed, ns.step + (uint64_t)step),
                        env0 + (uint64_t)env, xin, phid[grp][0], phid[grp][1], pact[grp], live && ns.logp_seq ? ns.logp_seq + row : nullptr);
      }
    } else if constexpr (NRM)
      mzp_group_net_act(cx.l, G, par, NOBS, 2, sh.actor, squash, action_scale, SMP, SMP ? mzp_noise_key(ns.seed, ns.step + (uint64_t)step) : 0,
                        env0 + (uint64_t)env, pnrm[grp], phid[grp][0], phid[grp][DEEP ? 1 : 0], pact[grp], true,
                        SMP && live && ns.logp_seq ? ns.logp_seq + row : nullptr, EXT ? ns.mode : MZ_NOISE_PRE_SQUASH);
    else if constexpr (DEEP)
      mzp_group_net_act(cx.l, G, par, NOBS, 2, sh.actor, squash, action_scale, SMP, SMP ? mzp_noise_key(ns.seed, ns.step + (uint64_t)step) : 0,
                        env0 + (uint64_t)env, o, phid[grp][0], phid[grp][DEEP ? 1 : 0], pact[grp], true,
                        SMP && live && ns.logp_seq ? ns.logp_seq + row : nullptr, EXT ? ns.mode : MZ_NOISE_PRE_SQUASH);
    else if constexpr (SMP)
      mzp_group_sample(cx.l, G, par, NOBS, 2, hidden, squash, action_scale, mzp_noise_key(ns.seed, ns.step + (uint64_t)step), env0 + (uint64_t)env, o,
                       phid[grp][0], pact[grp], true, live && ns.logp_seq ? ns.logp_seq + row : nullptr, EXT ? ns.mode : MZ_NOISE_PRE_SQUASH);
    else
      mzp_group_eval(cx.l, G, par, NOBS, 2, hidden, squash, action_scale, o, phid[grp][0], pact[grp], true);
    cx.sync();
    const float a0 = pact[grp][0], a1 = pact[grp][1];
    if (live && cx.l == 0 && actions_seq) { actions_seq[row * 2] = a0; actions_seq[row * 2 + 1] = a1; }
    double a[2] = {(double)a0, (double)a1};
    cx.sync();
    planar_env_step<NB, NS>(cx, P, s, a);
    const int t_new = t + 1;
    for (int i = cx.l; i < NOBS; i += G) { o[i] = planar_obs_elem<NB, NS>(P, s, i, t_new); stage(i); }
    cx.sync();
    float outer; int tm, gi;
    task_eval_dev(P.task, o, &outer, &tm, &gi, env);
    const uint8_t d = (uint8_t)((tm ? 1 : 0) | (t_new >= P.task.max_steps ? 2 : 0));
    const bool rst = auto_reset && d;
    float* oseq = obs_seq ? obs_seq + row * NOBS : nullptr;
    float* olast = step == nsteps - 1 ? obs + (size_t)env * NOBS : nullptr;
    if (live) {
      if constexpr (EXT) {  // the raw row this step produced, before a reset rewrites o
        if (next_obs_seq) for (int i = cx.l; i < NOBS; i += G) next_obs_seq[row * NOBS + i] = o[i];
      }
      if (rst) {
        if (final_obs) for (int i = cx.l; i < NOBS; i += G) final_obs[(size_t)env * NOBS + i] = o[i];
      } else {
        if (oseq) for (int i = cx.l; i < NOBS; i += G) oseq[i] = o[i];
        if (olast) for (int i = cx.l; i < NOBS; i += G) olast[i] = o[i];
      }
      if (cx.l == 0) {
        reward[row] = outer;
        done[row] = d;
        if (goal_idx) goal_idx[row] = gi;
        if (info) { info[row * 4] = o[0]; info[row * 4 + 1] = o[1]; info[row * 4 + 2] = 0.f; info[row * 4 + 3] = 0.f; }
        int st = s.status;
        bool badv = false;
        for (int k = 0; k < NV; k++) badv = badv || !(fabs(s.q[k]) < 1e10) || !(fabs(s.v[k]) < 1e10);
        if (badv) st |= MZ_STATUS_BAD_STATE;
        stacc |= st;
      }
    }
    cx.sync();  // lane 0 has read the whole state and the terminal row
    if constexpr (CRT) {  // V(the row this step produced), before a reset overwrites it; the actor's outputs were handed over above
      vcur = value_of_row();
      if (live && cx.l == 0 && cr.next_value_seq) cr.next_value_seq[row] = vcur;
    }
    if (rst) {
      ep += 1;
      const uint64_t es = episode_seed(seed, ep);
      for (int k = cx.l; k < NV; k += G) {
        s.q[k] = k < 3 ? (double)reset_qpos((float)P.qpos0[k], es, env0 + (uint64_t)env, k) : 0.0;
        s.v[k] = k < 3 ? (double)reset_qvel(P.reset_kind, NV, es, env0 + (uint64_t)env, k) : 0.0;
      }
      cx.sync();
      // the new episode's first row: what the policy acts on next (every lane stores the elements it has just written itself)
      for (int i = cx.l; i < NOBS; i += G) { o[i] = planar_obs_elem<NB, NS>(P, s, i, 0); stage(i); }
      if (live) {
        if (oseq) for (int i = cx.l; i < NOBS; i += G) oseq[i] = o[i];
        if (olast) for (int i = cx.l; i < NOBS; i += G) olast[i] = o[i];
      }
      cx.sync();  // the new row is complete (CRT: and the group's first lane has read the terminal value's hidden units)
      if constexpr (CRT) vcur = value_of_row();
    }
    t = rst ? 0 : t_new;
    // the state as the next launch of planar_step_kernel would load it
    for (int k = cx.l; k < NV; k += G) { s.q[k] = (double)(float)s.q[k]; s.v[k] = (double)(float)s.v[k]; }
    if constexpr (BARE) { for (int k = cx.l; k < 3; k += G) s.wds[k] = rst ? 0.0 : (double)(float)s.wds[k]; }
  }
  cx.sync();
  if (live) {
    for (int k = cx.l; k < NV; k += G) {
      st_q(S, n, NV, k, env) = (float)s.q[k];
      st_v(S, n, NV, k, env) = (float)s.v[k];
    }
    if (cx.l == 0) {
      st_t(S, NV, env) = t; st_ep(S, NV, env) = ep;
      if (stacc) atomicOr(&status[env], stacc);
    }
    if constexpr (BARE) { for (int k = cx.l; k < 3; k += G) S.qv[(size_t)env * S.rec + PT_WARM_OFF + k] = (float)s.wds[k]; }
  }
}

template <int NB, int NS>
__global__ void point_reset_kernel(const PointDev* Pp, int n, PointState S, const uint8_t* mask, uint64_t seed, uint64_t env0, float* obs,
                                   int ostride) {
  constexpr int NV = 3 + 2 * NB + 3 * NS, NOBS = 7 + 3 * NB + 3 * NS;
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  if (!mask || mask[env]) {
    for (int k = 0; k < NV; k++) {
      st_q(S, n, NV, k, env) = k < 3 ? reset_qpos((float)Pp->qpos0[k], seed, env0 + (uint64_t)env, k) : 0.f;
      st_v(S, n, NV, k, env) = k < 3 ? reset_qvel(Pp->reset_kind, NV, seed, env0 + (uint64_t)env, k) : 0.f;
    }
    st_t(S, NV, env) = 0;
    st_ep(S, NV, env) = 0;
    if (NB == 0 && NS == 0) for (int k = 0; k < 3; k++) S.qv[(size_t)env * S.rec + PT_WARM_OFF + k] = 0.f;
  }
  if (obs) {
    const int nb3 = (Pp->observe_blocks ? 3 * NB : 0) + (Pp->observe_balls ? 3 * NS : 0);
    float* o = obs + (size_t)env * ostride;
    for (int k = 0; k < 3; k++) { o[k] = st_q(S, n, NV, k, env); o[3 + nb3 + k] = st_v(S, n, NV, k, env); }
    // body origins exactly as the step kernels observe them (planar_origin_coord): the row of an env the mask leaves alone keeps
    // the bits the last step wrote
    if (NS > 0 && nb3) {
      o[3] = planar_origin_coord(Pp->ball_pos0[0], st_q(S, n, NV, 3, env)); o[4] = planar_origin_coord(Pp->ball_pos0[1], st_q(S, n, NV, 4, env));
      o[5] = (float)Pp->ball_pos0[2];
    }
    for (int b = 0; b < NB && nb3; b++) {
      float p3[3] = {(float)Pp->block_pos0[b][0], (float)Pp->block_pos0[b][1], (float)Pp->block_pos0[b][2]};
      for (int a = 0; a < 2; a++) p3[Pp->block_axis[a]] = planar_origin_coord(Pp->block_pos0[b][Pp->block_axis[a]], st_q(S, n, NV, 3 + a + 2 * b, env));
      o[3 + 3 * b] = p3[0]; o[4 + 3 * b] = p3[1]; o[5 + 3 * b] = p3[2];
    }
    if (ostride != NOBS)  // top-down view: block x, y parked for mzk_view_fill, time entry behind the view
      for (int b = 0; b < NB; b++) {
        float p3[3] = {(float)Pp->block_pos0[b][0], (float)Pp->block_pos0[b][1], (float)Pp->block_pos0[b][2]};
        for (int a = 0; a < 2; a++) p3[Pp->block_axis[a]] = planar_origin_coord(Pp->block_pos0[b][Pp->block_axis[a]], st_q(S, n, NV, 3 + a + 2 * b, env));
        o[NOBS - 1 + 2 * b] = p3[0]; o[NOBS + 2 * b] = p3[1];
      }
    o[ostride - 1] = (float)st_t(S, NV, env) * 0.001f;
  }
}

template <int KQ>
__global__ void point_set_state_kernel(int n, PointState S, const float* qpos, const float* qvel, const int* t) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  for (int k = 0; k < KQ; k++) {
    if (qpos) st_q(S, n, KQ, k, env) = qpos[(size_t)env * KQ + k];
    if (qvel) st_v(S, n, KQ, k, env) = qvel[(size_t)env * KQ + k];
  }
  if (t) st_t(S, KQ, env) = t[env];
  if (KQ == 3 && S.rec > PT_WARM_OFF && (qpos || qvel)) for (int k = 0; k < 3; k++) S.qv[(size_t)env * S.rec + PT_WARM_OFF + k] = 0.f;  // a new state: no guess
}
template <int KQ>
__global__ void point_get_state_kernel(int n, PointState S, float* qpos, float* qvel, float* warm, int* t) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  for (int k = 0; k < KQ; k++) {
    if (qpos) qpos[(size_t)env * KQ + k] = st_q(S, n, KQ, k, env);
    if (qvel) qvel[(size_t)env * KQ + k] = st_v(S, n, KQ, k, env);
    if (warm) warm[(size_t)env * KQ + k] = (KQ == 3 && S.rec > PT_WARM_OFF) ? S.qv[(size_t)env * S.rec + PT_WARM_OFF + k] : 0.f;
  }
  if (t) t[env] = st_t(S, KQ, env);
}

// ------------------------------------------------------------------ Swimmer / Reacher kernels (NL links, one movable block with BD
// slide dofs: 0 none, 2 or 3; SoA: q0..q[NV-1] v0..v[NV-1] | t | episode with NV = NL + 2 + BD)
//
// Observation / reset layout: swimmer_dyn.h (swimmer_obs_row).  Reset (swimmer.py:56-69): U(-0.1, 0.1) noise on ALL nq
// coordinates and ALL nv velocities, the block's included.
// one observation row o[NO] (swimmer_obs_row) into a row of `ostride` floats: NO, or NO + MZ_VIEW_DIM with the time entry behind
// the view and the movable block's x, y parked for mzk_view_fill (mz_device.h obs_slot)
template <int NL, int BD>
__device__ __forceinline__ void swimmer_store_row(const SwimmerDev& P, const float* qf, const float* o, int NO, int ostride, float* row) {
  for (int k = 0; k < NO; k++) row[obs_slot(k, NO, ostride)] = o[k];
  if constexpr (BD > 0) {
    if (ostride != NO) {
      double p[3] = {P.block_pos0[0][0], P.block_pos0[0][1], P.block_pos0[0][2]};
      for (int a = 0; a < BD; a++) p[P.bd_axis[a]] += (double)qf[NL + 2 + a];
      row[NO - 1] = (float)p[0];
      row[NO] = (float)p[1];
    }
  }
}

// lane-group context of the chain kernels (swimmer_dyn.h): G = 4 lanes per env for chains of up to four links, 8 beyond
template <int G>
struct SwimmerCtx {
  static constexpr int nlanes = G;
  int l;
  __device__ __forceinline__ int lane0() const { return l; }
  __device__ __forceinline__ double gsum(double x) const { return DevCtx<G>{l}.gsum(x); }
  // value of lane k of this lane's group (ds_bpermute on the two halves of the double; a handful per forward evaluation)
  __device__ __forceinline__ double from_lane(double x, int k) const { return __shfl(x, (int)(threadIdx.x & 63u) - l + k, 64); }
};

template <int NL, int NB, int G>
__global__ __launch_bounds__(256) void swimmer_step_kernel(const SwimmerDev* __restrict__ Pp, int n, PointState S,
                                                            const float* __restrict__ actions, float* __restrict__ obs,
                                                            float* __restrict__ reward, uint8_t* __restrict__ done,
                                                            int* __restrict__ goal_idx, float* __restrict__ info,
                                                            int* __restrict__ status, int auto_reset, uint64_t seed, uint64_t env0,
                                                            float* __restrict__ final_obs, int ostride) {
  // G adjacent lanes advance one env (lane b owns link b of the chain); everything outside the forward dynamics' per-link part
  // is computed redundantly by the G lanes, the group's first lane stores
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int env = gid / G;
  const SwimmerCtx<G> cx{(int)(threadIdx.x % G)};
  const bool live = env < n && cx.l == 0;
  if (env >= n) env = n - 1;  // surplus groups shadow the last env (no stores): every lane reaches the group sums
  constexpr int NR = NL + 2, NV = NR + NB, NH = NL - 1;  // NB: slide dofs of the movable block
  const SwimmerDev& P = *Pp;
  const int nb3 = (NB && P.observe_blocks) ? 3 : 0, NO = 2 * NV + 1 + nb3;
  float qf[NV], vf[NV], af[NH > 0 ? NH : 1], o[2 * NV + 4];
  double inner, inf4[4];
  for (int k = 0; k < NV; k++) { qf[k] = S.qv[(size_t)k * n + env]; vf[k] = S.qv[(size_t)(NV + k) * n + env]; }
  for (int k = 0; k < NH; k++) af[k] = actions[(size_t)env * NH + k];
  int t_new;
  int st = swimmer_maze_step<NL, NB>(P, qf, vf, af, S.t[env], o, &inner, inf4, &t_new, cx);
  if (!live) return;
  float outer; int tm, gi;
  task_eval_dev(P.task, o, &outer, &tm, &gi, env);
  uint8_t d = (uint8_t)((tm ? 1 : 0) | (t_new >= P.task.max_steps ? 2 : 0));
  const bool rst = auto_reset && d;
  if (!rst || final_obs) swimmer_store_row<NL, NB>(P, qf, o, NO, ostride, ((rst && final_obs) ? final_obs : obs) + (size_t)env * ostride);
  reward[env] = (float)(P.task.inner_scale * inner) + outer;
  done[env] = d;
  if (goal_idx) goal_idx[env] = gi;
  if (info) for (int k = 0; k < 4; k++) info[(size_t)env * 4 + k] = (float)inf4[k];
  if (st) atomicOr(&status[env], st);
  uint32_t ep = S.ep[env];
  if (rst) {
    ep += 1; t_new = 0;
    const uint64_t es = episode_seed(seed, ep);
    for (int k = 0; k < NV; k++) {
      qf[k] = reset_qpos(k < NR ? (float)P.qpos0[k] : 0.f, es, env0 + (uint64_t)env, k);
      vf[k] = reset_qvel(P.reset_kind, NV, es, env0 + (uint64_t)env, k);
    }
    swimmer_obs_row<NL, NB>(P, qf, vf, 0, o);
    swimmer_store_row<NL, NB>(P, qf, o, NO, ostride, obs + (size_t)env * ostride);
  }
  for (int k = 0; k < NV; k++) {
    S.qv[(size_t)k * n + env] = qf[k];
    S.qv[(size_t)(NV + k) * n + env] = vf[k];
  }
  S.t[env] = t_new;
  S.ep[env] = ep;
}

// `nsteps` successive swimmer_step_kernel launches in one (mz_rollout; arguments as planar_rollout_kernel): the fp32 state stays in
// registers.  A separate launch hands every lane of a group the state its first lane stored, so after each step the group takes its
// first lane's state (and the episode verdict that follows from it) before it goes on.
// EXT: as in planar_rollout_kernel, through swimmer_store_row (rows are NO floats apart).
template <int NL, int NB, int G, bool EXT = false>
__global__ __launch_bounds__(256) void swimmer_rollout_kernel(const SwimmerDev* __restrict__ Pp, int n, PointState S, int nsteps,
                                                               const float* __restrict__ actions, long astride, float* __restrict__ obs,
                                                               int last_obs_step, float* __restrict__ reward, uint8_t* __restrict__ done,
                                                               int* __restrict__ goal_idx, float* __restrict__ info, float* __restrict__ obs_seq,
                                                               int* __restrict__ status, int auto_reset, uint64_t seed, uint64_t env0,
                                                               float* __restrict__ final_obs, float* __restrict__ next_obs_seq) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int env = gid / G;
  const SwimmerCtx<G> cx{(int)(threadIdx.x % G)};
  const bool live = env < n && cx.l == 0;
  if (env >= n) env = n - 1;  // surplus groups shadow the last env (no stores)
  constexpr int NR = NL + 2, NV = NR + NB, NH = NL - 1;
  const SwimmerDev& P = *Pp;
  const int nb3 = (NB && P.observe_blocks) ? 3 : 0, NO = 2 * NV + 1 + nb3;
  float qf[NV], vf[NV], af[NH > 0 ? NH : 1], o[2 * NV + 4];
  double inner, inf4[4];
  for (int k = 0; k < NV; k++) { qf[k] = S.qv[(size_t)k * n + env]; vf[k] = S.qv[(size_t)(NV + k) * n + env]; }
  int t = S.t[env], stacc = 0;
  uint32_t ep = S.ep[env];
  const int lane0 = (int)(threadIdx.x & 63u) - cx.l;
  for (int step = 0; step < nsteps; step++) {
    const float* act = actions + (size_t)step * astride + (size_t)env * NH;
    for (int k = 0; k < NH; k++) af[k] = act[k];
    int t_new;
    stacc |= swimmer_maze_step<NL, NB>(P, qf, vf, af, t, o, &inner, inf4, &t_new, cx);
    for (int k = 0; k < NV; k++) { qf[k] = __shfl(qf[k], lane0, 64); vf[k] = __shfl(vf[k], lane0, 64); }
    swimmer_obs_row<NL, NB>(P, qf, vf, t_new, o);
    float outer; int tm, gi;
    task_eval_dev(P.task, o, &outer, &tm, &gi, env);
    const uint8_t d = (uint8_t)((tm ? 1 : 0) | (t_new >= P.task.max_steps ? 2 : 0));
    const bool rst = auto_reset && d;
    const size_t row = (size_t)step * n + env;
    float* oseq = obs_seq ? obs_seq + row * NO : nullptr;
    float* olast = step == last_obs_step ? obs + (size_t)env * NO : nullptr;
    if (live) {
      if constexpr (EXT) {  // the row this step produced, before any reset
        if (next_obs_seq) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, next_obs_seq + row * NO);
      }
      if (rst) {
        if (final_obs) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, final_obs + (size_t)env * NO);
      } else {
        if (oseq) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, oseq);
        if (olast) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, olast);
      }
      reward[row] = (float)(P.task.inner_scale * inner) + outer;
      done[row] = d;
      if (goal_idx) goal_idx[row] = gi;
      if (info) for (int k = 0; k < 4; k++) info[row * 4 + k] = (float)inf4[k];
    }
    if (rst) {
      ep += 1; t_new = 0;
      const uint64_t es = episode_seed(seed, ep);
      for (int k = 0; k < NV; k++) {
        qf[k] = reset_qpos(k < NR ? (float)P.qpos0[k] : 0.f, es, env0 + (uint64_t)env, k);
        vf[k] = reset_qvel(P.reset_kind, NV, es, env0 + (uint64_t)env, k);
      }
      if (live && (oseq || olast)) {
        swimmer_obs_row<NL, NB>(P, qf, vf, 0, o);
        if (oseq) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, oseq);
        if (olast) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, olast);
      }
    }
    t = t_new;
  }
  if (!live) return;
  for (int k = 0; k < NV; k++) {
    S.qv[(size_t)k * n + env] = qf[k];
    S.qv[(size_t)(NV + k) * n + env] = vf[k];
  }
  S.t[env] = t;
  S.ep[env] = ep;
  if (stacc) atomicOr(&status[env], stacc);
}

// swimmer_rollout_kernel with the actions computed on chip (mz_rollout_policy; see planar_policy_rollout_kernel).  The observation
// row lives in registers, redundantly in every lane of the group; the group's first lane puts it into LDS (px), the G lanes split the
// hidden units (phid) and the outputs (pact) over themselves and every lane reads the NH actions back.  Surplus groups shadow the
// last env through every hand-off and shuffle and store nothing.  SMP: as in planar_policy_rollout_kernel.
// CRT: as in planar_policy_rollout_kernel, on the rows in px — after every step the group's first lane puts the row the step produced
// there (the fp32 row swimmer_store_row writes to final_obs when the env is about to reset: rows are NO floats apart here, so both
// are o[0 .. NO - 1]), the group values it, and after a reset the new episode's first row follows and is valued once more.
// DEEP: as in planar_policy_rollout_kernel; the second hidden row takes the block's LDS from 20 KB to 36 KB.
// NRM: as in planar_policy_rollout_kernel.  Here the raw row lives in registers and px is what the networks read and nothing else
// reads, so px IS the staged row: wherever a lane puts raw elements there it puts mzp_norm_elem of them (px_elem), at the places px
// was written before, under the hand-offs it had before.  Stores, the task predicate and info go on reading the registers.
// EXT: as in planar_policy_rollout_kernel.
template <int NL, int NB, int G, bool SMP = false, bool CRT = false, bool DEEP = false, bool NRM = false, bool EXT = false>
__global__ __launch_bounds__(256) void swimmer_policy_rollout_kernel(const SwimmerDev* __restrict__ Pp, int n, PointState S, int nsteps,
                                                                      const float* __restrict__ params, long pstride, int hidden, int squash,
                                                                      float action_scale, float* __restrict__ obs, float* __restrict__ reward,
                                                                      uint8_t* __restrict__ done, int* __restrict__ goal_idx, float* __restrict__ info,
                                                                      float* __restrict__ obs_seq, float* __restrict__ actions_seq, int* __restrict__ status,
                                                                      int auto_reset, uint64_t seed, uint64_t env0, float* __restrict__ final_obs,
                                                                      PolicyNoise ns, PolicyCritic cr, PolicyShapes sh, mzp_norm nm,
                                                                      float* __restrict__ next_obs_seq) {
  static_assert(!NRM || DEEP, "the normalised row is staged in the DEEP instantiations only");
  constexpr int NR = NL + 2, NV = NR + NB, NH = NL - 1, NOMAX = 2 * NV + 4, GPB = 256 / G;
  __shared__ float px[GPB][NOMAX];
  __shared__ float phid[GPB][DEEP ? 2 : 1][MZ_POLICY_MAX_HIDDEN];
  __shared__ float pact[GPB][NH > 0 ? NH : 1];
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int env = gid / G;
  const int grp = (int)threadIdx.x / G;
  const SwimmerCtx<G> cx{(int)(threadIdx.x % G)};
  const bool lead = cx.l == 0, live = env < n && lead;
  if (env >= n) env = n - 1;  // surplus groups shadow the last env (no stores)
  const SwimmerDev& P = *Pp;
  const int nb3 = (NB && P.observe_blocks) ? 3 : 0, NO = 2 * NV + 1 + nb3;
  float qf[NV], vf[NV], af[NH > 0 ? NH : 1], o[NOMAX];
  double inner, inf4[4];
  const float* par = params + (size_t)env * pstride;
  float* x = px[grp];
  auto px_elem = [&](float v, int i) -> float {  // what px holds for the raw element v of column i
    if constexpr (NRM) return mzp_norm_elem(v, nm.mean[i], nm.inv_std[i], nm.clip);
    else return v;
  };
  for (int k = 0; k < NV; k++) { qf[k] = S.qv[(size_t)k * n + env]; vf[k] = S.qv[(size_t)(NV + k) * n + env]; }
  for (int i = cx.l; i < NO; i += G) x[i] = px_elem(obs[(size_t)env * NO + i], i);  // the observation the policy acts on first
  int t = S.t[env], stacc = 0;
  uint32_t ep = S.ep[env];
  const int lane0 = (int)(threadIdx.x & 63u) - cx.l;
  const float* vpar = nullptr;
  float vcur = 0.0f;  // the group's first lane: V(the row in x)
  auto value_of_row = [&]() -> float {  // every lane of the group; phid must be free (mzp_group_value)
    if constexpr (DEEP) return mzp_group_net_value(cx.l, G, vpar, NO, sh.critic, x, phid[grp][0], phid[grp][DEEP ? 1 : 0]);
    else return mzp_group_value(cx.l, G, vpar, NO, cr.hidden, x, phid[grp][0]);
  };
  if constexpr (CRT) {
    vpar = cr.params + (size_t)env * cr.stride;
    mzp_wave_sync();  // the row in x is complete
    vcur = value_of_row();
  }
  for (int step = 0; step < nsteps; step++) {
    const size_t row = (size_t)step * n + env;
    mzp_wave_sync();  // the row in x is complete (CRT: and the critic is done with phid)
    if constexpr (CRT) { if (live && cr.value_seq) cr.value_seq[row] = vcur; }
    // (as in planar_policy_rollout_kernel; NL <= 4: the five- and six-link kernels need all 512 registers and spill on top of them, and
    // with the branch compiled in <5, 0, 8, SMP, CRT, DEEP, , EXT> left its defining loop WITHOUT a head — tests/test_gpu_planar_ladder.py —
    // so they compile their source as it was and rollout_run, mazestep.hip, runs the loop for a head plan on such a chain)
    bool head = false;
    if constexpr (SMP && DEEP && EXT && NL <= 4) head = ns.head != 0;
    if (head) {
      if constexpr (SMP && DEEP && EXT && NL <= 4)
        planar_head_act(cx.l, G, par, NO, NH, sh.actor, squash, action_scale, ns.hd, mzp_noise_key(ns.seed, ns.step + (uint64_t)step),
                        env0 + (uint64_t)env, x, phid[grp][0], phid[grp][1], pact[grp], live && ns.logp_seq ? ns.logp_seq + row : nullptr);
    } else if constexpr (DEEP)
      mzp_group_net_act(cx.l, G, par, NO, NH, sh.actor, squash, action_scale, SMP, SMP ? mzp_noise_key(ns.seed, ns.step + (uint64_t)step) : 0,
                        env0 + (uint64_t)env, x, phid[grp][0], phid[grp][DEEP ? 1 : 0], pact[grp], true,
                        SMP && live && ns.logp_seq ? ns.logp_seq + row : nullptr, EXT ? ns.mode : MZ_NOISE_PRE_SQUASH);
    else if constexpr (SMP)
      mzp_group_sample(cx.l, G, par, NO, NH, hidden, squash, action_scale, mzp_noise_key(ns.seed, ns.step + (uint64_t)step), env0 + (uint64_t)env, x,
                       phid[grp][0], pact[grp], true, live && ns.logp_seq ? ns.logp_seq + row : nullptr, EXT ? ns.mode : MZ_NOISE_PRE_SQUASH);
    else
      mzp_group_eval(cx.l, G, par, NO, NH, hidden, squash, action_scale, x, phid[grp][0], pact[grp], true);
    mzp_wave_sync();
    for (int k = 0; k < NH; k++) af[k] = pact[grp][k];
    if (live && actions_seq) for (int k = 0; k < NH; k++) actions_seq[row * NH + k] = af[k];
    int t_new;
    stacc |= swimmer_maze_step<NL, NB>(P, qf, vf, af, t, o, &inner, inf4, &t_new, cx);
    for (int k = 0; k < NV; k++) { qf[k] = __shfl(qf[k], lane0, 64); vf[k] = __shfl(vf[k], lane0, 64); }
    swimmer_obs_row<NL, NB>(P, qf, vf, t_new, o);
    float outer; int tm, gi;
    task_eval_dev(P.task, o, &outer, &tm, &gi, env);
    const uint8_t d = (uint8_t)((tm ? 1 : 0) | (t_new >= P.task.max_steps ? 2 : 0));
    const bool rst = auto_reset && d;
    float* oseq = obs_seq ? obs_seq + row * NO : nullptr;
    float* olast = step == nsteps - 1 ? obs + (size_t)env * NO : nullptr;
    if (live) {
      if constexpr (EXT) {  // the raw row this step produced, before any reset
        if (next_obs_seq) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, next_obs_seq + row * NO);
      }
      if (rst) {
        if (final_obs) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, final_obs + (size_t)env * NO);
      } else {
        if (oseq) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, oseq);
        if (olast) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, olast);
      }
      reward[row] = (float)(P.task.inner_scale * inner) + outer;
      done[row] = d;
      if (goal_idx) goal_idx[row] = gi;
      if (info) for (int k = 0; k < 4; k++) info[row * 4 + k] = (float)inf4[k];
    }
    if constexpr (CRT) {  // V(the row this step produced), before a reset replaces it; x and phid were handed over with the actions
      if (lead) {
#pragma unroll
        for (int k = 0; k < NOMAX; k++) if (k < NO) x[k] = px_elem(o[k], k);
      }
      mzp_wave_sync();
      vcur = value_of_row();
      if (live && cr.next_value_seq) cr.next_value_seq[row] = vcur;
    }
    if (rst) {
      ep += 1; t_new = 0;
      const uint64_t es = episode_seed(seed, ep);
      for (int k = 0; k < NV; k++) {
        qf[k] = reset_qpos(k < NR ? (float)P.qpos0[k] : 0.f, es, env0 + (uint64_t)env, k);
        vf[k] = reset_qvel(P.reset_kind, NV, es, env0 + (uint64_t)env, k);
      }
      swimmer_obs_row<NL, NB>(P, qf, vf, 0, o);  // the new episode's first row: what the policy acts on next
      if (live) {
        if (oseq) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, oseq);
        if (olast) swimmer_store_row<NL, NB>(P, qf, o, NO, NO, olast);
      }
    }
    t = t_new;
    if constexpr (CRT) {
      if (rst) {  // (x already holds the row where the env goes on)
        mzp_wave_sync();  // the terminal row and its hidden units have been read
        if (lead) {
#pragma unroll
          for (int k = 0; k < NOMAX; k++) if (k < NO) x[k] = px_elem(o[k], k);
        }
        mzp_wave_sync();
        vcur = value_of_row();
      }
    } else {
      if (lead) {
#pragma unroll
        for (int k = 0; k < NOMAX; k++) if (k < NO) x[k] = px_elem(o[k], k);
      }
    }
  }
  if (!live) return;
  for (int k = 0; k < NV; k++) {
    S.qv[(size_t)k * n + env] = qf[k];
    S.qv[(size_t)(NV + k) * n + env] = vf[k];
  }
  S.t[env] = t;
  S.ep[env] = ep;
  if (stacc) atomicOr(&status[env], stacc);
}

template <int NL, int NB>
__global__ void swimmer_reset_kernel(const SwimmerDev* Pp, int n, PointState S, const uint8_t* mask, uint64_t seed, uint64_t env0, float* obs,
                                     int ostride) {
  constexpr int NR = NL + 2, NV = NR + NB;
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  if (!mask || mask[env]) {
    for (int k = 0; k < NV; k++) {
      S.qv[(size_t)k * n + env] = reset_qpos(k < NR ? (float)Pp->qpos0[k] : 0.f, seed, env0 + (uint64_t)env, k);
      S.qv[(size_t)(NV + k) * n + env] = reset_qvel(Pp->reset_kind, NV, seed, env0 + (uint64_t)env, k);
    }
    S.t[env] = 0;
    S.ep[env] = 0;
  }
  if (obs) {
    const int nb3 = (NB && Pp->observe_blocks) ? 3 : 0, NO = 2 * NV + 1 + nb3;
    float qf[NV], vf[NV], o[2 * NV + 4];
    for (int k = 0; k < NV; k++) { qf[k] = S.qv[(size_t)k * n + env]; vf[k] = S.qv[(size_t)(NV + k) * n + env]; }
    swimmer_obs_row<NL, NB>(*Pp, qf, vf, S.t[env], o);
    swimmer_store_row<NL, NB>(*Pp, qf, o, NO, ostride, obs + (size_t)env * ostride);
  }
}

// ------------------------------------------------------------------ top-down view (every robot; mz_view.h)
// One thread per env: fills the MZ_VIEW_DIM view entries of the env's observation row — and of its final_obs row when the env
// just finished under auto-reset — from the row's own torso position and the block positions the step / reset kernel parked.
__global__ void view_fill_kernel(ViewDev V, int n, int ostride, int view_off, float* __restrict__ obs, float* __restrict__ final_obs,
                                 const uint8_t* __restrict__ done) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  mzv_fill_row(V, obs + (size_t)env * ostride, view_off);
  if (final_obs && done && done[env]) mzv_fill_row(V, final_obs + (size_t)env * ostride, view_off);
}

#ifdef MZ_ISA_POINT  // developer aid (tools/isa_point.sh): the bare Point's kernel only, for a look at its ISA / register budget
template __global__ void planar_step_kernel<0, 0, 32>(const PointDev*, int, PointState, const float*, float*, float*, uint8_t*, int*, float*, int*, int, uint64_t,
                                                        uint64_t, float*, int);
#else
hipError_t mzk_view_fill(mz_handle* h, hipStream_t st, float* obs, float* final_obs, const uint8_t* done) {
  if (!h->view.on) return hipSuccess;
  hipLaunchKernelGGL(view_fill_kernel, dim3((h->n + 63) / 64), dim3(64), 0, st, h->view, h->n, h->model.obs_dim, h->base_obs - 1, obs, final_obs, done);
  return hipGetLastError();
}

// ------------------------------------------------------------------ parity-test kernels
// MazeTask.reward / termination on rows of observations: the task_eval_dev instance of this translation unit
__global__ void planar_task_eval_kernel(const TaskDev* __restrict__ Tp, int n, int nenv, int obs_dim, const float* __restrict__ obs,
                                        float* __restrict__ reward, uint8_t* __restrict__ done, int* __restrict__ goal_idx) {
  int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  float o6[6];
  for (int k = 0; k < 6; k++) o6[k] = obs[(size_t)row * obs_dim + k];
  float r; int tm, gi;
  task_eval_dev(*Tp, o6, &r, &tm, &gi, row < nenv ? row : -1);  // per-env goals (mz_bind_env_goals): row r is env r
  reward[row] = r;
  done[row] = (uint8_t)(tm ? 1 : 0);
  if (goal_idx) goal_idx[row] = gi;
}

// CollisionDetector.detect + the bounce / give-up rule of MazeEnv.step on rows of float64 (old_xy, new_xy) moves: the
// point_detect / point_bounce instances the Point step kernel runs.  hit: 0 none, 1 bounced, 2 gave up, -1 collinear.
__global__ void point_detect_kernel(const PointDev* __restrict__ Pp, int n, const double* __restrict__ old_xy,
                                    const double* __restrict__ new_xy, int* __restrict__ hit, double* __restrict__ point,
                                    double* __restrict__ final_xy) {
  __shared__ PointDev P;
  for (int i = threadIdx.x; i < (int)(sizeof(PointDev) / 4); i += blockDim.x) ((uint32_t*)&P)[i] = ((const uint32_t*)Pp)[i];
  __syncthreads();
  int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  double o[2] = {old_xy[2 * row], old_xy[2 * row + 1]}, nw[2] = {new_xy[2 * row], new_xy[2 * row + 1]}, fin[2], pt[2];
  int r = point_bounce(P, o, nw, fin, pt);
  hit[row] = r;
  if (point) { point[2 * row] = pt[0]; point[2 * row + 1] = pt[1]; }
  final_xy[2 * row] = fin[0]; final_xy[2 * row + 1] = fin[1];
}

// ------------------------------------------------------------------ entry points of this translation unit (mz_internal.h)
// floats per env of the Point's env-major state record (q | v | t | episode, padded to 16 bytes); 0 = SoA (the chains)
int mzk_planar_record_width(const mz_handle* h) {
  if (h->robot == MZ_ROBOT_POINT && h->point.nblock == 0 && h->point.nball == 0) return PT_WARM_OFF + 4;  // q[3] v[3] t episode | warm start[3] | pad: 48 B
  return h->robot == MZ_ROBOT_POINT ? (2 * mzk_planar_state_width(h) + 2 + 3) / 4 * 4 : 0;
}
int mzk_planar_state_width(const mz_handle* h) {
  return h->robot == MZ_ROBOT_SWIMMER ? h->swimmer.nlink + 2 + (h->swimmer.nblock ? h->swimmer.nbdof : 0) : 3 + 2 * h->point.nblock + 3 * h->point.nball;
}

// lanes per env by the handle's robot, blocks, batch size and options: the rule the ladders below read
static int planar_lane_rule(const mz_handle* h) {
  if (h->robot == MZ_ROBOT_SWIMMER) return h->swimmer.nlink <= 4 ? 4 : 8;
  if (h->point.nball || h->point.nblock == 1) return 32;
  if (h->point.nblock >= 2) return 64;
  // the bare Point: 16 lanes per env while that still gives every wave a SIMD of its own (up to 4096 envs on a 256-CU device), else 32
  const int lanes = h->lanes_set ? h->lanes : ((h->n + 3) / 4 <= h->simds ? 16 : 32);
  return (lanes == 8 || lanes == 16) ? lanes : 32;
}

// ---- the handle-to-instantiation ladder, once: the step, both rollout kernels and the reset launch what it picks, so a rollout
// cannot run another instantiation than the step it claims to equal.  f gets the template arguments as std::integral_constant's.
template <int V> using ic = std::integral_constant<int, V>;

// Swimmer / Reacher: f(NL, NB, G) — NL links, NB the movable block's degrees of freedom (0: none), G = 4 lanes per env up to four
// links, else 8.  The two rungs with NB = 3 (a block on three slides: a custom MultiFall task) have no handle: mz_create sends such a
// model to the general engine (gen_model_needs_general_engine)
template <class F>
static void swimmer_ladder(const mz_handle* h, F&& f) {
  const int bd = h->swimmer.nblock ? h->swimmer.nbdof : 0;
  if (h->swimmer.nlink == 3) { if (bd == 3) f(ic<3>{}, ic<3>{}, ic<4>{}); else if (bd == 2) f(ic<3>{}, ic<2>{}, ic<4>{}); else f(ic<3>{}, ic<0>{}, ic<4>{}); }
  else if (h->swimmer.nlink == 2) { if (bd == 3) f(ic<2>{}, ic<3>{}, ic<4>{}); else if (bd == 2) f(ic<2>{}, ic<2>{}, ic<4>{}); else f(ic<2>{}, ic<0>{}, ic<4>{}); }
  else if (h->swimmer.nlink == 4) f(ic<4>{}, ic<0>{}, ic<4>{});  // longer chains (user MJCF): no movable blocks
  else if (h->swimmer.nlink == 5) f(ic<5>{}, ic<0>{}, ic<8>{});
  else f(ic<6>{}, ic<0>{}, ic<8>{});
}
// the Swimmer kernels' launch geometry: workgroups of `waves_per_block` waves (option; default 4), G lanes per env
static unsigned swimmer_block(const mz_handle* h) { return 64u * (unsigned)(h->wpb_set ? h->waves_per_block : 4); }
static dim3 swimmer_grid(const mz_handle* h, int G) { return dim3((unsigned)(((size_t)h->n * G + swimmer_block(h) - 1) / swimmer_block(h))); }

// Point: f(NB, NS, G) — NB movable blocks or NS object balls, G lanes per env.
// Lanes per env: 32 for the bare robot — its 18 collision enumerators then share one round, and 4096 envs make two waves per
// SIMD: a wave runs as long as the slowest of its envs (only envs at a wall enumerate, fill and iterate), so two envs per wave
// and a second wave to fill the gaps beat four envs per wave (measured, round 3: 34.8 vs 31.6 M env-steps/s on PointUMaze) —
// 32 / 64 with blocks (bigger contact sets in LDS).
// Round 5: 16 lanes per env by default while that still gives every wave a SIMD of its own (up to 4096 envs on a 256-CU device).
// Round 3 measured the opposite (34.8 against 31.6 M at 32 lanes: two envs per wave and a second wave to fill the gaps); with
// the step in registers (point_bare.h) and the unit-step solver the waves are short and even enough that four envs per wave on
// a SIMD of their own win: PointUMaze 4096 envs 74.3 -> 79.6 M env-steps/s, Point4Rooms 79.6 -> 82.6 M; beyond (8192 envs:
// 108.0 at 32 lanes against 106.3) it stays at 32 (profiles/r05/point_knobs.txt).
template <class F>
static void point_ladder(const mz_handle* h, F&& f) {
  if (h->point.nball) f(ic<0>{}, ic<1>{}, ic<32>{});
  else switch (h->point.nblock) {
    case 0: {
      const int lanes = planar_lane_rule(h);
      if (lanes == 8) f(ic<0>{}, ic<0>{}, ic<8>{});
      else if (lanes == 16) f(ic<0>{}, ic<0>{}, ic<16>{});
      else f(ic<0>{}, ic<0>{}, ic<32>{});
      break;
    }
    case 1: f(ic<1>{}, ic<0>{}, ic<32>{}); break;
    case 2: f(ic<2>{}, ic<0>{}, ic<64>{}); break;
    default: f(ic<3>{}, ic<0>{}, ic<64>{}); break;
  }
}
// the Point kernels' launch geometry: one wave per workgroup, 64 / G envs in it
static dim3 point_grid(const mz_handle* h, int G) { return dim3((h->n + 64 / G - 1) / (64 / G)); }

// lanes per env of the next step launch, for mz_get_info: the G of the instantiation the ladder picks — not the rule's value, so a
// ladder that sent a lane count to another rung shows in launch_info() (tests/test_gpu_planar_ladder.py reads the rung from it)
int mzk_planar_lanes(const mz_handle* h) {
  int g = 0;
  if (h->robot == MZ_ROBOT_SWIMMER) swimmer_ladder(h, [&](auto, auto, auto G) { g = G; });
  else point_ladder(h, [&](auto, auto, auto G) { g = G; });
  return g;
}

hipError_t mzk_planar_step(mz_handle* h, hipStream_t st, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                           int* goal_idx_dev, float* info_dev) {
  PointState S{h->state, h->pt_t, h->pt_ep, h->pt_rec};
  if (h->robot == MZ_ROBOT_SWIMMER)
    swimmer_ladder(h, [&](auto NL, auto NB, auto G) {
      hipLaunchKernelGGL((swimmer_step_kernel<NL, NB, G>), swimmer_grid(h, G), dim3(swimmer_block(h)), 0, st, h->swimmer_dev, h->n, S, actions_dev, obs_dev,
                         reward_dev, done_dev, goal_idx_dev, info_dev, h->status, h->auto_reset, h->seed, h->env0, h->final_obs, h->model.obs_dim);
    });
  else
    point_ladder(h, [&](auto NB, auto NS, auto G) {
      hipLaunchKernelGGL((planar_step_kernel<NB, NS, G>), point_grid(h, G), dim3(64), 0, st, h->point_dev, h->n, S, actions_dev, obs_dev, reward_dev,
                         done_dev, goal_idx_dev, info_dev, h->status, h->auto_reset, h->seed, h->env0, h->final_obs, h->model.obs_dim);
    });
  return hipGetLastError();
}

// mz_rollout: does this handle take the fused kernels below?  (A top-down view is filled by a kernel of its own after every step,
// so such handles — like the Ant and the general engine — step launch by launch inside mz_rollout.)
int mzk_planar_rollout_fused(const mz_handle* h) {
  return (h->robot == MZ_ROBOT_POINT || h->robot == MZ_ROBOT_SWIMMER) && !h->view.on;
}

// f(std::bool_constant's) for run-time flags: the run-time to template switch of the rollout kernels' flags, once
template <class F>
static hipError_t flag_switch(F&& f) { return f(); }
template <class F, class... Rest>
static hipError_t flag_switch(F&& f, bool flag, Rest... rest) {
  auto with = [&](auto B) { return flag_switch([&](auto... r) { return f(B, r...); }, rest...); };
  return flag ? with(std::true_type{}) : with(std::false_type{});
}

// Steps k = 0 .. n_steps - 1 of a plan in launches of at most MZ_ROLLOUT_CHUNK steps, each with the launch geometry and the
// instantiation of the step kernel it stands for, every array advanced to the launch's first step; arrays as in mz_rollout_io.
// POL false: the open-loop kernels on the plan's action tensor (EXT alone is read); the launch that holds the rollout's last step writes
// obs_dev.  POL true: the policy kernels.  Every launch writes obs_dev at its last step, and the next one reads its first observation
// there — and continues at noise_step + the steps done so far.  What the kernels get of the plan's networks:
//   SMP   ns: the call's seed, the launch's first noise step, its logp rows and the noise mode (else zeros);
//   CRT   cr: the critic's parameters and the launch's value_seq / next_value_seq rows (else zeros);
//   DEEP  sh: both networks' shapes; `hidden` and cr.hidden are 0 — else sh is zeros and the two carry the one hidden width each;
//   NRM   (DEEP with a normaliser bound) nm: the handle's normaliser;
//   EXT   nseq: the launch's next_obs_seq rows (nullable), and ns.mode is honoured — with SMP and DEEP also ns.head / ns.hd, the plan's head.
template <bool POL, bool SMP, bool CRT, bool DEEP, bool NRM, bool EXT>
static hipError_t rollout_launches(mz_handle* h, hipStream_t st, const RolloutPlan& p) {
  PointState S{h->state, h->pt_t, h->pt_ep, h->pt_rec};
  const size_t n = (size_t)h->n, od = (size_t)h->model.obs_dim, nu = (size_t)h->model.nu;
  const mzp_norm nm{h->nrm_mean, h->nrm_inv_std, h->nrm_clip};
  const mz_net *A = p.actor, *C = p.critic;
  auto shape = [](const mz_net* net) { return mzp_shape{net->n_hidden, net->hidden[0], net->hidden[1], net->activation}; };
  const PolicyShapes sh{DEEP ? shape(A) : mzp_shape{0, 0, 0, 0}, DEEP && CRT ? shape(C) : mzp_shape{0, 0, 0, 0}};
  const int hidden = POL && !DEEP ? A->hidden[0] : 0, squash = POL ? A->squash : 0;
  const float action_scale = POL ? (float)A->action_scale : 0.0f;
  const float* params = POL ? A->params_dev : nullptr;
  const long pstride = POL ? (long)A->env_stride : 0, astride = p.action_step_stride;
  for (int k0 = 0; k0 < p.n_steps; k0 += MZ_ROLLOUT_CHUNK) {
    const int ks = p.n_steps - k0 < MZ_ROLLOUT_CHUNK ? p.n_steps - k0 : MZ_ROLLOUT_CHUNK;
    float* rew = p.reward_dev + k0 * n;
    uint8_t* dn = p.done_dev + k0 * n;
    int* gi = p.goal_idx_dev ? p.goal_idx_dev + k0 * n : nullptr;
    float* inf = p.info_dev ? p.info_dev + k0 * n * 4 : nullptr;
    float* oseq = p.obs_seq_dev ? p.obs_seq_dev + k0 * n * od : nullptr;
    float* nseq = p.next_obs_seq_dev ? p.next_obs_seq_dev + k0 * n * od : nullptr;  // this launch writes rows k0 .. k0 + ks - 1
    if constexpr (!POL) {
      const int last = k0 + ks == p.n_steps ? ks - 1 : -1;
      const float* act = p.actions_dev + (size_t)k0 * astride;
      if (h->robot == MZ_ROBOT_SWIMMER)
        swimmer_ladder(h, [&](auto NL, auto NB, auto G) {
          hipLaunchKernelGGL((swimmer_rollout_kernel<NL, NB, G, EXT>), swimmer_grid(h, G), dim3(swimmer_block(h)), 0, st, h->swimmer_dev, h->n, S, ks, act,
                             astride, p.obs_dev, last, rew, dn, gi, inf, oseq, h->status, h->auto_reset, h->seed, h->env0, h->final_obs, nseq);
        });
      else
        point_ladder(h, [&](auto NB, auto NS, auto G) {
          hipLaunchKernelGGL((planar_rollout_kernel<NB, NS, G, EXT>), point_grid(h, G), dim3(64), 0, st, h->point_dev, h->n, S, ks, act, astride, p.obs_dev,
                             last, rew, dn, gi, inf, oseq, h->status, h->auto_reset, h->seed, h->env0, h->final_obs, nseq);
        });
    } else {
      float* aseq = p.actions_seq_dev ? p.actions_seq_dev + k0 * n * nu : nullptr;
      const mzp_head hd = p.head ? mzp_head{p.head->log_std_min, p.head->log_std_max, p.head->logp_squashed, p.head_logA} : mzp_head{0.0f, 0.0f, 0, 0.0f};
      const PolicyNoise ns = SMP ? PolicyNoise{p.noise_seed, p.noise_step + (uint64_t)k0, p.logp_seq_dev ? p.logp_seq_dev + k0 * n : nullptr, p.noise_mode,
                                               p.head ? 1 : 0, hd}
                                 : PolicyNoise{0, 0, nullptr, 0, 0, hd};
      const PolicyCritic cr = CRT ? PolicyCritic{C->params_dev, (long)C->env_stride, DEEP ? 0 : C->hidden[0],
                                                 p.value_seq_dev ? p.value_seq_dev + k0 * n : nullptr,
                                                 p.next_value_seq_dev ? p.next_value_seq_dev + k0 * n : nullptr}
                                  : PolicyCritic{nullptr, 0, 0, nullptr, nullptr};
      if (h->robot == MZ_ROBOT_SWIMMER)
        swimmer_ladder(h, [&](auto NL, auto NB, auto G) {
          hipLaunchKernelGGL((swimmer_policy_rollout_kernel<NL, NB, G, SMP, CRT, DEEP, NRM, EXT>), swimmer_grid(h, G), dim3(swimmer_block(h)), 0, st,
                             h->swimmer_dev, h->n, S, ks, params, pstride, hidden, squash, action_scale, p.obs_dev, rew, dn, gi, inf, oseq, aseq, h->status,
                             h->auto_reset, h->seed, h->env0, h->final_obs, ns, cr, sh, nm, nseq);
        });
      else
        point_ladder(h, [&](auto NB, auto NS, auto G) {
          hipLaunchKernelGGL((planar_policy_rollout_kernel<NB, NS, G, SMP, CRT, DEEP, NRM, EXT>), point_grid(h, G), dim3(64), 0, st, h->point_dev, h->n, S, ks,
                             params, pstride, hidden, squash, action_scale, p.obs_dev, rew, dn, gi, inf, oseq, aseq, h->status, h->auto_reset, h->seed,
                             h->env0, h->final_obs, ns, cr, sh, nm, nseq);
        });
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t mzk_planar_rollout(mz_handle* h, hipStream_t st, const RolloutPlan& p) {
  const RolloutKernels kn = mzk_rollout_kernels(h, p);
  if (!p.actor) return flag_switch([&](auto EXT) { return rollout_launches<false, false, false, false, false, EXT>(h, st, p); }, kn.ext);
  return flag_switch(
      [&](auto SMP, auto CRT, auto DEEP, auto NRM, auto EXT) {
        if constexpr (NRM && !DEEP) return hipErrorInvalidValue;  // not instantiated: a bound normaliser makes every call DEEP
        else return rollout_launches<true, SMP, CRT, DEEP, NRM, EXT>(h, st, p);
      },
      p.sample != 0, p.critic != nullptr, kn.deep, kn.nrm, kn.ext);
}

hipError_t mzk_planar_reset(mz_handle* h, hipStream_t st, const uint8_t* mask_dev, uint64_t seed, float* obs_dev) {
  PointState S{h->state, h->pt_t, h->pt_ep, h->pt_rec};
  const int nb = (h->n + 255) / 256;  // one lane per env: the ladder's lane count is not read
  if (h->robot == MZ_ROBOT_SWIMMER)
    swimmer_ladder(h, [&](auto NL, auto NB, auto) {
      hipLaunchKernelGGL((swimmer_reset_kernel<NL, NB>), dim3(nb), dim3(256), 0, st, h->swimmer_dev, h->n, S, mask_dev, seed, h->env0, obs_dev, h->model.obs_dim);
    });
  else
    point_ladder(h, [&](auto NB, auto NS, auto) {
      hipLaunchKernelGGL((point_reset_kernel<NB, NS>), dim3(nb), dim3(256), 0, st, h->point_dev, h->n, S, mask_dev, seed, h->env0, obs_dev, h->model.obs_dim);
    });
  return hipGetLastError();
}

hipError_t mzk_planar_set_state(mz_handle* h, hipStream_t st, const float* qpos_dev, const float* qvel_dev, const int* t_dev) {
  PointState S{h->state, h->pt_t, h->pt_ep, h->pt_rec};
  const dim3 grid((h->n + 255) / 256), blk(256);
  switch (mzk_planar_state_width(h)) {
    case 3: hipLaunchKernelGGL(point_set_state_kernel<3>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
    case 4: hipLaunchKernelGGL(point_set_state_kernel<4>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
    case 5: hipLaunchKernelGGL(point_set_state_kernel<5>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
    case 6: hipLaunchKernelGGL(point_set_state_kernel<6>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
    case 7: hipLaunchKernelGGL(point_set_state_kernel<7>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
    case 8: hipLaunchKernelGGL(point_set_state_kernel<8>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
    default: hipLaunchKernelGGL(point_set_state_kernel<9>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, t_dev); break;
  }
  return hipGetLastError();
}

hipError_t mzk_planar_get_state(mz_handle* h, hipStream_t st, float* qpos_dev, float* qvel_dev, float* warmstart_dev, int* t_dev) {
  PointState S{h->state, h->pt_t, h->pt_ep, h->pt_rec};
  const dim3 grid((h->n + 255) / 256), blk(256);
  switch (mzk_planar_state_width(h)) {
    case 3: hipLaunchKernelGGL(point_get_state_kernel<3>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
    case 4: hipLaunchKernelGGL(point_get_state_kernel<4>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
    case 5: hipLaunchKernelGGL(point_get_state_kernel<5>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
    case 6: hipLaunchKernelGGL(point_get_state_kernel<6>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
    case 7: hipLaunchKernelGGL(point_get_state_kernel<7>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
    case 8: hipLaunchKernelGGL(point_get_state_kernel<8>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
    default: hipLaunchKernelGGL(point_get_state_kernel<9>, grid, blk, 0, st, h->n, S, qpos_dev, qvel_dev, warmstart_dev, t_dev); break;
  }
  return hipGetLastError();
}

hipError_t mzk_planar_task_eval(mz_handle* h, hipStream_t st, int n, const float* obs, float* reward, uint8_t* done, int* goal_idx) {
  const TaskDev* Tp = h->robot == MZ_ROBOT_SWIMMER ? &h->swimmer_dev->task : &h->point_dev->task;
  hipLaunchKernelGGL(planar_task_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, st, Tp, n, h->n, h->model.obs_dim, obs, reward, done, goal_idx);
  return hipGetLastError();
}

hipError_t mzk_point_detect(mz_handle* h, hipStream_t st, int n, const double* old_xy, const double* new_xy, int* hit, double* point,
                            double* final_xy) {
  hipLaunchKernelGGL(point_detect_kernel, dim3((n + 63) / 64), dim3(64), 0, st, h->point_dev, n, old_xy, new_xy, hit, point, final_xy);
  return hipGetLastError();
}
#endif  // MZ_ISA_POINT
