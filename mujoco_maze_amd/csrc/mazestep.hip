// mazestep.hip — the C-ABI of include/mazestep.h: handle life cycle, options, argument checks and the dispatch to the
// kernels of ant_kernels.hip (Ant) and planar_kernels.hip (Point / Swimmer / Reacher).  See mz_internal.h for how the
// library is split into translation units and why they are built with different floating-point flags.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "mz_gae.h"
#include "mz_internal.h"
#include "mz_net_tile.h"
#include "mz_policy.h"
#include "mz_render.h"
#include "mz_returns.h"

__global__ void fetch_clear_status_kernel(int n, int* status, int* out) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  out[env] = status[env];
  status[env] = 0;
}

// packed record [obs (obs_dim) | reward | done] of one step: the generic path (Point / Swimmer / Reacher, and any robot with a
// top-down view, whose rows are completed by mzk_view_fill after the step kernel).  The Ant step kernel writes the record
// itself (ant_kernels.hip epilogue).
__global__ void pack_record_kernel(int n, int obs_dim, const float* __restrict__ obs, const float* __restrict__ reward,
                                   const uint8_t* __restrict__ done, float* __restrict__ record) {
  const int w = obs_dim + 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n * w) return;
  const int env = (int)(idx / w), i = (int)(idx - (size_t)env * w);
  record[idx] = i < obs_dim ? obs[(size_t)env * obs_dim + i] : (i == obs_dim ? reward[env] : (float)done[env]);
}

// next_obs_seq row of one step where the handle steps launch by launch (mz_rollout_ex: the Ant, the general engine, top-down-view
// tasks): out[i][j] = done[i] ? final_obs[i][j] : obs[i][j], one thread per element — the row step k produced before any auto-reset,
// its view entries included (mzk_view_fill has completed both rows).  Runs under auto-reset only; without it the row is a copy.
__global__ __launch_bounds__(256) void next_obs_kernel(int n, int obs_dim, const float* __restrict__ obs, const float* __restrict__ final_obs,
                                                       const uint8_t* __restrict__ done, float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n * obs_dim) return;
  out[idx] = done[idx / obs_dim] ? final_obs[idx] : obs[idx];
}

// The relative transition of a context behind one step of mz_rollout_ctx (mz_policy.h mzp_ctx_next): one thread per (env, d < D),
// ctx[i][d] = (ctx[i][d] + s_old[i][d]) - obs[i][d] where done[i] == 0.  s_old [n][D]: the first D columns of the raw row the actor
// acted on, copied before the step; obs: the rows the step left — for an env that did not finish that IS the row it produced, with or
// without auto-reset, and an env that finished keeps its context.
__global__ __launch_bounds__(256) void ctx_transition_kernel(int n, int cdim, int D, int obs_dim, const float* __restrict__ s_old,
                                                             const float* __restrict__ obs, const uint8_t* __restrict__ done,
                                                             float* __restrict__ ctx) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n * D) return;
  const size_t env = idx / D, d = idx - env * D;
  if (done[env]) return;
  ctx[env * cdim + d] = mzp_ctx_next(ctx[env * cdim + d], s_old[idx], obs[env * obs_dim + d]);
}

// actions[r] = policy(obs[r]) for n rows (mz_policy_act; mz_rollout_policy where it steps launch by launch): the policy of mz_policy.h,
// one group of MZ_POLICY_LANES adjacent lanes per row — lanes l, l + 16, .. own hidden units, lanes 0 .. nu - 1 the outputs.  Engine-
// independent.  params: one policy (pstride = 0) or row r's own at params + r * pstride.  Surplus groups shadow the last row (no stores).
constexpr int MZ_POLICY_LANES = 16;
__global__ __launch_bounds__(256) void policy_act_kernel(int n, int obs_dim, int nu, int hidden, int squash, float action_scale,
                                                         const float* __restrict__ params, long pstride, const float* __restrict__ obs,
                                                         float* __restrict__ actions) {
  __shared__ float hid[256 / MZ_POLICY_LANES][MZ_POLICY_MAX_HIDDEN];
  const int l = (int)threadIdx.x % MZ_POLICY_LANES, grp = (int)threadIdx.x / MZ_POLICY_LANES;
  size_t row = (size_t)blockIdx.x * (256 / MZ_POLICY_LANES) + grp;
  const bool live = row < (size_t)n;
  if (!live) row = (size_t)n - 1;
  mzp_group_eval(l, MZ_POLICY_LANES, params + row * pstride, obs_dim, nu, hidden, squash, action_scale, obs + row * obs_dim, hid[grp],
                 actions + row * nu, live);
}

// policy_act_kernel for a stochastic policy (mz_policy_sample; mz_rollout_policy_sample where it steps launch by launch): the same
// groups, lanes 0 .. nu - 1 own the outputs and their eps, lane 0 the row's log-prob (logp nullable).  key: mzp_noise_key of the
// draw; row r is global env slot env0 + r; mode: MZ_NOISE_* (mz_net_sample; every older entry passes MZ_NOISE_PRE_SQUASH).
__global__ __launch_bounds__(256) void policy_sample_kernel(int n, int obs_dim, int nu, int hidden, int squash, float action_scale,
                                                            const float* __restrict__ params, long pstride, uint64_t key, uint64_t env0,
                                                            const float* __restrict__ obs, float* __restrict__ actions,
                                                            float* __restrict__ logp, int mode) {
  __shared__ float hid[256 / MZ_POLICY_LANES][MZ_POLICY_MAX_HIDDEN];
  const int l = (int)threadIdx.x % MZ_POLICY_LANES, grp = (int)threadIdx.x / MZ_POLICY_LANES;
  size_t row = (size_t)blockIdx.x * (256 / MZ_POLICY_LANES) + grp;
  const bool live = row < (size_t)n;
  if (!live) row = (size_t)n - 1;
  mzp_group_sample(l, MZ_POLICY_LANES, params + row * pstride, obs_dim, nu, hidden, squash, action_scale, key, env0 + row, obs + row * obs_dim,
                   hid[grp], actions + row * nu, live, live && logp ? logp + row : nullptr, mode);
}

// values[r] = V(obs[r]) for n rows (mz_value; mz_rollout_actor_critic where it steps launch by launch): the critic of mz_policy.h on
// the groups of policy_act_kernel — lanes l, l + 16, .. own hidden units, the group's first lane the output.  With `done` (the step
// under auto-reset) row r is taken from final_obs where done[r] != 0: the terminal row, which obs no longer holds.
__global__ __launch_bounds__(256) void value_kernel(int n, int obs_dim, int hidden, const float* __restrict__ vparams, long vstride,
                                                    const float* __restrict__ obs, const float* __restrict__ final_obs,
                                                    const uint8_t* __restrict__ done, float* __restrict__ values) {
  __shared__ float hid[256 / MZ_POLICY_LANES][MZ_POLICY_MAX_HIDDEN];
  const int l = (int)threadIdx.x % MZ_POLICY_LANES, grp = (int)threadIdx.x / MZ_POLICY_LANES;
  size_t row = (size_t)blockIdx.x * (256 / MZ_POLICY_LANES) + grp;
  const bool live = row < (size_t)n;
  if (!live) row = (size_t)n - 1;
  const float* x = (done && done[row] ? final_obs : obs) + row * obs_dim;
  const float v = mzp_group_value(l, MZ_POLICY_LANES, vparams + row * vstride, obs_dim, hidden, x, hid[grp]);
  if (live && l == 0) values[row] = v;
}

// policy_act_kernel (sample == 0: key, env0 and logp are not read) and policy_sample_kernel (sample == 1) for a network of shape s
// (mz_net_act; mz_rollout_net where it steps launch by launch): the same groups, a second LDS row per group for the second hidden
// vector.  Kernels of their own beside the three above, whose code stays what it was.
// NRM (a normaliser bound with mz_bind_obs_norm; every entry, the legacy ones included, then runs these two kernels): the group first
// stages the normalised row of mz_policy.h in a third LDS row — lanes l, l + 16, .. own its elements —, hands it over and evaluates
// the network on it.  obs_dim <= MZ_MAX_OBS + MZ_VIEW_DIM on every handle (mz_create; mz_bind_obs_norm checks it again).  NRM == false
// compiles the source as it was and never reads `nm`.  mode: MZ_NOISE_* of a sampled action.
// A context (mz_context: nm.cdim > 0) rides on the NRM instantiations: the row's nm.cdim context floats are staged behind the
// normalised row — the row has MZ_MAX_CONTEXT floats more for them — and the network runs on obs_dim + nm.cdim inputs; without a
// bound normaliser nm is the identity (ctx_norm below), which returns the raw bits.  nm.cdim == 0 stages and reads what it did.
template <bool NRM = false>
__global__ __launch_bounds__(256) void net_act_kernel(int n, int obs_dim, int nu, mzp_shape s, int squash, float action_scale,
                                                      const float* __restrict__ params, long pstride, int sample, uint64_t key, uint64_t env0,
                                                      const float* __restrict__ obs, float* __restrict__ actions, float* __restrict__ logp,
                                                      mzp_norm nm, int mode) {
  __shared__ float hid[256 / MZ_POLICY_LANES][MZ_NET_MAX_HIDDEN_LAYERS][MZ_POLICY_MAX_HIDDEN];
  const int l = (int)threadIdx.x % MZ_POLICY_LANES, grp = (int)threadIdx.x / MZ_POLICY_LANES;
  size_t row = (size_t)blockIdx.x * (256 / MZ_POLICY_LANES) + grp;
  const bool live = row < (size_t)n;
  if (!live) row = (size_t)n - 1;
  if constexpr (NRM) {
    __shared__ float xn[256 / MZ_POLICY_LANES][MZ_MAX_OBS + MZ_VIEW_DIM + MZ_MAX_CONTEXT];
    mzp_group_norm(l, MZ_POLICY_LANES, nm, obs_dim, obs + row * obs_dim, xn[grp]);
    mzp_group_ctx(l, MZ_POLICY_LANES, nm.ctx + row * nm.cdim, nm.cdim, xn[grp] + obs_dim);
    mzp_wave_sync();
    mzp_group_net_act(l, MZ_POLICY_LANES, params + row * pstride, obs_dim + nm.cdim, nu, s, squash, action_scale, sample != 0, key, env0 + row, xn[grp],
                      hid[grp][0], hid[grp][1], actions + row * nu, live, live && logp ? logp + row : nullptr, mode);
  } else {
    mzp_group_net_act(l, MZ_POLICY_LANES, params + row * pstride, obs_dim, nu, s, squash, action_scale, sample != 0, key, env0 + row,
                      obs + row * obs_dim, hid[grp][0], hid[grp][1], actions + row * nu, live, live && logp ? logp + row : nullptr, mode);
  }
}

// net_act_kernel for an actor with a state-dependent log-std head (mz_net_sample_head; mz_rollout_head where it steps launch by launch):
// the same groups and LDS rows, the output layer 2 nu units wide, mzp_group_net_sample_head of mz_policy.h.  A kernel of its own: the
// two instantiations of net_act_kernel compile as they did.
template <bool NRM = false>
__global__ __launch_bounds__(256) void net_sample_head_kernel(int n, int obs_dim, int nu, mzp_shape s, int squash, float action_scale, mzp_head hd,
                                                              const float* __restrict__ params, long pstride, uint64_t key, uint64_t env0,
                                                              const float* __restrict__ obs, float* __restrict__ actions, float* __restrict__ logp,
                                                              mzp_norm nm) {
  __shared__ float hid[256 / MZ_POLICY_LANES][MZ_NET_MAX_HIDDEN_LAYERS][MZ_POLICY_MAX_HIDDEN];
  const int l = (int)threadIdx.x % MZ_POLICY_LANES, grp = (int)threadIdx.x / MZ_POLICY_LANES;
  size_t row = (size_t)blockIdx.x * (256 / MZ_POLICY_LANES) + grp;
  const bool live = row < (size_t)n;
  if (!live) row = (size_t)n - 1;
  if constexpr (NRM) {
    __shared__ float xn[256 / MZ_POLICY_LANES][MZ_MAX_OBS + MZ_VIEW_DIM + MZ_MAX_CONTEXT];
    mzp_group_norm(l, MZ_POLICY_LANES, nm, obs_dim, obs + row * obs_dim, xn[grp]);
    mzp_group_ctx(l, MZ_POLICY_LANES, nm.ctx + row * nm.cdim, nm.cdim, xn[grp] + obs_dim);
    mzp_wave_sync();
    mzp_group_net_sample_head(l, MZ_POLICY_LANES, params + row * pstride, obs_dim + nm.cdim, nu, s, squash, action_scale, hd, key, env0 + row, xn[grp],
                              hid[grp][0], hid[grp][1], actions + row * nu, live, live && logp ? logp + row : nullptr);
  } else {
    mzp_group_net_sample_head(l, MZ_POLICY_LANES, params + row * pstride, obs_dim, nu, s, squash, action_scale, hd, key, env0 + row,
                              obs + row * obs_dim, hid[grp][0], hid[grp][1], actions + row * nu, live, live && logp ? logp + row : nullptr);
  }
}

// value_kernel for a critic of shape s (mz_net_value; mz_rollout_net where it steps launch by launch); NRM as in net_act_kernel: the
// row that is staged is the one the critic values, the final_obs row where the env finished
template <bool NRM = false>
__global__ __launch_bounds__(256) void net_value_kernel(int n, int obs_dim, mzp_shape s, const float* __restrict__ vparams, long vstride,
                                                        const float* __restrict__ obs, const float* __restrict__ final_obs,
                                                        const uint8_t* __restrict__ done, float* __restrict__ values, mzp_norm nm) {
  __shared__ float hid[256 / MZ_POLICY_LANES][MZ_NET_MAX_HIDDEN_LAYERS][MZ_POLICY_MAX_HIDDEN];
  const int l = (int)threadIdx.x % MZ_POLICY_LANES, grp = (int)threadIdx.x / MZ_POLICY_LANES;
  size_t row = (size_t)blockIdx.x * (256 / MZ_POLICY_LANES) + grp;
  const bool live = row < (size_t)n;
  if (!live) row = (size_t)n - 1;
  const float* x = (done && done[row] ? final_obs : obs) + row * obs_dim;
  float v;
  if constexpr (NRM) {
    __shared__ float xn[256 / MZ_POLICY_LANES][MZ_MAX_OBS + MZ_VIEW_DIM + MZ_MAX_CONTEXT];
    mzp_group_norm(l, MZ_POLICY_LANES, nm, obs_dim, x, xn[grp]);
    mzp_group_ctx(l, MZ_POLICY_LANES, nm.ctx + row * nm.cdim, nm.cdim, xn[grp] + obs_dim);
    mzp_wave_sync();
    v = mzp_group_net_value(l, MZ_POLICY_LANES, vparams + row * vstride, obs_dim + nm.cdim, s, xn[grp], hid[grp][0], hid[grp][1]);
  } else {
    v = mzp_group_net_value(l, MZ_POLICY_LANES, vparams + row * vstride, obs_dim, s, x, hid[grp][0], hid[grp][1]);
  }
  if (live && l == 0) values[row] = v;
}

// mz_gae: one lane per env, rows [k][env] coalesced across the lanes; the scan of mz_gae.h (mzg_step) from the last step back.  The
// four loads of a step do not depend on the carry: a block of MZ_GAE_DEPTH steps is loaded before its dependent chain runs.
constexpr int MZ_GAE_DEPTH = 8;
__global__ __launch_bounds__(64) void gae_kernel(int n, int nsteps, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                 const float* __restrict__ value, const float* __restrict__ next_value, float g, float gl,
                                                 float* __restrict__ adv, float* __restrict__ ret) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  float carry = 0.0f;
  for (int k1 = nsteps - 1; k1 >= 0; k1 -= MZ_GAE_DEPTH) {
    float r[MZ_GAE_DEPTH], v[MZ_GAE_DEPTH], nv[MZ_GAE_DEPTH];
    uint8_t d[MZ_GAE_DEPTH];
#pragma unroll
    for (int j = 0; j < MZ_GAE_DEPTH; j++) {
      const int k = k1 - j;
      if (k >= 0) {
        const size_t i = (size_t)k * n + env;
        r[j] = reward[i]; d[j] = done[i]; v[j] = value[i]; nv[j] = next_value[i];
      }
    }
#pragma unroll
    for (int j = 0; j < MZ_GAE_DEPTH; j++) {
      const int k = k1 - j;
      if (k >= 0) {
        const size_t i = (size_t)k * n + env;
        float rt;
        carry = mzg_step(r[j], d[j], v[j], nv[j], g, gl, carry, &rt);
        adv[i] = carry;
        if (ret) ret[i] = rt;
      }
    }
  }
}

// mz_return_scan: one lane per env, rows [k][env] coalesced across the lanes; the scan of mz_returns.h (mzr_step) from the first step
// on.  The two loads of a step do not depend on the carries: a block of MZ_GAE_DEPTH steps is loaded before its dependent chain runs.
// len_carry NULL: the length is not tracked (len_seq is NULL then: mz_return_scan).
__global__ __launch_bounds__(64) void return_scan_kernel(int n, int nsteps, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                         float g, float* __restrict__ carry, int32_t* __restrict__ len_carry,
                                                         float* __restrict__ ret_seq, int32_t* __restrict__ len_seq) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  float c = carry[env];
  int32_t len = len_carry ? len_carry[env] : 0;
  for (int k0 = 0; k0 < nsteps; k0 += MZ_GAE_DEPTH) {
    float r[MZ_GAE_DEPTH];
    uint8_t d[MZ_GAE_DEPTH];
#pragma unroll
    for (int j = 0; j < MZ_GAE_DEPTH; j++) {
      const int k = k0 + j;
      if (k < nsteps) {
        const size_t i = (size_t)k * n + env;
        r[j] = reward[i]; d[j] = done[i];
      }
    }
#pragma unroll
    for (int j = 0; j < MZ_GAE_DEPTH; j++) {
      const int k = k0 + j;
      if (k < nsteps) {
        const size_t i = (size_t)k * n + env;
        int32_t lo;
        ret_seq[i] = mzr_step(r[j], d[j], g, &c, &len, &lo);
        if (len_seq) len_seq[i] = lo;
      }
    }
  }
  carry[env] = c;
  if (len_carry) len_carry[env] = len;
}

static int set_err(mz_handle* h, int code, const char* what, hipError_t e) {
  if (h) snprintf(h->err, sizeof(h->err), "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
  return code;
}
#define HIPCHK(h, call)                                                      \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess) return set_err((h), MZ_ERR_HIP, #call, _e);        \
  } while (0)

// Every entry point runs with the handle's device current and restores the caller's device on return, so that a
// handle on GPU 1 in a process whose current device is GPU 0 (or a C caller passing stream = NULL) allocates, sets
// kernel attributes and launches on the right device — and torch's notion of the current device is left alone.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

extern "C" {

int mz_abi_version(void) { return MZ_ABI_VERSION; }
uint64_t mz_model_sizeof(void) { return sizeof(mz_model); }

mz_handle* mz_create(const mz_model* model, int32_t num_envs, int32_t device, char* err, int32_t errlen) {
  auto fail = [&](const char* msg) -> mz_handle* {
    if (err && errlen > 0) { strncpy(err, msg, (size_t)errlen - 1); err[errlen - 1] = 0; }
    return nullptr;
  };
  if (!model || num_envs <= 0) return fail("mz_create: bad arguments");
  if (model->abi_version != MZ_ABI_VERSION) return fail("mz_create: mz_model.abi_version mismatch");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("mz_create: no HIP device (the stepper has no CPU path)");
  if (device < 0 || device >= ndev) return fail("mz_create: device index out of range");
  DeviceScope scope(device);
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != device) return fail("mz_create: hipSetDevice failed");
  mz_handle* h = new (std::nothrow) mz_handle();
  if (!h) return fail("mz_create: out of memory");
  memset(h, 0, sizeof(*h));
  h->model = *model; h->n = num_envs; h->device = device; h->robot = model->robot; h->lanes = 32; h->waves_per_block = 1; h->seed = 0x5EEDULL;
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu <= 0) cu = 256;
    h->simds = 4 * cu;
  }
  // the general engine (generic_dyn.h) steps what no specialised kernel does — user robots, SPIN plates, more than three blocks —
  // and whatever the caller asks it to (mz_model.engine = 1); h->robot is the dispatch key, h->model.robot stays the family
  if (mzk_generic_needed(model)) h->robot = MZ_ROBOT_GENERIC;
  char msg[200] = {0};
  int rc = MZ_OK;
  if (h->robot == MZ_ROBOT_GENERIC) rc = MZ_OK;  // checked by mzk_generic_create below (it needs the device)
  else if (model->robot == MZ_ROBOT_ANT) rc = ant_dev_from_model(&h->ant, model, msg, sizeof(msg));
  else if (model->robot == MZ_ROBOT_POINT) rc = point_dev_from_model(&h->point, model, msg, sizeof(msg));
  else if (model->robot == MZ_ROBOT_SWIMMER) rc = swimmer_dev_from_model(&h->swimmer, model, msg, sizeof(msg));
  else { rc = MZ_ERR_UNSUPPORTED; snprintf(msg, sizeof(msg), "mz_create: robot kind %d has no device kernel yet", model->robot); }
  if (rc != MZ_OK) { delete h; return fail(msg); }
  hipError_t e = hipSuccess;
  view_dev_from_model(model, &h->view);
  const int vdim = model->top_down_view ? MZ_VIEW_DIM : 0;
  if (model->top_down_view && model->nblock > 4) { delete h; return fail("mz_create: top-down view with more than 4 movable blocks"); }
  if (h->robot == MZ_ROBOT_GENERIC) {
    rc = mzk_generic_create(h, msg, sizeof(msg));
    if (rc != MZ_OK) { mz_destroy(h); return fail(msg); }
    h->base_obs = model->obs_dim - vdim;
    const size_t rec = (size_t)model->nq + 2 * model->nv + 2;
    e = hipMalloc(&h->state, (size_t)num_envs * rec * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->state, 0, (size_t)num_envs * rec * sizeof(float));
  } else if (h->robot == MZ_ROBOT_ANT) {
    const int nb = h->ant.nblock;
    if (nb > 3) { delete h; return fail("mz_create: more than 3 movable blocks are not instantiated"); }
    h->lay.nq = ANT_NQ + h->ant.block_nax * nb + 7 * h->ant.nball; h->lay.nv = ANT_NV + h->ant.block_nax * nb + 6 * h->ant.nball;
    h->lay.rec_t = h->lay.nq + 2 * h->lay.nv;
    h->lay.rec = (h->lay.rec_t + 2 + 15) / 16 * 16;
    h->lay.nblock3 = model->observe_blocks ? 3 * nb : 0;
    h->lay.obs_dim = ANT_OBS + h->lay.nblock3 + ((h->ant.nball && model->observe_balls) ? 3 : 0);
    h->base_obs = h->lay.obs_dim;
    h->lay.ostride = h->lay.obs_dim + vdim;
    if (h->base_obs + vdim != model->obs_dim || h->base_obs > MZ_MAX_OBS) { delete h; return fail("mz_create: obs_dim mismatch"); }
    e = hipMalloc(&h->ant_dev, sizeof(AntDev));
    h->ant_dirty = 1;
    if (e == hipSuccess) e = hipMalloc(&h->state, (size_t)num_envs * h->lay.rec * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->state, 0, (size_t)num_envs * h->lay.rec * sizeof(float));
  } else {
    const int kq = mzk_planar_state_width(h);
    const int nb3 = h->robot == MZ_ROBOT_SWIMMER ? ((h->swimmer.observe_blocks && h->swimmer.nblock) ? 3 : 0)
                                                 : (h->point.observe_blocks ? 3 * h->point.nblock : 0) + (h->point.observe_balls ? 3 * h->point.nball : 0);
    const int want = h->robot == MZ_ROBOT_SWIMMER ? 2 * kq + 1 + nb3 : 7 + nb3;
    h->base_obs = want;
    if (want + vdim != model->obs_dim || want > MZ_MAX_OBS) { delete h; return fail("mz_create: obs_dim mismatch"); }
    h->pt_rec = mzk_planar_record_width(h);
    const size_t state_floats = (size_t)num_envs * (h->pt_rec ? h->pt_rec : 2 * kq);
    e = hipMalloc(&h->state, state_floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&h->pt_t, (size_t)num_envs * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&h->pt_ep, (size_t)num_envs * sizeof(uint32_t));
    if (h->robot == MZ_ROBOT_SWIMMER) {
      if (e == hipSuccess) e = hipMalloc(&h->swimmer_dev, sizeof(SwimmerDev));
      if (e == hipSuccess) e = hipMemcpy(h->swimmer_dev, &h->swimmer, sizeof(SwimmerDev), hipMemcpyHostToDevice);
    } else {
      if (e == hipSuccess) e = hipMalloc(&h->point_dev, sizeof(PointDev));
      if (e == hipSuccess) e = hipMemcpy(h->point_dev, &h->point, sizeof(PointDev), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemset(h->state, 0, state_floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->pt_t, 0, (size_t)num_envs * sizeof(int));
    if (e == hipSuccess) e = hipMemset(h->pt_ep, 0, (size_t)num_envs * sizeof(uint32_t));
  }
  if (e == hipSuccess) e = hipMalloc(&h->status, (size_t)num_envs * sizeof(int));
  if (e == hipSuccess) e = hipMemset(h->status, 0, (size_t)num_envs * sizeof(int));
  if (e != hipSuccess) {
    snprintf(msg, sizeof(msg), "mz_create: device allocation failed: %s", hipGetErrorString(e));
    mz_destroy(h);
    return fail(msg);
  }
  return h;
}

void mz_destroy(mz_handle* h) {
  if (!h) return;
  DeviceScope scope(h->device);
  if (h->state) (void)hipFree(h->state);
  if (h->pt_t) (void)hipFree(h->pt_t);
  if (h->pt_ep) (void)hipFree(h->pt_ep);
  if (h->point_dev) (void)hipFree(h->point_dev);
  if (h->swimmer_dev) (void)hipFree(h->swimmer_dev);
  if (h->ant_dev) (void)hipFree(h->ant_dev);
  mzk_generic_destroy(h);
  if (h->status) (void)hipFree(h->status);
  if (h->prof) (void)hipFree(h->prof);
  if (h->render_qpos) (void)hipFree(h->render_qpos);
  if (h->policy_act) (void)hipFree(h->policy_act);
  if (h->ctx_ident) (void)hipFree(h->ctx_ident);
  if (h->ctx_old) (void)hipFree(h->ctx_old);
  if (h->ev) { for (int i = 0; i < 2 * h->ntime; i++) (void)hipEventDestroy(h->ev[i]); free(h->ev); }
  delete h;
}

const char* mz_last_error(const mz_handle* h) { return h ? h->err : "null handle"; }
int32_t mz_num_envs(const mz_handle* h) { return h ? h->n : MZ_ERR_ARG; }
int32_t mz_obs_dim(const mz_handle* h) { return h ? h->model.obs_dim : MZ_ERR_ARG; }
int32_t mz_nq(const mz_handle* h) { return h ? h->model.nq : MZ_ERR_ARG; }
int32_t mz_nv(const mz_handle* h) { return h ? h->model.nv : MZ_ERR_ARG; }
int32_t mz_nu(const mz_handle* h) { return h ? h->model.nu : MZ_ERR_ARG; }

int32_t mz_set_option(mz_handle* h, const char* key, double value) {
  if (!h || !key) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  if (!strcmp(key, "auto_reset")) { h->auto_reset = value != 0; return MZ_OK; }
  if (!strcmp(key, "seed")) { h->seed = (uint64_t)value; return MZ_OK; }
  if (!strcmp(key, "env_index_offset")) { h->env0 = (uint64_t)value; return MZ_OK; }
  if (!strcmp(key, "wide_nets")) {  // mz_net networks of up to MZ_NET_MAX_WIDTH units per layer on the tiled kernel (include/mazestep.h)
    if (value != 0.0 && value != 1.0 && value != 2.0) return set_err(h, MZ_ERR_ARG, "wide_nets must be 0, 1 or 2", hipSuccess);
    h->wide_nets = (int)value;
    return MZ_OK;
  }
  if (h->robot == MZ_ROBOT_POINT && !strcmp(key, "ls_fast_iterations")) {  // the Point's float64 solvers: unit steps before the exact search (0 = search in every iteration)
    if (value < 0 || value > 50) return set_err(h, MZ_ERR_ARG, "ls_fast_iterations must be 0 .. 50", hipSuccess);
    h->point.unit_steps = (int)value;
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(h->point_dev, &h->point, sizeof(PointDev), hipMemcpyHostToDevice));
    return MZ_OK;
  }
  if (h->robot != MZ_ROBOT_ANT && (!strcmp(key, "solver_iterations") || !strcmp(key, "solver_tolerance") || !strcmp(key, "solver_rtol") ||
                                   !strcmp(key, "ls_iterations") || !strcmp(key, "ls_fast_iterations") || !strcmp(key, "ls_fast") || !strcmp(key, "debug_frame_skip") || !strcmp(key, "waves_per_block") || !strcmp(key, "waves_per_simd")))
    return set_err(h, MZ_ERR_UNSUPPORTED, "mz_set_option: this key tunes the Ant kernels only (the other robots' solvers have fixed settings)", hipSuccess);
  if (h->robot == MZ_ROBOT_GENERIC && !strcmp(key, "lanes_per_env"))
    return set_err(h, MZ_ERR_UNSUPPORTED, "mz_set_option: the generic-robot kernel runs one wavefront per env", hipSuccess);
  if (!strcmp(key, "solver_iterations")) { h->ant_dirty = 1; h->ant.max_iter = (int)value; return MZ_OK; }
  if (!strcmp(key, "solver_tolerance")) { h->ant_dirty = 1; h->ant.tol = (float)value; return MZ_OK; }
  if (!strcmp(key, "solver_rtol")) { h->ant_dirty = 1; h->ant.rtol = (float)value; return MZ_OK; }
  if (!strcmp(key, "ls_iterations")) { h->ant_dirty = 1; h->ant.ls_iter = (int)value; return MZ_OK; }
  if (!strcmp(key, "ls_fast_iterations")) { h->ant_dirty = 1; h->ant.ls_fast_iters = (int)value; return MZ_OK; }
  if (!strcmp(key, "ls_fast")) { h->ant_dirty = 1; h->ant.ls_fast = (int)value; return MZ_OK; }
  if (!strcmp(key, "debug_frame_skip")) { h->ant_dirty = 1; h->ant.frame_skip = (int)value; return MZ_OK; }  // diagnostics: mj_steps per env.step (Ant)
  if (!strcmp(key, "lanes_per_env")) {
    int g = (int)value;
    if (g != 8 && g != 16 && g != 32 && g != 64) return set_err(h, MZ_ERR_ARG, "lanes_per_env must be 8, 16, 32 or 64", hipSuccess);
    if (h->robot == MZ_ROBOT_ANT && !mzk_ant_lanes_ok(h, g))  // no fall-back to another width: launch_info() names the kernel that steps
      return set_err(h, MZ_ERR_UNSUPPORTED, "mz_set_option: lanes_per_env = 8 exists for the plain Ant only; an Ant with movable blocks or a ball steps at 16, 32 or 64 lanes", hipSuccess);
    h->lanes = g; h->lanes_set = 1;
    return MZ_OK;
  }
  if (!strcmp(key, "profile_phases")) {
    if (value != 0 && !h->prof) {  // 16 accumulators + one total per workgroup (at most one workgroup per env)
      HIPCHK(h, hipMalloc(&h->prof, (16 + 17 * (size_t)h->n) * sizeof(unsigned long long)));
      HIPCHK(h, hipMemset(h->prof, 0, (16 + 17 * (size_t)h->n) * sizeof(unsigned long long)));
    }
    if (value == 0 && h->prof) {
      HIPCHK(h, hipDeviceSynchronize());  // an instrumented step kernel may still be adding to the accumulators
      (void)hipFree(h->prof); h->prof = nullptr;
    }
    return MZ_OK;
  }
  if (!strcmp(key, "waves_per_block")) {
    int w = (int)value;
    if (w != 1 && w != 2 && w != 4) return set_err(h, MZ_ERR_ARG, "waves_per_block must be 1, 2 or 4", hipSuccess);
    h->waves_per_block = w; h->wpb_set = 1;
    return MZ_OK;
  }
  if (!strcmp(key, "waves_per_simd")) {
    int w = (int)value;
    if (w < 0 || w > 2) return set_err(h, MZ_ERR_ARG, "waves_per_simd must be 0 (by the launch's wave count), 1 or 2", hipSuccess);
    h->waves_per_simd = w;
    return MZ_OK;
  }
  if (!strcmp(key, "time_kernels")) {
    if (h->ev) { for (int i = 0; i < 2 * h->ntime; i++) (void)hipEventDestroy(h->ev[i]); free(h->ev); h->ev = nullptr; }
    h->ntime = (int)value; h->itime = 0; h->time_phase = 0;
    if (h->ntime > 0) {
      h->ev = (hipEvent_t*)calloc((size_t)2 * h->ntime, sizeof(hipEvent_t));
      // (no system-scope fence: the default event writes back and invalidates the caches at every record — the timestamps are read by this process
      // after a synchronise, nothing on the host polls the memory the kernels write)
      for (int i = 0; i < 2 * h->ntime; i++) HIPCHK(h, hipEventCreateWithFlags(&h->ev[i], hipEventDisableSystemFence));
    }
    return MZ_OK;
  }
  if (!strcmp(key, "time_kernels_stride")) {  // time every k-th launch only: an event pair costs a small kernel 7.6 us of its 45 (profiles/r06/event_overhead.txt)
    if (value < 1) return set_err(h, MZ_ERR_ARG, "time_kernels_stride must be >= 1", hipSuccess);
    h->time_stride = (int)value; h->time_phase = 0;
    return MZ_OK;
  }
  return set_err(h, MZ_ERR_ARG, "unknown option", hipSuccess);
}

// What the next mz_step will launch — the kernel instantiation depends on the robot, the batch size and the device's compute-unit
// count (include/mazestep.h), so a caller that compares runs across batch sizes or devices can record it.
int32_t mz_get_info(const mz_handle* h, const char* key, double* value) {
  if (!h || !key || !value) return MZ_ERR_ARG;
  if (!strcmp(key, "engine")) { *value = h->robot == MZ_ROBOT_GENERIC ? 1.0 : 0.0; return MZ_OK; }
  if (!strcmp(key, "device_simds")) { *value = (double)h->simds; return MZ_OK; }
  if (!strcmp(key, "obs_norm")) { *value = h->nrm_mean ? 1.0 : 0.0; return MZ_OK; }  // mz_bind_obs_norm: a normaliser is bound (1) or not (0)
  if (!strcmp(key, "rollout_fused")) { *value = (double)mzk_planar_rollout_fused(h); return MZ_OK; }  // mz_rollout: fused kernels (1) or the step's launches in a loop (0)
  if (!strcmp(key, "wide_nets")) { *value = (double)h->wide_nets; return MZ_OK; }  // the option's mode
  if (!strcmp(key, "ls_fast_iterations")) {  // Newton iterations of a solve that take unit steps (-1: this handle's kernels have no such phase)
    *value = h->robot == MZ_ROBOT_ANT ? (double)h->ant.ls_fast_iters : (h->robot == MZ_ROBOT_POINT ? (double)h->point.unit_steps : -1.0);
    return MZ_OK;
  }
  if (!strcmp(key, "lanes_per_env") || !strcmp(key, "waves_per_simd")) {
    int lanes = 64, wps = 1;
    if (h->robot == MZ_ROBOT_ANT) mzk_ant_shape(h, &lanes, &wps);
    else if (h->robot != MZ_ROBOT_GENERIC) lanes = mzk_planar_lanes(h);
    *value = (double)(key[0] == 'l' ? lanes : wps);
    return MZ_OK;
  }
  return MZ_ERR_ARG;
}

int32_t mz_bind_final_obs(mz_handle* h, float* final_obs_dev) {
  if (!h) return MZ_ERR_ARG;
  h->final_obs = final_obs_dev;
  return MZ_OK;
}

int32_t mz_bind_record(mz_handle* h, float* record_dev) {
  if (!h) return MZ_ERR_ARG;
  h->record = record_dev;
  return MZ_OK;
}

// stores the two pointers and the clip and nothing else: no launch, no synchronisation (include/mazestep.h); a refused call leaves
// the previous binding in place
int32_t mz_bind_obs_norm(mz_handle* h, const float* mean_dev, const float* inv_std_dev, double clip, void* stream) {
  (void)stream;
  if (!h) return MZ_ERR_ARG;
  if (!mean_dev && !inv_std_dev) { h->nrm_mean = h->nrm_inv_std = nullptr; h->nrm_clip = 0.0f; return MZ_OK; }
  if (!mean_dev) return set_err(h, MZ_ERR_ARG, "mz_bind_obs_norm: mean_dev is NULL and inv_std_dev is not (both NULL unbinds)", hipSuccess);
  if (!inv_std_dev) return set_err(h, MZ_ERR_ARG, "mz_bind_obs_norm: inv_std_dev is NULL and mean_dev is not (both NULL unbinds)", hipSuccess);
  if (!(clip > 0.0)) return set_err(h, MZ_ERR_ARG, "mz_bind_obs_norm: clip must be > 0 (+inf switches the clip off) and not NaN", hipSuccess);
  if (h->model.obs_dim > MZ_MAX_OBS + MZ_VIEW_DIM)  // the staged row of the NRM kernels; no handle mz_create makes is wider
    return set_err(h, MZ_ERR_UNSUPPORTED, "mz_bind_obs_norm: obs_dim exceeds MZ_MAX_OBS + MZ_VIEW_DIM", hipSuccess);
  h->nrm_mean = mean_dev; h->nrm_inv_std = inv_std_dev; h->nrm_clip = (float)clip;
  return MZ_OK;
}

}  // extern "C"
// (re)build the task block from h->model (+ the bound per-env goal table) and upload it to the handle's kernels
static int upload_task(mz_handle* h) {
  mz_model* m = &h->model;
  if (h->robot == MZ_ROBOT_ANT) {
    task_dev_from_model(&h->ant.task, m); h->ant.task.env_goals = h->env_goals;
    HIPCHK(h, hipMemcpy(reinterpret_cast<char*>(h->ant_dev) + offsetof(AntDev, task), &h->ant.task, sizeof(TaskDev), hipMemcpyHostToDevice));
  } else if (h->robot == MZ_ROBOT_POINT) {
    task_dev_from_model(&h->point.task, m); h->point.task.env_goals = h->env_goals;
    HIPCHK(h, hipMemcpy(reinterpret_cast<char*>(h->point_dev) + offsetof(PointDev, task), &h->point.task, sizeof(TaskDev), hipMemcpyHostToDevice));
  } else if (h->robot == MZ_ROBOT_SWIMMER) {
    task_dev_from_model(&h->swimmer.task, m); h->swimmer.task.env_goals = h->env_goals;
    HIPCHK(h, hipMemcpy(reinterpret_cast<char*>(h->swimmer_dev) + offsetof(SwimmerDev, task), &h->swimmer.task, sizeof(TaskDev), hipMemcpyHostToDevice));
  } else {
    TaskDev t;
    task_dev_from_model(&t, m); t.env_goals = h->env_goals;
    HIPCHK(h, mzk_generic_set_task(h, &t));
  }
  return MZ_OK;
}
extern "C" {

// Per-env goal positions.  The reference gives every env its own task object and resamples its goals at EVERY episode reset
// (MazeEnv.reset -> MazeTask.sample_goals, maze_env.py:374-376); a batch that shares one goal table cannot.  goal_pos_dev: DEVICE
// pointer, [num_envs][MZ_MAX_GOAL][3] float64, caller-owned and caller-updated (the host mirror rewrites the rows of the envs
// whose episode ended, between two steps); NULL unbinds (back to the shared table of mz_set_goals / the model).  Thresholds, reward
// scales, dims and the goal COUNT stay those of the shared table.  Synchronises on `stream` first.  Returns MZ_OK or an error code.
int32_t mz_bind_env_goals(mz_handle* h, const double* goal_pos_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  h->env_goals = goal_pos_dev;
  return upload_task(h);
}

int32_t mz_set_goals(mz_handle* h, int32_t ngoal, const double* pos, const double* threshold, const double* reward_scale, const int32_t* dim,
                     void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (ngoal < 0 || ngoal > MZ_MAX_GOAL || (ngoal > 0 && (!pos || !threshold || !reward_scale || !dim)))
    return set_err(h, MZ_ERR_ARG, "mz_set_goals: 0 <= ngoal <= MZ_MAX_GOAL rows of pos / threshold / reward_scale / dim", hipSuccess);
  for (int g = 0; g < ngoal; g++)
    if ((dim[g] != 2 && dim[g] != 3) || !(threshold[g] >= 0.0)) return set_err(h, MZ_ERR_ARG, "mz_set_goals: dim must be 2 or 3, threshold >= 0", hipSuccess);
  DeviceScope scope(h->device);
  mz_model* m = &h->model;
  m->ngoal = ngoal;
  for (int g = 0; g < ngoal; g++) {
    for (int k = 0; k < 3; k++) m->goal_pos[g][k] = pos[3 * g + k];
    m->goal_threshold[g] = threshold[g]; m->goal_reward_scale[g] = reward_scale[g]; m->goal_dim[g] = dim[g];
  }
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));  // steps already queued keep the goals they were launched with
  return upload_task(h);
}

int32_t mz_reset(mz_handle* h, const uint8_t* mask_dev, uint64_t seed, float* obs_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  hipStream_t st = (hipStream_t)stream;
  h->seed = seed;
  if (h->robot == MZ_ROBOT_ANT) HIPCHK(h, mzk_ant_reset(h, st, mask_dev, seed, obs_dev));
  else if (h->robot == MZ_ROBOT_GENERIC) HIPCHK(h, mzk_generic_reset(h, st, mask_dev, seed, obs_dev));
  else HIPCHK(h, mzk_planar_reset(h, st, mask_dev, seed, obs_dev));
  if (h->view.on && obs_dev) HIPCHK(h, mzk_view_fill(h, st, obs_dev, NULL, NULL));
  return MZ_OK;
}

int32_t mz_set_state(mz_handle* h, const float* qpos_dev, const float* qvel_dev, const float* warmstart_dev, const int32_t* t_dev,
                     void* stream) {
  if (!h) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  hipStream_t st = (hipStream_t)stream;
  if (h->robot == MZ_ROBOT_ANT) HIPCHK(h, mzk_ant_set_state(h, st, qpos_dev, qvel_dev, warmstart_dev, t_dev));
  else if (h->robot == MZ_ROBOT_GENERIC) HIPCHK(h, mzk_generic_set_state(h, st, qpos_dev, qvel_dev, warmstart_dev, t_dev));
  else HIPCHK(h, mzk_planar_set_state(h, st, qpos_dev, qvel_dev, t_dev));
  return MZ_OK;
}

int32_t mz_get_state(mz_handle* h, float* qpos_dev, float* qvel_dev, float* warmstart_dev, int32_t* t_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  hipStream_t st = (hipStream_t)stream;
  if (h->robot == MZ_ROBOT_ANT) HIPCHK(h, mzk_ant_get_state(h, st, qpos_dev, qvel_dev, warmstart_dev, t_dev));
  else if (h->robot == MZ_ROBOT_GENERIC) HIPCHK(h, mzk_generic_get_state(h, st, qpos_dev, qvel_dev, warmstart_dev, t_dev));
  else HIPCHK(h, mzk_planar_get_state(h, st, qpos_dev, qvel_dev, warmstart_dev, t_dev));
  return MZ_OK;
}

// one step's launches: the engine's step kernel, the top-down view of the rows it wrote, the packed record (mz_step, and mz_rollout
// where it steps launch by launch)
static int step_launches(mz_handle* h, hipStream_t st, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                         int32_t* goal_idx_dev, float* info_dev) {
  if (h->robot == MZ_ROBOT_ANT) HIPCHK(h, mzk_ant_step(h, st, actions_dev, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev));
  else if (h->robot == MZ_ROBOT_GENERIC) HIPCHK(h, mzk_generic_step(h, st, actions_dev, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev));
  else HIPCHK(h, mzk_planar_step(h, st, actions_dev, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev));
  if (h->view.on) HIPCHK(h, mzk_view_fill(h, st, obs_dev, h->auto_reset ? h->final_obs : NULL, done_dev));
  if (h->record && ((h->robot != MZ_ROBOT_ANT && h->robot != MZ_ROBOT_GENERIC) || h->view.on)) {
    const size_t tot = (size_t)h->n * (h->model.obs_dim + 2);
    hipLaunchKernelGGL(pack_record_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->n, h->model.obs_dim, obs_dev, reward_dev, done_dev, h->record);
  }
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

int32_t mz_step(mz_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev,
                float* info_dev, void* stream) {
  if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev) return h ? set_err(h, MZ_ERR_ARG, "mz_step: null array", hipSuccess) : MZ_ERR_ARG;
  DeviceScope scope(h->device);
  hipStream_t st = (hipStream_t)stream;
  int slot = -1;
  if (h->ntime > 0 && (h->time_phase++ % (h->time_stride > 0 ? h->time_stride : 1)) == 0) { slot = h->itime % h->ntime; HIPCHK(h, hipEventRecord(h->ev[2 * slot], st)); }
  const int rc = step_launches(h, st, actions_dev, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev);
  if (rc != MZ_OK) return rc;
  if (slot >= 0) { HIPCHK(h, hipEventRecord(h->ev[2 * slot + 1], st)); h->itime++; }
  h->nsteps++;
  return MZ_OK;
}

// A legacy network (int `hidden`, tanh) as the mz_net it is.  While a normaliser is bound (mz_bind_obs_norm) the legacy entries run
// the network entries' kernels, which return the bits of the legacy ones for such a network and have the NRM instantiations; unbound
// handles launch what they always launched (the single calls below; the rollouts: mzk_rollout_kernels).
static mz_net legacy_net(const float* params_dev, int64_t env_stride, int hidden, int squash, double action_scale) {
  return mz_net{(uint32_t)sizeof(mz_net), hidden > 0 ? 1 : 0, {hidden, 0}, MZ_ACT_TANH, squash, action_scale, params_dev, env_stride};
}
static void net_act_launch(mz_handle* h, hipStream_t st, const mz_net* actor, int sample, uint64_t noise_seed, uint64_t noise_step,
                           const float* obs_dev, float* actions_dev, float* logp_dev, int noise_mode = MZ_NOISE_PRE_SQUASH,
                           const mz_context* ctx = nullptr);
static void net_value_launch(mz_handle* h, hipStream_t st, const mz_net* critic, const float* obs_dev, const float* final_obs_dev,
                             const uint8_t* done_dev, float* values_dev, const mz_context* ctx = nullptr);

// the checks the four policy entries share (stochastic: the vector carries log_std[nu] behind the network); MZ_OK or MZ_ERR_ARG with
// the message set
static int policy_args(mz_handle* h, const char* who, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash,
                       bool stochastic = false) {
  char msg[160];
  const char* why = nullptr;
  if (!params_dev) why = "null params_dev";
  else if (hidden < 0 || hidden > MZ_POLICY_MAX_HIDDEN) why = "hidden must be 0 .. MZ_POLICY_MAX_HIDDEN (64)";
  else if (squash != 0 && squash != 1) why = "squash must be 0 or 1";
  else if (param_env_stride != 0 && param_env_stride != (int64_t)mzp_param_count(h->model.obs_dim, h->model.nu, hidden) + (stochastic ? h->model.nu : 0))
    why = stochastic ? "param_env_stride must be 0 (one shared policy) or npar_s = npar + nu (one policy per env, log_std behind the network)"
                     : "param_env_stride must be 0 (one shared policy) or npar (one policy per env)";
  if (!why) return MZ_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
}

static void policy_act_launch(mz_handle* h, hipStream_t st, const float* params_dev, int64_t pstride, int hidden, int squash, float scale,
                              const float* obs_dev, float* actions_dev) {
  const int rows = 256 / MZ_POLICY_LANES;
  hipLaunchKernelGGL(policy_act_kernel, dim3((unsigned)((h->n + rows - 1) / rows)), dim3(256), 0, st, h->n, h->model.obs_dim, h->model.nu, hidden, squash,
                     scale, params_dev, (long)pstride, obs_dev, actions_dev);
}

int32_t mz_policy_act(mz_handle* h, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash, double action_scale,
                      const float* obs_dev, float* actions_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!obs_dev || !actions_dev) return set_err(h, MZ_ERR_ARG, "mz_policy_act: null array", hipSuccess);
  const int rc = policy_args(h, "mz_policy_act", params_dev, param_env_stride, hidden, squash);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  if (h->nrm_mean) {
    const mz_net a = legacy_net(params_dev, param_env_stride, hidden, squash, action_scale);
    net_act_launch(h, (hipStream_t)stream, &a, 0, 0, 0, obs_dev, actions_dev, NULL);
  } else {
    policy_act_launch(h, (hipStream_t)stream, params_dev, param_env_stride, hidden, squash, (float)action_scale, obs_dev, actions_dev);
  }
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

static void policy_sample_launch(mz_handle* h, hipStream_t st, const float* params_dev, int64_t pstride, int hidden, int squash, float scale,
                                 uint64_t noise_seed, uint64_t noise_step, const float* obs_dev, float* actions_dev, float* logp_dev) {
  const int rows = 256 / MZ_POLICY_LANES;
  hipLaunchKernelGGL(policy_sample_kernel, dim3((unsigned)((h->n + rows - 1) / rows)), dim3(256), 0, st, h->n, h->model.obs_dim, h->model.nu, hidden,
                     squash, scale, params_dev, (long)pstride, mzp_noise_key(noise_seed, noise_step), h->env0, obs_dev, actions_dev, logp_dev,
                     MZ_NOISE_PRE_SQUASH);
}

int32_t mz_policy_sample(mz_handle* h, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash, double action_scale,
                         uint64_t noise_seed, uint64_t noise_step, const float* obs_dev, float* actions_dev, float* logp_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!obs_dev || !actions_dev) return set_err(h, MZ_ERR_ARG, "mz_policy_sample: null array", hipSuccess);
  const int rc = policy_args(h, "mz_policy_sample", params_dev, param_env_stride, hidden, squash, true);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  if (h->nrm_mean) {
    const mz_net a = legacy_net(params_dev, param_env_stride, hidden, squash, action_scale);
    net_act_launch(h, (hipStream_t)stream, &a, 1, noise_seed, noise_step, obs_dev, actions_dev, logp_dev);
  } else {
    policy_sample_launch(h, (hipStream_t)stream, params_dev, param_env_stride, hidden, squash, (float)action_scale, noise_seed, noise_step, obs_dev,
                         actions_dev, logp_dev);
  }
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// the checks mz_value and mz_rollout_actor_critic share: a critic is a policy with nu = 1 in a vector of its own
static int critic_args(mz_handle* h, const char* who, const float* vparams_dev, int64_t env_stride, int32_t hidden) {
  char msg[160];
  const char* why = nullptr;
  if (!vparams_dev) why = "null critic parameters (params_dev)";
  else if (hidden < 0 || hidden > MZ_POLICY_MAX_HIDDEN) why = "the critic's hidden must be 0 .. MZ_POLICY_MAX_HIDDEN (64)";
  else if (env_stride != 0 && env_stride != (int64_t)mzp_param_count(h->model.obs_dim, 1, hidden))
    why = "the critic's env_stride must be 0 (one shared critic) or nvpar (one critic per env)";
  if (!why) return MZ_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
}

static void value_launch(mz_handle* h, hipStream_t st, const float* vparams_dev, int64_t vstride, int hidden, const float* obs_dev,
                         const float* final_obs_dev, const uint8_t* done_dev, float* values_dev) {
  const int rows = 256 / MZ_POLICY_LANES;
  hipLaunchKernelGGL(value_kernel, dim3((unsigned)((h->n + rows - 1) / rows)), dim3(256), 0, st, h->n, h->model.obs_dim, hidden, vparams_dev,
                     (long)vstride, obs_dev, final_obs_dev, done_dev, values_dev);
}

int32_t mz_value(mz_handle* h, const float* vparams_dev, int64_t env_stride, int32_t hidden, const float* obs_dev, float* values_dev,
                 void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!obs_dev || !values_dev) return set_err(h, MZ_ERR_ARG, "mz_value: null array", hipSuccess);
  const int rc = critic_args(h, "mz_value", vparams_dev, env_stride, hidden);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  if (h->nrm_mean) {
    const mz_net c = legacy_net(vparams_dev, env_stride, hidden, 0, 1.0);
    net_value_launch(h, (hipStream_t)stream, &c, obs_dev, NULL, NULL, values_dev);
  } else {
    value_launch(h, (hipStream_t)stream, vparams_dev, env_stride, hidden, obs_dev, NULL, NULL, values_dev);
  }
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// the checks the three mz_net entries share; `which`: the argument's name ("actor" / "critic"), nout: nu or 1, stochastic: the
// vector carries log_std[nu] behind the network — unless `head`: the output layer is 2 nu units wide and nothing follows it.
// MZ_OK or MZ_ERR_ARG with the message set.
// Which kernel family evaluates an mz_net on this handle (option "wide_nets"): the tiled kernel of mz_net_tile.h for a network with a
// layer wider than MZ_POLICY_MAX_HIDDEN (modes 1 and 2) and for every network in mode 2, the group kernels above otherwise.  The
// entries that take an int `hidden` never ask: their networks stay on the group kernels in every mode.
static bool net_tiled(const mz_handle* h, const mz_net* net) {
  if (h->wide_nets == 2) return true;
  if (h->wide_nets == 1)
    for (int k = 0; k < net->n_hidden && k < MZ_NET_MAX_HIDDEN_LAYERS; k++)
      if (net->hidden[k] > MZ_POLICY_MAX_HIDDEN) return true;
  return false;
}

static int net_args(mz_handle* h, const char* who, const char* which, const mz_net* net, int nout, bool stochastic, bool is_critic,
                    bool head = false, int cdim = 0) {
  char msg[200];
  auto fail = [&](const char* field, const char* why) {
    snprintf(msg, sizeof(msg), "%s: %s%s %s", who, which, field, why);
    return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
  };
  if (!net) return fail("", "is NULL");
  if (net->struct_size != sizeof(mz_net)) return fail("->struct_size", "must be sizeof(mz_net)");
  if (net->n_hidden < 0 || net->n_hidden > MZ_NET_MAX_HIDDEN_LAYERS) return fail("->n_hidden", "must be 0 .. MZ_NET_MAX_HIDDEN_LAYERS (2)");
  for (int k = 0; k < MZ_NET_MAX_HIDDEN_LAYERS; k++) {
    const char* field = k ? "->hidden[1]" : "->hidden[0]";
    if (k < net->n_hidden && (net->hidden[k] < 1 || net->hidden[k] > (h->wide_nets ? MZ_NET_MAX_WIDTH : MZ_POLICY_MAX_HIDDEN)))
      return fail(field, h->wide_nets ? "must be 1 .. MZ_NET_MAX_WIDTH (256): option wide_nets is on"
                                      : "must be 1 .. MZ_POLICY_MAX_HIDDEN (64); option wide_nets = 1 admits up to MZ_NET_MAX_WIDTH (256)");
    if (k >= net->n_hidden && net->hidden[k] != 0) return fail(field, "must be 0: the layer is not in use");
  }
  if (net->activation != MZ_ACT_TANH && net->activation != MZ_ACT_RELU) return fail("->activation", "must be MZ_ACT_TANH (0) or MZ_ACT_RELU (1)");
  if (net->squash != 0 && net->squash != 1) return fail("->squash", "must be 0 or 1");
  if (is_critic && net->squash != 0) return fail("->squash", "must be 0: a critic is never squashed");
  if (!net->params_dev) return fail("->params_dev", "is NULL");
  const int64_t count = (int64_t)mzp_net_param_count(h->model.obs_dim + cdim, head ? 2 * nout : nout,
                                                     mzp_shape{net->n_hidden, net->hidden[0], net->hidden[1], net->activation}) +
                        (stochastic && !head ? h->model.nu : 0);
  if (net->env_stride != 0 && net->env_stride != count)
    return fail("->env_stride", cdim ? "must be 0 (one shared network) or the count for obs_dim + ctx->dim inputs (one per env)"
                                : head ? "must be 0 (one shared network) or the head count (one per env; an output layer of 2 nu units, no log_std behind it)"
                                : stochastic ? "must be 0 (one shared network) or count (one per env; log_std[nu] behind the network counts)"
                                           : "must be 0 (one shared network) or count (one per env)");
  // the LDS rows of the tiled kernel (mz_net_tile.h)
  if (net_tiled(h, net) && (h->model.obs_dim + cdim > MZT_IN_MAX || (head ? 2 * nout : nout) > MZT_OUT_MAX)) {
    snprintf(msg, sizeof(msg), "%s: %s runs the tiled kernel (wide_nets), which takes at most %d inputs and %d output units", who, which, MZT_IN_MAX,
             MZT_OUT_MAX);
    return set_err(h, MZ_ERR_UNSUPPORTED, msg, hipSuccess);
  }
  return MZ_OK;
}

static mzp_shape net_shape(const mz_net* net) { return mzp_shape{net->n_hidden, net->hidden[0], net->hidden[1], net->activation}; }

// The normaliser a network launch gets: the handle's, or — for a call with a context on a handle without one — the identity, which
// returns the raw bits (mz_policy.h); with the context rows of the launch behind it.  ctx_prepare has allocated the identity.
static mzp_norm ctx_norm(const mz_handle* h, const mz_context* ctx) {
  if (!ctx) return mzp_norm{h->nrm_mean, h->nrm_inv_std, h->nrm_clip, 0, nullptr};
  if (h->nrm_mean) return mzp_norm{h->nrm_mean, h->nrm_inv_std, h->nrm_clip, ctx->dim, ctx->ctx_dev};
  return mzp_norm{h->ctx_ident, h->ctx_ident + h->model.obs_dim, INFINITY, ctx->dim, ctx->ctx_dev};
}

// what a checked call with a context needs on the handle before its first launch: the identity normaliser, and for the relative
// transition the scratch of the old columns.  Synchronous copies on first use only.
static int ctx_prepare(mz_handle* h, const mz_context* ctx) {
  const size_t od = (size_t)h->model.obs_dim;
  if (!h->ctx_ident) {
    float* host = (float*)malloc(2 * od * sizeof(float));
    if (!host) return set_err(h, MZ_ERR_HIP, "mz_context: out of memory", hipSuccess);
    for (size_t i = 0; i < od; i++) { host[i] = 0.0f; host[od + i] = 1.0f; }
    float* dev = nullptr;
    hipError_t e = hipMalloc(&dev, 2 * od * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dev, host, 2 * od * sizeof(float), hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess) { if (dev) (void)hipFree(dev); return set_err(h, MZ_ERR_HIP, "mz_context: identity normaliser", e); }
    h->ctx_ident = dev;
  }
  if (ctx->update == MZ_CTX_RELATIVE && !h->ctx_old) HIPCHK(h, hipMalloc(&h->ctx_old, (size_t)h->n * MZ_MAX_CONTEXT * sizeof(float)));
  return MZ_OK;
}

static void net_act_launch(mz_handle* h, hipStream_t st, const mz_net* actor, int sample, uint64_t noise_seed, uint64_t noise_step,
                           const float* obs_dev, float* actions_dev, float* logp_dev, int noise_mode, const mz_context* ctx) {
  const int rows = 256 / MZ_POLICY_LANES;
  const mzp_norm nm = ctx_norm(h, ctx);
#define MZ_NET_ACT(NRM)                                                                                                                         \
  hipLaunchKernelGGL(net_act_kernel<NRM>, dim3((unsigned)((h->n + rows - 1) / rows)), dim3(256), 0, st, h->n, h->model.obs_dim, h->model.nu,     \
                     net_shape(actor), actor->squash, (float)actor->action_scale, actor->params_dev, (long)actor->env_stride, sample,           \
                     sample ? mzp_noise_key(noise_seed, noise_step) : 0, h->env0, obs_dev, actions_dev, sample ? logp_dev : NULL, nm, noise_mode)
  if (nm.mean) MZ_NET_ACT(true); else MZ_NET_ACT(false);
#undef MZ_NET_ACT
}

static void net_value_launch(mz_handle* h, hipStream_t st, const mz_net* critic, const float* obs_dev, const float* final_obs_dev,
                             const uint8_t* done_dev, float* values_dev, const mz_context* ctx) {
  const int rows = 256 / MZ_POLICY_LANES;
  const mzp_norm nm = ctx_norm(h, ctx);
#define MZ_NET_VALUE(NRM)                                                                                                                        \
  hipLaunchKernelGGL(net_value_kernel<NRM>, dim3((unsigned)((h->n + rows - 1) / rows)), dim3(256), 0, st, h->n, h->model.obs_dim, net_shape(critic), \
                     critic->params_dev, (long)critic->env_stride, obs_dev, final_obs_dev, done_dev, values_dev, nm)
  if (nm.mean) MZ_NET_VALUE(true); else MZ_NET_VALUE(false);
#undef MZ_NET_VALUE
}

static void net_sample_head_launch(mz_handle* h, hipStream_t st, const mz_net* actor, const mz_head* head, float logA, uint64_t noise_seed,
                                   uint64_t noise_step, const float* obs_dev, float* actions_dev, float* logp_dev,
                                   const mz_context* ctx = nullptr);

// One launch of the tiled kernel (mz_net_tile.h): the rows, the normaliser and the context of the group kernels' launches — ctx_norm,
// so a context without a bound normaliser goes through the identity here too —, a tile of MZT_ROWS rows per block.
static mzt_job tile_job(mz_handle* h, int kind, const mz_net* net, const mz_context* ctx, const float* obs_dev) {
  const mzp_norm nm = ctx_norm(h, ctx);
  mzt_job J{};
  J.kind = kind; J.n = h->n; J.obs_dim = h->model.obs_dim; J.cdim = nm.cdim; J.nu = h->model.nu;
  J.s = net_shape(net); J.squash = net->squash; J.action_scale = (float)net->action_scale; J.mode = MZ_NOISE_PRE_SQUASH;
  J.params = net->params_dev; J.pstride = (long)net->env_stride; J.env0 = h->env0;
  J.obs = obs_dev; J.mean = nm.mean; J.inv_std = nm.inv_std; J.clip = nm.clip; J.ctx = nm.ctx;
  return J;
}
static void tile_launch(mz_handle* h, hipStream_t st, const mzt_job& J) {
  hipLaunchKernelGGL(net_tile_kernel, dim3((unsigned)((h->n + MZT_ROWS - 1) / MZT_ROWS)), dim3(MZT_THREADS), 0, st, J);
}

// The three launches of an mz_net entry, each on the kernel family net_tiled names for the network: net_act_launch /
// net_sample_head_launch / net_value_launch with the same arguments, or the tiled kernel.
static void net_act_run(mz_handle* h, hipStream_t st, const mz_net* actor, int sample, uint64_t noise_seed, uint64_t noise_step,
                        const float* obs_dev, float* actions_dev, float* logp_dev, int noise_mode = MZ_NOISE_PRE_SQUASH,
                        const mz_context* ctx = nullptr) {
  if (!net_tiled(h, actor)) return net_act_launch(h, st, actor, sample, noise_seed, noise_step, obs_dev, actions_dev, logp_dev, noise_mode, ctx);
  mzt_job J = tile_job(h, sample ? MZT_SAMPLE : MZT_ACT, actor, ctx, obs_dev);
  J.mode = noise_mode; J.key = sample ? mzp_noise_key(noise_seed, noise_step) : 0;
  J.actions = actions_dev; J.logp = sample ? logp_dev : NULL;
  tile_launch(h, st, J);
}
static void net_head_run(mz_handle* h, hipStream_t st, const mz_net* actor, const mz_head* head, float logA, uint64_t noise_seed,
                         uint64_t noise_step, const float* obs_dev, float* actions_dev, float* logp_dev, const mz_context* ctx = nullptr) {
  if (!net_tiled(h, actor)) return net_sample_head_launch(h, st, actor, head, logA, noise_seed, noise_step, obs_dev, actions_dev, logp_dev, ctx);
  mzt_job J = tile_job(h, MZT_HEAD, actor, ctx, obs_dev);
  J.hd = mzp_head{head->log_std_min, head->log_std_max, head->logp_squashed, logA};
  J.key = mzp_noise_key(noise_seed, noise_step);
  J.actions = actions_dev; J.logp = logp_dev;
  tile_launch(h, st, J);
}
static void net_value_run(mz_handle* h, hipStream_t st, const mz_net* critic, const float* obs_dev, const float* final_obs_dev,
                          const uint8_t* done_dev, float* values_dev, const mz_context* ctx = nullptr) {
  if (!net_tiled(h, critic)) return net_value_launch(h, st, critic, obs_dev, final_obs_dev, done_dev, values_dev, ctx);
  mzt_job J = tile_job(h, MZT_VALUE, critic, ctx, obs_dev);
  J.final_obs = final_obs_dev; J.done = done_dev; J.values = values_dev;
  tile_launch(h, st, J);
}

int32_t mz_net_act(mz_handle* h, const mz_net* actor, int32_t sample, uint64_t noise_seed, uint64_t noise_step, const float* obs_dev,
                   float* actions_dev, float* logp_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (sample != 0 && sample != 1) return set_err(h, MZ_ERR_ARG, "mz_net_act: sample must be 0 or 1", hipSuccess);
  if (!obs_dev || !actions_dev) return set_err(h, MZ_ERR_ARG, "mz_net_act: null array", hipSuccess);
  const int rc = net_args(h, "mz_net_act", "actor", actor, h->model.nu, sample != 0, false);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  net_act_run(h, (hipStream_t)stream, actor, sample, noise_seed, noise_step, obs_dev, actions_dev, logp_dev);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

int32_t mz_net_value(mz_handle* h, const mz_net* critic, const float* obs_dev, float* values_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!obs_dev || !values_dev) return set_err(h, MZ_ERR_ARG, "mz_net_value: null array", hipSuccess);
  const int rc = net_args(h, "mz_net_value", "critic", critic, 1, false, true);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  net_value_run(h, (hipStream_t)stream, critic, obs_dev, NULL, NULL, values_dev);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// the checks mz_net_sample and mz_rollout_ex share; MZ_OK or MZ_ERR_ARG with the message set
static int noise_args(mz_handle* h, const char* who, const mz_noise* noise) {
  char msg[160];
  const char* why = nullptr;
  if (noise->struct_size != sizeof(mz_noise)) why = "noise->struct_size must be sizeof(mz_noise)";
  else if (noise->mode != MZ_NOISE_PRE_SQUASH && noise->mode != MZ_NOISE_ACTION) why = "noise->mode must be MZ_NOISE_PRE_SQUASH (0) or MZ_NOISE_ACTION (1)";
  if (!why) return MZ_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
}

// mz_net_act with sample == 1 and the noise of `noise`, mode included (include/mazestep.h)
int32_t mz_net_sample(mz_handle* h, const mz_net* actor, const mz_noise* noise, const float* obs_dev, float* actions_dev, float* logp_dev,
                      void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!noise) return set_err(h, MZ_ERR_ARG, "mz_net_sample: noise is NULL", hipSuccess);
  if (!obs_dev || !actions_dev) return set_err(h, MZ_ERR_ARG, "mz_net_sample: null array", hipSuccess);
  int rc = noise_args(h, "mz_net_sample", noise);
  if (rc != MZ_OK) return rc;
  rc = net_args(h, "mz_net_sample", "actor", actor, h->model.nu, true, false);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  net_act_run(h, (hipStream_t)stream, actor, 1, noise->seed, noise->step, obs_dev, actions_dev, logp_dev, noise->mode);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// the checks mz_net_sample_head and mz_rollout_head share, on a head that is not NULL: the struct, then what it asks of the actor and
// the noise (both may be NULL here: a head samples).  MZ_OK, MZ_ERR_ARG or MZ_ERR_UNSUPPORTED with the message set.
static int head_args(mz_handle* h, const char* who, const mz_head* head, const mz_net* actor, const mz_noise* noise, bool in_io) {
  char msg[200];
  const char* why = nullptr;
  int code = MZ_ERR_ARG;
  if (head->struct_size != sizeof(mz_head)) why = "head->struct_size must be sizeof(mz_head)";
  else if (head->kind != MZ_HEAD_STATE_STD) why = "head->kind must be MZ_HEAD_STATE_STD (1)";
  else if (head->reserved != 0) why = "head->reserved must be 0";
  else if (head->logp_squashed != 0 && head->logp_squashed != 1) why = "head->logp_squashed must be 0 or 1";
  else if (head->log_std_min != head->log_std_min || head->log_std_max != head->log_std_max) why = "head->log_std_min / log_std_max must not be NaN";
  else if (head->log_std_min > head->log_std_max) why = "head->log_std_min must not exceed head->log_std_max";
  else if (!actor) why = in_io ? "a head needs an actor: io->actor is NULL" : "a head needs an actor: actor is NULL";
  else if (!noise) why = in_io ? "a head samples: io->noise is NULL" : "a head samples: noise is NULL";
  else if (noise->struct_size == sizeof(mz_noise) && noise->mode != MZ_NOISE_PRE_SQUASH) why = "noise->mode must be MZ_NOISE_PRE_SQUASH (0) with a head";
  else if (head->logp_squashed && actor->struct_size == sizeof(mz_net) && actor->squash == 0) why = "head->logp_squashed needs actor->squash == 1";
  else if (h->model.nu > MZ_POLICY_MAX_HIDDEN) { why = "a head needs nu <= MZ_POLICY_MAX_HIDDEN (64)"; code = MZ_ERR_UNSUPPORTED; }
  if (!why) return MZ_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_err(h, code, msg, hipSuccess);
}

static void net_sample_head_launch(mz_handle* h, hipStream_t st, const mz_net* actor, const mz_head* head, float logA, uint64_t noise_seed,
                                   uint64_t noise_step, const float* obs_dev, float* actions_dev, float* logp_dev, const mz_context* ctx) {
  const int rows = 256 / MZ_POLICY_LANES;
  const mzp_norm nm = ctx_norm(h, ctx);
  const mzp_head hd{head->log_std_min, head->log_std_max, head->logp_squashed, logA};
#define MZ_NET_HEAD(NRM)                                                                                                                          \
  hipLaunchKernelGGL(net_sample_head_kernel<NRM>, dim3((unsigned)((h->n + rows - 1) / rows)), dim3(256), 0, st, h->n, h->model.obs_dim, h->model.nu, \
                     net_shape(actor), actor->squash, (float)actor->action_scale, hd, actor->params_dev, (long)actor->env_stride,                  \
                     mzp_noise_key(noise_seed, noise_step), h->env0, obs_dev, actions_dev, logp_dev, nm)
  if (nm.mean) MZ_NET_HEAD(true); else MZ_NET_HEAD(false);
#undef MZ_NET_HEAD
}

// mz_net_sample for an actor with a state-dependent log-std head (include/mazestep.h); head == NULL: mz_net_sample itself
int32_t mz_net_sample_head(mz_handle* h, const mz_net* actor, const mz_head* head, const mz_noise* noise, const float* obs_dev,
                           float* actions_dev, float* logp_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!head) return mz_net_sample(h, actor, noise, obs_dev, actions_dev, logp_dev, stream);
  if (!obs_dev || !actions_dev) return set_err(h, MZ_ERR_ARG, "mz_net_sample_head: null array", hipSuccess);
  int rc = head_args(h, "mz_net_sample_head", head, actor, noise, false);
  if (rc != MZ_OK) return rc;
  rc = noise_args(h, "mz_net_sample_head", noise);
  if (rc != MZ_OK) return rc;
  rc = net_args(h, "mz_net_sample_head", "actor", actor, h->model.nu, true, false, true);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  net_head_run(h, (hipStream_t)stream, actor, head, logf((float)actor->action_scale), noise->seed, noise->step, obs_dev, actions_dev, logp_dev);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// ------------------------------------------------------------------ rollouts: six entries, one plan (mz_internal.h), one driver
// row k of next_obs_seq_dev on a handle that steps launch by launch: behind the step's launches, before anything overwrites obs_dev or
// the final_obs row (the caller has checked that final_obs is bound under auto-reset)
static hipError_t next_obs_row(mz_handle* h, hipStream_t st, const float* obs_dev, const uint8_t* done_dev, float* out) {
  const size_t tot = (size_t)h->n * h->model.obs_dim;
  if (!h->auto_reset) return hipMemcpyAsync(out, obs_dev, tot * sizeof(float), hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(next_obs_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->n, h->model.obs_dim, obs_dev, h->final_obs, done_dev, out);
  return hipGetLastError();
}

// the plan's actor on the rows of obs_dev into `actions`, with the noise of step k: the kernels of mzk_rollout_kernels' loop column
static void rollout_act_launch(mz_handle* h, hipStream_t st, const RolloutPlan& p, bool one_layer, size_t k, float* actions) {
  const mz_net* a = p.actor;
  float* logp = p.logp_seq_dev ? p.logp_seq_dev + k * (size_t)h->n : NULL;
  // (a plan of an entry that takes an int `hidden` stays on the group kernels in every mode of "wide_nets")
  if (p.head) net_head_run(h, st, a, p.head, p.head_logA, p.noise_seed, p.noise_step + k, p.obs_dev, actions, logp, p.ctx);
  else if (p.legacy && !one_layer) net_act_launch(h, st, a, p.sample, p.noise_seed, p.noise_step + k, p.obs_dev, actions, logp, p.noise_mode, p.ctx);
  else if (!one_layer) net_act_run(h, st, a, p.sample, p.noise_seed, p.noise_step + k, p.obs_dev, actions, logp, p.noise_mode, p.ctx);
  else if (p.sample)
    policy_sample_launch(h, st, a->params_dev, a->env_stride, a->hidden[0], a->squash, (float)a->action_scale, p.noise_seed, p.noise_step + k, p.obs_dev,
                         actions, logp);
  else policy_act_launch(h, st, a->params_dev, a->env_stride, a->hidden[0], a->squash, (float)a->action_scale, p.obs_dev, actions);
}

// the plan's critic on the rows of obs_dev — the final_obs row where done (both NULL: every row from obs_dev) — likewise
static void rollout_value_launch(mz_handle* h, hipStream_t st, const RolloutPlan& p, bool one_layer, const float* final_obs_dev,
                                 const uint8_t* done_dev, float* values_dev) {
  const mz_net* c = p.critic;
  if (one_layer) value_launch(h, st, c->params_dev, c->env_stride, c->hidden[0], p.obs_dev, final_obs_dev, done_dev, values_dev);
  else if (p.legacy) net_value_launch(h, st, c, p.obs_dev, final_obs_dev, done_dev, values_dev, p.ctx);
  else net_value_run(h, st, c, p.obs_dev, final_obs_dev, done_dev, values_dev, p.ctx);
}

// The driver behind every rollout entry: n_steps times [a = the plan's actor on obs, or row k of its action tensor]; step(a) in one
// call (include/mazestep.h).  Fused handles (mzk_planar_rollout_fused) advance up to MZ_ROLLOUT_CHUNK steps per launch on a state that
// stays on chip and evaluate the networks inside the kernels; the record then gets the last step's row from one launch behind them.
// Every other handle runs the defining loop itself with the output pointers advanced, which is sequential stepping by construction:
//   [value of obs] -> actor -> the step's own launches (mzk_view_fill among them: the view entries of both rows are in place)
//   -> [next value: of the final_obs row where the env finished under auto-reset] -> [next_obs_row] -> [obs_seq copy]
// with the actions in row k of actions_seq_dev, or in the handle's scratch.  Which kernels evaluate the networks: mzk_rollout_kernels.
// The entry has checked the plan.
static int32_t rollout_run(mz_handle* h, const RolloutPlan& plan, void* stream) {
  RolloutPlan p = plan;
  if (!p.critic) p.value_seq_dev = p.next_value_seq_dev = NULL;
  if (!p.sample) p.logp_seq_dev = NULL;
  const size_t n = (size_t)h->n, od = (size_t)h->model.obs_dim, nu = (size_t)h->model.nu;
  DeviceScope scope(h->device);
  hipStream_t st = (hipStream_t)stream;
  // A six-link chain's closed-loop plans run the defining loop below: swimmer_policy_rollout_kernel<6, 0, 8, ...> needs all 512 registers
  // and spills on top of them, and two of its instantiations — (CRT, DEEP, EXT) and (SMP, CRT, DEEP, NRM, EXT) — leave the loop behind
  // the first step (tests/test_gpu_planar_ladder.py found it; the cause is not known, the source is the five-link kernel's, which agrees
  // by bits).  Its open-loop kernel and every kernel of the shorter chains agree with stepping by bits and stay fused.
  const bool six_link_policy = p.actor && h->robot == MZ_ROBOT_SWIMMER && h->swimmer.nlink == 6;
  // A head plan on a five- or six-link chain runs the loop too: their fused kernels compile without the head's branch (planar_kernels.hip).
  const bool long_chain_head = p.head && h->robot == MZ_ROBOT_SWIMMER && h->swimmer.nlink >= 5;
  // A plan with a context runs the loop on every handle: the fused kernels do not stage one.
  // So does a plan in which the actor or the critic runs the tiled kernel (option "wide_nets"): the fused kernels hold no wide rows.
  const bool tiled = !p.legacy && ((p.actor && net_tiled(h, p.actor)) || (p.critic && net_tiled(h, p.critic)));
  if (mzk_planar_rollout_fused(h) && !six_link_policy && !long_chain_head && !p.ctx && !tiled) {
    HIPCHK(h, mzk_planar_rollout(h, st, p));
    if (h->record) {  // the last step's row
      const size_t tot = n * (od + 2), last = (size_t)(p.n_steps - 1) * n;
      hipLaunchKernelGGL(pack_record_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->n, h->model.obs_dim, p.obs_dev, p.reward_dev + last, p.done_dev + last, h->record);
      HIPCHK(h, hipGetLastError());
    }
  } else {
    const bool one_layer = !p.ctx && mzk_rollout_kernels(h, p).one_layer;  // a context rides on the net kernels' NRM instantiations
    const mz_context* cx = p.ctx;
    const int D = cx && cx->update == MZ_CTX_RELATIVE ? cx->rel_dims : 0;
    if (p.actor && !p.actions_seq_dev && !h->policy_act) HIPCHK(h, hipMalloc(&h->policy_act, n * nu * sizeof(float)));
    for (size_t k = 0; k < (size_t)p.n_steps; k++) {
      uint8_t* done_k = p.done_dev + k * n;
      const float* a;
      if (p.actor) {
        float* out = p.actions_seq_dev ? p.actions_seq_dev + k * n * nu : h->policy_act;
        if (cx && cx->ctx_seq_dev)  // the context the networks read at step k
          HIPCHK(h, hipMemcpyAsync(cx->ctx_seq_dev + k * n * cx->dim, cx->ctx_dev, n * cx->dim * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (D)  // the D old columns of the raw row the actor acts on, which the step overwrites
          HIPCHK(h, hipMemcpy2DAsync(h->ctx_old, D * sizeof(float), p.obs_dev, od * sizeof(float), D * sizeof(float), n, hipMemcpyDeviceToDevice, st));
        if (p.value_seq_dev) rollout_value_launch(h, st, p, one_layer, NULL, NULL, p.value_seq_dev + k * n);
        rollout_act_launch(h, st, p, one_layer, k, out);
        HIPCHK(h, hipGetLastError());
        a = out;
      } else {
        a = p.actions_dev + k * (size_t)p.action_step_stride;
      }
      const int rc = step_launches(h, st, a, p.obs_dev, p.reward_dev + k * n, done_k, p.goal_idx_dev ? p.goal_idx_dev + k * n : NULL,
                                   p.info_dev ? p.info_dev + k * n * 4 : NULL);
      if (rc != MZ_OK) return rc;
      if (D) {  // before the next value, which reads the context after the transition
        hipLaunchKernelGGL(ctx_transition_kernel, dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, st, h->n, cx->dim, D, h->model.obs_dim, h->ctx_old,
                           p.obs_dev, done_k, cx->ctx_dev);
        HIPCHK(h, hipGetLastError());
      }
      if (p.next_value_seq_dev) {
        rollout_value_launch(h, st, p, one_layer, h->auto_reset ? h->final_obs : NULL, h->auto_reset ? done_k : NULL, p.next_value_seq_dev + k * n);
        HIPCHK(h, hipGetLastError());
      }
      if (p.next_obs_seq_dev) HIPCHK(h, next_obs_row(h, st, p.obs_dev, done_k, p.next_obs_seq_dev + k * n * od));
      if (p.obs_seq_dev) HIPCHK(h, hipMemcpyAsync(p.obs_seq_dev + k * n * od, p.obs_dev, n * od * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
  }
  h->nsteps += p.n_steps;
  return MZ_OK;
}

// a plan with what every entry has: its name, the step count and the outputs of mz_rollout; everything else zero
static RolloutPlan rollout_plan(const char* who, int32_t n_steps, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev,
                                float* info_dev, float* obs_seq_dev) {
  RolloutPlan p{};
  p.who = who; p.n_steps = n_steps; p.noise_mode = MZ_NOISE_PRE_SQUASH;
  p.obs_dev = obs_dev; p.reward_dev = reward_dev; p.done_dev = done_dev; p.goal_idx_dev = goal_idx_dev; p.info_dev = info_dev; p.obs_seq_dev = obs_seq_dev;
  return p;
}

// the two checks every entry makes, each at its own place among the entry's other checks — the first message of a refused call is
// part of the interface —, under the name of the entry the call stands for
static int rollout_args(mz_handle* h, const RolloutPlan& p) {
  char msg[96];
  const char* why = nullptr;
  if (!p.obs_dev || !p.reward_dev || !p.done_dev) why = "null array";
  else if (p.n_steps < 1 || p.n_steps > 65536) why = "n_steps must be 1 .. 65536";
  if (!why) return MZ_OK;
  snprintf(msg, sizeof(msg), "%s: %s", p.who, why);
  return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
}

// what mz_rollout refuses, on its plan (mz_rollout_ex with a tensor of actions stands for it)
static int open_loop_args(mz_handle* h, const RolloutPlan& p) {
  if (!p.actions_dev) return set_err(h, MZ_ERR_ARG, "mz_rollout: null array", hipSuccess);
  const int rc = rollout_args(h, p);
  if (rc != MZ_OK) return rc;
  if (p.action_step_stride != 0 && p.action_step_stride != (long)h->n * h->model.nu)
    return set_err(h, MZ_ERR_ARG, "mz_rollout: action_step_stride must be num_envs * nu ([K, N, nu] actions) or 0 (one [N, nu] block repeated)", hipSuccess);
  return MZ_OK;
}

// what mz_rollout_net refuses, on its plan (mz_rollout_ex with an actor stands for it)
static int net_rollout_args(mz_handle* h, const RolloutPlan& p) {
  if (p.sample != 0 && p.sample != 1) return set_err(h, MZ_ERR_ARG, "mz_rollout_net: sample must be 0 or 1", hipSuccess);
  int rc = rollout_args(h, p);
  if (rc != MZ_OK) return rc;
  const int cdim = p.ctx ? p.ctx->dim : 0;
  rc = net_args(h, p.who, "actor", p.actor, h->model.nu, p.sample != 0, false, p.head != nullptr, cdim);
  if (rc != MZ_OK || !p.critic) return rc;
  rc = net_args(h, p.who, "critic", p.critic, 1, false, true, false, cdim);
  if (rc != MZ_OK) return rc;
  if (p.next_value_seq_dev && h->auto_reset && !h->final_obs)
    return set_err(h, MZ_ERR_ARG, "mz_rollout_net: next_value_seq_dev under auto-reset needs a bound final_obs buffer (mz_bind_final_obs): "
                                  "the terminal rows are valued there", hipSuccess);
  return MZ_OK;
}

// The three entries that take an int `hidden`: their checks under the name `who`, then the plan with both networks as legacy_net's.
// mz_rollout_policy is sample = 0 without a critic, mz_rollout_policy_sample sample = 1 without one.
static int32_t rollout_legacy(mz_handle* h, const char* who, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden,
                              int32_t squash, double action_scale, int32_t sample, uint64_t noise_seed, uint64_t noise_step, const mz_critic* critic,
                              float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev,
                              float* actions_seq_dev, float* logp_seq_dev, void* stream) {
  RolloutPlan p = rollout_plan(who, n_steps, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev, obs_seq_dev);
  int rc = rollout_args(h, p);
  if (rc != MZ_OK) return rc;
  rc = policy_args(h, who, params_dev, param_env_stride, hidden, squash, sample != 0);
  if (rc != MZ_OK) return rc;
  const mz_net a = legacy_net(params_dev, param_env_stride, hidden, squash, action_scale);
  mz_net c{};
  if (critic) {
    if (critic->reserved != 0) return set_err(h, MZ_ERR_ARG, "mz_rollout_actor_critic: critic->reserved must be 0", hipSuccess);
    rc = critic_args(h, who, critic->params_dev, critic->env_stride, critic->hidden);
    if (rc != MZ_OK) return rc;
    if (critic->next_value_seq_dev && h->auto_reset && !h->final_obs)
      return set_err(h, MZ_ERR_ARG, "mz_rollout_actor_critic: critic->next_value_seq_dev under auto-reset needs a bound final_obs buffer "
                                    "(mz_bind_final_obs): the terminal rows are valued there", hipSuccess);
    c = legacy_net(critic->params_dev, critic->env_stride, critic->hidden, 0, 1.0);
    p.critic = &c; p.value_seq_dev = critic->value_seq_dev; p.next_value_seq_dev = critic->next_value_seq_dev;
  }
  p.legacy = 1;
  p.actor = &a; p.sample = sample; p.noise_seed = noise_seed; p.noise_step = noise_step;
  p.actions_seq_dev = actions_seq_dev; p.logp_seq_dev = logp_seq_dev;
  return rollout_run(h, p, stream);
}

int32_t mz_rollout(mz_handle* h, int32_t n_steps, const float* actions_dev, int64_t action_step_stride, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  RolloutPlan p = rollout_plan("mz_rollout", n_steps, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev, obs_seq_dev);
  p.actions_dev = actions_dev; p.action_step_stride = (long)action_step_stride;
  const int rc = open_loop_args(h, p);
  return rc != MZ_OK ? rc : rollout_run(h, p, stream);
}

int32_t mz_rollout_policy(mz_handle* h, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash,
                          double action_scale, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev,
                          float* obs_seq_dev, float* actions_seq_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  return rollout_legacy(h, "mz_rollout_policy", n_steps, params_dev, param_env_stride, hidden, squash, action_scale, 0, 0, 0, NULL, obs_dev, reward_dev,
                        done_dev, goal_idx_dev, info_dev, obs_seq_dev, actions_seq_dev, NULL, stream);
}

int32_t mz_rollout_policy_sample(mz_handle* h, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash,
                                 double action_scale, uint64_t noise_seed, uint64_t noise_step, float* obs_dev, float* reward_dev,
                                 uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev, float* actions_seq_dev,
                                 float* logp_seq_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  return rollout_legacy(h, "mz_rollout_policy_sample", n_steps, params_dev, param_env_stride, hidden, squash, action_scale, 1, noise_seed, noise_step,
                        NULL, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev, obs_seq_dev, actions_seq_dev, logp_seq_dev, stream);
}

// without a critic the call IS mz_rollout_policy_sample / mz_rollout_policy (include/mazestep.h), down to the name in a refusal
int32_t mz_rollout_actor_critic(mz_handle* h, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash,
                                double action_scale, int32_t sample, uint64_t noise_seed, uint64_t noise_step, const mz_critic* critic,
                                float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev,
                                float* actions_seq_dev, float* logp_seq_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (sample != 0 && sample != 1) return set_err(h, MZ_ERR_ARG, "mz_rollout_actor_critic: sample must be 0 or 1", hipSuccess);
  const char* who = critic ? "mz_rollout_actor_critic" : (sample ? "mz_rollout_policy_sample" : "mz_rollout_policy");
  return rollout_legacy(h, who, n_steps, params_dev, param_env_stride, hidden, squash, action_scale, sample, noise_seed, noise_step, critic, obs_dev,
                        reward_dev, done_dev, goal_idx_dev, info_dev, obs_seq_dev, actions_seq_dev, logp_seq_dev, stream);
}

int32_t mz_rollout_net(mz_handle* h, int32_t n_steps, const mz_net* actor, int32_t sample, uint64_t noise_seed, uint64_t noise_step,
                       const mz_net* critic, float* value_seq_dev, float* next_value_seq_dev, float* obs_dev, float* reward_dev,
                       uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev, float* actions_seq_dev,
                       float* logp_seq_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  RolloutPlan p = rollout_plan("mz_rollout_net", n_steps, obs_dev, reward_dev, done_dev, goal_idx_dev, info_dev, obs_seq_dev);
  p.actor = actor; p.sample = sample; p.noise_seed = noise_seed; p.noise_step = noise_step;
  p.critic = critic; p.value_seq_dev = value_seq_dev; p.next_value_seq_dev = next_value_seq_dev;
  p.actions_seq_dev = actions_seq_dev; p.logp_seq_dev = logp_seq_dev;
  const int rc = net_rollout_args(h, p);
  return rc != MZ_OK ? rc : rollout_run(h, p, stream);
}

// mz_rollout / mz_rollout_net behind one struct, with the per-step pre-reset rows and the noise mode (include/mazestep.h).  The
// checks here are those the struct adds; everything else is refused as by the entry the call stands for, whose plan it fills.
static int32_t rollout_ex(mz_handle* h, const mz_rollout_io* io, const mz_head* head, void* stream, const mz_context* ctx = nullptr);
int32_t mz_rollout_ex(mz_handle* h, const mz_rollout_io* io, void* stream) { return rollout_ex(h, io, NULL, stream); }
// mz_rollout_ex with a state-dependent log-std head on the actor (include/mazestep.h); head == NULL: mz_rollout_ex itself
int32_t mz_rollout_head(mz_handle* h, const mz_rollout_io* io, const mz_head* head, void* stream) { return rollout_ex(h, io, head, stream); }

// the checks of a context that is not NULL (rollout: MZ_CTX_RELATIVE and ctx_seq_dev are the rollout's); MZ_OK or MZ_ERR_ARG with the
// message set
static int ctx_args(mz_handle* h, const char* who, const mz_context* ctx, bool rollout) {
  char msg[200];
  const char* why = nullptr;
  const int dmax = ctx->dim < h->model.obs_dim ? ctx->dim : h->model.obs_dim;
  if (ctx->struct_size != sizeof(mz_context)) why = "ctx->struct_size must be sizeof(mz_context)";
  else if (ctx->dim < 1 || ctx->dim > MZ_MAX_CONTEXT) why = "ctx->dim must be 1 .. MZ_MAX_CONTEXT (32)";
  else if (ctx->update != MZ_CTX_HOLD && ctx->update != MZ_CTX_RELATIVE) why = "ctx->update must be MZ_CTX_HOLD (0) or MZ_CTX_RELATIVE (1)";
  else if (ctx->update == MZ_CTX_HOLD && ctx->rel_dims != 0) why = "ctx->rel_dims must be 0 with MZ_CTX_HOLD";
  else if (ctx->update == MZ_CTX_RELATIVE && !rollout) why = "ctx->update must be MZ_CTX_HOLD in a single call: a transition needs a step";
  else if (ctx->update == MZ_CTX_RELATIVE && (ctx->rel_dims < 1 || ctx->rel_dims > dmax)) why = "ctx->rel_dims must be 1 .. min(ctx->dim, obs_dim) with MZ_CTX_RELATIVE";
  else if (ctx->reserved != 0) why = "ctx->reserved must be 0";
  else if (!ctx->ctx_dev) why = "ctx->ctx_dev is NULL";
  else if (ctx->ctx_seq_dev && !rollout) why = "ctx->ctx_seq_dev must be NULL in a single call";
  if (!why) return MZ_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
}

// mz_net_act / mz_net_sample / mz_net_sample_head on the rows [obs | ctx] (include/mazestep.h); ctx == NULL: those calls themselves
int32_t mz_net_eval_ctx(mz_handle* h, const mz_net* actor, const mz_head* head, const mz_noise* noise, const mz_context* ctx,
                        const float* obs_dev, float* actions_dev, float* logp_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!ctx) {
    if (head) return mz_net_sample_head(h, actor, head, noise, obs_dev, actions_dev, logp_dev, stream);
    if (noise) return mz_net_sample(h, actor, noise, obs_dev, actions_dev, logp_dev, stream);
    return mz_net_act(h, actor, 0, 0, 0, obs_dev, actions_dev, NULL, stream);
  }
  const char* who = "mz_net_eval_ctx";
  if (!obs_dev || !actions_dev) return set_err(h, MZ_ERR_ARG, "mz_net_eval_ctx: null array", hipSuccess);
  int rc = ctx_args(h, who, ctx, false);
  if (rc != MZ_OK) return rc;
  if (head) {
    rc = head_args(h, who, head, actor, noise, false);
    if (rc != MZ_OK) return rc;
  }
  if (noise) {
    rc = noise_args(h, who, noise);
    if (rc != MZ_OK) return rc;
  }
  rc = net_args(h, who, "actor", actor, h->model.nu, noise != nullptr, false, head != nullptr, ctx->dim);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  rc = ctx_prepare(h, ctx);
  if (rc != MZ_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (head) net_head_run(h, st, actor, head, logf((float)actor->action_scale), noise->seed, noise->step, obs_dev, actions_dev, logp_dev, ctx);
  else if (noise) net_act_run(h, st, actor, 1, noise->seed, noise->step, obs_dev, actions_dev, logp_dev, noise->mode, ctx);
  else net_act_run(h, st, actor, 0, 0, 0, obs_dev, actions_dev, NULL, MZ_NOISE_PRE_SQUASH, ctx);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// mz_net_value on the rows [obs | ctx]; ctx == NULL: mz_net_value itself
int32_t mz_net_value_ctx(mz_handle* h, const mz_net* critic, const mz_context* ctx, const float* obs_dev, float* values_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!ctx) return mz_net_value(h, critic, obs_dev, values_dev, stream);
  if (!obs_dev || !values_dev) return set_err(h, MZ_ERR_ARG, "mz_net_value_ctx: null array", hipSuccess);
  int rc = ctx_args(h, "mz_net_value_ctx", ctx, false);
  if (rc != MZ_OK) return rc;
  rc = net_args(h, "mz_net_value_ctx", "critic", critic, 1, false, true, false, ctx->dim);
  if (rc != MZ_OK) return rc;
  DeviceScope scope(h->device);
  rc = ctx_prepare(h, ctx);
  if (rc != MZ_OK) return rc;
  net_value_run(h, (hipStream_t)stream, critic, obs_dev, NULL, NULL, values_dev, ctx);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// mz_rollout_head with a context (include/mazestep.h); ctx == NULL: mz_rollout_head itself
int32_t mz_rollout_ctx(mz_handle* h, const mz_rollout_io* io, const mz_head* head, const mz_context* ctx, void* stream) {
  return rollout_ex(h, io, head, stream, ctx);
}

static int32_t rollout_ex(mz_handle* h, const mz_rollout_io* io, const mz_head* head, void* stream, const mz_context* ctx) {
  if (!h) return MZ_ERR_ARG;
  // a refusal names the entry the caller used: with a head that is mz_rollout_head, for the io-level checks and for the plan's
  const char* who = ctx ? "mz_rollout_ctx" : head ? "mz_rollout_head" : "mz_rollout_ex";
  auto fail = [&](const char* why) {
    char msg[224];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return set_err(h, MZ_ERR_ARG, msg, hipSuccess);
  };
  if (!io) return fail("io is NULL");
  if (io->struct_size != sizeof(mz_rollout_io)) return fail("io->struct_size must be sizeof(mz_rollout_io)");
  if (io->actions_dev && io->actor) return fail("both io->actions_dev and io->actor are given: exactly one is the action source");
  if (!io->actions_dev && !io->actor) return fail("neither io->actions_dev nor io->actor is given: exactly one is the action source");
  if (!io->actor && io->noise) return fail("io->noise without io->actor");
  if (!io->actor && io->critic) return fail("io->critic without io->actor");
  if (ctx) {
    if (!io->actor) return fail("a context needs io->actor: an open-loop rollout evaluates no network");
    const int rc = ctx_args(h, who, ctx, true);
    if (rc != MZ_OK) return rc;
  }
  if (head) {
    const int rc = head_args(h, who, head, io->actor, io->noise, true);
    if (rc != MZ_OK) return rc;
  }
  if (io->noise) {
    const int rc = noise_args(h, who, io->noise);
    if (rc != MZ_OK) return rc;
  }
  if (io->next_obs_seq_dev && h->auto_reset && !h->final_obs)
    return fail("next_obs_seq_dev under auto-reset needs a bound final_obs buffer (mz_bind_final_obs): the contract is the same on every handle");
  RolloutPlan p = rollout_plan(head || ctx ? who : (io->actor ? "mz_rollout_net" : "mz_rollout"), io->n_steps, io->obs_dev, io->reward_dev, io->done_dev,
                               io->goal_idx_dev, io->info_dev, io->obs_seq_dev);
  p.next_obs_seq_dev = io->next_obs_seq_dev;
  if (!io->actor) {
    p.actions_dev = io->actions_dev; p.action_step_stride = (long)io->action_step_stride;
  } else {
    p.actor = io->actor; p.critic = io->critic; p.value_seq_dev = io->value_seq_dev; p.next_value_seq_dev = io->next_value_seq_dev;
    p.actions_seq_dev = io->actions_seq_dev; p.logp_seq_dev = io->logp_seq_dev;
    if (io->noise) { p.sample = 1; p.noise_seed = io->noise->seed; p.noise_step = io->noise->step; p.noise_mode = io->noise->mode; }
    if (head) { p.head = head; p.head_logA = logf((float)io->actor->action_scale); }
  }
  p.ctx = ctx;
  int rc = io->actor ? net_rollout_args(h, p) : open_loop_args(h, p);
  if (rc == MZ_OK && ctx) {
    DeviceScope scope(h->device);
    rc = ctx_prepare(h, ctx);
  }
  return rc != MZ_OK ? rc : rollout_run(h, p, stream);
}

int32_t mz_gae(mz_handle* h, int32_t n_steps, const float* reward_dev, const uint8_t* done_dev, const float* value_dev,
               const float* next_value_dev, double gamma, double lam, float* adv_dev, float* ret_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!reward_dev || !done_dev || !value_dev || !next_value_dev || !adv_dev) return set_err(h, MZ_ERR_ARG, "mz_gae: null array", hipSuccess);
  if (n_steps < 1 || n_steps > 65536) return set_err(h, MZ_ERR_ARG, "mz_gae: n_steps must be 1 .. 65536", hipSuccess);
  float g, gl;
  mzg_coeffs(gamma, lam, &g, &gl);
  DeviceScope scope(h->device);
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((h->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, h->n, n_steps, reward_dev, done_dev, value_dev,
                     next_value_dev, g, gl, adv_dev, ret_dev);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

int32_t mz_return_scan(mz_handle* h, int32_t n_steps, const float* reward_dev, const uint8_t* done_dev, double gamma, float* carry_dev,
                       int32_t* len_carry_dev, float* ret_seq_dev, int32_t* len_seq_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  if (!reward_dev || !done_dev) return set_err(h, MZ_ERR_ARG, "mz_return_scan: null array (reward_dev, done_dev)", hipSuccess);
  if (!carry_dev) return set_err(h, MZ_ERR_ARG, "mz_return_scan: carry_dev is NULL", hipSuccess);
  if (!ret_seq_dev) return set_err(h, MZ_ERR_ARG, "mz_return_scan: ret_seq_dev is NULL", hipSuccess);
  if (len_seq_dev && !len_carry_dev)
    return set_err(h, MZ_ERR_ARG, "mz_return_scan: len_seq_dev without len_carry_dev (a NULL len_carry_dev means the length is not tracked)", hipSuccess);
  if (n_steps < 1 || n_steps > 65536) return set_err(h, MZ_ERR_ARG, "mz_return_scan: n_steps must be 1 .. 65536", hipSuccess);
  DeviceScope scope(h->device);
  hipLaunchKernelGGL(return_scan_kernel, dim3((unsigned)((h->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, h->n, n_steps, reward_dev, done_dev,
                     (float)gamma, carry_dev, len_carry_dev, ret_seq_dev, len_seq_dev);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

// render.render_top_down for `count` env states (include/mazestep.h).  Without a caller's qpos the engine's own get-state kernel
// first copies the batch's qpos into the handle's scratch on the same stream: the images show what mz_get_state would return.
int32_t mz_render(mz_handle* h, const float* qpos_dev, const int32_t* env_idx_dev, int32_t count, int32_t width, int32_t height,
                  int32_t ngoal_style, const uint8_t* goal_rgb, const double* goal_size, uint8_t* rgb_dev, void* stream) {
  if (!h) return MZ_ERR_ARG;
  RenderDev R;
  const char* why = nullptr;
  if (ngoal_style != h->model.ngoal || (ngoal_style > 0 && (!goal_rgb || !goal_size)))
    return set_err(h, MZ_ERR_ARG, "mz_render: ngoal_style must equal the goal table's count, with that many goal_rgb / goal_size rows", hipSuccess);
  const int rc = render_dev_from_model(&h->model, goal_rgb, goal_size, &R, &why);
  if (rc != MZ_OK) {
    snprintf(h->err, sizeof(h->err), "mz_render: %s", why ? why : "unsupported model");
    return rc;
  }
  if (width < 2 || height < 2 || width > 16384 || height > 16384)
    return set_err(h, MZ_ERR_ARG, "mz_render: width and height must be 2 .. 16384 (render.py divides by width - 1 and height - 1)", hipSuccess);
  if (count < 0 || (!env_idx_dev && count > h->n))
    return set_err(h, MZ_ERR_ARG, "mz_render: count must be >= 0, and <= num_envs without env_idx", hipSuccess);
  if (count == 0) return MZ_OK;
  if (!rgb_dev) return set_err(h, MZ_ERR_ARG, "mz_render: null rgb_dev", hipSuccess);
  DeviceScope scope(h->device);
  hipStream_t st = (hipStream_t)stream;
  const float* q = qpos_dev;
  if (!q) {
    if (!h->render_qpos) HIPCHK(h, hipMalloc(&h->render_qpos, (size_t)h->n * h->model.nq * sizeof(float)));
    if (h->robot == MZ_ROBOT_ANT) HIPCHK(h, mzk_ant_get_state(h, st, h->render_qpos, NULL, NULL, NULL));
    else if (h->robot == MZ_ROBOT_GENERIC) HIPCHK(h, mzk_generic_get_state(h, st, h->render_qpos, NULL, NULL, NULL));
    else HIPCHK(h, mzk_planar_get_state(h, st, h->render_qpos, NULL, NULL, NULL));
    q = h->render_qpos;
  }
  HIPCHK(h, mzk_render(h, st, &R, q, qpos_dev ? 0 : 1, env_idx_dev, count, width, height, rgb_dev));
  return MZ_OK;
}

int32_t mz_get_status(mz_handle* h, int32_t* status_dev, void* stream) {
  if (!h || !status_dev) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  hipLaunchKernelGGL(fetch_clear_status_kernel, dim3((h->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->n, h->status, status_dev);
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

int32_t mz_debug_forward(mz_handle* h, const float* actions_dev, float* qacc_dev, int32_t* counts_dev, void* stream) {
  if (!h || !qacc_dev) return MZ_ERR_ARG;
  if (h->robot != MZ_ROBOT_ANT) return set_err(h, MZ_ERR_UNSUPPORTED, "mz_debug_forward: ant only", hipSuccess);
  DeviceScope scope(h->device);
  HIPCHK(h, mzk_ant_forward(h, (hipStream_t)stream, actions_dev, qacc_dev, counts_dev));
  HIPCHK(h, hipGetLastError());
  return MZ_OK;
}

int32_t mz_debug_task_eval(mz_handle* h, int32_t n_rows, const float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev,
                           void* stream) {
  if (!h || n_rows <= 0 || !obs_dev || !reward_dev || !done_dev) return h ? set_err(h, MZ_ERR_ARG, "mz_debug_task_eval: bad arguments", hipSuccess) : MZ_ERR_ARG;
  DeviceScope scope(h->device);
  if (h->robot == MZ_ROBOT_ANT) HIPCHK(h, mzk_ant_task_eval(h, (hipStream_t)stream, n_rows, obs_dev, reward_dev, done_dev, goal_idx_dev));
  else if (h->robot == MZ_ROBOT_GENERIC) HIPCHK(h, mzk_generic_task_eval(h, (hipStream_t)stream, n_rows, obs_dev, reward_dev, done_dev, goal_idx_dev));
  else HIPCHK(h, mzk_planar_task_eval(h, (hipStream_t)stream, n_rows, obs_dev, reward_dev, done_dev, goal_idx_dev));
  return MZ_OK;
}

int32_t mz_debug_detect(mz_handle* h, int32_t n_rows, const double* old_xy_dev, const double* new_xy_dev, int32_t* hit_dev, double* point_dev,
                        double* final_xy_dev, void* stream) {
  if (!h || n_rows <= 0 || !old_xy_dev || !new_xy_dev || !hit_dev || !final_xy_dev)
    return h ? set_err(h, MZ_ERR_ARG, "mz_debug_detect: bad arguments", hipSuccess) : MZ_ERR_ARG;
  if (h->robot != MZ_ROBOT_POINT || h->point.nseg <= 0) return set_err(h, MZ_ERR_UNSUPPORTED, "mz_debug_detect: the manual wall detector exists for the Point only", hipSuccess);
  DeviceScope scope(h->device);
  HIPCHK(h, mzk_point_detect(h, (hipStream_t)stream, n_rows, old_xy_dev, new_xy_dev, hit_dev, point_dev, final_xy_dev));
  return MZ_OK;
}

// Phase timers of the PROF kernel build: copies the 16 accumulators to host memory and clears them.
int32_t mz_read_phase_cycles(mz_handle* h, uint64_t* out16_host) {
  if (!h || !out16_host || !h->prof) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  HIPCHK(h, hipDeviceSynchronize());
  // the step kernels write per-workgroup slots only (no same-address atomics: they disturbed what they measured, ant_kernels.hip);
  // the 16 launch-wide accumulators are reduced here from the per-workgroup phase slots — accumulated since the last
  // mz_read_wave_phase_cycles, which hands those slots out and clears them; this call clears nothing
  const size_t nw = (size_t)h->n;
  unsigned long long* buf = (unsigned long long*)malloc(17 * nw * sizeof(unsigned long long));
  if (!buf) return set_err(h, MZ_ERR_HIP, "mz_read_phase_cycles: out of memory", hipSuccess);
  hipError_t e = hipMemcpy(buf, h->prof + 16, 17 * nw * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { free(buf); return set_err(h, MZ_ERR_HIP, "mz_read_phase_cycles", e); }
  for (int k = 0; k < 16; k++) out16_host[k] = 0;
  for (size_t w = 0; w < nw; w++) {
    const unsigned long long* ph = buf + nw + 16 * w;
    unsigned long long tot = 0;
    for (int k = 0; k < 13; k++) tot += ph[k];
    if (!tot) continue;  // (slots of workgroups that do not exist at this lane width stay empty)
    for (int k = 0; k < 16; k++) if (k != 13 && k != 14) out16_host[k] += ph[k];
    if (tot > out16_host[13]) out16_host[13] = tot;   // slowest workgroup of the window (per-workgroup sums over the window's steps)
    out16_host[14] += (tot >> 8) * (tot >> 8);         // sum of squares of the per-workgroup totals (units of 256 cycles)
  }
  free(buf);
  return MZ_OK;
}

// Per-workgroup totals accumulated by the PROF kernel build since the last call (then cleared): n_host entries, each
// cycles (low 40 bits) + the Newton iterations the workgroup ran (bits 40 and up).
int32_t mz_read_wave_cycles(mz_handle* h, uint64_t* out_host, int32_t n_host) {
  if (!h || !out_host || !h->prof || n_host <= 0 || n_host > h->n) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(out_host, h->prof + 16, (size_t)n_host * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->prof + 16, 0, (size_t)h->n * sizeof(unsigned long long)));
  return MZ_OK;
}

// Per-workgroup, per-phase cycles of the PROF kernel build accumulated since the last call (then cleared): [n_host][16].
int32_t mz_read_wave_phase_cycles(mz_handle* h, uint64_t* out_host, int32_t n_host) {
  if (!h || !out_host || !h->prof || n_host <= 0 || n_host > h->n) return MZ_ERR_ARG;
  DeviceScope scope(h->device);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(out_host, h->prof + 16 + h->n, (size_t)n_host * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->prof + 16 + h->n, 0, (size_t)h->n * 16 * sizeof(unsigned long long)));
  return MZ_OK;
}

// Average duration (ms) of the step kernel over the recorded ring (after synchronising on the last event).
double mz_last_kernel_ms(const mz_handle* h) {
  if (!h || h->ntime <= 0 || h->itime <= 0) return -1.0;
  DeviceScope scope(h->device);
  int cnt = h->itime < h->ntime ? h->itime : h->ntime;
  double tot = 0.0;
  for (int i = 0; i < cnt; i++) {
    if (hipEventSynchronize(h->ev[2 * i + 1]) != hipSuccess) return -1.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]) != hipSuccess) return -1.0;
    tot += ms;
  }
  return tot / cnt;
}

}  // extern "C"
