// mz_policy.h — the device-side policy of mz_policy_act / mz_rollout_policy (include/mazestep.h): one fp32 observation row in, one
// fp32 action row out.  Shared by the stand-alone kernel (mazestep.hip policy_act_kernel), the fused closed-loop rollout kernels
// (planar_kernels.hip) and a host build (tests/policy_host) that pins it against mujoco_maze_amd/policy.py.
//
// One policy is `npar` floats, weights input-major (nn.Linear.weight.T), so that adjacent lanes — which own adjacent output units —
// read adjacent addresses:
//   H == 0 (affine)                       Wt [obs_dim][nu], b [nu]
//   1 <= H <= MZ_POLICY_MAX_HIDDEN        W1t [obs_dim][H], b1 [H], W2t [H][nu], b2 [nu]       (one tanh hidden layer)
//
// Arithmetic, chosen so that the result does not depend on how many lanes share the work: every unit is computed by ONE lane,
// serially, in fp32 — acc = bias, then acc = acc + w * x over the inputs in index order, the product and the sum rounded
// separately (mzp_dot opens with `#pragma clang fp contract(off) reassociate(off)`; a host build adds -ffp-contract=off).  Hidden
// units are tanhf(acc); an output is acc (squash == 0) or action_scale * tanhf(acc) (squash == 1).  NaN propagates.  numpy
// reproduces the affine path bit for bit in float32, operation by operation; the tanh paths carry the tanhf of whichever library
// runs them and are bit-equal only between kernels built from this header under the same flags (mazestep.hip and planar_kernels.hip:
// STRICT in csrc/Makefile) — which is what makes the fused rollout equal the loop of mz_policy_act and mz_step.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mazestep.h"

#if defined(__HIPCC__)
#define MZP_HD __host__ __device__ __forceinline__
#else
#define MZP_HD inline
#endif

MZP_HD int mzp_param_count(int obs_dim, int nu, int hidden) {
  return hidden > 0 ? obs_dim * hidden + hidden + hidden * nu + nu : obs_dim * nu + nu;
}

// bias + sum over i < n of w[i * stride] * x[i], in index order, two roundings per term
MZP_HD float mzp_dot(const float* w, int stride, float bias, const float* x, int n) {
#pragma clang fp contract(off) reassociate(off)
  float acc = bias;
  for (int i = 0; i < n; i++) {
    const float p = w[(size_t)i * stride] * x[i];
    acc = acc + p;
  }
  return acc;
}

// hidden unit j of a policy with H >= 1 hidden units: tanhf(b1[j] + sum_i W1t[i][j] * x[i])
MZP_HD float mzp_hidden_unit(const float* par, int obs_dim, int H, const float* x, int j) {
  return tanhf(mzp_dot(par + j, H, par[(size_t)obs_dim * H + j], x, obs_dim));
}

// output unit u from its input row `in`: the observation (H == 0) or the hidden vector (H >= 1)
MZP_HD float mzp_output_unit(const float* par, int obs_dim, int nu, int H, int squash, float action_scale, const float* in, int u) {
  const float* W = H > 0 ? par + (size_t)obs_dim * H + H : par;
  const int nin = H > 0 ? H : obs_dim;
  const float acc = mzp_dot(W + u, nu, W[(size_t)nin * nu + u], in, nin);
  return squash ? action_scale * tanhf(acc) : acc;
}

// THE policy: act[nu] = policy(x[obs_dim]).  (The kernels spread the same unit functions over the lanes of a group: mzp_group_eval.)
MZP_HD void mzp_policy_row(const float* par, int obs_dim, int nu, int H, int squash, float action_scale, const float* x, float* act) {
  float hid[MZ_POLICY_MAX_HIDDEN];
  for (int j = 0; j < H; j++) hid[j] = mzp_hidden_unit(par, obs_dim, H, x, j);
  for (int u = 0; u < nu; u++) act[u] = mzp_output_unit(par, obs_dim, nu, H, squash, action_scale, H > 0 ? hid : x, u);
}

#if defined(__HIPCC__)
// hand-off between the lanes of a group inside one wavefront (the DevCtx::sync of mz_device.h: LDS operations of a wavefront
// execute in order, so a wavefront-scope fence that pins the compiler's ordering is a complete phase boundary)
__device__ __forceinline__ void mzp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One row on a group of G adjacent lanes of a wavefront (this lane: l): lanes l, l + G, ... each own one hidden unit, the hidden
// vector goes through `hid` (LDS, MZ_POLICY_MAX_HIDDEN floats of this group), then lanes 0 .. nu - 1 own the outputs and store
// them to act[nu] if `store`.  x: the row, complete and visible to the group on entry (global memory or LDS).  Every lane of the
// group must make the call; the caller hands `act` over (mzp_wave_sync) where it is LDS that the group reads back.
__device__ __forceinline__ void mzp_group_eval(int l, int G, const float* par, int obs_dim, int nu, int H, int squash, float action_scale,
                                               const float* x, float* hid, float* act, bool store) {
  if (H > 0) {
    for (int j = l; j < H; j += G) hid[j] = mzp_hidden_unit(par, obs_dim, H, x, j);
    mzp_wave_sync();
  }
  for (int u = l; u < nu; u += G) {
    // (two calls, not a select of the pointers: hid is LDS, x may be global memory)
    const float a = H > 0 ? mzp_output_unit(par, obs_dim, nu, H, squash, action_scale, hid, u)
                          : mzp_output_unit(par, obs_dim, nu, H, squash, action_scale, x, u);
    if (store) act[u] = a;
  }
}
#endif
