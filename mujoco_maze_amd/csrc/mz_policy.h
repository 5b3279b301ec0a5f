// mz_policy.h — the device-side policy of mz_policy_act / mz_rollout_policy and of their sampling twins mz_policy_sample /
// mz_rollout_policy_sample (include/mazestep.h): one fp32 observation row in, one fp32 action row out.  Shared by the stand-alone
// kernels (mazestep.hip policy_act_kernel, policy_sample_kernel), the fused closed-loop rollout kernels (planar_kernels.hip) and two
// host builds (tests/policy_host, tests/policy_sample_host) that pin it against mujoco_maze_amd/policy.py.
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
//
// Stochastic policies (mz_policy_sample / mz_rollout_policy_sample): a diagonal Gaussian around the same network.  The packed vector
// is followed by log_std[nu]: npar_s = mzp_param_count(obs_dim, nu, H) + nu floats.
//   noise    eps(noise_seed, noise_step, slot, u) is a pure function of four integers — slot: the GLOBAL env slot (env_index_offset + i),
//            u: the action index — and of nothing else (not N, nu, H, lanes per env, engine or kernel).  In uint64 arithmetic with
//            wrap-around (mix64, rng_u32: mz_rng.h):
//              key = mix64(noise_seed ^ (0xA24BAED4963EE407 * (noise_step + 1)))                                      mzp_noise_key
//              x1 = rng_u32(key, slot, 2u), x2 = rng_u32(key, slot, 2u + 1)
//              u1 = ((float)(x1 >> 8) + 1.0f) * 2^-24,  u2 = (float)(x2 >> 8) * 2^-24         (both exact: 24-bit integers)
//              eps = sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2)                          (the Box-Muller of mz_device.h rng_normal)
//            |eps| <= sqrt(48 ln 2) ~ 5.77, always finite.                                                            mzp_eps
//   sample   m_u = the pre-squash sum of output unit u (mzp_output_pre), s_u = expf(log_std[u]), p = s_u * eps_u, z_u = m_u + p — the
//            product and the sum rounded separately; the action is z_u (squash == 0) or action_scale * tanhf(z_u).    mzp_sample_unit
//   log-prob the density of z under N(m, diag(s^2)) — with squash the PRE-tanh density: the caller applies the tanh correction
//            sum_u log(action_scale * (1 - tanh(z_u)^2)) from the returned actions.  From eps itself, not from (z - m) / s; ONE lane,
//            serially in u order, fp32, every operation rounded separately:
//              acc = 0.0f;  for u = 0 .. nu - 1:  q = eps_u * eps_u;  h = -0.5f * q;  t = h - log_std[u];  t = t - 0.9189385f;
//              acc = acc + t                                                                                           mzp_logp
// NaN in log_std propagates to that unit's action and to the row's logp; log_std = -inf gives s = 0, z = m + (+-0) and logp = +inf.
//   noise on the action (mode MZ_NOISE_ACTION; TD3 / DDPG exploration): the tanh belongs to the deterministic actor and the noise goes
//            on its output — b = squash ? action_scale * tanhf(m_u) : m_u, z = b + p, every operation rounded separately, and with
//            squash the action is z clipped to +-action_scale by two selects (z < -A ? -A : (z > A ? A : z): a NaN passes).  eps, the
//            key schedule and logp are those of the default mode MZ_NOISE_PRE_SQUASH — logp is the density of the unclipped z around
//            b, the same bits for the same seed and step —, and without squash the two modes are the same operations.
// mujoco_maze_amd/policy.py mirrors all of it operation by operation (noise, sample_reference).
//
// Critics (mz_value / mz_rollout_actor_critic; value_kernel in mazestep.hip, the CRT instantiations of the fused kernels, the host
// build tests/critic_host): the same unit functions with nu = 1 and no squash — mzp_value_row, mzp_group_value below;
// policy.py value_reference.
//
// Deeper networks (mz_net_act / mz_net_value / mz_rollout_net; the mzp_net_* functions below): 0, 1 or 2 hidden layers of 1 ..
// MZ_POLICY_MAX_HIDDEN units each (mzp_shape), one activation for both — MZ_ACT_TANH: tanhf(acc), or MZ_ACT_RELU:
// acc < 0.0f ? 0.0f : acc, a select that adds no rounding, keeps -0.0f and lets a NaN through (fmaxf would drop it).  Packed vector,
// input-major as above; n_hidden 0 and 1 are the two layouts above, and
//   n_hidden == 2                         W1t [obs_dim][H1], b1 [H1], W2t [H1][H2], b2 [H2], W3t [H2][nout], b3 [nout]
// followed by log_std[nu] for a stochastic actor.  The same rules: one lane per unit, mzp_dot; a layer-2 unit reads the complete
// layer-1 vector.  A one-layer tanh network through mzp_net_* runs the operations of the functions above in the same order and gives
// the same bits; a ReLU network without squash is reproduced bit for bit by numpy at any depth (policy.py).
//
// Normalised observations (mz_bind_obs_norm; mzp_norm_elem below): while a normaliser is bound to the handle every network above reads
// the row y in place of the raw row x — element i, fp32, every operation rounded separately:
//     d = x[i] - mean[i];   y = d * inv_std[i];   y = y < -c ? -c : (y > c ? c : y)
// A product with inv_std, not a quotient (mazestep.hip and planar_kernels.hip build with -freciprocal-math); two selects, not fminf /
// fmaxf: a NaN passes through, c = +inf switches the clip off, x = +-inf becomes +-c, and a constant column (d == 0) becomes 0
// whatever inv_std is — NaN and +-inf excepted, where 0 * inv_std is NaN.  Elementwise and pure, so the bits do not depend on the lane
// that computes an element nor on whether a kernel stages the row (the NRM kernels: a second row in LDS) or computes it again; numpy
// reproduces it bit for bit (policy.py normalize_reference), so an affine or ReLU network without squash on normalised rows stays
// bit-reproducible.  The env itself never sees y: observations, the task predicate and info stay raw.
//
// Context inputs (mz_context; mzp_input_row, mzp_ctx_next below): a per-env row c of cdim <= MZ_MAX_CONTEXT floats that every network
// reads BEHIND the observation.  The input row is r = [y | c], obs_dim + cdim entries: y the observation, normalised as above while a
// normaliser is bound and the raw bits otherwise, c never normalised and never clipped; the unit functions below then run on r with
// obs_dim + cdim in place of obs_dim, so the context terms are the last terms of every first-layer sum and the packed layouts are
// those of a wider observation.  The kernels stage r once per group in the row the normaliser already stages (the NRM instantiations,
// grown by MZ_MAX_CONTEXT floats); without a bound normaliser they run with the identity normaliser — mean 0, inv_std 1, clip +inf —
// through which every bit pattern passes unchanged: x - 0 = x (-0 stays -0), x * 1 = x, neither select fires, a NaN stays one.
// HIRO's goal transition of a rollout (MZ_CTX_RELATIVE), element d < D, fp32, two roundings:  tmp = c[d] + s[d];  c[d] = tmp - s'[d]
// with s, s' the RAW rows before and behind the step; applied where the step did not end the episode.
//
// Wide networks (option "wide_nets"; mz_net_tile.h): a handle that has opted in takes hidden layers of up to MZ_NET_MAX_WIDTH (256)
// units through the mz_net entries.  Nothing in this file changes for them — MZ_POLICY_MAX_HIDDEN stays the bound of the group
// functions below and of their LDS rows —: the tiled kernels of mz_net_tile.h evaluate a tile of rows per block, load each shared
// weight once per tile, and run the SAME serial dot product per (unit, row) and the same unit functions behind it, so they return
// the bits of the functions here wherever both apply, and policy.py stays the model at every width.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mazestep.h"
#include "mz_rng.h"

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

// pre-squash sum of output unit u from its input row `in`: the observation (H == 0) or the hidden vector (H >= 1)
MZP_HD float mzp_output_pre(const float* par, int obs_dim, int nu, int H, const float* in, int u) {
  const float* W = H > 0 ? par + (size_t)obs_dim * H + H : par;
  const int nin = H > 0 ? H : obs_dim;
  return mzp_dot(W + u, nu, W[(size_t)nin * nu + u], in, nin);
}

// output unit u
MZP_HD float mzp_output_unit(const float* par, int obs_dim, int nu, int H, int squash, float action_scale, const float* in, int u) {
  const float acc = mzp_output_pre(par, obs_dim, nu, H, in, u);
  return squash ? action_scale * tanhf(acc) : acc;
}

// THE policy: act[nu] = policy(x[obs_dim]).  (The kernels spread the same unit functions over the lanes of a group: mzp_group_eval.)
MZP_HD void mzp_policy_row(const float* par, int obs_dim, int nu, int H, int squash, float action_scale, const float* x, float* act) {
  float hid[MZ_POLICY_MAX_HIDDEN];
  for (int j = 0; j < H; j++) hid[j] = mzp_hidden_unit(par, obs_dim, H, x, j);
  for (int u = 0; u < nu; u++) act[u] = mzp_output_unit(par, obs_dim, nu, H, squash, action_scale, H > 0 ? hid : x, u);
}

// element i of the normalised row (mz_bind_obs_norm; the head of this file): x = raw[i], mean = mean[i], inv_std = inv_std[i]
MZP_HD float mzp_norm_elem(float x, float mean, float inv_std, float c) {
#pragma clang fp contract(off) reassociate(off)
  const float d = x - mean;
  float y = d * inv_std;
  y = y < -c ? -c : (y > c ? c : y);
  return y;
}

// THE normalised row: y[obs_dim] from x[obs_dim] (the kernels spread the elements over the lanes of a group: mzp_group_norm)
MZP_HD void mzp_norm_row(const float* x, const float* mean, const float* inv_std, float c, int obs_dim, float* y) {
  for (int i = 0; i < obs_dim; i++) y[i] = mzp_norm_elem(x[i], mean[i], inv_std[i], c);
}

// ------------------------------------------------------------------ context inputs (the head of this file)
// THE input row r[obs_dim + cdim] = [y | c]: y = mzp_norm_row of x with a normaliser (mean != NULL), else x; c as it is
MZP_HD void mzp_input_row(const float* x, int obs_dim, const float* mean, const float* inv_std, float clip, const float* c, int cdim, float* r) {
  for (int i = 0; i < obs_dim; i++) r[i] = mean ? mzp_norm_elem(x[i], mean[i], inv_std[i], clip) : x[i];
  for (int i = 0; i < cdim; i++) r[obs_dim + i] = c[i];
}

// one element of the relative transition: the context that goes with s2 when c went with s
MZP_HD float mzp_ctx_next(float c, float s, float s2) {
#pragma clang fp contract(off) reassociate(off)
  const float tmp = c + s;
  return tmp - s2;
}

// THE transition of one row: c[d] for d < rel_dims from the raw rows s (acted on) and s2 (produced), unless the step ended the episode
MZP_HD void mzp_ctx_transition_row(float* c, int rel_dims, const float* s, const float* s2, int done) {
  if (done) return;
  for (int d = 0; d < rel_dims; d++) c[d] = mzp_ctx_next(c[d], s[d], s2[d]);
}

// ------------------------------------------------------------------ stochastic policies (definitions: the head of this file)
MZP_HD uint64_t mzp_noise_key(uint64_t noise_seed, uint64_t noise_step) {
  return mix64(noise_seed ^ (0xA24BAED4963EE407ULL * (noise_step + 1)));
}

MZP_HD float mzp_eps(uint64_t key, uint64_t slot, int u) {
#pragma clang fp contract(off) reassociate(off)
  const uint32_t x1 = rng_u32(key, slot, 2u * (uint32_t)u), x2 = rng_u32(key, slot, 2u * (uint32_t)u + 1u);
  const float u1 = ((float)(x1 >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u2 = (float)(x2 >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u1)), c = cosf(6.2831855f * u2);
  return r * c;
}

// the action of output unit u from its pre-squash mean m; mode: MZ_NOISE_PRE_SQUASH (the noise goes through the squash) or
// MZ_NOISE_ACTION (the noise goes on the squashed action, which is then clipped to +-action_scale: the head of this file)
MZP_HD float mzp_sample_unit(float m, float log_std, float eps, int squash, float action_scale, int mode = MZ_NOISE_PRE_SQUASH) {
#pragma clang fp contract(off) reassociate(off)
  const float s = expf(log_std);
  const float p = s * eps;
  if (mode == MZ_NOISE_ACTION && squash) {
    const float b = action_scale * tanhf(m);
    const float z = b + p;
    return z < -action_scale ? -action_scale : (z > action_scale ? action_scale : z);
  }
  const float z = m + p;
  return squash ? action_scale * tanhf(z) : z;
}

// log-prob of a row: one lane, u = 0 .. nu - 1 in order (the nu values of eps are computed again here)
MZP_HD float mzp_logp(const float* log_std, int nu, uint64_t key, uint64_t slot) {
#pragma clang fp contract(off) reassociate(off)
  float acc = 0.0f;
  for (int u = 0; u < nu; u++) {
    const float e = mzp_eps(key, slot, u);
    const float q = e * e;
    const float h = -0.5f * q;
    float t = h - log_std[u];
    t = t - 0.9189385f;
    acc = acc + t;
  }
  return acc;
}

// THE stochastic policy: act[nu] ~ N(mean(x), diag(exp(log_std))^2) with the noise of (noise_seed, noise_step, slot); *logp (nullable)
MZP_HD void mzp_sample_row(const float* par, int obs_dim, int nu, int H, int squash, float action_scale, uint64_t noise_seed,
                           uint64_t noise_step, uint64_t slot, const float* x, float* act, float* logp, int mode = MZ_NOISE_PRE_SQUASH) {
  float hid[MZ_POLICY_MAX_HIDDEN];
  const float* ls = par + mzp_param_count(obs_dim, nu, H);
  const uint64_t key = mzp_noise_key(noise_seed, noise_step);
  for (int j = 0; j < H; j++) hid[j] = mzp_hidden_unit(par, obs_dim, H, x, j);
  for (int u = 0; u < nu; u++)
    act[u] = mzp_sample_unit(mzp_output_pre(par, obs_dim, nu, H, H > 0 ? hid : x, u), ls[u], mzp_eps(key, slot, u), squash, action_scale, mode);
  if (logp) *logp = mzp_logp(ls, nu, key, slot);
}

// ------------------------------------------------------------------ critics (mz_value / mz_rollout_actor_critic)
// A critic is a policy with nu = 1, never squashed, in a parameter vector of its own: mzp_param_count(obs_dim, 1, Hv) floats, Hv == 0
// affine, 1 <= Hv <= MZ_POLICY_MAX_HIDDEN one tanh hidden layer.  THE value of a row: the pre-squash sum of its one output unit.
MZP_HD float mzp_value_row(const float* vpar, int obs_dim, int Hv, const float* x) {
  float hid[MZ_POLICY_MAX_HIDDEN];
  for (int j = 0; j < Hv; j++) hid[j] = mzp_hidden_unit(vpar, obs_dim, Hv, x, j);
  return mzp_output_pre(vpar, obs_dim, 1, Hv, Hv > 0 ? hid : x, 0);
}

// ------------------------------------------------------------------ networks of up to two hidden layers (mz_net_*: the head of this file)
typedef struct mzp_shape {
  int n_hidden, h1, h2;  // hidden layers in use and their widths (unused: 0)
  int act;               // MZ_ACT_* of the hidden units
} mzp_shape;

MZP_HD int mzp_net_param_count(int obs_dim, int nout, mzp_shape s) {
  if (s.n_hidden == 2) return obs_dim * s.h1 + s.h1 + s.h1 * s.h2 + s.h2 + s.h2 * nout + nout;
  return mzp_param_count(obs_dim, nout, s.n_hidden == 1 ? s.h1 : 0);
}

MZP_HD float mzp_activate(float acc, int act) {
  if (act == MZ_ACT_RELU) return acc < 0.0f ? 0.0f : acc;
  return tanhf(acc);
}

// unit j of hidden layer `layer` (0: from the observation row, 1: from the complete first hidden vector) — `in` is that input row
MZP_HD float mzp_net_hidden_unit(const float* par, int obs_dim, mzp_shape s, int layer, const float* in, int j) {
  const float* W = layer ? par + (size_t)obs_dim * s.h1 + s.h1 : par;
  const int nin = layer ? s.h1 : obs_dim, w = layer ? s.h2 : s.h1;
  return mzp_activate(mzp_dot(W + j, w, W[(size_t)nin * w + j], in, nin), s.act);
}

// pre-squash sum of output unit u from the input row of the output layer: the observation or the last hidden vector
MZP_HD float mzp_net_output_pre(const float* par, int obs_dim, int nout, mzp_shape s, const float* in, int u) {
  const float* W = par;
  int nin = obs_dim;
  if (s.n_hidden >= 1) { W += (size_t)obs_dim * s.h1 + s.h1; nin = s.h1; }
  if (s.n_hidden == 2) { W += (size_t)s.h1 * s.h2 + s.h2; nin = s.h2; }
  return mzp_dot(W + u, nout, W[(size_t)nin * nout + u], in, nin);
}

// the hidden layers of one row, serially; returns the input row of the output layer (x, hid1 or hid2)
MZP_HD const float* mzp_net_hidden_row(const float* par, int obs_dim, mzp_shape s, const float* x, float* hid1, float* hid2) {
  if (s.n_hidden < 1) return x;
  for (int j = 0; j < s.h1; j++) hid1[j] = mzp_net_hidden_unit(par, obs_dim, s, 0, x, j);
  if (s.n_hidden < 2) return hid1;
  for (int j = 0; j < s.h2; j++) hid2[j] = mzp_net_hidden_unit(par, obs_dim, s, 1, hid1, j);
  return hid2;
}

// mzp_policy_row, mzp_sample_row and mzp_value_row for a network of shape s
MZP_HD void mzp_net_policy_row(const float* par, int obs_dim, int nu, mzp_shape s, int squash, float action_scale, const float* x, float* act) {
  float hid1[MZ_POLICY_MAX_HIDDEN], hid2[MZ_POLICY_MAX_HIDDEN];
  const float* in = mzp_net_hidden_row(par, obs_dim, s, x, hid1, hid2);
  for (int u = 0; u < nu; u++) {
    const float acc = mzp_net_output_pre(par, obs_dim, nu, s, in, u);
    act[u] = squash ? action_scale * tanhf(acc) : acc;
  }
}

MZP_HD void mzp_net_sample_row(const float* par, int obs_dim, int nu, mzp_shape s, int squash, float action_scale, uint64_t noise_seed,
                               uint64_t noise_step, uint64_t slot, const float* x, float* act, float* logp, int mode = MZ_NOISE_PRE_SQUASH) {
  float hid1[MZ_POLICY_MAX_HIDDEN], hid2[MZ_POLICY_MAX_HIDDEN];
  const float* ls = par + mzp_net_param_count(obs_dim, nu, s);
  const uint64_t key = mzp_noise_key(noise_seed, noise_step);
  const float* in = mzp_net_hidden_row(par, obs_dim, s, x, hid1, hid2);
  for (int u = 0; u < nu; u++)
    act[u] = mzp_sample_unit(mzp_net_output_pre(par, obs_dim, nu, s, in, u), ls[u], mzp_eps(key, slot, u), squash, action_scale, mode);
  if (logp) *logp = mzp_logp(ls, nu, key, slot);
}

MZP_HD float mzp_net_value_row(const float* vpar, int obs_dim, mzp_shape s, const float* x) {
  float hid1[MZ_POLICY_MAX_HIDDEN], hid2[MZ_POLICY_MAX_HIDDEN];
  return mzp_net_output_pre(vpar, obs_dim, 1, s, mzp_net_hidden_row(vpar, obs_dim, s, x, hid1, hid2), 0);
}

// ------------------------------------------------------------------ a state-dependent log-std head (mz_net_sample_head / mz_rollout_head)
// A head actor is a network of shape s whose output layer has 2 nu units: units 0 .. nu - 1 are the means m_u, units nu .. 2 nu - 1 the
// raw log-stds r_u — W_out_t [nin][2 nu], b_out [2 nu]; mzp_net_param_count(obs_dim, 2 nu, s) floats, no trailing log_std.  Every unit
// is one lane through mzp_dot, as everywhere above.  In fp32, every operation rounded separately:
//   ls_u = r_u < lo ? lo : (r_u > hi ? hi : r_u)                two selects: a NaN passes, lo = -inf / hi = +inf switch a side off
//   z_u  = m_u + expf(ls_u) * eps_u;  a_u = squash ? A * tanhf(z_u) : z_u        mzp_sample_unit's operations in MZ_NOISE_PRE_SQUASH, written
//                                                               once more so that z_u is at hand (mzp_head_z, mzp_head_action); eps, key as above
//   logp = sum over u, in order, of t_u:
//          q = eps_u * eps_u;  h = -0.5f * q;  t = h - ls_u;  t = t - 0.9189385f                  (mzp_logp's, with the clamped ls_u)
//          logp_squashed: the density of the action A tanh(z), log |d(A tanh z) / dz| = log A + 2 (log 2 - z - softplus(-2 z)):
//            x = -2.0f * z_u;  ax = fabsf(x);  e = expf(-ax);  l = log1pf(e);  sp = (x > 0.0f ? x : 0.0f) + l
//            c = 0.6931472f - z_u;  c = c - sp;  c = 2.0f * c;  c = c + logA;  t = t - c
// logA = logf(A) is computed once per call on the host and handed to every kernel of the call.  Never log(1 - tanh^2), which is -inf
// in fp32 from |z| ~ 9.  t_u is a pure function of the row, the parameters and four integers, so the lane that owns unit u computes
// it and the group's first lane adds the nu terms in order: the bits of one lane computing everything (mzp_net_sample_head_row).
typedef struct mzp_head {
  float lo, hi;       // the clamp of the raw log-std
  int logp_squashed;  // 0: density of z; 1: density of A * tanh(z)
  float logA;         // logf((float)action_scale), from the host
} mzp_head;

MZP_HD float mzp_head_clamp(float r, float lo, float hi) { return r < lo ? lo : (r > hi ? hi : r); }

// z_u and the action from it: together the operations of mzp_sample_unit in MZ_NOISE_PRE_SQUASH, so the same bits (pinned by the
// constant-head tests: tests/test_sac_head_api.py, tests/test_gpu_sac_head.py)
MZP_HD float mzp_head_z(float m, float ls, float eps) {
#pragma clang fp contract(off) reassociate(off)
  const float s = expf(ls);
  const float p = s * eps;
  return m + p;
}
MZP_HD float mzp_head_action(float z, int squash, float action_scale) { return squash ? action_scale * tanhf(z) : z; }

// t_u (the head of this section)
MZP_HD float mzp_head_logp_term(float eps, float ls, float z, int logp_squashed, float logA) {
#pragma clang fp contract(off) reassociate(off)
  const float q = eps * eps;
  const float h = -0.5f * q;
  float t = h - ls;
  t = t - 0.9189385f;
  if (logp_squashed) {
    const float x = -2.0f * z;
    const float ax = fabsf(x);
    const float e = expf(-ax);
    const float l = log1pf(e);
    const float sp = (x > 0.0f ? x : 0.0f) + l;
    float c = 0.6931472f - z;
    c = c - sp;
    c = 2.0f * c;
    c = c + logA;
    t = t - c;
  }
  return t;
}

MZP_HD float mzp_head_logp_add(float acc, float t) {
#pragma clang fp contract(off) reassociate(off)
  return acc + t;
}

// THE head actor: act[nu] and *logp (nullable) of one row
MZP_HD void mzp_net_sample_head_row(const float* par, int obs_dim, int nu, mzp_shape s, int squash, float action_scale, mzp_head hd,
                                    uint64_t noise_seed, uint64_t noise_step, uint64_t slot, const float* x, float* act, float* logp) {
  float hid1[MZ_POLICY_MAX_HIDDEN], hid2[MZ_POLICY_MAX_HIDDEN];
  const uint64_t key = mzp_noise_key(noise_seed, noise_step);
  const float* in = mzp_net_hidden_row(par, obs_dim, s, x, hid1, hid2);
  float acc = 0.0f;
  for (int u = 0; u < nu; u++) {
    const float m = mzp_net_output_pre(par, obs_dim, 2 * nu, s, in, u);
    const float ls = mzp_head_clamp(mzp_net_output_pre(par, obs_dim, 2 * nu, s, in, nu + u), hd.lo, hd.hi);
    const float eps = mzp_eps(key, slot, u);
    const float z = mzp_head_z(m, ls, eps);
    act[u] = mzp_head_action(z, squash, action_scale);
    acc = mzp_head_logp_add(acc, mzp_head_logp_term(eps, ls, z, hd.logp_squashed, hd.logA));
  }
  if (logp) *logp = acc;
}

#if defined(__HIPCC__)
// hand-off between the lanes of a group inside one wavefront (the DevCtx::sync of mz_device.h: LDS operations of a wavefront
// execute in order, so a wavefront-scope fence that pins the compiler's ordering is a complete phase boundary)
__device__ __forceinline__ void mzp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the normaliser of one launch (mz_bind_obs_norm): [obs_dim] device arrays shared by all envs, read in stream order
// and, with a context bound to the call, the context rows: ctx [rows][cdim] (cdim == 0: none), staged behind the normalised row
struct mzp_norm {
  const float* mean;
  const float* inv_std;
  float clip;
  int cdim;
  const float* ctx;
};

// mzp_norm_row on a group: lanes l, l + G, ... each own the elements i = l, l + G, ... of y (LDS of this group), read from the raw
// row x.  No lane of the group may still read y on entry, and the caller hands y over (mzp_wave_sync) before a unit reads it.
__device__ __forceinline__ void mzp_group_norm(int l, int G, mzp_norm nm, int obs_dim, const float* x, float* y) {
  for (int i = l; i < obs_dim; i += G) y[i] = mzp_norm_elem(x[i], nm.mean[i], nm.inv_std[i], nm.clip);
}

// the context half of mzp_input_row on a group: lanes l, l + G, ... each own the elements i = l, l + G, ... of yc = y + obs_dim, the
// tail of the staged row, copied from the row's context c; under the hand-offs of mzp_group_norm
__device__ __forceinline__ void mzp_group_ctx(int l, int G, const float* c, int cdim, float* yc) {
  for (int i = l; i < cdim; i += G) yc[i] = c[i];
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

// mzp_group_eval for a stochastic policy: lanes 0 .. nu - 1 own the outputs and their eps, the group's first lane the row's log-prob,
// which it stores to *logp unless that is NULL.  key: mzp_noise_key of the step; slot: the row's global env slot; mode: MZ_NOISE_*.
__device__ __forceinline__ void mzp_group_sample(int l, int G, const float* par, int obs_dim, int nu, int H, int squash, float action_scale,
                                                 uint64_t key, uint64_t slot, const float* x, float* hid, float* act, bool store, float* logp,
                                                 int mode) {
  if (H > 0) {
    for (int j = l; j < H; j += G) hid[j] = mzp_hidden_unit(par, obs_dim, H, x, j);
    mzp_wave_sync();
  }
  const float* ls = par + mzp_param_count(obs_dim, nu, H);
  for (int u = l; u < nu; u += G) {
    const float m = H > 0 ? mzp_output_pre(par, obs_dim, nu, H, hid, u) : mzp_output_pre(par, obs_dim, nu, H, x, u);
    const float a = mzp_sample_unit(m, ls[u], mzp_eps(key, slot, u), squash, action_scale, mode);
    if (store) act[u] = a;
  }
  if (l == 0 && logp) *logp = mzp_logp(ls, nu, key, slot);
}

// mzp_value_row on a group: lanes l, l + G, ... each own one hidden unit, the group's first lane owns the output and returns the
// value (every other lane returns 0).  `hid` may be the row mzp_group_eval / mzp_group_sample used, once the actor's outputs have
// been handed over: on entry no lane of the group may still read it, and the caller hands it (and x) over again (mzp_wave_sync)
// before anything rewrites either.  Every lane of the group must make the call.
__device__ __forceinline__ float mzp_group_value(int l, int G, const float* vpar, int obs_dim, int Hv, const float* x, float* hid) {
  if (Hv > 0) {
    for (int j = l; j < Hv; j += G) hid[j] = mzp_hidden_unit(vpar, obs_dim, Hv, x, j);
    mzp_wave_sync();
  }
  float v = 0.0f;
  // (two calls, not a select of the pointers: hid is LDS, x may be global memory)
  if (l == 0) v = Hv > 0 ? mzp_output_pre(vpar, obs_dim, 1, Hv, hid, 0) : mzp_output_pre(vpar, obs_dim, 1, Hv, x, 0);
  return v;
}

// The hidden layers of a network of shape s on a group: lanes l, l + G, ... each own one unit of a layer; the first hidden vector
// goes through `hid`, the second through `hid2` (LDS, MZ_POLICY_MAX_HIDDEN floats of this group each), with the group's phase
// boundary behind each layer: a layer-2 unit reads the complete layer-1 vector.  Every lane of the group must make the call.
__device__ __forceinline__ void mzp_group_net_hidden(int l, int G, const float* par, int obs_dim, mzp_shape s, const float* x, float* hid,
                                                     float* hid2) {
  if (s.n_hidden >= 1) {
    for (int j = l; j < s.h1; j += G) hid[j] = mzp_net_hidden_unit(par, obs_dim, s, 0, x, j);
    mzp_wave_sync();
  }
  if (s.n_hidden == 2) {
    for (int j = l; j < s.h2; j += G) hid2[j] = mzp_net_hidden_unit(par, obs_dim, s, 1, hid, j);
    mzp_wave_sync();
  }
}

// pre-squash sum of output unit u behind mzp_group_net_hidden (three calls, not a select of the pointers: hid and hid2 are LDS, x may
// be global memory)
__device__ __forceinline__ float mzp_group_net_pre(const float* par, int obs_dim, int nout, mzp_shape s, const float* x, const float* hid,
                                                   const float* hid2, int u) {
  if (s.n_hidden == 2) return mzp_net_output_pre(par, obs_dim, nout, s, hid2, u);
  if (s.n_hidden == 1) return mzp_net_output_pre(par, obs_dim, nout, s, hid, u);
  return mzp_net_output_pre(par, obs_dim, nout, s, x, u);
}

// mzp_group_eval (sample == false: key, slot, logp and mode are not read) and mzp_group_sample (sample == true) for a network of shape s
__device__ __forceinline__ void mzp_group_net_act(int l, int G, const float* par, int obs_dim, int nu, mzp_shape s, int squash, float action_scale,
                                                  bool sample, uint64_t key, uint64_t slot, const float* x, float* hid, float* hid2, float* act,
                                                  bool store, float* logp, int mode) {
  mzp_group_net_hidden(l, G, par, obs_dim, s, x, hid, hid2);
  const float* ls = par + mzp_net_param_count(obs_dim, nu, s);
  for (int u = l; u < nu; u += G) {
    const float m = mzp_group_net_pre(par, obs_dim, nu, s, x, hid, hid2, u);
    const float a = sample ? mzp_sample_unit(m, ls[u], mzp_eps(key, slot, u), squash, action_scale, mode) : (squash ? action_scale * tanhf(m) : m);
    if (store) act[u] = a;
  }
  if (sample && l == 0 && logp) *logp = mzp_logp(ls, nu, key, slot);
}

// mzp_net_sample_head_row on a group: lanes 0 .. nu - 1 own unit u's mean, raw log-std, eps, action and log-prob term t_u; the terms go
// to the group's first lane through the hidden row the output layer does not read (`hid` behind two hidden layers, else `hid2`: the
// phase boundary behind the last hidden layer has retired its readers; nu <= MZ_POLICY_MAX_HIDDEN), which adds them in order and
// stores *logp unless that is NULL.  The caller hands `act` over, and both hidden rows stay untouched until then.
__device__ __forceinline__ void mzp_group_net_sample_head(int l, int G, const float* par, int obs_dim, int nu, mzp_shape s, int squash,
                                                          float action_scale, mzp_head hd, uint64_t key, uint64_t slot, const float* x, float* hid,
                                                          float* hid2, float* act, bool store, float* logp) {
  mzp_group_net_hidden(l, G, par, obs_dim, s, x, hid, hid2);
  float* terms = s.n_hidden == 2 ? hid : hid2;
  for (int u = l; u < nu; u += G) {
    const float m = mzp_group_net_pre(par, obs_dim, 2 * nu, s, x, hid, hid2, u);
    const float ls = mzp_head_clamp(mzp_group_net_pre(par, obs_dim, 2 * nu, s, x, hid, hid2, nu + u), hd.lo, hd.hi);
    const float eps = mzp_eps(key, slot, u);
    const float z = mzp_head_z(m, ls, eps);
    if (store) act[u] = mzp_head_action(z, squash, action_scale);
    terms[u] = mzp_head_logp_term(eps, ls, z, hd.logp_squashed, hd.logA);
  }
  mzp_wave_sync();
  if (l == 0 && logp) {
    float acc = 0.0f;
    for (int u = 0; u < nu; u++) acc = mzp_head_logp_add(acc, terms[u]);
    *logp = acc;
  }
}

// mzp_group_value for a network of shape s: `hid` and `hid2` may be the rows the actor used, under the rule of mzp_group_value
__device__ __forceinline__ float mzp_group_net_value(int l, int G, const float* vpar, int obs_dim, mzp_shape s, const float* x, float* hid,
                                                     float* hid2) {
  mzp_group_net_hidden(l, G, vpar, obs_dim, s, x, hid, hid2);
  float v = 0.0f;
  if (l == 0) v = mzp_group_net_pre(vpar, obs_dim, 1, s, x, hid, hid2, 0);
  return v;
}
#endif
