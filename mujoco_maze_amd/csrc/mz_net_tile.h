// mz_net_tile.h — the tiled network kernel behind option "wide_nets" (include/mazestep.h): networks of up to MZ_NET_MAX_WIDTH units per
// hidden layer for every entry that takes an mz_net.  Included by mazestep.hip alone, and by the host build tests/wide_host.
//
// The group kernels of mazestep.hip evaluate one row per 16 lanes and read every weight again for every row, which is the right
// shape up to 64 units and the wrong one at 256-256 (75 k weights per row).  Here one block of MZT_THREADS threads evaluates a tile
// of MZT_ROWS rows, in phases with a block barrier between them:
//   1 mzt_stage     the input rows r = [y | c] of mz_policy.h into LDS — y through mzp_norm_elem while the launch has a normaliser
//                   (the handle's, or the identity behind a context alone), else the raw bits; the row is the final_obs row where
//                   `done` says so (a critic under auto-reset)
//   2 mzt_hidden    hidden layer 1 into LDS [MZT_ROWS][MZ_NET_MAX_WIDTH]
//   3 mzt_hidden    hidden layer 2 likewise
//   4 mzt_output    the pre-squash sums of the nout = nu, 2 nu (a head) or 1 (a critic) output units
//   5 mzt_epilogue_units / mzt_epilogue_logp   the operations of mzp_group_net_act / mzp_group_net_sample_head / mzp_group_net_value
//                   behind their hidden layers, through the same unit functions
// Shared parameters (pstride == 0): a thread owns a unit j of the layer and a subset of the tile's rows — rows g, g + G, .. with
// G = threads / width row groups, one group holding all rows from 256 units on —, with one accumulator per row in registers.  It walks
// the inputs in index order, loads w[i][j] ONCE (adjacent threads, adjacent addresses) and for each of its rows does
// p = w * x[r][i]; acc[r] = acc[r] + p with x[r][i] from LDS, where lanes of one row group read one address.  Per (unit, row) that is
// the serial dot product of mzp_dot, operation by operation, so the bits depend neither on MZT_ROWS, nor on the mapping, nor on the
// other rows of the tile (a NaN row poisons its own accumulators only).  Per-env parameters: every row reads its own vector, nothing
// is shared, and a thread computes (row, unit) pairs through mzp_net_hidden_unit itself.  The output layer is narrow, so it runs as
// (row, unit) pairs through mzp_net_output_pre in both cases.
// Rows beyond n shadow row n - 1 and store nothing; every thread reaches every barrier.
// The phase functions are MZP_HD and take the thread index, the block size and the LDS arrays as plain pointers: a host build loops
// the thread indices of a block through each phase in turn (tests/wide_host), which checks the index arithmetic without a GPU.
#pragma once
#include "mz_policy.h"

#define MZT_ROWS 16                                               // rows of a tile
#define MZT_THREADS 256                                           // threads of a block
#define MZT_IN_MAX (MZ_MAX_OBS + MZ_VIEW_DIM + MZ_MAX_CONTEXT)    // floats of a staged input row
#define MZT_OUT_MAX (2 * MZ_POLICY_MAX_HIDDEN)                    // output units of a network: 2 nu of a head with nu <= 64
#define MZT_DEPTH 8                                               // weights of a unit in flight ahead of their sums

enum { MZT_ACT = 0, MZT_SAMPLE = 1, MZT_HEAD = 2, MZT_VALUE = 3 };

// one launch: what to evaluate (kind), on which rows, with which outputs
struct mzt_job {
  int kind;                    // MZT_ACT: actions = the network's outputs; MZT_SAMPLE: a draw, log_std [nu] behind the network;
                               // MZT_HEAD: a draw of a head actor; MZT_VALUE: values = the one output unit
  int n, obs_dim, cdim, nu;    // rows, floats of an observation row, of a context row (0: none), actions
  mzp_shape s;
  int squash;
  float action_scale;
  int mode;                    // MZ_NOISE_* (MZT_SAMPLE)
  mzp_head hd;                 // (MZT_HEAD)
  const float* params;
  long pstride;                // 0: one network for all rows, else floats between the rows' networks
  uint64_t key, env0;          // mzp_noise_key of the draw; row r is global env slot env0 + r
  const float* obs;
  const float* final_obs;      // with `done` (both NULL: every row from obs): row r is read from final_obs where done[r] != 0
  const uint8_t* done;
  const float* mean;           // the normaliser (NULL: the raw bits) ..
  const float* inv_std;
  float clip;
  const float* ctx;            // .. and the context rows [n][cdim]
  float* actions;              // [n][nu]
  float* logp;                 // [n], nullable
  float* values;               // [n] (MZT_VALUE)
};

MZP_HD int mzt_in_dim(const mzt_job& J) { return J.obs_dim + J.cdim; }
MZP_HD int mzt_nout(const mzt_job& J) { return J.kind == MZT_VALUE ? 1 : (J.kind == MZT_HEAD ? 2 * J.nu : J.nu); }
// the row that slot r of the tile at row0 evaluates: rows beyond n shadow the last one
MZP_HD size_t mzt_row(const mzt_job& J, size_t row0, int r) {
  const size_t row = row0 + (size_t)r;
  return row < (size_t)J.n ? row : (size_t)J.n - 1;
}

// phase 1: xin [MZT_ROWS][MZT_IN_MAX], one thread per element
MZP_HD void mzt_stage(int tid, int T, const mzt_job& J, size_t row0, float* xin) {
  const int nin = mzt_in_dim(J);
  for (int idx = tid; idx < MZT_ROWS * nin; idx += T) {
    const int r = idx / nin, i = idx - r * nin;
    const size_t row = mzt_row(J, row0, r);
    float v;
    if (i < J.obs_dim) {
      const float* src = (J.done && J.done[row]) ? J.final_obs : J.obs;
      const float x = src[row * (size_t)J.obs_dim + i];
      v = J.mean ? mzp_norm_elem(x, J.mean[i], J.inv_std[i], J.clip) : x;
    } else {
      v = J.ctx[row * (size_t)J.cdim + (i - J.obs_dim)];
    }
    xin[r * MZT_IN_MAX + i] = v;
  }
}

// phases 2 and 3: hidden layer `layer` (0: from the staged rows, 1: from the first hidden rows) of the tile; in [MZT_ROWS][in_stride],
// out [MZT_ROWS][MZ_NET_MAX_WIDTH]
MZP_HD void mzt_hidden(int tid, int T, const mzt_job& J, size_t row0, int layer, const float* in, int in_stride, float* out) {
#pragma clang fp contract(off) reassociate(off)
  const int in_dim = mzt_in_dim(J);
  const int nin = layer ? J.s.h1 : in_dim, w = layer ? J.s.h2 : J.s.h1;
  if (J.pstride != 0) {  // one network per row: (row, unit) pairs
    for (int idx = tid; idx < MZT_ROWS * w; idx += T) {
      const int r = idx / w, j = idx - r * w;
      const float* par = J.params + mzt_row(J, row0, r) * (size_t)J.pstride;
      out[r * MZ_NET_MAX_WIDTH + j] = mzp_net_hidden_unit(par, in_dim, J.s, layer, in + r * in_stride, j);
    }
    return;
  }
  const float* W = layer ? J.params + (size_t)in_dim * J.s.h1 + J.s.h1 : J.params;
  const int span = w >= T ? T : w;  // threads of one row group
  int G = T / span;                 // row groups
  if (G > MZT_ROWS) G = MZT_ROWS;
  const int g = tid / span;
  if (g >= G) return;
  for (int j = tid - g * span; j < w; j += span) {
    float acc[MZT_ROWS];
    const float b = W[(size_t)nin * w + j];
#pragma unroll
    for (int k = 0; k < MZT_ROWS; k++) acc[k] = b;
    // the weights of MZT_DEPTH inputs are loaded before their dependent chains run (the loads do not depend on the sums); the
    // inputs are still walked in index order
    int i = 0;
    for (; i + MZT_DEPTH <= nin; i += MZT_DEPTH) {
      float wv[MZT_DEPTH];
#pragma unroll
      for (int d = 0; d < MZT_DEPTH; d++) wv[d] = W[(size_t)(i + d) * w + j];
#pragma unroll
      for (int d = 0; d < MZT_DEPTH; d++) {
#pragma unroll
        for (int k = 0; k < MZT_ROWS; k++) {
          const int r = g + k * G;
          if (r < MZT_ROWS) {
            const float p = wv[d] * in[r * in_stride + i + d];
            acc[k] = acc[k] + p;
          }
        }
      }
    }
    for (; i < nin; i++) {
      const float wv = W[(size_t)i * w + j];
#pragma unroll
      for (int k = 0; k < MZT_ROWS; k++) {
        const int r = g + k * G;
        if (r < MZT_ROWS) {
          const float p = wv * in[r * in_stride + i];
          acc[k] = acc[k] + p;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < MZT_ROWS; k++) {
      const int r = g + k * G;
      if (r < MZT_ROWS) out[r * MZ_NET_MAX_WIDTH + j] = mzp_activate(acc[k], J.s.act);
    }
  }
}

// phase 4: the pre-squash sums of the output units, outs [MZT_ROWS][MZT_OUT_MAX]; `in`: the input rows of the output layer (the staged
// rows, or the last hidden rows)
MZP_HD void mzt_output(int tid, int T, const mzt_job& J, size_t row0, const float* in, int in_stride, float* outs) {
  const int in_dim = mzt_in_dim(J), nout = mzt_nout(J);
  for (int idx = tid; idx < MZT_ROWS * nout; idx += T) {
    const int r = idx / nout, u = idx - r * nout;
    const float* par = J.params + mzt_row(J, row0, r) * (size_t)J.pstride;
    outs[r * MZT_OUT_MAX + u] = mzp_net_output_pre(par, in_dim, nout, J.s, in + r * in_stride, u);
  }
}

// phase 5a: one thread per (row, action) — the action from the unit's sum; a head leaves the unit's log-prob term t_u in outs[r][u]
// (its own sum: no other thread reads it).  A critic: one thread per row.
MZP_HD void mzt_epilogue_units(int tid, int T, const mzt_job& J, size_t row0, float* outs) {
  if (J.kind == MZT_VALUE) {
    for (int r = tid; r < MZT_ROWS; r += T) {
      const size_t row = row0 + (size_t)r;
      if (row < (size_t)J.n) J.values[row] = outs[r * MZT_OUT_MAX];
    }
    return;
  }
  const int nu = J.nu;
  const int count = mzp_net_param_count(mzt_in_dim(J), mzt_nout(J), J.s);
  for (int idx = tid; idx < MZT_ROWS * nu; idx += T) {
    const int r = idx / nu, u = idx - r * nu;
    const size_t row = mzt_row(J, row0, r);
    const bool live = row0 + (size_t)r < (size_t)J.n;
    const float m = outs[r * MZT_OUT_MAX + u];
    float a;
    if (J.kind == MZT_ACT) {
      a = J.squash ? J.action_scale * tanhf(m) : m;
    } else if (J.kind == MZT_SAMPLE) {
      const float* ls = J.params + row * (size_t)J.pstride + count;
      a = mzp_sample_unit(m, ls[u], mzp_eps(J.key, J.env0 + row, u), J.squash, J.action_scale, J.mode);
    } else {
      const float ls = mzp_head_clamp(outs[r * MZT_OUT_MAX + nu + u], J.hd.lo, J.hd.hi);
      const float eps = mzp_eps(J.key, J.env0 + row, u);
      const float z = mzp_head_z(m, ls, eps);
      a = mzp_head_action(z, J.squash, J.action_scale);
      outs[r * MZT_OUT_MAX + u] = mzp_head_logp_term(eps, ls, z, J.hd.logp_squashed, J.hd.logA);
    }
    if (live) J.actions[row * (size_t)nu + u] = a;
  }
}

// phase 5b: the row's log-prob, one thread per row, u in order
MZP_HD void mzt_epilogue_logp(int tid, int T, const mzt_job& J, size_t row0, const float* outs) {
  if ((J.kind != MZT_SAMPLE && J.kind != MZT_HEAD) || !J.logp) return;
  const int count = mzp_net_param_count(mzt_in_dim(J), mzt_nout(J), J.s);
  for (int r = tid; r < MZT_ROWS; r += T) {
    const size_t row = row0 + (size_t)r;
    if (row >= (size_t)J.n) continue;
    if (J.kind == MZT_SAMPLE) {
      J.logp[row] = mzp_logp(J.params + row * (size_t)J.pstride + count, J.nu, J.key, J.env0 + row);
    } else {
      float acc = 0.0f;
      for (int u = 0; u < J.nu; u++) acc = mzp_head_logp_add(acc, outs[r * MZT_OUT_MAX + u]);
      J.logp[row] = acc;
    }
  }
}

#if defined(__HIPCC__)
// the tile at blockIdx.x: 49.7 KB of static LDS, three blocks to a compute unit's 160 KB
__global__ __launch_bounds__(MZT_THREADS) void net_tile_kernel(mzt_job J) {
  __shared__ float xin[MZT_ROWS * MZT_IN_MAX];
  __shared__ float hid1[MZT_ROWS * MZ_NET_MAX_WIDTH];
  __shared__ float hid2[MZT_ROWS * MZ_NET_MAX_WIDTH];
  __shared__ float outs[MZT_ROWS * MZT_OUT_MAX];
  const int tid = (int)threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * MZT_ROWS;
  mzt_stage(tid, MZT_THREADS, J, row0, xin);
  __syncthreads();
  if (J.s.n_hidden >= 1) {
    mzt_hidden(tid, MZT_THREADS, J, row0, 0, xin, MZT_IN_MAX, hid1);
    __syncthreads();
  }
  if (J.s.n_hidden == 2) {
    mzt_hidden(tid, MZT_THREADS, J, row0, 1, hid1, MZ_NET_MAX_WIDTH, hid2);
    __syncthreads();
  }
  // (three calls, not a select of the pointers, as in mzp_group_net_pre)
  if (J.s.n_hidden == 2) mzt_output(tid, MZT_THREADS, J, row0, hid2, MZ_NET_MAX_WIDTH, outs);
  else if (J.s.n_hidden == 1) mzt_output(tid, MZT_THREADS, J, row0, hid1, MZ_NET_MAX_WIDTH, outs);
  else mzt_output(tid, MZT_THREADS, J, row0, xin, MZT_IN_MAX, outs);
  __syncthreads();
  mzt_epilogue_units(tid, MZT_THREADS, J, row0, outs);
  __syncthreads();
  mzt_epilogue_logp(tid, MZT_THREADS, J, row0, outs);
}
#endif
