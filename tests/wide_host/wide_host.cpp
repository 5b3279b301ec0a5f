// Host build of the tiled network kernel of csrc/mz_net_tile.h (TEST INFRASTRUCTURE ONLY): the per-thread phase functions of
// net_tile_kernel, run the way a block runs them — every thread index of the block through one phase, then the next phase —, on arrays
// that stand for the block's LDS.  tests/test_wide_nets_api.py compares the results with mujoco_maze_amd/policy.py and with the row
// functions of tests/net_host on a machine without a GPU: that is where the index arithmetic of the tile is checked.  With
// -DWIDE_HOST_MAIN the same file is a stand-alone program (`make sanitize` builds and runs it with -fsanitize=address,undefined):
// nothing of that program is loaded into Python.
#include <math.h>

#include <vector>

#include "../../mujoco_maze_amd/csrc/mz_net_tile.h"

// net_tile_kernel for the tile at `block`, with `T` threads; the four LDS arrays are exact-size heap allocations filled with NaN, so a
// read of an element no phase wrote shows in the result and an access past an array is an AddressSanitizer report
static void run_tile(const mzt_job& J, size_t block, int T) {
  std::vector<float> xin((size_t)MZT_ROWS * MZT_IN_MAX, NAN), hid1((size_t)MZT_ROWS * MZ_NET_MAX_WIDTH, NAN),
      hid2((size_t)MZT_ROWS * MZ_NET_MAX_WIDTH, NAN), outs((size_t)MZT_ROWS * MZT_OUT_MAX, NAN);
  const size_t row0 = block * MZT_ROWS;
  for (int tid = 0; tid < T; tid++) mzt_stage(tid, T, J, row0, xin.data());
  if (J.s.n_hidden >= 1)
    for (int tid = 0; tid < T; tid++) mzt_hidden(tid, T, J, row0, 0, xin.data(), MZT_IN_MAX, hid1.data());
  if (J.s.n_hidden == 2)
    for (int tid = 0; tid < T; tid++) mzt_hidden(tid, T, J, row0, 1, hid1.data(), MZ_NET_MAX_WIDTH, hid2.data());
  const float* in = J.s.n_hidden == 2 ? hid2.data() : (J.s.n_hidden == 1 ? hid1.data() : xin.data());
  const int stride = J.s.n_hidden ? MZ_NET_MAX_WIDTH : MZT_IN_MAX;
  for (int tid = 0; tid < T; tid++) mzt_output(tid, T, J, row0, in, stride, outs.data());
  for (int tid = 0; tid < T; tid++) mzt_epilogue_units(tid, T, J, row0, outs.data());
  for (int tid = 0; tid < T; tid++) mzt_epilogue_logp(tid, T, J, row0, outs.data());
}

extern "C" {

int mzw_host_max_width(void) { return MZ_NET_MAX_WIDTH; }
int mzw_host_rows(void) { return MZT_ROWS; }
int mzw_host_in_max(void) { return MZT_IN_MAX; }

// One launch of the tiled kernel on `rows` rows with blocks of `threads` threads (the device's: MZT_THREADS; any count >= 1 gives the
// same bits).  kind: MZT_ACT 0, MZT_SAMPLE 1, MZT_HEAD 2, MZT_VALUE 3.  shape: n_hidden, h1, h2, activation.  obs [rows][obs_dim];
// final_obs / done nullable (row r from final_obs where done[r]); mean / inv_std nullable (the raw bits); ctx [rows][cdim] with
// cdim > 0.  params: one network (param_stride 0) or row r's at params + r * param_stride.  actions [rows][nu], logp [rows]
// (nullable), values [rows] by kind.  MZ_OK or MZ_ERR_ARG.
int mzw_host_run(int kind, int rows, int obs_dim, int cdim, int nu, const int* shape, int squash, double action_scale, int mode, float lo, float hi,
                 int logp_squashed, const float* params, long long param_stride, unsigned long long noise_seed, unsigned long long noise_step,
                 unsigned long long env0, const float* obs, const float* final_obs, const unsigned char* done, const float* mean,
                 const float* inv_std, float clip, const float* ctx, float* actions, float* logp, float* values, int threads) {
  if (kind < MZT_ACT || kind > MZT_VALUE || rows < 1 || obs_dim < 1 || cdim < 0 || nu < 1 || !shape || !params || !obs || threads < 1) return MZ_ERR_ARG;
  if (shape[0] < 0 || shape[0] > MZ_NET_MAX_HIDDEN_LAYERS || (shape[3] != MZ_ACT_TANH && shape[3] != MZ_ACT_RELU)) return MZ_ERR_ARG;
  for (int k = 0; k < MZ_NET_MAX_HIDDEN_LAYERS; k++)
    if (k < shape[0] ? (shape[1 + k] < 1 || shape[1 + k] > MZ_NET_MAX_WIDTH) : shape[1 + k] != 0) return MZ_ERR_ARG;
  if (obs_dim + cdim > MZT_IN_MAX || (cdim > 0 && !ctx) || (!mean) != (!inv_std) || (!final_obs) != (!done)) return MZ_ERR_ARG;
  if (kind == MZT_VALUE ? !values : !actions) return MZ_ERR_ARG;
  mzt_job J{};
  J.kind = kind; J.n = rows; J.obs_dim = obs_dim; J.cdim = cdim; J.nu = nu;
  J.s = mzp_shape{shape[0], shape[1], shape[2], shape[3]};
  if (mzt_nout(J) > MZT_OUT_MAX) return MZ_ERR_ARG;
  const long long count = mzp_net_param_count(obs_dim + cdim, mzt_nout(J), J.s) + (kind == MZT_SAMPLE ? nu : 0);
  if (param_stride != 0 && param_stride != count) return MZ_ERR_ARG;
  J.squash = squash; J.action_scale = (float)action_scale; J.mode = mode;
  J.hd = mzp_head{lo, hi, logp_squashed, logf((float)action_scale)};
  J.params = params; J.pstride = (long)param_stride;
  J.key = mzp_noise_key(noise_seed, noise_step); J.env0 = env0;
  J.obs = obs; J.final_obs = final_obs; J.done = done; J.mean = mean; J.inv_std = inv_std; J.clip = clip; J.ctx = ctx;
  J.actions = actions; J.logp = logp; J.values = values;
  for (size_t b = 0; b < ((size_t)rows + MZT_ROWS - 1) / MZT_ROWS; b++) run_tile(J, b, threads);
  return MZ_OK;
}

}  // extern "C"

#ifdef WIDE_HOST_MAIN
// The stand-alone program: every array an exact-size heap allocation; the shapes, observation widths, action counts and row counts of
// tests/test_wide_nets_api.py, shared and per-row parameters, every kind, both block sizes; NaN and +-inf in the observations.
#include <stdio.h>

int main() {
  const int shapes[][3] = {{0, 0, 0}, {1, 65, 0}, {1, 200, 0}, {2, 96, 130}, {2, 256, 256}, {2, 64, 64}, {2, 5, 3}, {1, 1, 0}, {2, 256, 1}};
  const int dims[][2] = {{6, 0}, {30, 0}, {123, 32}, {1, 1}};
  long checked = 0;
  for (const auto& sh : shapes)
    for (const auto& d : dims)
      for (int nu : {2, 8})
        for (int rows : {1, 3, MZT_ROWS + 5, 37})
          for (int per_row = 0; per_row <= 1; per_row++)
            for (int kind = MZT_ACT; kind <= MZT_VALUE; kind++) {
              if (per_row && (rows == 37 || (sh[1] == 256 && rows > 3))) continue;  // (keeps the run short: the mapping does not depend on it)
              const int obs_dim = d[0], cdim = d[1], act = (kind + rows) & 1;
              const int shape[4] = {sh[0], sh[1], sh[2], act};
              const int nout = kind == MZT_VALUE ? 1 : (kind == MZT_HEAD ? 2 * nu : nu);
              const int count = mzp_net_param_count(obs_dim + cdim, nout, mzp_shape{sh[0], sh[1], sh[2], act}) + (kind == MZT_SAMPLE ? nu : 0);
              std::vector<float> par((size_t)(per_row ? rows : 1) * count), obs((size_t)rows * obs_dim), fin((size_t)rows * obs_dim),
                  ctx((size_t)rows * cdim), mean(obs_dim, 0.1f), inv(obs_dim, 1.5f), actions((size_t)rows * nu), logp(rows), values(rows);
              std::vector<unsigned char> done(rows);
              for (size_t i = 0; i < par.size(); i++) par[i] = 0.01f * (float)((int)(i * 2654435761u % 201u) - 100);
              for (size_t i = 0; i < obs.size(); i++) { obs[i] = 0.03f * (float)((int)(i * 40503u % 201u) - 100); fin[i] = -obs[i]; }
              for (size_t i = 0; i < ctx.size(); i++) ctx[i] = 0.02f * (float)((int)(i * 7919u % 101u) - 50);
              for (int r = 0; r < rows; r++) done[r] = (unsigned char)(r % 3 == 1);
              obs[0] = NAN;
              if (rows > 2 && obs_dim > 1) { obs[obs_dim] = INFINITY; obs[2 * obs_dim + 1] = -INFINITY; }
              for (int threads : {MZT_THREADS, 64}) {
                const int with_norm = (rows + threads) & 1, with_done = kind == MZT_VALUE;
                const int rc = mzw_host_run(kind, rows, obs_dim, cdim, nu, shape, kind != MZT_VALUE, 0.9, kind == MZT_SAMPLE ? (rows & 1) : 0, -20.0f, 2.0f,
                                            kind == MZT_HEAD, par.data(), per_row ? count : 0, 77ULL, ~0ULL, 1000003ULL, obs.data(),
                                            with_done ? fin.data() : nullptr, with_done ? done.data() : nullptr, with_norm ? mean.data() : nullptr,
                                            with_norm ? inv.data() : nullptr, 5.0f, cdim ? ctx.data() : nullptr, actions.data(), logp.data(),
                                            values.data(), threads);
                if (rc != MZ_OK) { printf("refused: rc %d\n", rc); return 1; }
                if (kind != MZT_VALUE)
                  for (float a : actions)
                    if (!(isnan(a) || fabsf(a) <= 0.9f)) { printf("an action outside the range: %g\n", a); return 1; }
                checked += rows;
              }
            }
  printf("wide_host under the sanitizers: %ld rows, no report\n", checked);
  return 0;
}
#endif
