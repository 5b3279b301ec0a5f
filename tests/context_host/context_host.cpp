// Host build of the context inputs of mz_policy.h (TEST INFRASTRUCTURE ONLY): mzp_input_row, the network row functions on the row
// it stages and mzp_ctx_transition_row, evaluated row by row on the CPU, so that tests/test_context_api.py can compare them with
// mujoco_maze_amd/policy.py on a machine without a GPU.  With -DCONTEXT_HOST_MAIN the same file is a stand-alone program
// (`make sanitize` builds and runs it with -fsanitize=address,undefined): nothing of that program is loaded into Python.
#include "../../mujoco_maze_amd/csrc/mz_policy.h"

#include <vector>

extern "C" {

int mzc_host_max_context(void) { return MZ_MAX_CONTEXT; }

int mzc_host_param_count(int obs_dim, int cdim, int nout, int n_hidden, int h1, int h2) {
  return mzp_net_param_count(obs_dim + cdim, nout, mzp_shape{n_hidden, h1, h2, 0});
}

// out[r] = the network on r_r = [y | c] (mzp_input_row): an actor's nout actions (value == 0) or a critic's one value (value == 1:
// nout is 1 and squash is not read).  obs [rows][obs_dim], ctx [rows][cdim], mean / inv_std [obs_dim] or both NULL (no normaliser),
// out [rows][nout]; row r reads its network at params + r * param_stride (0: one for all rows).  The staged row is an exact-size
// allocation of obs_dim + cdim floats.  MZ_OK or MZ_ERR_ARG.
int mzc_host_eval(const float* params, long long param_stride, int obs_dim, int cdim, int nout, int n_hidden, int h1, int h2, int activation,
                  int squash, double action_scale, const float* mean, const float* inv_std, double clip, const float* obs, const float* ctx, int rows,
                  int value, float* out) {
  if (!params || !obs || !ctx || !out || obs_dim < 1 || nout < 1 || rows < 0 || n_hidden < 0 || n_hidden > MZ_NET_MAX_HIDDEN_LAYERS) return MZ_ERR_ARG;
  if (cdim < 1 || cdim > MZ_MAX_CONTEXT || (mean == nullptr) != (inv_std == nullptr)) return MZ_ERR_ARG;
  if (h1 < 0 || h1 > MZ_POLICY_MAX_HIDDEN || h2 < 0 || h2 > MZ_POLICY_MAX_HIDDEN || (value && nout != 1)) return MZ_ERR_ARG;
  const mzp_shape s{n_hidden, h1, h2, activation};
  const int nin = obs_dim + cdim;
  if (param_stride != 0 && param_stride != (long long)mzp_net_param_count(nin, nout, s)) return MZ_ERR_ARG;
  std::vector<float> r((size_t)nin);
  for (int k = 0; k < rows; k++) {
    mzp_input_row(obs + (size_t)k * obs_dim, obs_dim, mean, inv_std, (float)clip, ctx + (size_t)k * cdim, cdim, r.data());
    const float* par = params + (size_t)k * param_stride;
    if (value) out[k] = mzp_net_value_row(par, nin, s, r.data());
    else mzp_net_policy_row(par, nin, nout, s, squash, (float)action_scale, r.data(), out + (size_t)k * nout);
  }
  return MZ_OK;
}

// the relative transition of `rows` rows in place (mzp_ctx_transition_row): ctx [rows][cdim], s and s2 [rows][obs_dim], done [rows]
int mzc_host_transition(float* ctx, int rows, int cdim, int rel_dims, const float* s, const float* s2, int obs_dim, const unsigned char* done) {
  if (!ctx || !s || !s2 || !done || rows < 0 || cdim < 1 || cdim > MZ_MAX_CONTEXT) return MZ_ERR_ARG;
  if (rel_dims < 1 || rel_dims > cdim || rel_dims > obs_dim) return MZ_ERR_ARG;
  for (int k = 0; k < rows; k++)
    mzp_ctx_transition_row(ctx + (size_t)k * cdim, rel_dims, s + (size_t)k * obs_dim, s2 + (size_t)k * obs_dim, done[k]);
  return MZ_OK;
}

}  // extern "C"

#ifdef CONTEXT_HOST_MAIN
// The stand-alone program: every array an exact-size heap allocation, so a read or write past a row is an AddressSanitizer report;
// the context runs through NaN and +-inf, the widths through 1 and MZ_MAX_CONTEXT.
#include <stdio.h>

int main() {
  const int shapes[][3] = {{0, 0, 0}, {1, 5, 0}, {2, 5, 3}, {2, 64, 64}};
  long checked = 0;
  for (const auto& sh : shapes)
    for (int obs_dim : {1, 7, 123})
      for (int cdim : {1, 5, MZ_MAX_CONTEXT})
        for (int nout : {1, 2, 8})
          for (int norm = 0; norm <= 1; norm++) {
            const int rows = 6, nin = obs_dim + cdim;
            const int count = mzc_host_param_count(obs_dim, cdim, nout, sh[0], sh[1], sh[2]);
            std::vector<float> par((size_t)rows * count), obs((size_t)rows * obs_dim), ctx((size_t)rows * cdim), out((size_t)rows * nout), val(rows);
            std::vector<float> mean(obs_dim, 0.25f), inv(obs_dim, 2.0f), s2((size_t)rows * obs_dim);
            std::vector<unsigned char> done(rows);
            for (size_t i = 0; i < par.size(); i++) par[i] = 0.01f * (float)((int)(i * 2654435761u % 201u) - 100);
            for (size_t i = 0; i < obs.size(); i++) { obs[i] = 0.03f * (float)((int)(i * 40503u % 201u) - 100); s2[i] = obs[i] + 0.5f; }
            for (size_t i = 0; i < ctx.size(); i++) ctx[i] = 0.02f * (float)((int)(i * 7919u % 201u) - 100);
            ctx[0] = NAN; ctx[cdim - 1 + cdim] = INFINITY; ctx[2 * cdim] = -INFINITY;
            for (int r = 0; r < rows; r++) done[r] = (unsigned char)(r % 3 == 1);
            int rc = mzc_host_eval(par.data(), count, obs_dim, cdim, nout, sh[0], sh[1], sh[2], MZ_ACT_RELU, 0, 1.0, norm ? mean.data() : nullptr,
                                   norm ? inv.data() : nullptr, 5.0, obs.data(), ctx.data(), rows, 0, out.data());
            if (rc == MZ_OK) {
              const int vcount = mzc_host_param_count(obs_dim, cdim, 1, sh[0], sh[1], sh[2]);
              std::vector<float> vpar((size_t)vcount, 0.125f);
              rc = mzc_host_eval(vpar.data(), 0, obs_dim, cdim, 1, sh[0], sh[1], sh[2], MZ_ACT_TANH, 0, 1.0, norm ? mean.data() : nullptr,
                                 norm ? inv.data() : nullptr, 5.0, obs.data(), ctx.data(), rows, 1, val.data());
            }
            const int D = cdim < obs_dim ? cdim : obs_dim;
            if (rc == MZ_OK) rc = mzc_host_transition(ctx.data(), rows, cdim, D, obs.data(), s2.data(), obs_dim, done.data());
            if (rc != MZ_OK) { printf("refused: rc %d\n", rc); return 1; }
            // rows 3 .. 5 are finite: so are their outputs, and row 4 (done) kept its context
            for (int r = 3; r < rows; r++)
              for (int u = 0; u < nout; u++)
                if (!(out[(size_t)r * nout + u] == out[(size_t)r * nout + u])) { printf("NaN output in a finite row\n"); return 1; }
            if (ctx[(size_t)4 * cdim] != 0.02f * (float)((int)((size_t)4 * cdim * 7919u % 201u) - 100)) { printf("a done row moved\n"); return 1; }
            (void)nin;
            checked += rows;
          }
  printf("context_host under the sanitizers: %ld rows, no report\n", checked);
  return 0;
}
#endif
