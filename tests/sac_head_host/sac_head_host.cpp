// Host build of the state-dependent log-std head of mz_policy.h (TEST INFRASTRUCTURE ONLY): mzp_net_sample_head_row and its unit
// functions evaluated row by row on the CPU, so that tests/test_sac_head_api.py can compare them with mujoco_maze_amd/policy.py on a
// machine without a GPU.  With -DSAC_HEAD_HOST_MAIN the same file is a stand-alone program (`make sanitize` builds and runs it with
// -fsanitize=address,undefined): nothing of that program is loaded into Python.
#include "../../mujoco_maze_amd/csrc/mz_policy.h"

extern "C" {

// t_u of one unit (mzp_head_logp_term): the Gaussian term with the clamped log-std, minus the tanh correction where logp_squashed
float mzh_host_logp_term(float eps, float ls, float z, int logp_squashed, float logA) { return mzp_head_logp_term(eps, ls, z, logp_squashed, logA); }

float mzh_host_clamp(float r, float lo, float hi) { return mzp_head_clamp(r, lo, hi); }

int mzh_host_param_count(int obs_dim, int nu, int n_hidden, int h1, int h2) { return mzp_net_param_count(obs_dim, 2 * nu, mzp_shape{n_hidden, h1, h2, 0}); }

// act[r], logp[r] = one draw of a head actor for row r, global env slot slots[r] (mzp_net_sample_head_row).  obs [rows][obs_dim], act
// [rows][nu], logp [rows] (nullable); row r reads its actor at params + r * param_stride (0: one for all rows).  logA is computed here
// as the library computes it: logf((float)action_scale).  MZ_OK or MZ_ERR_ARG.
int mzh_host_sample_head(const float* params, long long param_stride, int obs_dim, int nu, int n_hidden, int h1, int h2, int activation, int squash,
                         double action_scale, float lo, float hi, int logp_squashed, unsigned long long noise_seed, unsigned long long noise_step,
                         const unsigned long long* slots, const float* obs, int rows, float* act, float* logp) {
  if (!params || !obs || !act || !slots || obs_dim < 1 || nu < 1 || rows < 0 || n_hidden < 0 || n_hidden > MZ_NET_MAX_HIDDEN_LAYERS) return MZ_ERR_ARG;
  if ((squash != 0 && squash != 1) || (logp_squashed != 0 && logp_squashed != 1) || (logp_squashed && !squash)) return MZ_ERR_ARG;
  if (h1 < 0 || h1 > MZ_POLICY_MAX_HIDDEN || h2 < 0 || h2 > MZ_POLICY_MAX_HIDDEN) return MZ_ERR_ARG;
  if (lo != lo || hi != hi || lo > hi) return MZ_ERR_ARG;
  const mzp_shape s{n_hidden, h1, h2, activation};
  if (param_stride != 0 && param_stride != (long long)mzp_net_param_count(obs_dim, 2 * nu, s)) return MZ_ERR_ARG;
  const float scale = (float)action_scale;
  const mzp_head hd{lo, hi, logp_squashed, logf(scale)};
  for (int r = 0; r < rows; r++)
    mzp_net_sample_head_row(params + (size_t)r * param_stride, obs_dim, nu, s, squash, scale, hd, noise_seed, noise_step, slots[r],
                            obs + (size_t)r * obs_dim, act + (size_t)r * nu, logp ? logp + r : nullptr);
  return MZ_OK;
}

}  // extern "C"

#ifdef SAC_HEAD_HOST_MAIN
// The stand-alone program: every array an exact-size heap allocation, so a read or write past a row is an AddressSanitizer report; the
// raw log-std biases run through NaN, +-inf and values far outside the clamp, the observations through NaN and +-inf, the bounds
// through (-20, 2), (-inf, +inf) and a single point.
#include <stdio.h>

#include <vector>

int main() {
  const int shapes[][3] = {{0, 0, 0}, {1, 5, 0}, {1, 64, 0}, {2, 5, 3}, {2, 64, 64}};
  const float specials[] = {NAN, INFINITY, -INFINITY, 100.0f, -100.0f, 2.0f, 0.0f};
  const float bounds[][2] = {{-20.0f, 2.0f}, {-INFINITY, INFINITY}, {-1.0f, -1.0f}};
  long checked = 0;
  for (const auto& sh : shapes)
    for (int obs_dim : {1, 7, 123})
      for (int nu : {1, 2, 8})
        for (int activation : {MZ_ACT_TANH, MZ_ACT_RELU})
          for (int squash = 0; squash <= 1; squash++)
            for (int lsq = 0; lsq <= squash; lsq++)
              for (const auto& b : bounds) {
                const int rows = 9;
                const int count = mzh_host_param_count(obs_dim, nu, sh[0], sh[1], sh[2]);
                std::vector<float> par((size_t)rows * count), obs((size_t)rows * obs_dim), act((size_t)rows * nu), logp(rows);
                std::vector<unsigned long long> slots(rows);
                for (size_t i = 0; i < par.size(); i++) par[i] = 0.01f * (float)((int)(i * 2654435761u % 201u) - 100);
                for (size_t i = 0; i < obs.size(); i++) obs[i] = 0.03f * (float)((int)(i * 40503u % 201u) - 100);
                for (int r = 0; r < rows; r++) {
                  slots[r] = r == 8 ? ~0ULL : (unsigned long long)r * 1000003ULL;
                  if (r < 7) par[(size_t)r * count + count - 1] = specials[r];  // the bias of the last raw log-std unit
                }
                obs[0] = NAN;
                if (obs_dim > 1) { obs[obs_dim] = INFINITY; obs[2 * obs_dim + 1] = -INFINITY; }
                for (int with_logp = 0; with_logp <= 1; with_logp++) {
                  const int rc = mzh_host_sample_head(par.data(), count, obs_dim, nu, sh[0], sh[1], sh[2], activation, squash, 0.9, b[0], b[1], lsq, 77ULL,
                                                      ~0ULL, slots.data(), obs.data(), rows, act.data(), with_logp ? logp.data() : nullptr);
                  if (rc != MZ_OK) { printf("refused: rc %d\n", rc); return 1; }
                  if (squash)
                    for (float a : act)
                      if (!(isnan(a) || fabsf(a) <= 0.9f)) { printf("an action outside the range: %g\n", a); return 1; }
                  checked += rows;
                }
                // row 8 is finite (no special, finite obs from row 3 on): its log-prob is a number unless the bounds allow an overflow
                if (b[1] <= 2.0f && !(logp[8] == logp[8])) { printf("NaN log-prob in a finite row\n"); return 1; }
              }
  printf("sac_head_host under the sanitizers: %ld rows, no report\n", checked);
  return 0;
}
#endif
