// Host build of the two noise modes of mz_policy.h (TEST INFRASTRUCTURE ONLY): mzp_sample_unit and the row functions mzp_sample_row /
// mzp_net_sample_row with the mode as an argument, evaluated row by row on the CPU, so that tests/test_transitions_api.py can compare
// MZ_NOISE_PRE_SQUASH and MZ_NOISE_ACTION with mujoco_maze_amd/policy.py on a machine without a GPU.
#include "../../mujoco_maze_amd/csrc/mz_policy.h"

extern "C" {

float mzp_host_sample_unit(float m, float log_std, float eps, int squash, float action_scale, int mode) {
  return mzp_sample_unit(m, log_std, eps, squash, action_scale, mode);
}

// act[r], logp[r] = one draw for row r, global env slot slots[r], through mzp_sample_row (legacy != 0: n_hidden <= 1, tanh, width h1)
// or mzp_net_sample_row (a network of shape n_hidden / h1 / h2 / activation).  obs [rows][obs_dim], act [rows][nu], logp [rows]
// (nullable); row r reads its policy at params + r * param_stride (0: one for all rows).  MZ_OK or MZ_ERR_ARG.
int mzp_host_noise_sample(int legacy, const float* params, long long param_stride, int obs_dim, int nu, int n_hidden, int h1, int h2, int activation,
                          int squash, double action_scale, int mode, unsigned long long noise_seed, unsigned long long noise_step,
                          const unsigned long long* slots, const float* obs, int rows, float* act, float* logp) {
  if (!params || !obs || !act || !slots || obs_dim < 1 || nu < 1 || rows < 0 || n_hidden < 0 || n_hidden > MZ_NET_MAX_HIDDEN_LAYERS) return MZ_ERR_ARG;
  if ((squash != 0 && squash != 1) || (mode != MZ_NOISE_PRE_SQUASH && mode != MZ_NOISE_ACTION)) return MZ_ERR_ARG;
  if (h1 < 0 || h1 > MZ_POLICY_MAX_HIDDEN || h2 < 0 || h2 > MZ_POLICY_MAX_HIDDEN) return MZ_ERR_ARG;
  if (legacy && (n_hidden > 1 || activation != MZ_ACT_TANH)) return MZ_ERR_ARG;
  const mzp_shape s{n_hidden, h1, h2, activation};
  if (param_stride != 0 && param_stride != (long long)mzp_net_param_count(obs_dim, nu, s) + nu) return MZ_ERR_ARG;
  const float scale = (float)action_scale;
  for (int r = 0; r < rows; r++) {
    const float* p = params + (size_t)r * param_stride;
    const float* x = obs + (size_t)r * obs_dim;
    if (legacy)
      mzp_sample_row(p, obs_dim, nu, n_hidden ? h1 : 0, squash, scale, noise_seed, noise_step, slots[r], x, act + (size_t)r * nu, logp ? logp + r : nullptr, mode);
    else
      mzp_net_sample_row(p, obs_dim, nu, s, squash, scale, noise_seed, noise_step, slots[r], x, act + (size_t)r * nu, logp ? logp + r : nullptr, mode);
  }
  return MZ_OK;
}

}  // extern "C"
