// Host build of the critic of mz_policy.h and of the scan of mz_gae.h (TEST INFRASTRUCTURE ONLY): mz_value and mz_gae evaluated on the
// CPU, so that tests/test_critic_api.py can compare them with mujoco_maze_amd/policy.py on a machine without a GPU.
#include "../../mujoco_maze_amd/csrc/mz_gae.h"
#include "../../mujoco_maze_amd/csrc/mz_policy.h"

extern "C" {

unsigned long long mzc_host_sizeof_critic(void) { return sizeof(mz_critic); }

// values[r] = V(obs[r]) for `rows` rows: obs [rows][obs_dim]; row r reads its critic at vparams + r * stride (0: one critic for all
// rows).  MZ_OK or MZ_ERR_ARG.
int mzc_host_value(const float* vparams, long long stride, int obs_dim, int hidden, const float* obs, int rows, float* values) {
  if (!vparams || !obs || !values || obs_dim < 1 || rows < 0 || hidden < 0 || hidden > MZ_POLICY_MAX_HIDDEN) return MZ_ERR_ARG;
  if (stride != 0 && stride != (long long)mzp_param_count(obs_dim, 1, hidden)) return MZ_ERR_ARG;
  for (int r = 0; r < rows; r++) values[r] = mzp_value_row(vparams + (size_t)r * stride, obs_dim, hidden, obs + (size_t)r * obs_dim);
  return MZ_OK;
}

// mz_gae on [n_steps][n] rows: the scan of every env in turn; ret nullable
int mzc_host_gae(int n_steps, int n, const float* reward, const unsigned char* done, const float* value, const float* next_value, double gamma,
                 double lam, float* adv, float* ret) {
  if (!reward || !done || !value || !next_value || !adv || n_steps < 1 || n < 1) return MZ_ERR_ARG;
  for (int e = 0; e < n; e++)
    mzg_scan(n_steps, (size_t)n, reward + e, done + e, value + e, next_value + e, gamma, lam, adv + e, ret ? ret + e : nullptr);
  return MZ_OK;
}

}  // extern "C"
