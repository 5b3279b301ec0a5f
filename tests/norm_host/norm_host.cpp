// Host build of the normalised rows of mz_policy.h and of the scan of mz_returns.h (TEST INFRASTRUCTURE ONLY): what a bound handle's
// networks read, a network on such rows, and mz_return_scan, evaluated on the CPU, so that tests/test_obs_norm_api.py can compare them
// with mujoco_maze_amd/policy.py on a machine without a GPU.
#include <vector>

#include "../../mujoco_maze_amd/csrc/mz_policy.h"
#include "../../mujoco_maze_amd/csrc/mz_returns.h"

extern "C" {

// y[r] = the normalised row of obs[r] for `rows` rows of obs_dim floats; clip as the C-ABI takes it.  MZ_OK or MZ_ERR_ARG.
int mzh_norm_rows(const float* obs, int rows, int obs_dim, const float* mean, const float* inv_std, double clip, float* y) {
  if (!obs || !mean || !inv_std || !y || rows < 0 || obs_dim < 1 || !(clip > 0.0)) return MZ_ERR_ARG;
  for (int r = 0; r < rows; r++) mzp_norm_row(obs + (size_t)r * obs_dim, mean, inv_std, (float)clip, obs_dim, y + (size_t)r * obs_dim);
  return MZ_OK;
}

// act[r] = network(normalised row of obs[r]): shape = {n_hidden, h1, h2, activation}, no squash; row r reads its parameters at
// params + r * stride (0: one network for all rows)
int mzh_norm_policy(const float* params, long long stride, int obs_dim, int nu, const int* shape, const float* obs, int rows,
                    const float* mean, const float* inv_std, double clip, float* act) {
  if (!params || !shape || !obs || !mean || !inv_std || !act || obs_dim < 1 || nu < 1 || rows < 0 || !(clip > 0.0)) return MZ_ERR_ARG;
  const mzp_shape s{shape[0], shape[1], shape[2], shape[3]};
  std::vector<float> y((size_t)obs_dim);
  for (int r = 0; r < rows; r++) {
    mzp_norm_row(obs + (size_t)r * obs_dim, mean, inv_std, (float)clip, obs_dim, y.data());
    mzp_net_policy_row(params + (size_t)r * stride, obs_dim, nu, s, 0, 1.0f, y.data(), act + (size_t)r * nu);
  }
  return MZ_OK;
}

// mz_return_scan on [n_steps][n] rows: the scan of every env in turn; len_carry and len_seq nullable as in the C-ABI
int mzh_return_scan(int n_steps, int n, const float* reward, const unsigned char* done, double gamma, float* carry, int* len_carry,
                    float* ret_seq, int* len_seq) {
  if (!reward || !done || !carry || !ret_seq || n_steps < 1 || n < 1 || (len_seq && !len_carry)) return MZ_ERR_ARG;
  for (int e = 0; e < n; e++)
    mzr_scan(n_steps, (size_t)n, reward + e, done + e, gamma, carry + e, len_carry ? len_carry + e : nullptr, ret_seq + e,
             len_seq ? len_seq + e : nullptr);
  return MZ_OK;
}

}  // extern "C"
