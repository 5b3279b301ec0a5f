// Host build of mz_policy.h (TEST INFRASTRUCTURE ONLY): the policy of mz_policy_act / mz_rollout_policy evaluated row by row on the
// CPU, so that tests/test_policy_api.py can compare it with mujoco_maze_amd/policy.py on a machine without a GPU.
#include "../../mujoco_maze_amd/csrc/mz_policy.h"

extern "C" {

int mzp_host_param_count(int obs_dim, int nu, int hidden) { return mzp_param_count(obs_dim, nu, hidden); }

// act[r] = policy(obs[r]) for `rows` rows: obs [rows][obs_dim], act [rows][nu]; row r reads its policy at params + r * param_stride
// (0: one policy for all rows).  action_scale is narrowed to fp32 once, as the C-ABI does.  MZ_OK or MZ_ERR_ARG.
int mzp_host_policy(const float* params, long long param_stride, int obs_dim, int nu, int hidden, int squash, double action_scale,
                    const float* obs, int rows, float* act) {
  if (!params || !obs || !act || obs_dim < 1 || nu < 1 || rows < 0 || hidden < 0 || hidden > MZ_POLICY_MAX_HIDDEN || (squash != 0 && squash != 1))
    return MZ_ERR_ARG;
  if (param_stride != 0 && param_stride != (long long)mzp_param_count(obs_dim, nu, hidden)) return MZ_ERR_ARG;
  const float scale = (float)action_scale;
  for (int r = 0; r < rows; r++)
    mzp_policy_row(params + (size_t)r * param_stride, obs_dim, nu, hidden, squash, scale, obs + (size_t)r * obs_dim, act + (size_t)r * nu);
  return MZ_OK;
}

}  // extern "C"
