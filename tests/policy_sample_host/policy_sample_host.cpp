// Host build of the stochastic policy of mz_policy.h (TEST INFRASTRUCTURE ONLY): the noise stream, the sample and the log-prob of
// mz_policy_sample / mz_rollout_policy_sample evaluated row by row on the CPU, so that tests/test_policy_sample_api.py can compare
// them with mujoco_maze_amd/policy.py on a machine without a GPU.
#include "../../mujoco_maze_amd/csrc/mz_policy.h"

extern "C" {

unsigned long long mzp_host_noise_key(unsigned long long noise_seed, unsigned long long noise_step) { return mzp_noise_key(noise_seed, noise_step); }

// the two words behind eps(key, slot, u)
void mzp_host_noise_words(unsigned long long key, unsigned long long slot, int u, unsigned int* words) {
  words[0] = rng_u32(key, slot, 2u * (uint32_t)u);
  words[1] = rng_u32(key, slot, 2u * (uint32_t)u + 1u);
}

// the seed of an env's episode (mz_rng.h): what every reset kernel and every in-step auto-reset keys its draws by
unsigned long long mzp_host_episode_seed(unsigned long long seed, unsigned int episode) { return episode_seed(seed, episode); }

float mzp_host_eps(unsigned long long noise_seed, unsigned long long noise_step, unsigned long long slot, int u) {
  return mzp_eps(mzp_noise_key(noise_seed, noise_step), slot, u);
}

// act[r], logp[r] = one draw for row r, global env slot slots[r]: obs [rows][obs_dim], act [rows][nu], logp [rows] (nullable); row r
// reads its policy at params + r * param_stride (0: one for all rows; else npar_s).  MZ_OK or MZ_ERR_ARG.
int mzp_host_sample(const float* params, long long param_stride, int obs_dim, int nu, int hidden, int squash, double action_scale,
                    unsigned long long noise_seed, unsigned long long noise_step, const unsigned long long* slots, const float* obs, int rows,
                    float* act, float* logp) {
  if (!params || !obs || !act || !slots || obs_dim < 1 || nu < 1 || rows < 0 || hidden < 0 || hidden > MZ_POLICY_MAX_HIDDEN || (squash != 0 && squash != 1))
    return MZ_ERR_ARG;
  if (param_stride != 0 && param_stride != (long long)mzp_param_count(obs_dim, nu, hidden) + nu) return MZ_ERR_ARG;
  const float scale = (float)action_scale;
  for (int r = 0; r < rows; r++)
    mzp_sample_row(params + (size_t)r * param_stride, obs_dim, nu, hidden, squash, scale, noise_seed, noise_step, slots[r],
                   obs + (size_t)r * obs_dim, act + (size_t)r * nu, logp ? logp + r : nullptr);
  return MZ_OK;
}

}  // extern "C"
