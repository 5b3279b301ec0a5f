// mz_gae.h — the backward scan of mz_gae (include/mazestep.h): generalised advantage estimates and returns of one env from the rows
// a rollout wrote.  Shared by gae_kernel (mazestep.hip: one lane per env) and a host build (tests/critic_host) that pins it against
// mujoco_maze_amd/policy.py gae_reference.
//
// fp32 throughout, every operation rounded separately (the pragma below; a host build adds -ffp-contract=off), k from n_steps - 1
// down to 0 with carry = 0 at the start:
//     g = (float)gamma;  gl = g * (float)lam                                                                          mzg_coeffs
//     b     = (done & 1) ? 0.0f : g * next_value      true termination: no bootstrap; a time limit alone (done == 2) bootstraps
//     delta = (reward + b) - value                    from the value of the terminal observation
//     c     = done ? 0.0f : gl * carry                any episode end cuts the recursion
//     adv   = delta + c;  carry = adv;  ret = adv + value                                                             mzg_step
// Selects, not multiplications by a mask: a NaN bootstrap value behind a true termination, or a NaN carry behind an episode end,
// does not reach the result.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MZG_HD __host__ __device__ __forceinline__
#else
#define MZG_HD inline
#endif

MZG_HD void mzg_coeffs(double gamma, double lam, float* g, float* gl) {
#pragma clang fp contract(off) reassociate(off)
  *g = (float)gamma;
  *gl = *g * (float)lam;
}

// step k of one env: returns adv (the new carry), *ret = adv + value
MZG_HD float mzg_step(float reward, uint8_t done, float value, float next_value, float g, float gl, float carry, float* ret) {
#pragma clang fp contract(off) reassociate(off)
  const float gb = g * next_value;
  const float b = (done & 1) ? 0.0f : gb;
  const float s = reward + b;
  const float delta = s - value;
  const float gc = gl * carry;
  const float c = done ? 0.0f : gc;
  const float adv = delta + c;
  *ret = adv + value;
  return adv;
}

// THE scan of one env: element k of every array at [k * stride] (stride = num_envs for the [n_steps, N] rows of a rollout); ret nullable
MZG_HD void mzg_scan(int n_steps, size_t stride, const float* reward, const uint8_t* done, const float* value, const float* next_value,
                     double gamma, double lam, float* adv, float* ret) {
  float g, gl, carry = 0.0f;
  mzg_coeffs(gamma, lam, &g, &gl);
  for (int k = n_steps - 1; k >= 0; k--) {
    const size_t i = (size_t)k * stride;
    float r;
    carry = mzg_step(reward[i], done[i], value[i], next_value[i], g, gl, carry, &r);
    adv[i] = carry;
    if (ret) ret[i] = r;
  }
}
