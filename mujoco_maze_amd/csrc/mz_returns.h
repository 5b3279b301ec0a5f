// mz_returns.h — the forward scan of mz_return_scan (include/mazestep.h): the running discounted return and the episode step count of
// one env over the rows a rollout wrote, cut at episode ends and carried from one call to the next.  The twin of mz_gae.h; shared
// by return_scan_kernel (mazestep.hip: one lane per env) and a host build (tests/norm_host) that pins it against
// mujoco_maze_amd/policy.py return_scan_reference.
//
// fp32 throughout, every operation rounded separately (the pragma below; a host build adds -ffp-contract=off), k from 0 up to
// n_steps - 1, `carry` (float) and `len` (int32) per env, in and out:
//     g = (float)gamma
//     p = g * carry;  s = p + reward[k];  ret_seq[k] = s;  len = len + 1;  len_seq[k] = len                            mzr_step
//     carry = done[k] ? 0.0f : s;         len = done[k] ? 0 : len
// Selects, not multiplications by a mask: a NaN return does not survive the episode's end.  With gamma == 1 the product is exact, so
// ret_seq[k] where done[k] != 0 is that episode's return (the sequential fp32 sum of its rewards) and len_seq[k] its length; with
// gamma < 1 ret_seq is the series whose running variance reward scaling divides by.  A scan over K1 steps followed by a scan over K2
// steps with the carries it left equals one scan over K1 + K2 steps.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MZRS_HD __host__ __device__ __forceinline__
#else
#define MZRS_HD inline
#endif

// step k of one env: returns ret_seq[k]; *carry and *len are updated, *len_out = len_seq[k]
MZRS_HD float mzr_step(float reward, uint8_t done, float g, float* carry, int32_t* len, int32_t* len_out) {
#pragma clang fp contract(off) reassociate(off)
  const float p = g * *carry;
  const float s = p + reward;
  const int32_t n = *len + 1;
  *len_out = n;
  *carry = done ? 0.0f : s;
  *len = done ? 0 : n;
  return s;
}

// THE scan of one env: element k of every [n_steps, N] array at [k * stride] (stride = num_envs); len_carry and len_seq nullable
// (without len_carry the length is not tracked and len_seq is not written)
MZRS_HD void mzr_scan(int n_steps, size_t stride, const float* reward, const uint8_t* done, double gamma, float* carry, int32_t* len_carry,
                     float* ret_seq, int32_t* len_seq) {
  const float g = (float)gamma;
  float c = *carry;
  int32_t len = len_carry ? *len_carry : 0;
  for (int k = 0; k < n_steps; k++) {
    const size_t i = (size_t)k * stride;
    int32_t lo;
    ret_seq[i] = mzr_step(reward[i], done[i], g, &c, &len, &lo);
    if (len_carry && len_seq) len_seq[i] = lo;
  }
  *carry = c;
  if (len_carry) *len_carry = len;
}
