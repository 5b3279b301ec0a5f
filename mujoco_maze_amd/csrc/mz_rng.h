// mz_rng.h — the integer part of the counter-based RNG, ONE definition for the device kernels (through mz_device.h: the reset
// distribution; through mz_policy.h: the policy noise) and for host builds (tests/policy_sample_host compiles it with g++).  Same
// definition as the oracle's mzo_rng_u32.  No floating point here: what a stream makes of the words is its own business.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MZ_RNG_HD __host__ __device__ __forceinline__
#else
#define MZ_RNG_HD inline
#endif

MZ_RNG_HD uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
MZ_RNG_HD uint32_t rng_u32(uint64_t seed, uint64_t env, uint32_t counter) {
  uint64_t z = mix64(seed + 0x9E3779B97F4A7C15ULL * (env + 1));
  z = mix64(z + 0x9E3779B97F4A7C15ULL * ((uint64_t)counter + 1));
  return (uint32_t)(z >> 32);
}
// the seed an env's episode draws its reset state from: the handle's seed for episode 0 (what mz_reset draws), a mix of seed and
// episode count for every in-step auto-reset after it
MZ_RNG_HD uint64_t episode_seed(uint64_t seed, uint32_t episode) {
  return episode == 0 ? seed : mix64(seed ^ (0xD6E8FEB86659FD93ULL * (uint64_t)episode));
}
