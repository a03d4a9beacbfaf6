// The counter-based generator of the learner kernels: one 64-bit mix of (seed, a, b, c) and the N(0,1) pair built on it.  Every
// draw is a function of its four coordinates alone (seed, row / env, draw counter, index), so a test can restate each of them.
#ifndef DM_RNG_H
#define DM_RNG_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// same mix as oracle/dm_oracle.c (hash32)
__device__ __host__ __forceinline__ uint32_t dm_hash32(uint64_t seed, uint32_t a, uint32_t b, uint32_t c) {
  uint64_t x = seed ^ ((uint64_t)a * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)b * 0xBF58476D1CE4E5B9ull) ^ ((uint64_t)c * 0x94D049BB133111EBull);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (uint32_t)(x >> 32);
}

// N(0,1) pair of the indices (j, j + 1): Box-Muller with u1 in (0, 1] from index j, u2 in [0, 1) from index j + 1; cosine first
struct DmNormal2 { float e0, e1; };
__device__ __forceinline__ DmNormal2 dm_normal2(uint64_t seed, uint32_t r, uint32_t ctr, uint32_t j) {
  const float u1 = ((float)(dm_hash32(seed, r, ctr, j) >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u2 = (float)(dm_hash32(seed, r, ctr, j + 1u) >> 8) * (1.0f / 16777216.0f);
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return {rad * cs, rad * sn};
}

}  // namespace
#endif
