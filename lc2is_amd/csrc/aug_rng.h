// The counter-based RNG of the data-path kernels (augment.hip, mix.hip, strong.hip), their exact small-quotient division and the
// composition of colour maps (aug_left_mul).  Every random number is a pure function of (seed, epoch, key, draw number); the
// definition is in include/lc2is_hip.h (lc2is_aug_params) and tests/augment_ref.py restates it in numpy, bit for bit.
#pragma once
#include "common.h"

namespace {

constexpr unsigned AUG_GOLD = 0x9E3779B9u;

__device__ __forceinline__ unsigned aug_key(unsigned seed_lo, unsigned seed_hi, int epoch, long long key) {
  unsigned h = mix32((unsigned)key + seed_lo);
  h = mix32(h ^ ((unsigned)((unsigned long long)key >> 32) + seed_hi));
  return mix32(h ^ ((unsigned)epoch * AUG_GOLD + 0x85EBCA6Bu));
}
__device__ __forceinline__ unsigned aug_u24(unsigned h, unsigned k) { return mix32(h + k * AUG_GOLD) >> 8; }
__device__ __forceinline__ float aug_range(unsigned u24, float lo, float hi) {
  return lo + (hi - lo) * ((float)u24 * (1.0f / 16777216.0f));
}

// n / d and the remainder for 0 <= n < 2^31, 1 <= d < 2^24, n / d <= 4096, rcp_d = v_rcp_f32(d) (1 ulp): the fp32 estimate is off
// by less than 4097 * 2^-22 < 1, so its floor is the quotient or one next to it and one integer correction makes it exact.
__device__ __forceinline__ int aug_div(int n, int d, float rcp_d, int& rem) {
  int q = (int)((float)n * rcp_d);
  int r = (int)((unsigned)n - (unsigned)q * (unsigned)d);
  if (r < 0) { q -= 1; r += d; }
  else if (r >= d) { q += 1; r -= d; }
  rem = r;
  return q;
}

// (M, o) = A (M, o)
__device__ __forceinline__ void aug_left_mul(const float (&A)[9], float (&M)[9], float (&o)[3]) {
  float N[9], p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) N[3 * r + c] = A[3 * r] * M[c] + A[3 * r + 1] * M[3 + c] + A[3 * r + 2] * M[6 + c];
    p[r] = A[3 * r] * o[0] + A[3 * r + 1] * o[1] + A[3 * r + 2] * o[2];
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) M[e] = N[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) o[e] = p[e];
}

}  // namespace
