// The counter-based RNG of the data-path kernels (augment.hip, mix.hip, strong.hip, geo.hip), its two uniform ranges, the exact
// small-quotient division and the builders of colour maps (aug_left_mul and the saturation / hue / grey steps on top of it).  Every
// random number is a pure function of (seed, epoch, key, draw number); the definition is in include/lc2is_hip.h (lc2is_aug_params)
// and tests/augment_ref.py restates it in numpy, bit for bit.  What the kernels of a view share beyond that is in view_common.h.
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
// lo + (hi - lo) * t as a product and a sum (TWO roundings as written): the colour draws, restated within a tolerance, not bit for bit
__device__ __forceinline__ float aug_range(unsigned u24, float lo, float hi) {
  return lo + (hi - lo) * ((float)u24 * (1.0f / 16777216.0f));
}
// the same with ONE rounding after the difference (an fma): sigma and the geometric draws, whose restatements form the same fp32 number
__device__ __forceinline__ float aug_range1(unsigned u24, float lo, float hi) {
  return __builtin_fmaf(hi - lo, (float)u24 * (1.0f / 16777216.0f), lo);
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

// The colour steps both parameter kernels fold into rgb' = M rgb + o.  Saturation: blend with the 0.299 / 0.587 / 0.114 grey by sa
__device__ __forceinline__ void aug_saturation(float sa, float (&M)[9], float (&o)[3]) {
  const float g0 = (1.f - sa) * 0.299f, g1 = (1.f - sa) * 0.587f, g2 = (1.f - sa) * 0.114f;
  const float A[9] = {sa + g0, g1, g2, g0, sa + g1, g2, g0, g1, sa + g2};
  aug_left_mul(A, M, o);
}
// hue: rotation about the grey axis by the angle whose cosine and sine are cs, sn
__device__ __forceinline__ void aug_hue(float cs, float sn, float (&M)[9], float (&o)[3]) {
  const float d = cs + (1.f - cs) * (1.f / 3.f), p = (1.f - cs) * (1.f / 3.f), q = sn * 0.57735026918962576f;
  const float A[9] = {d, p - q, p + q, p + q, d, p - q, p - q, p + q, d};
  aug_left_mul(A, M, o);
}
// grey: every channel becomes the luma
__device__ __forceinline__ void aug_grey(float (&M)[9], float (&o)[3]) {
  const float A[9] = {0.299f, 0.587f, 0.114f, 0.299f, 0.587f, 0.114f, 0.299f, 0.587f, 0.114f};
  aug_left_mul(A, M, o);
}

}  // namespace
