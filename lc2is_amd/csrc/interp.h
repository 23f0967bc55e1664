// Source taps of torch's upsample_bicubic2d / upsample_bilinear2d (align_corners=False), shared by the head kernels (head.hip,
// integer factors) and the resize + argmax kernel (resize_argmax.hip, any output size).
#pragma once
#include <hip/hip_runtime.h>

#include "lc2is_hip.h"

namespace {

__device__ __forceinline__ float cubic1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.f; }          // A=-0.75
__device__ __forceinline__ float cubic2(float x) { return ((-0.75f * x + 3.75f) * x - 6.f) * x + 3.f; }

// taps of one output coordinate: up to 4 (index, weight) pairs, indices clamped to [0, n-1]
struct Taps { int idx[4]; float w[4]; };

__device__ __forceinline__ Taps make_taps(int dst, float inv_scale, int n_in, int mode) {
  Taps t;
  if (mode == LC2IS_INTERP_BICUBIC) {
    const float src = inv_scale * ((float)dst + 0.5f) - 0.5f;
    const float fl = floorf(src);
    const float tt = src - fl;
    const int i0 = (int)fl;
    t.w[0] = cubic2(tt + 1.f); t.w[1] = cubic1(tt); t.w[2] = cubic1(1.f - tt); t.w[3] = cubic2(2.f - tt);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int ii = i0 - 1 + k;
      t.idx[k] = ii < 0 ? 0 : (ii > n_in - 1 ? n_in - 1 : ii);
    }
  } else {  // bilinear, align_corners=False
    float src = inv_scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    const int i0 = (int)src;
    const int i1 = i0 < n_in - 1 ? i0 + 1 : i0;
    const float l1 = src - (float)i0;
    t.idx[0] = i0; t.w[0] = 1.f - l1; t.idx[1] = i1; t.w[1] = l1;
    t.idx[2] = i0; t.w[2] = 0.f; t.idx[3] = i0; t.w[3] = 0.f;
  }
  return t;
}

}  // namespace
