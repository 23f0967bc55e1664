// What the kernels of the device data views (augment.hip, strong.hip, geo.hip) share beyond the RNG of aug_rng.h, each rule once.
// Device functions only, forced inline; every helper keeps the expression order of the definition in include/lc2is_hip.h (the library
// is built with -ffp-contract=fast: nothing here may be reassociated).
#pragma once
#include "common.h"
#include "aug_rng.h"
#include "lc2is_hip.h"

namespace {

static_assert(LC2IS_AUG_M + 9 == LC2IS_AUG_O && LC2IS_STRONG_M + 9 == LC2IS_STRONG_O, "a colour map is M[9] then o[3]");

struct ColourMap { float M[9], o[3]; };   // block-uniform
// the map held as 12 fp32 bit patterns from word `at` of a parameter row
__device__ __forceinline__ ColourMap colour_load(const int32_t* __restrict__ prow, int at) {
  ColourMap k;
#pragma unroll
  for (int e = 0; e < 9; ++e) k.M[e] = __builtin_bit_cast(float, prow[at + e]);
#pragma unroll
  for (int e = 0; e < 3; ++e) k.o[e] = __builtin_bit_cast(float, prow[at + 9 + e]);
  return k;
}
// channel c of clamp(M a + o, 0, 255), a on the 0..255 scale
__device__ __forceinline__ float colour_apply(const ColourMap& k, const float (&a)[3], int c) {
  const float v = k.M[3 * c] * a[0] + k.M[3 * c + 1] * a[1] + k.M[3 * c + 2] * a[2] + k.o[c];
  return fminf(fmaxf(v, 0.f), 255.f);
}

// The streamed copy of a sample's three planes, as a pair: quads q0 + u * THREADS (u < N) below `total` are loaded into r.v[u][c], all before
// the first use (a block waits for HBM once), and stored from there: geo_apply_kernel's copy row, strong_apply_kernel's no-blur path.
template <int N> struct ViewQuads { f32x4_t v[N][3]; };
template <int N, int THREADS>
__device__ __forceinline__ ViewQuads<N> view_load_quads(const float* src, size_t plane, int total, int q0) {
  ViewQuads<N> r;
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int q = q0 + u * THREADS;
    if (q < total) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r.v[u][c] = *(const f32x4_t*)(src + c * plane + 4 * (size_t)q);
    }
  }
  return r;
}
template <int N, int THREADS>
__device__ __forceinline__ void view_store_quads(float* dst, size_t plane, int total, int q0, const ViewQuads<N>& r) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int q = q0 + u * THREADS;
    if (q < total) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *(f32x4_t*)(dst + c * plane + 4 * (size_t)q) = r.v[u][c];
    }
  }
}

// ---- the augmenter's label cells (aug_apply_kernel writes them, aug_crop_select_kernel counts them) ----
// Cell (ci, cj) of q x q pixels takes the label at its centre: the centre's (yr, xr) in the resized nh x nw image under the S x S window at
// (top, left), flipped or not; false where `ok` is or in the padding ...
__device__ __forceinline__ bool aug_cell_pos(bool ok, int ci, int cj, int q, int S, int top, int left, int flip, int nh, int nw, int& yr, int& xr) {
  const int i = ci * q + (q >> 1), j = cj * q + (q >> 1);
  yr = (int)((unsigned)top + (unsigned)i);
  xr = (int)((unsigned)left + (unsigned)(flip ? S - 1 - j : j));
  return ok && (unsigned)yr < (unsigned)nh && (unsigned)xr < (unsigned)nw;
}
// ... and, for a position in frame, the nearest-exact pixel (ys, xs) of the H x W label map (dy = 2 nh, dx = 2 nw, rdy = 1 / dy, rdx = 1 / dx)
__device__ __forceinline__ void aug_cell_src(int yr, int xr, int H, int W, int dy, int dx, float rdy, float rdx, int& ys, int& xs) {
  int rem;
  ys = aug_div((2 * yr + 1) * H, dy, rdy, rem);
  xs = aug_div((2 * xr + 1) * W, dx, rdx, rem);
}

// ---- geometric views ----
struct GeoMap {   // block-uniform: one sample per blockIdx.y
  bool mapped;    // false: the copy
  long long m00, m01, m10, m11, tx, ty;
};
__device__ __forceinline__ GeoMap geo_map(const int32_t* __restrict__ prow) {
  GeoMap g;
  const int flags = prow[LC2IS_GEO_FLAGS];
  bool ok = flags != 0 && !(flags & ~(LC2IS_GEO_WARP | LC2IS_GEO_FLIP));
  int w[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) w[e] = prow[LC2IS_GEO_M + e];
  // (-MAX <= v && v <= MAX, not abs: INT32_MIN has no absolute value)
#pragma unroll
  for (int e = 0; e < 4; ++e) ok = ok && w[e] >= -LC2IS_GEO_MAX_M && w[e] <= LC2IS_GEO_MAX_M;
#pragma unroll
  for (int e = 4; e < 6; ++e) ok = ok && w[e] >= -LC2IS_GEO_MAX_T && w[e] <= LC2IS_GEO_MAX_T;
  g.mapped = ok;
  g.m00 = w[0]; g.m01 = w[1]; g.m10 = w[2]; g.m11 = w[3]; g.tx = w[4]; g.ty = w[5];
  return g;
}
// A 64-bit source index, range-checked before it is narrowed: every value below -2 or above n behaves as -2 / n (all taps outside).
__device__ __forceinline__ int geo_narrow(long long i, int n) { return (int)(i < -2 ? -2ll : (i > (long long)n ? (long long)n : i)); }

// The cell rule of labels and weights: cell `cell` of an L x L map takes the nearest source cell (xs, ys) of the same map; false
// where that lies out of frame (checked in 64 bits: the caller narrows xs, ys only under the result).
__device__ __forceinline__ bool geo_cell(const GeoMap& g, int cell, int L, long long& xs, long long& ys) {
  int x;
  const int y = aug_div(cell, L, __builtin_amdgcn_rcpf((float)L), x);
  const long long u = 2 * x + 1 - L, v = 2 * y + 1 - L, n = L;
  xs = (g.m00 * u + g.m01 * v + 2 * g.tx * n + n * 65536) >> 17;
  ys = (g.m10 * u + g.m11 * v + 2 * g.ty * n + n * 65536) >> 17;
  return xs >= 0 && xs < n && ys >= 0 && ys < n;
}

// A source position in units of 2^-17 pixel: the 64-bit index (to be narrowed), the 17-bit fraction and the fraction as fp32 (exact)
__device__ __forceinline__ long long geo_split(long long X, int& fi, float& f) {
  fi = (int)(X & 0x1FFFF);
  f = (float)fi * (1.0f / 131072.0f);
  return X >> 17;
}
// The bilinear blend of four taps (float, or f32x4_t for four channels alike), guarded: an axis whose fraction is 0 takes its near
// tap's bits and the far tap (which then need not exist) has no say.
template <class T>
__device__ __forceinline__ T geo_lerp(const T& p00, const T& p01, const T& p10, const T& p11, bool hx, bool hy, float fx, float fy) {
  const T top = hx ? p00 + fx * (p01 - p00) : p00;
  const T bot = hx ? p10 + fx * (p11 - p10) : p10;
  return hy ? top + fy * (bot - top) : top;
}

}  // namespace
