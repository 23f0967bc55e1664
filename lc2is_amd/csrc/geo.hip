// Geometric views on the device: a per-sample random affine warp (rotation, isotropic scale, shear, translation, horizontal flip) of a
// batch - pixels fp32 [B,3,S,S] bilinear, labels int64 [B,L,L] and per-pixel weights fp32 [B,L,L] nearest, all under the SAME map: the
// step self-training lacked (the student gets another geometry and the pseudo-labels follow).  Two launches, nothing but device memory
// decides the result, so the pair captures into a graph and a replay draws again from the epoch / key tensors.
//   * geo_params_kernel: one thread per sample draws its switches and values from the counter RNG of aug_rng.h (a stream of its own)
//     and writes the output-to-source map as Q16 integers.
//   * geo_apply_kernel: one launch, one sample per blockIdx.y, pixel blocks followed by label-cell blocks (mix_apply_kernel's layout),
//     the branches block-uniform.  A copy row streams 512 pixel quads of all three channels per block with 16-byte loads and stores.
//     A mapped row makes a 32 x 32 output tile per block, 4 consecutive x of all three channels per lane: the source position is
//     formed in int64 from the integers of the row (exact index and fraction), clamped into [-2, S] before it is narrowed, and the
//     four taps are predicated reads.  A wave's output patch is 32 columns x 8 rows: every store instruction still fills whole
//     128-byte lines, and the patch's rotated footprint is squarer than a 64 x 4 one (at 45 degrees about 28 source rows of 2 lines
//     against 48 rows of 2 - 3 lines per channel).  STAGED form: the block's source bounding box (from the tile's corners, clipped
//     to the image, whole quads) is loaded into LDS once with 16-byte loads when it fits 4096 words per channel (48 KB, three blocks
//     per CU) and the taps are LDS reads; DIRECT form otherwise (zooming far out): 4-byte gathers from global memory.  Measured at
//     B = 32, S = 512 (tools/probes/geo_staged): 10 degrees 108 -> 54 us, 45 degrees at scale 0.8 121 -> 58 us, same bits.
//     No atomics, no scratch.
//   * geo_scores_kernel: a teacher's low-resolution score map [B][g][g][ld] follows the view under the same table (the soft-teacher
//     step), bilinear with border padding, and writes the weight map / in-frame mask at label resolution; described at the kernel.
// The exact definition is in include/lc2is_hip.h; tests/geo_ref.py and tests/geo_scores_ref.py restate it in numpy.  The draws' range
// (aug_range1) lives in aug_rng.h; the table row (geo_map), the cell rule (geo_cell), the position split and guarded blend (geo_split,
// geo_lerp) and the streamed copy live in view_common.h; the launchers' overlap predicate in common.h.
#include <math.h>
#include "common.h"
#include "aug_rng.h"
#include "view_common.h"
#include "lc2is_hip.h"

namespace {

constexpr int GEO_P = LC2IS_GEO_PARAM_WORDS;
constexpr int GEO_THREADS = 256;
constexpr int GEO_TW = 32, GEO_TH = 32;            // the output tile of a block on a mapped row: 8 quads x 32 rows
constexpr int GEO_COPY_QUADS = 2 * GEO_THREADS;   // pixel quads of a block on a copy row: two per lane, half the blocks idle
constexpr int GEO_BOX_WORDS = 4096;                // the staged source box per channel: 48 KB of LDS, three blocks per CU
static_assert(GEO_TW * GEO_TH / 4 == GEO_THREADS && GEO_BOX_WORDS % (4 * GEO_THREADS) == 0 && LC2IS_GEO_REC + 5 <= GEO_P && LC2IS_GEO_M + 4 == LC2IS_GEO_T &&
              LC2IS_GEO_T + 2 == LC2IS_GEO_REC, "one quad per lane; parameter row layout");

__global__ __launch_bounds__(64) void geo_params_kernel(const int64_t* __restrict__ keys, int B, const int32_t* __restrict__ epoch,
                                                         const lc2is_geo_config cfg, int32_t* __restrict__ params) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int32_t* row = params + (size_t)b * GEO_P;
  const unsigned h = aug_key(cfg.seed_lo, cfg.seed_hi, *epoch, (long long)keys[b]) ^ LC2IS_GEO_STREAM;
  const bool warp = aug_u24(h, 0) < cfg.warp_thr, flip = aug_u24(h, 6) < cfg.flip_thr;
  const float theta = aug_range1(aug_u24(h, 1), -cfg.rotate, cfg.rotate);
  const float s = aug_range1(aug_u24(h, 2), cfg.scale_lo, cfg.scale_hi);
  const float phi = aug_range1(aug_u24(h, 3), -cfg.shear, cfg.shear);
  const float fx = aug_range1(aug_u24(h, 4), -cfg.translate, cfg.translate);
  const float fy = aug_range1(aug_u24(h, 5), -cfg.translate, cfg.translate);
  int m00 = LC2IS_GEO_ONE, m01 = 0, m10 = 0, m11 = LC2IS_GEO_ONE, tx = 0, ty = 0;
  if (warp) {   // M = (1/s) R(theta) H(phi)
    const float cs = cosf(theta), sn = sinf(theta), tn = tanf(phi), inv = 65536.0f / s;
    m00 = (int)rintf(cs * inv);
    m01 = (int)rintf((cs * tn - sn) * inv);
    m10 = (int)rintf(sn * inv);
    m11 = (int)rintf((sn * tn + cs) * inv);
    tx = (int)rintf(fx * 65536.0f);
    ty = (int)rintf(fy * 65536.0f);
  }
  if (flip) { m00 = -m00; m10 = -m10; }
  row[LC2IS_GEO_FLAGS] = (warp ? LC2IS_GEO_WARP : 0) | (flip ? LC2IS_GEO_FLIP : 0);
  row[LC2IS_GEO_M] = m00; row[LC2IS_GEO_M + 1] = m01; row[LC2IS_GEO_M + 2] = m10; row[LC2IS_GEO_M + 3] = m11;
  row[LC2IS_GEO_T] = tx; row[LC2IS_GEO_T + 1] = ty;
  row[LC2IS_GEO_REC] = __builtin_bit_cast(int, theta);
  row[LC2IS_GEO_REC + 1] = __builtin_bit_cast(int, s);
  row[LC2IS_GEO_REC + 2] = __builtin_bit_cast(int, phi);
  row[LC2IS_GEO_REC + 3] = __builtin_bit_cast(int, fx);
  row[LC2IS_GEO_REC + 4] = __builtin_bit_cast(int, fy);
#pragma unroll
  for (int e = LC2IS_GEO_REC + 5; e < GEO_P; ++e) row[e] = 0;
}

// One output pixel of all three channels.  X, Y: the source position in units of 2^-17 pixel (|X|, |Y| < 2^36 for a valid row).  The
// taps are taken from base[c * cstride + (y - by) * w + (x - bx)]: the image itself (base = the sample, w = S, bx = by = 0) or the
// staged box in LDS.  Every call site is inlined with its own address space.
__device__ __forceinline__ void geo_pixel(const float* base, size_t cstride, int w, int bx, int by, int S, long long X, long long Y,
                                          const lc2is_geo_config& cfg, float (&out)[3]) {
  int fxi, fyi;
  float fx, fy;
  const int x0 = geo_narrow(geo_split(X, fxi, fx), S), y0 = geo_narrow(geo_split(Y, fyi, fy), S);
  // a far tap is needed only where its fraction is not 0; every tap that is read lies inside [0, S)^2 (and so inside the box)
  const bool r0 = (unsigned)y0 < (unsigned)S, r1 = fyi != 0 && (unsigned)(y0 + 1) < (unsigned)S;
  const bool c0 = (unsigned)x0 < (unsigned)S, c1 = fxi != 0 && (unsigned)(x0 + 1) < (unsigned)S;
  const int o00 = (y0 - by) * w + (x0 - bx);   // |o00| <= (S + 2) * S < 2^25; followed only under its predicates
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = base + c * cstride;
    const float f = cfg.fill[c];
    const float p00 = (r0 && c0) ? p[o00] : f, p01 = (r0 && c1) ? p[o00 + 1] : f;
    const float p10 = (r1 && c0) ? p[o00 + w] : f, p11 = (r1 && c1) ? p[o00 + w + 1] : f;
    out[c] = geo_lerp(p00, p01, p10, p11, fxi != 0, fyi != 0, fx, fy);
  }
}

// WORDS: the staged box's budget per channel (GEO_BOX_WORDS in the library; 0: the direct form only, for tools/probes/geo_staged)
template <int WORDS>
__global__ __launch_bounds__(GEO_THREADS) void geo_apply_kernel(const float* __restrict__ in_px, const int64_t* __restrict__ in_lab,
                                                                 const float* __restrict__ in_pw, const int32_t* __restrict__ params,
                                                                 const lc2is_geo_config cfg, int S, int L, int img_blocks, int tiles_x,
                                                                 float* __restrict__ out_px, int64_t* __restrict__ out_lab,
                                                                 float* __restrict__ out_pw) {
  __shared__ __attribute__((aligned(16))) float s_box[WORDS ? 3 * WORDS : 4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const GeoMap g = geo_map(params + (size_t)b * GEO_P);

  if ((int)blockIdx.x >= img_blocks) {   // ---- label and weight cells, one per lane ----
    const int LL = L * L;
    const int cell = ((int)blockIdx.x - img_blocks) * GEO_THREADS + tid;
    if (cell >= LL) return;
    const size_t base = (size_t)b * LL;
    if (!g.mapped) {   // block-uniform
      if (in_lab) out_lab[base + cell] = in_lab[base + cell];
      if (in_pw) out_pw[base + cell] = in_pw[base + cell];
      return;
    }
    long long xs, ys;
    const bool inside = geo_cell(g, cell, L, xs, ys);   // checked in 64 bits, then narrowed
    const size_t from = base + (inside ? (size_t)((int)ys * L + (int)xs) : 0);
    if (in_lab) out_lab[base + cell] = inside ? in_lab[from] : cfg.ignore_index;
    if (in_pw) out_pw[base + cell] = inside ? in_pw[from] : 0.0f;
    return;
  }

  const size_t plane = (size_t)S * S;
  const float* src = in_px + (size_t)b * 3 * plane;
  float* dst = out_px + (size_t)b * 3 * plane;

  if (!g.mapped) {   // block-uniform: stream GEO_COPY_QUADS consecutive quads of the plane, all 3 channels; the later blocks have none
    const int total = S * (S >> 2), q0 = (int)blockIdx.x * GEO_COPY_QUADS + tid;
    const auto v = view_load_quads<GEO_COPY_QUADS / GEO_THREADS, GEO_THREADS>(src, plane, total, q0);
    view_store_quads<GEO_COPY_QUADS / GEO_THREADS, GEO_THREADS>(dst, plane, total, q0, v);
    return;
  }

  // ---- the mapped tile: lane = (row tid / 8, quad tid % 8); a wave is 32 columns x 8 rows ----
  int tx;
  const int ty = aug_div((int)blockIdx.x, tiles_x, __builtin_amdgcn_rcpf((float)tiles_x), tx);
  const int tx0 = tx * GEO_TW, ty0 = ty * GEO_TH;
  const long long n = S, offx = 2 * g.tx * n + (n - 1) * 65536, offy = 2 * g.ty * n + (n - 1) * 65536;

  // The source box of the tile, from its four corners: the map is affine and the floor is monotone, so the least and the greatest
  // near tap of the tile's pixels belong to corners; + 1 for the far taps; clipped to the image in 64 bits, then narrowed.
  bool staged = false;
  int bx = 0, by = 0, w = 4;
  if (WORDS) {
    const int xe = (tx0 + GEO_TW < S ? tx0 + GEO_TW : S) - 1, ye = (ty0 + GEO_TH < S ? ty0 + GEO_TH : S) - 1;
    long long xlo = 1ll << 40, xhi = -(1ll << 40), ylo = 1ll << 40, yhi = -(1ll << 40);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long u = 2 * ((k & 1) ? xe : tx0) + 1 - S, v = 2 * ((k & 2) ? ye : ty0) + 1 - S;
      const long long X = (g.m00 * u + g.m01 * v + offx) >> 17, Y = (g.m10 * u + g.m11 * v + offy) >> 17;
      xlo = X < xlo ? X : xlo; xhi = X > xhi ? X : xhi; ylo = Y < ylo ? Y : ylo; yhi = Y > yhi ? Y : yhi;
    }
    xhi += 1; yhi += 1;
    xlo = xlo < 0 ? 0 : xlo; ylo = ylo < 0 ? 0 : ylo;
    xhi = xhi > S - 1 ? S - 1 : xhi; yhi = yhi > S - 1 ? S - 1 : yhi;
    const bool empty = xlo > xhi || ylo > yhi;   // the whole tile looks outside the image: nothing to stage, no tap is read
    int h = 0;
    if (!empty) {
      bx = (int)xlo & ~3; by = (int)ylo;
      w = (((int)xhi - bx + 1) + 3) & ~3;        // whole quads; bx + w <= S because S % 4 == 0
      h = (int)yhi - by + 1;
    }
    staged = w * h <= WORDS;                     // block-uniform; w, h <= 4096
    if (staged) {
      const int gw = w >> 2, total = h * gw;     // at most WORDS / 4 quads; every load of the lane is issued before the first use
      const float rgw = __builtin_amdgcn_rcpf((float)gw);
      constexpr int NST = WORDS ? WORDS / 4 / GEO_THREADS : 1;
      f32x4_t v[NST][3];
      int at[NST];
#pragma unroll
      for (int e = 0; e < NST; ++e) {
        const int idx = tid + e * GEO_THREADS;
        if (idx < total) {
          int q;
          const int r = aug_div(idx, gw, rgw, q);
          at[e] = r * w + 4 * q;
          const float* p = src + (size_t)(by + r) * S + bx + 4 * q;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[e][c] = *(const f32x4_t*)(p + c * plane);
        }
      }
#pragma unroll
      for (int e = 0; e < NST; ++e) {
        if (tid + e * GEO_THREADS < total) {
#pragma unroll
          for (int c = 0; c < 3; ++c) *(f32x4_t*)&s_box[c * WORDS + at[e]] = v[e][c];
        }
      }
      __syncthreads();
    }
  }

  const int x = tx0 + 4 * (tid & 7), y = ty0 + (tid >> 3);
  if (x >= S || y >= S) return;   // S % 4 == 0: a quad is inside or outside as a whole (after the barrier: every lane staged)
  const long long u = 2 * x + 1 - S, v = 2 * y + 1 - S;
  long long X = g.m00 * u + g.m01 * v + offx, Y = g.m10 * u + g.m11 * v + offy;
  f32x4_t o[3];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float px[3];
    if (staged) geo_pixel(s_box, (size_t)WORDS, w, bx, by, S, X, Y, cfg, px);
    else geo_pixel(src, plane, S, 0, 0, S, X, Y, cfg, px);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c][e] = px[c];
    X += 2 * g.m00;   // u grows by 2 per pixel
    Y += 2 * g.m10;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) *(f32x4_t*)(dst + c * plane + (size_t)y * S + x) = o[c];
}

// The teacher's low-resolution score map under the same table: scores fp32 [B][G][G][4 Q] channel-last (head_scores' layout), bilinear
// with BORDER padding (the position is clamped before it is split, so every tap lies inside the sample and no fill exists), and an
// optional weight map fp32 [B][L][L] under geo_apply's cell rule (in_tw NULL: the in-frame mask).  One launch, one sample per
// blockIdx.y, score blocks followed by weight-cell blocks, the branches block-uniform.  A score block owns a GS_PATCH x GS_PATCH patch
// of output cells and a lane a float4 column group of a cell (16-byte loads and stores along the channel axis; the lanes of a cell
// read whole rows of 16 Q bytes, and the cells of a patch share their taps in cache); a copy row streams the 16 Q quads that follow
// blockIdx.x * 16 Q with no index arithmetic.  No LDS, no atomics, no scratch.
constexpr int GS_PATCH = 4, GS_CELLS = GS_PATCH * GS_PATCH, GS_COPY = 4;   // GS_COPY: quads a lane of a copy row has in flight

__global__ __launch_bounds__(GEO_THREADS) void geo_scores_kernel(const float* __restrict__ in_sc, const float* __restrict__ in_tw,
                                                                  const int32_t* __restrict__ params, int G, int Q, int L,
                                                                  int score_blocks, int patches_x, float* __restrict__ out_sc,
                                                                  float* __restrict__ out_tw) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const GeoMap mp = geo_map(params + (size_t)b * GEO_P);

  if ((int)blockIdx.x >= score_blocks) {   // ---- weight cells, one per lane (launched only when the weight map is wanted) ----
    const int LL = L * L;
    const int cell = ((int)blockIdx.x - score_blocks) * GEO_THREADS + tid;
    if (cell >= LL) return;
    const size_t base = (size_t)b * LL;
    if (!mp.mapped) {   // block-uniform
      out_tw[base + cell] = in_tw ? in_tw[base + cell] : 1.0f;
      return;
    }
    long long xs, ys;
    float w = 0.0f;
    if (geo_cell(mp, cell, L, xs, ys))   // checked in 64 bits, then narrowed
      w = in_tw ? in_tw[base + (size_t)(geo_narrow(ys, L - 1) * L + geo_narrow(xs, L - 1))] : 1.0f;
    out_tw[base + cell] = w;
    return;
  }

  const int items = GS_CELLS * Q, total = G * G * Q;   // quads: of a block, of the sample (<= 2^26)
  const f32x4_t* src = (const f32x4_t*)in_sc + (size_t)b * total;
  f32x4_t* dst = (f32x4_t*)out_sc + (size_t)b * total;

  if (!mp.mapped) {   // block-uniform: the block's share of the sample's quads, in order; the last blocks may have none
    const int q0 = (int)blockIdx.x * items;   // < 2^27
    for (int i0 = tid; i0 < items; i0 += GS_COPY * GEO_THREADS) {
      f32x4_t v[GS_COPY];
#pragma unroll
      for (int e = 0; e < GS_COPY; ++e) {
        const int i = i0 + e * GEO_THREADS;
        if (i < items && q0 + i < total) v[e] = src[q0 + i];
      }
#pragma unroll
      for (int e = 0; e < GS_COPY; ++e) {
        const int i = i0 + e * GEO_THREADS;
        if (i < items && q0 + i < total) dst[q0 + i] = v[e];
      }
    }
    return;
  }

  // ---- the mapped patch: item i = (cell i / Q of the patch, column group i % Q) ----
  int px;
  const int py = aug_div((int)blockIdx.x, patches_x, __builtin_amdgcn_rcpf((float)patches_x), px);
  const long long n = G, offx = 2 * mp.tx * n + (n - 1) * 65536, offy = 2 * mp.ty * n + (n - 1) * 65536, last = (n - 1) << 17;
  const float rq = __builtin_amdgcn_rcpf((float)Q);
  const int down = G * Q;
  for (int i = tid; i < items; i += GEO_THREADS) {
    int q;
    const int c = aug_div(i, Q, rq, q);
    const int x = px * GS_PATCH + (c & (GS_PATCH - 1)), y = py * GS_PATCH + c / GS_PATCH;
    if (x >= G || y >= G) continue;
    const long long u = 2 * x + 1 - G, v = 2 * y + 1 - G;
    long long X = mp.m00 * u + mp.m01 * v + offx, Y = mp.m10 * u + mp.m11 * v + offy;
    // clamped BEFORE the split: an out-of-frame position is the border cell with fraction 0, and a far tap that is read (its
    // fraction is not 0, so the near index is at most G - 2) lies inside the sample too
    X = X < 0 ? 0 : (X > last ? last : X);
    Y = Y < 0 ? 0 : (Y > last ? last : Y);
    int fxi, fyi;
    float fx, fy;
    const int x0 = geo_narrow(geo_split(X, fxi, fx), G - 1), y0 = geo_narrow(geo_split(Y, fyi, fy), G - 1);   // in [0, G - 1] by the clamp
    const bool hx = fxi != 0, hy = fyi != 0;
    const f32x4_t* p = src + ((y0 * G + x0) * Q + q);
    const f32x4_t p00 = p[0];
    const f32x4_t p01 = hx ? p[Q] : p00, p10 = hy ? p[down] : p00, p11 = (hx && hy) ? p[down + Q] : p00;
    dst[(y * G + x) * Q + q] = geo_lerp(p00, p01, p10, p11, hx, hy, fx, fy);
  }
}

bool geo_overlap(const void* a, const void* b, size_t n) { return lc2is_bytes_overlap(a, n, b, n); }   // an output and its input, one size

// the limits of include/lc2is_hip.h; a NaN fails every comparison and is refused
bool geo_config_ok(const lc2is_geo_config* c) {
  const float pi = 3.14159274f, quarter_pi = 0.785398185f;   // the fp32 neighbours of pi and pi / 4
  return c->warp_thr <= (1u << 24) && c->flip_thr <= (1u << 24) && c->rotate >= 0.f && c->rotate <= pi && c->scale_lo >= 0.25f &&
         c->scale_lo <= c->scale_hi && c->scale_hi <= 4.0f && c->shear >= 0.f && c->shear <= quarter_pi && c->translate >= 0.f &&
         c->translate <= 0.5f;
}

}  // namespace

extern "C" int lc2is_geo_params(const int64_t* keys, int B, const int32_t* epoch, const lc2is_geo_config* cfg, int32_t* params,
                                lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!keys || !epoch || !cfg || !params) return LC2IS_ERR_NULL;
  if (B <= 0 || !geo_config_ok(cfg) || ((uintptr_t)keys & 7) || ((uintptr_t)epoch & 3) || ((uintptr_t)params & 3))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(geo_params_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, keys, B, epoch, *cfg, params);
  return lc2is_check_launch();
}

extern "C" int lc2is_geo_apply(const float* in_px, const int64_t* in_lab, const float* in_pw, const int32_t* params,
                               const lc2is_geo_config* cfg, int B, int S, int L, float* out_px, int64_t* out_lab, float* out_pw,
                               lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in_px || !params || !cfg || !out_px || (in_lab && !out_lab) || (in_pw && !out_pw)) return LC2IS_ERR_NULL;
  if (!in_lab) out_lab = nullptr;
  if (!in_pw) out_pw = nullptr;
  if (B <= 0 || B > 65535 || S < LC2IS_GEO_MIN_SIDE || S > LC2IS_AUG_MAX_SIDE || (S & 3) || L <= 0 || S % L || !geo_config_ok(cfg) ||
      (((uintptr_t)in_px | (uintptr_t)out_px) & 15) || (((uintptr_t)in_lab | (uintptr_t)out_lab) & 7) ||
      (((uintptr_t)in_pw | (uintptr_t)out_pw | (uintptr_t)params) & 3))
    return LC2IS_ERR_SHAPE;
  const size_t cells = (size_t)L * L, px = (size_t)B * 3 * S * S * sizeof(float);
  if (geo_overlap(out_px, in_px, px) || geo_overlap(out_lab, in_lab, B * cells * 8) ||
      geo_overlap(out_pw, in_pw, B * cells * 4))
    return LC2IS_ERR_SHAPE;
  // the tiles of a mapped row; a copy row needs S * S / 2048 blocks of quads, never more than that
  const int tiles_x = (S + GEO_TW - 1) / GEO_TW, img_blocks = tiles_x * ((S + GEO_TH - 1) / GEO_TH);
  const int lab_blocks = (in_lab || in_pw) ? (int)((cells + GEO_THREADS - 1) / GEO_THREADS) : 0;
  hipLaunchKernelGGL(geo_apply_kernel<GEO_BOX_WORDS>, dim3(img_blocks + lab_blocks, B), dim3(GEO_THREADS), 0, stream, in_px, in_lab, in_pw, params,
                     *cfg, S, L, img_blocks, tiles_x, out_px, out_lab, out_pw);
  return lc2is_check_launch();
}

extern "C" int lc2is_geo_scores(const float* in_scores, const float* in_tw, const int32_t* params, int B, int g, int ld, int L,
                                int want_tw, float* out_scores, float* out_tw, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in_scores || !params || !out_scores || (want_tw && !out_tw)) return LC2IS_ERR_NULL;
  if (!want_tw) in_tw = nullptr, out_tw = nullptr;   // neither weight pointer is looked at
  if (B <= 0 || B > 65535 || g < 1 || g > 512 || ld < 4 || ld > 1024 || (ld & 3) ||
      (want_tw && (L < 1 || L > LC2IS_AUG_MAX_SIDE || L % g)) || (((uintptr_t)in_scores | (uintptr_t)out_scores) & 15) ||
      (((uintptr_t)in_tw | (uintptr_t)out_tw | (uintptr_t)params) & 3))
    return LC2IS_ERR_SHAPE;
  const size_t sc = (size_t)B * g * g * ld * sizeof(float), tw = (size_t)B * L * L * sizeof(float);
  if (geo_overlap(out_scores, in_scores, sc) || (want_tw && geo_overlap(out_tw, in_tw, tw)))
    return LC2IS_ERR_SHAPE;
  // a mapped row: one block per 4 x 4 patch of cells; a copy row needs g * g / 16 blocks of 16 cells' quads, never more than that
  const int patches_x = (g + GS_PATCH - 1) / GS_PATCH, score_blocks = patches_x * patches_x;
  const int tw_blocks = want_tw ? (int)(((size_t)L * L + GEO_THREADS - 1) / GEO_THREADS) : 0;
  hipLaunchKernelGGL(geo_scores_kernel, dim3(score_blocks + tw_blocks, B), dim3(GEO_THREADS), 0, stream, in_scores, in_tw, params, g,
                     ld / 4, L, score_blocks, patches_x, out_scores, out_tw);
  return lc2is_check_launch();
}
