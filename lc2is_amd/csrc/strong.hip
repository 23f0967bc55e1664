// Strong photometric views on the device: colour jitter, random greyscale and Gaussian blur of a normalised fp32 batch [B,3,S,S],
// the student's view in self-training (the same geometry as the view the teacher labelled, another colour).  Two launches, nothing
// but device memory decides the result, so the pair captures into a graph and a replay draws again from the epoch / key tensors.
//   * strong_params_kernel: one thread per sample draws its switches and values from the counter RNG of aug_rng.h (a stream of its
//     own), folds jitter and grey into one 3x3 matrix + offset and forms the blur's radius and taps.
//   * strong_apply_kernel: one launch, one sample per blockIdx.y, the branch block-uniform.  Without blur a block streams 512 pixel
//     quads of all three channels with 16-byte loads and stores (HBM-bound; flags 0 is a copy of bits).  With blur a block makes a
//     32 x 64 tile: the colour-mapped tile plus a halo of R is staged in LDS once (16-byte loads where a quad lies inside the image,
//     reflected scalar reads at the border), the row pass reads a lane's 4 + 2R-wide window as 16-byte LDS reads and writes one
//     channel's rows, the column pass reads 2R + 1 16-byte rows per quad and stores 16 bytes.  The passes are instantiated per
//     radius, so the window lives in registers (no scratch) and taps past R are never touched.  LDS: 45 KB tile + 12 KB row-pass
//     buffer = 57 KB, two blocks per CU.  The staged row stride of 80 words leaves a 16-byte LDS read two-way conflicted between
//     neighbouring rows at worst; the LDS is not the limit (about 25 16-byte reads per 32 bytes of HBM traffic at R = 8).
// The exact definition is in include/lc2is_hip.h; tests/strong_ref.py restates it in numpy.  The colour steps and sigma's one-rounding
// range live in aug_rng.h; the colour map's load and apply and the no-blur path's streamed copy in view_common.h.
#include "common.h"
#include "aug_rng.h"
#include "view_common.h"
#include "lc2is_hip.h"

namespace {

constexpr int ST_P = LC2IS_STRONG_PARAM_WORDS;
constexpr int ST_RMAX = LC2IS_STRONG_MAX_RADIUS;
constexpr int ST_TW = 64, ST_TH = 32;                         // the tile of a block: 32 rows x 64 columns
constexpr int ST_SW = ST_TW + 2 * ST_RMAX;                    // staged row stride (words)
constexpr int ST_SH = ST_TH + 2 * ST_RMAX;                    // staged rows
constexpr int ST_THREADS = 256;
constexpr int ST_QUADS = ST_TW * ST_TH / 4;                   // pixel quads of a block, both paths
static_assert(LC2IS_STRONG_W + ST_RMAX + 1 <= ST_P && LC2IS_STRONG_O + 3 == LC2IS_STRONG_W && LC2IS_STRONG_M + 9 == LC2IS_STRONG_O,
              "parameter row layout");
static_assert((3 * ST_SH * ST_SW + ST_SH * ST_TW) * 4 <= 64 * 1024, "two blocks per CU");

__global__ __launch_bounds__(64) void strong_params_kernel(const int64_t* __restrict__ keys, int B, const int32_t* __restrict__ epoch,
                                                            const lc2is_strong_config cfg, int32_t* __restrict__ params) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int32_t* row = params + (size_t)b * ST_P;
  const unsigned h = aug_key(cfg.seed_lo, cfg.seed_hi, *epoch, (long long)keys[b]) ^ LC2IS_STRONG_STREAM;
  const bool jitter = aug_u24(h, 0) < cfg.jitter_thr, grey = aug_u24(h, 5) < cfg.gray_thr, blur = aug_u24(h, 6) < cfg.blur_thr;

  // jitter and grey folded into rgb' = M rgb + o (0..255 scale); one clamp, in strong_apply
  float M[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, o[3] = {0.f, 0.f, 0.f};
  if (jitter) {
    const float d = aug_range(aug_u24(h, 1), -cfg.brightness_delta, cfg.brightness_delta);
    const float c = aug_range(aug_u24(h, 2), cfg.contrast_lo, cfg.contrast_hi);
    const float sa = aug_range(aug_u24(h, 3), cfg.saturation_lo, cfg.saturation_hi);
    const float a = aug_range(aug_u24(h, 4), -cfg.hue_delta, cfg.hue_delta);
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = (o[e] + d) * c;
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] *= c;
    aug_saturation(sa, M, o);
    aug_hue(cosf(a), sinf(a), M, o);
  }
  if (grey) aug_grey(M, o);

  // sigma with ONE rounding (the restatement forms the same fp32 number, so R agrees exactly), R and the normalised taps
  const float sigma = aug_range1(aug_u24(h, 7), cfg.sigma_lo, cfg.sigma_hi);
  int R = (int)ceilf(4.f * sigma);
  R = R < 0 ? 0 : (R > ST_RMAX ? ST_RMAX : R);
  const float s2 = -1.f / (2.f * sigma * sigma);
  float w[ST_RMAX + 1], sum = 0.f;
#pragma unroll
  for (int k = 0; k <= ST_RMAX; ++k) {
    w[k] = k <= R ? expf((float)(k * k) * s2) : 0.f;
    sum += k ? 2.f * w[k] : w[k];
  }
  const float inv = 1.f / sum;

  row[LC2IS_STRONG_FLAGS] = ((jitter || grey) ? LC2IS_STRONG_COLOUR : 0) | (grey ? LC2IS_STRONG_GREY : 0) | (blur ? LC2IS_STRONG_BLUR : 0);
  row[LC2IS_STRONG_R] = R;
  row[LC2IS_STRONG_SIGMA] = __builtin_bit_cast(int, sigma);
#pragma unroll
  for (int e = 0; e < 9; ++e) row[LC2IS_STRONG_M + e] = __builtin_bit_cast(int, M[e]);
#pragma unroll
  for (int e = 0; e < 3; ++e) row[LC2IS_STRONG_O + e] = __builtin_bit_cast(int, o[e]);
#pragma unroll
  for (int k = 0; k <= ST_RMAX; ++k) row[LC2IS_STRONG_W + k] = __builtin_bit_cast(int, w[k] * inv);
#pragma unroll
  for (int e = LC2IS_STRONG_W + ST_RMAX + 1; e < ST_P; ++e) row[e] = 0;
}

// normalised rgb of 4 pixels -> v' = clamp(M v + o, 0, 255) on the 0..255 scale
__device__ __forceinline__ void strong_map(f32x4_t (&v)[3], const ColourMap& k, const lc2is_strong_config& cfg) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = 255.f * (v[c][e] * cfg.std[c] + cfg.mean[c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][e] = colour_apply(k, a, c);
  }
}
__device__ __forceinline__ f32x4_t strong_renorm(f32x4_t v, int c, const lc2is_strong_config& cfg) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (v[e] * (1.0f / 255.0f) - cfg.mean[c]) * cfg.inv_std[c];
  return v;
}
// torch's "reflect", then clamped into the image: in bounds whatever i is
__device__ __forceinline__ int strong_reflect(int i, int S) {
  i = i < 0 ? -i : i;
  i = i >= S ? 2 * (S - 1) - i : i;
  return i < 0 ? 0 : (i > S - 1 ? S - 1 : i);
}

// The blurred tile (ty0, tx0) of one sample; `in` / `out` point at the sample.  Block-uniform arguments; every lane takes part.
template <int R>
__device__ __forceinline__ void strong_blur_tile(const float* __restrict__ in, float* __restrict__ out,
                                                 const int32_t* __restrict__ prow, const lc2is_strong_config& cfg, bool colour, int S,
                                                 int ty0, int tx0, float* s_in, float* s_tmp) {
  constexpr int HR = (R + 3) & ~3;   // the column halo in whole quads; staged column j is image x = tx0 - HR + j
  const int tid = threadIdx.x;
  const int cols = S - tx0 < ST_TW ? S - tx0 : ST_TW, rows = S - ty0 < ST_TH ? S - ty0 : ST_TH;   // of the output; cols % 4 == 0
  const int rows_st = rows + 2 * R, gw = (cols + 2 * HR) >> 2, ow = cols >> 2;   // staged row r is image y = ty0 - R + r
  const float rgw = __builtin_amdgcn_rcpf((float)gw), row_ = __builtin_amdgcn_rcpf((float)ow);
  const size_t plane = (size_t)S * S;
  const ColourMap k = colour_load(prow, LC2IS_STRONG_M);
  float w[R + 1];
#pragma unroll
  for (int e = 0; e <= R; ++e) w[e] = __builtin_bit_cast(float, prow[LC2IS_STRONG_W + e]);

  // ---- stage: every input pixel of the tile and its halo once, colour-mapped ----
  // Every load of the lane is issued before the first one is used: a block waits for HBM once, not once per quad.
  constexpr int NST = ((ST_TH + 2 * R) * ((ST_TW + 2 * HR) / 4) + ST_THREADS - 1) / ST_THREADS;   // quads per lane, at most 4
  f32x4_t v[NST][3];
  int at[NST];   // the quad's word in a channel's staged tile
#pragma unroll
  for (int u = 0; u < NST; ++u) {
    const int idx = tid + u * ST_THREADS;
    if (idx < rows_st * gw) {
      int g;
      const int r = aug_div(idx, gw, rgw, g);
      const int y = strong_reflect(ty0 - R + r, S), gx = tx0 - HR + 4 * g;
      const float* src = in + (size_t)y * S;
      at[u] = r * ST_SW + 4 * g;
      if (gx >= 0 && gx + 4 <= S) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[u][c] = *(const f32x4_t*)(src + c * plane + gx);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int x = strong_reflect(gx + e, S);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[u][c][e] = src[c * plane + x];
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NST; ++u) {
    if (tid + u * ST_THREADS < rows_st * gw) {
      if (colour) strong_map(v[u], k, cfg);
#pragma unroll
      for (int c = 0; c < 3; ++c) *(f32x4_t*)&s_in[c * ST_SH * ST_SW + at[u]] = v[u][c];
    }
  }
  __syncthreads();

  for (int c = 0; c < 3; ++c) {
    // ---- rows: output quad xg of staged row r from its window of 4 + 2 HR staged words ----
    for (int idx = tid; idx < rows_st * ow; idx += ST_THREADS) {
      int xg;
      const int r = aug_div(idx, ow, row_, xg);
      const float* p = &s_in[(c * ST_SH + r) * ST_SW + 4 * xg];
      float win[4 + 2 * HR];
#pragma unroll
      for (int q = 0; q < 1 + HR / 2; ++q) {
        const f32x4_t t = *(const f32x4_t*)(p + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) win[4 * q + e] = t[e];
      }
      f32x4_t acc;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = w[0] * win[HR + e];
#pragma unroll
        for (int d = 1; d <= R; ++d) a = __builtin_fmaf(w[d], win[HR + e - d] + win[HR + e + d], a);
        acc[e] = a;
      }
      *(f32x4_t*)&s_tmp[r * ST_TW + 4 * xg] = acc;
    }
    __syncthreads();
    // ---- columns: output row i is staged row i + R ----
    for (int idx = tid; idx < rows * ow; idx += ST_THREADS) {
      int xg;
      const int i = aug_div(idx, ow, row_, xg);
      const float* p = &s_tmp[(i + R) * ST_TW + 4 * xg];
      const f32x4_t mid = *(const f32x4_t*)p;
      f32x4_t acc;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = w[0] * mid[e];
#pragma unroll
      for (int d = 1; d <= R; ++d) {
        const f32x4_t up = *(const f32x4_t*)(p - d * ST_TW), dn = *(const f32x4_t*)(p + d * ST_TW);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w[d], up[e] + dn[e], acc[e]);
      }
      if (colour) acc = strong_renorm(acc, c, cfg);
      *(f32x4_t*)(out + c * plane + (size_t)(ty0 + i) * S + tx0 + 4 * xg) = acc;
    }
    __syncthreads();   // the row-pass buffer is read: the next channel may write it
  }
}

__global__ __launch_bounds__(ST_THREADS) void strong_apply_kernel(const float* __restrict__ in, const int32_t* __restrict__ params,
                                                                   const lc2is_strong_config cfg, int S, int tiles_x,
                                                                   float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_in[3 * ST_SH * ST_SW];
  __shared__ __attribute__((aligned(16))) float s_tmp[ST_SH * ST_TW];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int32_t* prow = params + (size_t)b * ST_P;
  const int flags = prow[LC2IS_STRONG_FLAGS], R = prow[LC2IS_STRONG_R];
  const bool valid = !(flags & ~(LC2IS_STRONG_COLOUR | LC2IS_STRONG_GREY | LC2IS_STRONG_BLUR)) && (unsigned)R <= (unsigned)ST_RMAX;
  const bool colour = valid && (flags & LC2IS_STRONG_COLOUR), blur = valid && (flags & LC2IS_STRONG_BLUR);
  const size_t plane = (size_t)S * S;
  const float* src = in + (size_t)b * 3 * plane;
  float* dst = out + (size_t)b * 3 * plane;

  if (!blur) {   // block-uniform: stream ST_QUADS consecutive quads of the plane, all 3 channels
    const int total = S * (S >> 2);
    const int q0 = (int)blockIdx.x * ST_QUADS + tid;
    auto r = view_load_quads<ST_QUADS / ST_THREADS, ST_THREADS>(src, plane, total, q0);
    auto& v = r.v;
    if (colour) {
      const ColourMap k = colour_load(prow, LC2IS_STRONG_M);
#pragma unroll
      for (int u = 0; u < ST_QUADS / ST_THREADS; ++u) {
        if (q0 + u * ST_THREADS < total) {
          strong_map(v[u], k, cfg);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[u][c] = strong_renorm(v[u][c], c, cfg);
        }
      }
    }
    view_store_quads<ST_QUADS / ST_THREADS, ST_THREADS>(dst, plane, total, q0, r);
    return;
  }

  int tx;
  const int ty = aug_div((int)blockIdx.x, tiles_x, __builtin_amdgcn_rcpf((float)tiles_x), tx);
  const int ty0 = ty * ST_TH, tx0 = tx * ST_TW;
  switch (R) {   // block-uniform
    case 0: strong_blur_tile<0>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 1: strong_blur_tile<1>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 2: strong_blur_tile<2>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 3: strong_blur_tile<3>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 4: strong_blur_tile<4>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 5: strong_blur_tile<5>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 6: strong_blur_tile<6>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    case 7: strong_blur_tile<7>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
    default: strong_blur_tile<8>(src, dst, prow, cfg, colour, S, ty0, tx0, s_in, s_tmp); break;
  }
}

}  // namespace

extern "C" int lc2is_strong_params(const int64_t* keys, int B, const int32_t* epoch, const lc2is_strong_config* cfg, int32_t* params,
                                   lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!keys || !epoch || !cfg || !params) return LC2IS_ERR_NULL;
  if (B <= 0 || cfg->jitter_thr > (1u << 24) || cfg->gray_thr > (1u << 24) || cfg->blur_thr > (1u << 24) ||
      !(cfg->sigma_lo > 0.f && cfg->sigma_lo <= cfg->sigma_hi && cfg->sigma_hi <= 2.0f) || ((uintptr_t)keys & 7) ||
      ((uintptr_t)epoch & 3) || ((uintptr_t)params & 3))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(strong_params_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, keys, B, epoch, *cfg, params);
  return lc2is_check_launch();
}

extern "C" int lc2is_strong_apply(const float* in, const int32_t* params, const lc2is_strong_config* cfg, int B, int S, float* out,
                                  lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !params || !cfg || !out) return LC2IS_ERR_NULL;
  if (B <= 0 || B > 65535 || S < 12 || S > LC2IS_AUG_MAX_SIDE || (S & 3) || (((uintptr_t)in | (uintptr_t)out) & 15) ||
      ((uintptr_t)params & 3))
    return LC2IS_ERR_SHAPE;
  const size_t bytes = (size_t)B * 3 * S * S * sizeof(float);
  if (lc2is_bytes_overlap(out, bytes, in, bytes)) return LC2IS_ERR_SHAPE;   // the blur reads a halo: not in place
  const int tiles_x = (S + ST_TW - 1) / ST_TW, tiles_y = (S + ST_TH - 1) / ST_TH;
  hipLaunchKernelGGL(strong_apply_kernel, dim3(tiles_x * tiles_y, B), dim3(ST_THREADS), 0, stream, in, params, *cfg, S, tiles_x, out);
  return lc2is_check_launch();
}
