// Class map and {intersection, predicted, labelled} counts of the fused head at its own output size (gfx950), forward only.
// replaces: model(inputs)["outputs"].argmax(1) — a second forward that materialises the [B,K,H,W] fp32 logits (158 MB per 512 x 512
//   image at K = 151) — followed by mmseg's accuracy() / intersect_and_union() on the training batch (decode.acc_seg, train mIoU).
//
// head_argmax_grp_kernel is the argmax sibling of head_px_grp_kernel (head.hip): head_grp_plan's tiles and grid, the same S x S-pixel
// groups in units of 16 pixels, the same footprint staging and the same forward product Wm x lo on the fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32), channels at or past C masked to -inf in the accumulators.  Nothing of the softmax: the accumulator of
// channel tile t holds, per lane, channel 16 t + (lane & 15) of four pixels, so the argmax over the channels is an in-lane walk over
// the tiles (ascending, strict >: the first maximum stays) and four row_dpp steps that combine (value, index) pairs inside a row of 16
// lanes — the larger value wins, equal values keep the lower index: torch.argmax's tie rule.  The index is clamped into [0, C): a NaN
// score may pick any class but never indexes outside a histogram row; a pixel whose scores are all -inf gets class 0.
// The 16 results of a unit go to a [16][16] tile in LDS beside the labels' tile; after one barrier the first 256 threads own one pixel
// each (as in the kernels of resize_argmax.hip): pred[b, Y, X] leaves as a byte, and waves 0-3 count their 64 pixels into wave-private
// LDS rows [3][cq] with wave_hist (label_hist.h: ballot + popcount, one plain add per distinct class, the wave the only writer).
// Counting rule (the loss's own, and mmseg's): a pixel counts iff label != ignore_index && 0 <= label < C; it adds to
// predicted[pred] and labelled[label], and to intersection[pred] when pred == label; any other pixel adds to none of the three.
// The block sums its four waves in wave order into its own slab [3][cq] of the workspace and head_argmax_finish_kernel sums each
// image's slabs in a fixed order.  NO read-modify-write atomics, LDS included: integer counts, the same bytes every run.
// A file of its own with the few helpers of head.hip restated, so that head.hip compiles to the object it was.
#include "common.h"
#include "interp.h"
#include "label_hist.h"
#include "lc2is_hip.h"

namespace {

constexpr int HT = 16;          // output tile edge
constexpr int HEAD_THREADS = 512;
constexpr int CMAX = 192;
constexpr int HEAD_PAD = 4;     // floats added to a footprint cell's LDS stride (head.hip)
constexpr int NHW = 4;          // waves that own pixels after the barrier (256 pixels, 64 each)

struct ArgmaxArgs {
  const float* lo; int ld;       // [B, h, w, ld] scores, C valid channels
  const int64_t* labels;         // [B, H, W] or null (pred only)
  uint8_t* pred;                 // [B, H, W] or null
  int* slab;                     // [blocks][3][cq] per-tile counts or null
  int B, h, w, H, W, C, cq;
  long ignore_index;
};

template <int MODE, int S> __device__ __forceinline__ float tap_w(int ph, int k) {
  const float t = ((float)ph + 0.5f) * (1.f / (float)S);
  if constexpr (MODE == LC2IS_INTERP_BICUBIC)
    return k == 0 ? cubic2(t + 1.f) : (k == 1 ? cubic1(t) : (k == 2 ? cubic1(1.f - t) : cubic2(2.f - t)));
  else
    return k == 0 ? 1.f - t : t;
}

template <int CTRL> __device__ __forceinline__ int row_dpp_i(int v) {   // lane permutation inside each row of 16 lanes
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
// one exchange of (value, index) pairs: the larger value wins, equal values keep the lower index (a NaN never wins)
template <int CTRL> __device__ __forceinline__ void argmax_step(float& v, int& i) {
  const float ov = __builtin_bit_cast(float, row_dpp_i<CTRL>(__builtin_bit_cast(int, v)));
  const int oi = row_dpp_i<CTRL>(i);
  const bool take = ov > v || (ov == v && oi < i);
  v = take ? ov : v;
  i = take ? oi : i;
}
__device__ __forceinline__ int row16_argmax(float v, int i) {   // every lane of the row ends with the row's winner
  argmax_step<0xB1>(v, i); argmax_step<0x4E>(v, i); argmax_step<0x141>(v, i); argmax_step<0x140>(v, i);
  return i;
}

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_argmax_grp_kernel(ArgmaxArgs p) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int G = HT / S;
  constexpr int F4 = G + NT - 1;
  constexpr int NQ = NT * NT / 4;
  constexpr int UPG = S * S / 16;
  static_assert(S == 4 || S == 8 || S == 16, "group kernel: S x S pixel groups inside a 16 x 16 tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_x = (p.W + S / 2 + HT - 1) / HT, tiles_y = (p.H + S / 2 + HT - 1) / HT;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int tyi = (blockIdx.x / tiles_x) % tiles_y, txi = blockIdx.x % tiles_x;
  const int a0 = G * tyi - 1, b0 = G * txi - 1;
  const int Y0 = S * a0 + S / 2, X0 = S * b0 + S / 2;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;
  float* s_lo = (float*)smem;
  int* s_lab = (int*)(s_lo + F4 * F4 * CS);      // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  int* s_arg = s_lab + HT * HT;                  // [16][16] class of the pixel (read only where s_lab is not -2)
  int* s_hist = s_arg + HT * HT;                 // counts wanted: [NHW waves][intersection | predicted | labelled][cq]
  const int fsize = F4 * F4 * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    int ry = a0 - OFF + cell / F4, rx = b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > p.h - 1 ? p.h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > p.w - 1 ? p.w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(p.lo + (((size_t)b * p.h + ry) * p.w + rx) * p.ld + c);
  }
  if (tid < HT * HT) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    int code = -2;
    if (Y >= 0 && X >= 0 && Y < p.H && X < p.W) {
      code = -1;
      if (p.labels) {
        const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
        if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
      }
    }
    s_lab[tid] = code;
    if (p.slab) {   // this wave's rows, which no other wave writes
      int* hw = s_hist + wid * 3 * p.cq;
      for (int i = lane; i < 3 * p.cq; i += 64) hw[i] = 0;
    }
  }
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    if (!active) continue;   // no pixel of the unit is inside the image: nothing reads its part of s_arg
    const int gbase = (gy * F4 + gx) * CS;
    const int py_m = prow + m / S, px_m = m % S;
    float Af[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % NT);
    f32x4_t acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float* bp = s_lo + gbase + cell_off[q] + m;
      float bv[TN];
#pragma unroll
      for (int t = 0; t < TN; ++t) bv[t] = bp[16 * t];
#pragma unroll
      for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Af[q], bv[t], acc[t], 0, 0, 0);
    }
    // in-lane: channels 16 t + m, t ascending, strict > (the lowest channel of equal scores stays)
    float best[4] = {NEG, NEG, NEG, NEG};
    int arg[4] = {m, m, m, m};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C
        if (16 * t + m >= p.C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (acc[t][r] > best[r]) { best[r] = acc[t][r]; arg[r] = 16 * t + m; }
    }
    i32x4_t out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = row16_argmax(best[r], arg[r]);
      out[r] = a < 0 ? 0 : (a > p.C - 1 ? p.C - 1 : a);
    }
    // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
    const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
    if (m == 0) *reinterpret_cast<i32x4_t*>(s_arg + (S * gy + py4) * 16 + S * gx + px4) = out;
  }
  __syncthreads();

  // the first 256 threads own one pixel each; the other waves only help with the block's sum
  const int code = tid < HT * HT ? s_lab[tid] : -2;
  const bool inside = code != -2;
  const int cls = inside ? s_arg[tid] : 0;
  if (inside && p.pred) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    p.pred[((size_t)b * p.H + Y) * p.W + X] = (uint8_t)cls;
  }
  if (!p.slab) return;
  if (wid < NHW) {
    int* hw = s_hist + wid * 3 * p.cq;   // this wave's {intersection, predicted, labelled}
    const bool counted = code >= 0;
    wave_hist(hw + p.cq, counted, cls, lane);
    wave_hist(hw, counted && cls == code, cls, lane);
    wave_hist(hw + 2 * p.cq, counted, code, lane);
  }
  __syncthreads();
  const int n = 3 * p.cq;
  int* o = p.slab + (size_t)blockIdx.x * n;
  for (int i = tid; i < n; i += HEAD_THREADS) o[i] = ((s_hist[i] + s_hist[n + i]) + s_hist[2 * n + i]) + s_hist[3 * n + i];
}

// counts[b][e] = sum over the image's tiles of slab[tile][e], tiles in increasing order within each of 4 strided parts, the parts
// added in order (the shape of ra_finish_kernel): grid (ceil(3C / 64), B), 256 threads.  Slab rows are cq wide, counts rows C.
__global__ __launch_bounds__(256) void head_argmax_finish_kernel(const int* __restrict__ slab, int* __restrict__ counts, int C, int cq,
                                                                 int t4) {
  __shared__ int part[4][64];
  const int b = blockIdx.y, tid = threadIdx.x, q = tid >> 6;
  const int e = blockIdx.x * 64 + (tid & 63);
  int s = 0;
  if (e < 3 * C) {
    const int k = e / C, c = e - k * C;
    const int* src = slab + (size_t)b * t4 * 3 * cq + k * cq + c;
    for (int i = q; i < t4; i += 4) s += src[(size_t)i * 3 * cq];
  }
  part[q][tid & 63] = s;
  __syncthreads();
  if (q == 0 && e < 3 * C) counts[(size_t)b * 3 * C + e] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// head_grp_plan's tile count and slab cell width (head.hip)
struct ArgmaxPlan { int f4, t4, cq; size_t slab_bytes; };
ArgmaxPlan argmax_plan(int B, int h, int w, int C, int S, int mode) {
  ArgmaxPlan g;
  g.f4 = HT / S + (mode == LC2IS_INTERP_BICUBIC ? 4 : 2) - 1;
  const int H = h * S, W = w * S;
  g.t4 = ((H + S / 2 + HT - 1) / HT) * ((W + S / 2 + HT - 1) / HT);
  g.cq = (C + 3) & ~3;
  g.slab_bytes = (size_t)B * g.t4 * 3 * g.cq * sizeof(int);
  return g;
}

}  // namespace

extern "C" size_t lc2is_head_upsample_argmax_workspace_bytes(int B, int h, int w, int C, int S, int mode) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || !(S == 4 || S == 8 || S == 16)) return 0;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return 0;
  return argmax_plan(B, h, w, C, S, mode).slab_bytes;
}

extern "C" int lc2is_head_upsample_argmax(const float* scores_lo, int ld, const int64_t* labels, uint8_t* pred, int32_t* counts,
                                          int B, int h, int w, int C, int S, int mode, long ignore_index, void* workspace,
                                          size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && !labels) return LC2IS_ERR_NULL;
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if ((size_t)scores_lo & 15) return LC2IS_ERR_SHAPE;
  if (!(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  const ArgmaxPlan gp = argmax_plan(B, h, w, C, S, mode);
  if (counts && (!workspace || ((size_t)workspace & 15) || workspace_bytes < gp.slab_bytes)) return LC2IS_ERR_WORKSPACE;
  const int H = h * S, W = w * S;
  ArgmaxArgs a{scores_lo, ld, labels, pred, counts ? (int*)workspace : nullptr, B, h, w, H, W, C, gp.cq, ignore_index};
  const int nt = (C + 15) / 16;
  const int tn = nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));   // head_upsample_ce's channel-tile counts
  // the footprint, the two [16][16] tiles and the four waves' rows: at most 7 * 7 * 196 * 4 + 2048 + 4 * 3 * 192 * 4 = 49 680 bytes,
  // inside the default dynamic LDS limit
  const int lds = gp.f4 * gp.f4 * (ld + HEAD_PAD) * (int)sizeof(float) + 2 * HT * HT * (int)sizeof(int) +
                  (counts ? NHW * 3 * gp.cq * (int)sizeof(int) : 0);
#define LC2IS_HEAD_AM(MODE_, TN_, S_) \
  hipLaunchKernelGGL((head_argmax_grp_kernel<MODE_, TN_, S_>), dim3(B * gp.t4), dim3(HEAD_THREADS), lds, stream, a)
#define LC2IS_HEAD_AM_TN(MODE_, S_)                                                                 \
  do {                                                                                              \
    if (tn == 4) LC2IS_HEAD_AM(MODE_, 4, S_); else if (tn == 8) LC2IS_HEAD_AM(MODE_, 8, S_);        \
    else if (tn == 10) LC2IS_HEAD_AM(MODE_, 10, S_); else LC2IS_HEAD_AM(MODE_, 12, S_);             \
  } while (0)
#define LC2IS_HEAD_AM_S(MODE_)                                                                                            \
  do {                                                                                                                    \
    if (S == 4) LC2IS_HEAD_AM_TN(MODE_, 4); else if (S == 8) LC2IS_HEAD_AM_TN(MODE_, 8); else LC2IS_HEAD_AM_TN(MODE_, 16); \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_HEAD_AM_S(LC2IS_INTERP_BICUBIC);
  else LC2IS_HEAD_AM_S(LC2IS_INTERP_BILINEAR);
#undef LC2IS_HEAD_AM_S
#undef LC2IS_HEAD_AM_TN
#undef LC2IS_HEAD_AM
  int rc = lc2is_check_launch();
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(head_argmax_finish_kernel, dim3((3 * C + 63) / 64, B), dim3(256), 0, stream, (const int*)workspace, counts, C,
                     gp.cq, gp.t4);
  return lc2is_check_launch();
}
