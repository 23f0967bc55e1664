// Bicubic resize of per-class scores to each image's ORIGINAL size fused with the argmax over the classes and the per-class
// confusion counts of the original-size mIoU (gfx950).
// replaces: metrics.py:61-79 (compute_gt_mIOU: F.interpolate(size=) + Softmax2d + JaccardIndex per image) and
//   metrics.py:35-42,137-143 (prepare_for_gt_metrics / original_size_interpolate, then argmax).
//
// The [K, H, W] fp32 score map of the reference (211 MB for a 683 x 512 ADE20K image at K = 151, 1.9 GB at 2048 x 1536) is never
// formed.  A block owns a 16 x 16 tile of one image's OUTPUT pixels, one thread per pixel, and walks the channels in chunks of 32.
// Per chunk: the tile's low-resolution footprint is staged in LDS, a horizontal pass interpolates the tile's columns on every
// footprint row, and a vertical pass finishes each pixel.  A downscaled tile (output size below the score grid) reads a wider
// footprint: the tile is then walked in bands of rows / columns whose footprint fits RA_FMAX, chosen in the kernel from the same
// taps it uses (correct at every scale, full tiles whenever the image is upscaled by about 3 or more).
//
// Three kernels, each in a narrow (K <= 192, uint8 pred) and a wide (K <= 1024, int16 pred) form that differ in the tile's end
// alone, and one of everything they have in common:
//   ra_locate       the block's image and tile from the descriptor table (binary search, bounds checks)
//   RaLds           the carve-up of the dynamic LDS
//   ra_walk         bands, tap tables, footprint staging, horizontal and vertical pass.  It reads source cells through a SOURCE
//                   functor and hands every finished group of four channels of the thread's pixel to a SINK functor
//   ra_tile_counts  pred store, gt read, counting rule, wave histograms, the tile's slab (<WIDE>: int16 pred, one row of
//                   counts at a time)
// ra_kernel (lc2is_resize_argmax): the source is one score grid per image (RaGridSrc), the sink the running (max, argmax) in
//   registers: channels in increasing order, strict > (exact ties: the lowest index wins, as torch.argmax).
// ra_win_kernel (lc2is_resize_argmax_windows), sliding-window evaluation: the source of an image is a canvas of Hc x Wc score
//   cells that is never formed, each cell the mean of the window views that cover it (mmseg's slide_inference, with an optional
//   mirrored copy of every window): RaWinSrc sums a cell over the image's window list (staged once per block in LDS) in list order
//   and divides by the cover count.  The sink is ra_kernel's.
//   replaces: nothing in the reference, which scores the centre crop only (metrics.py:137-143 on one forward).
// ra_ms_kernel<MODE> (lc2is_resize_argmax_multiscale): several canvases per image, RaWinSrc on each, summed per class as logits or
//   as softmax probabilities before the argmax (see there).
// Counts: every wave histograms its own 64 pixels in LDS (one writer per histogram: ballot + popcount per distinct class), the
// block sums its waves in a fixed order into a per-tile slab of the workspace, and ra_finish_kernel sums each image's slabs in a
// fixed order.  No read-modify-write atomics: pred and counts are bitwise reproducible and independent of the batch.
// The wide forms (lc2is_resize_argmax*_wide): the channel walk has no class limit, so they are the same kernels with
// ra_tile_counts<true>; per class the arithmetic is the narrow kernels', so at K <= 192 pred values and count bytes are equal.
#include "common.h"
#include "interp.h"
#include "label_hist.h"
#include "lc2is_hip.h"

namespace {

constexpr int RA_T = LC2IS_RESIZE_TILE;   // output tile edge; one thread per pixel
constexpr int RA_THREADS = RA_T * RA_T;
constexpr int RA_FMAX = 10;               // footprint edge (source rows / columns) of one band
constexpr int RA_CC = 32;                 // channels per chunk
constexpr int RA_CP = RA_CC + 4;          // LDS floats per footprint cell: 16 lanes reading 16 B each across x hit distinct banks
constexpr int RA_KMAX = 192;
constexpr int RA_KMAX_WIDE = LC2IS_RESIZE_WIDE_KMAX;
constexpr int RA_WMAX = LC2IS_SLIDE_MAX_WIN;
constexpr int RA_AMAX = LC2IS_MS_MAX_CANVAS;

// the arguments of the three kernels; each launcher fills what its kernel reads
struct RaArgs {
  const float* src;         // [N, h, w, ld] score grids (ra_kernel) or [V, h, w, ld] window views: channels-last fp32, K valid channels
  const int64_t* desc;      // [N][DS], every kernel: H, W, first pixel of the image in pred / gt, first tile; then
                            //   windows (DS = 8): Hc, Wc (canvas cells), first window, n_windows
                            //   multiscale (DS = 6): first canvas, n_canvases
  const int64_t* canv;      // multiscale: [n_canv][4]: Hc, Wc, first window, n_windows
  const int32_t* win;       // [n_win][4]: view, oy, ox (origin in canvas cells), flags (bit 0: the view is mirrored along x)
  const void* gt;           // packed like pred: uint8 / int32 / int64 (gt_bytes = 1 / 4 / 8), or null
  void* pred;               // [total_px] uint8 (narrow kernels) / int16 (wide kernels), or null
  int* slab;                // [n_tiles][3][K] per-tile counts, or null (no counts)
  long total_px, n_canv, n_win;
  int N, V, h, w, ld, K, n_tiles, gt_bytes;
  int ignore_index;         // < 0: every pixel counts in "predicted" (lc2is_resize_argmax's rule, always ra_kernel's)
};

// the dynamic LDS of a block
struct RaLds {
  float* foot;    // [RA_FMAX * RA_FMAX][RA_CP]  footprint of the band, one chunk
  float* hb;      // [RA_FMAX][RA_T][RA_CP]     footprint rows interpolated along x
  int4* xi;       // [RA_T] x taps of the band (relative to its first column)
  float4* xw;     // [RA_T] x weights
  int4* win;      // [RA_WMAX] windowed kernels: the usable windows of the canvas being walked, in list order
  int* nw;        // their number
  float* stats;   // ra_ms_kernel<PROB>: the softmax statistics
  int* hist;      // after the channel loops: [4 waves][3][K] (narrow: aliases foot) or [4 waves][K] (wide: aliases foot + hb)
  __device__ explicit RaLds(char* smem) {
    foot = (float*)smem;
    hb = foot + RA_FMAX * RA_FMAX * RA_CP;
    xi = (int4*)(hb + RA_FMAX * RA_T * RA_CP);
    xw = (float4*)(xi + RA_T);
    win = (int4*)(xw + RA_T);
    nw = (int*)(win + RA_WMAX);
    stats = (float*)(nw + 4);
    hist = (int*)smem;
  }
};
constexpr size_t RA_LDS = (size_t)(RA_FMAX * RA_FMAX + RA_FMAX * RA_T) * RA_CP * sizeof(float) + RA_T * (sizeof(int4) + sizeof(float4));
constexpr size_t RA_WIN_LDS = RA_LDS + RA_WMAX * sizeof(int4) + 16;
constexpr size_t RA_MS_LDS_PROB = RA_WIN_LDS + 2 * (size_t)RA_AMAX * RA_THREADS * sizeof(float);
static_assert((size_t)RA_FMAX * RA_FMAX * RA_CP * sizeof(float) >= 4 * 3 * RA_KMAX * sizeof(int), "histograms fit the footprint");
static_assert((size_t)(RA_FMAX * RA_FMAX + RA_FMAX * RA_T) * RA_CP * sizeof(float) >= 4 * RA_KMAX_WIDE * sizeof(int),
              "one row of wide histograms fits foot + hb");
static_assert(RA_MS_LDS_PROB <= 80 * 1024, "two blocks per CU");

// the block's tile and the thread's pixel in it
struct RaTile {
  const int64_t* d;   // the image's descriptor row
  long H, W, pix0;    // output size, first pixel in pred / gt
  int b, Y0, X0, TH, TW;
  int py, px;
  bool valid;         // the pixel lies in the image
};

// The image of tile blockIdx.x: the last one whose first tile is <= blockIdx.x (desc[i][3] ascending).  DS: int64 words per
// descriptor.  False when the descriptor does not fit the buffers: it is then not followed (nothing outside them is read or written).
template <int DS>
__device__ __forceinline__ bool ra_locate(const RaArgs& p, RaTile& t) {
  const int tile = blockIdx.x;
  int lo = 0, hi = p.N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.desc[DS * mid + 3] <= tile) lo = mid; else hi = mid - 1;
  }
  t.b = lo;
  t.d = p.desc + DS * lo;
  t.H = t.d[0]; t.W = t.d[1]; t.pix0 = t.d[2];
  const long tile0 = t.d[3];
  if (t.H < 1 || t.W < 1 || tile < tile0 || t.pix0 < 0 || t.pix0 + t.H * t.W > p.total_px) return false;
  const long tiles_x = (t.W + RA_T - 1) / RA_T, tl = tile - tile0;
  t.Y0 = (int)(tl / tiles_x) * RA_T; t.X0 = (int)(tl % tiles_x) * RA_T;
  if (t.Y0 >= t.H) return false;
  t.TH = (int)min((long)RA_T, t.H - t.Y0); t.TW = (int)min((long)RA_T, t.W - t.X0);
  t.py = threadIdx.x / RA_T; t.px = threadIdx.x % RA_T;
  t.valid = t.py < t.TH && t.px < t.TW;
  return true;
}

// (lowest, highest) source index the output band [d0, d1] reads: taps are monotone in dst and clamped
__device__ __forceinline__ int2 ra_span(int d0, int d1, float s, int n) {
  const Taps a = make_taps(d0, s, n, LC2IS_INTERP_BICUBIC), b = make_taps(d1, s, n, LC2IS_INTERP_BICUBIC);
  return make_int2(a.idx[0], b.idx[3]);
}

// output rows (columns) of the band starting at d0: up to `left`, halved until the band's footprint fits RA_FMAX (a single row
// reads at most 4)
__device__ __forceinline__ int ra_band(int d0, int left, float s, int n) {
  int r = left < RA_T ? left : RA_T;
  while (r > 1) {
    const int2 sp = ra_span(d0, d0 + r - 1, s, n);
    if (sp.y - sp.x + 1 <= RA_FMAX) break;
    r = (r + 1) >> 1;
  }
  return r;
}

__device__ __forceinline__ float4 fma4(float a, float4 x, float4 acc) {
  return make_float4(fmaf(a, x.x, acc.x), fmaf(a, x.y, acc.y), fmaf(a, x.z, acc.z), fmaf(a, x.w, acc.w));
}

// The channels [c_lo, c_hi) of a source grid of Hs x Ws cells, resized over the block's tile.  c_lo is a multiple of RA_CC and
// c_hi <= K; the chunk loop runs inside the bands, so the taps are computed once per band.
// src(cy, cx, c): channels c .. c + 3 of source cell (cy, cx), c < ld (channels at or past ld read as 0).
// sink(c0, c4, y): channels c0 + 4 * c4 .. + 3 of the thread's pixel, the first of them below c_hi, c4 a constant after unrolling;
// channels at or past c_hi hold values that must not be used.  Ends on a barrier: the caller may restage s.win or reuse s.foot at once.
template <class Src, class Sink>
__device__ __forceinline__ void ra_walk(const RaLds& s, const RaTile& t, int Hs, int Ws, int ld, int c_lo, int c_hi, Src src,
                                        Sink sink) {
  const int tid = threadIdx.x;
  const int Y0 = t.Y0, X0 = t.X0, TH = t.TH, TW = t.TW, py = t.py, px = t.px;
  const float sy = (float)Hs / (float)t.H, sx = (float)Ws / (float)t.W;   // torch: input_size / output_size

  for (int rb0 = 0; rb0 < TH;) {
    const int R = ra_band(Y0 + rb0, TH - rb0, sy, Hs);
    const int2 ys = ra_span(Y0 + rb0, Y0 + rb0 + R - 1, sy, Hs);
    const int fy0 = ys.x, FH = ys.y - ys.x + 1;
    const bool row_in = t.valid && py >= rb0 && py < rb0 + R;
    int yi[4] = {0, 0, 0, 0};
    float yw[4] = {0.f, 0.f, 0.f, 0.f};
    if (row_in) {
      const Taps ty = make_taps(Y0 + py, sy, Hs, LC2IS_INTERP_BICUBIC);
#pragma unroll
      for (int k = 0; k < 4; ++k) { yi[k] = ty.idx[k] - fy0; yw[k] = ty.w[k]; }
    }
    for (int cb0 = 0; cb0 < TW;) {
      const int CW = ra_band(X0 + cb0, TW - cb0, sx, Ws);
      const int2 xs = ra_span(X0 + cb0, X0 + cb0 + CW - 1, sx, Ws);
      const int fx0 = xs.x, FW = xs.y - xs.x + 1;
      const bool in = row_in && px >= cb0 && px < cb0 + CW;
      __syncthreads();   // the previous band's last reads of s.xi / s.xw / s.hb are done
      if (tid < CW) {
        const Taps tx = make_taps(X0 + cb0 + tid, sx, Ws, LC2IS_INTERP_BICUBIC);
        s.xi[tid] = make_int4(tx.idx[0] - fx0, tx.idx[1] - fx0, tx.idx[2] - fx0, tx.idx[3] - fx0);
        s.xw[tid] = make_float4(tx.w[0], tx.w[1], tx.w[2], tx.w[3]);
      }
      for (int c0 = c_lo; c0 < c_hi; c0 += RA_CC) {
        // stage the footprint's channels [c0, c0 + 32)
        for (int i = tid; i < FH * FW * (RA_CC / 4); i += RA_THREADS) {
          const int c4 = i % (RA_CC / 4), cell = i / (RA_CC / 4);
          const int c = c0 + 4 * c4;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < ld) v = src(fy0 + cell / FW, fx0 + cell % FW, c);
          *reinterpret_cast<float4*>(s.foot + cell * RA_CP + 4 * c4) = v;
        }
        __syncthreads();
        // horizontal: s.hb[r][x] = sum_k wx[x][k] * foot[r][xi[x][k]]
        for (int i = tid; i < FH * CW * (RA_CC / 4); i += RA_THREADS) {
          const int c4 = i % (RA_CC / 4), x = (i / (RA_CC / 4)) % CW, r = i / (RA_CC / 4 * CW);
          const int4 xi = s.xi[x];
          const float4 xw = s.xw[x];
          const float* row = s.foot + r * FW * RA_CP + 4 * c4;
          float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
          a = fma4(xw.x, *reinterpret_cast<const float4*>(row + xi.x * RA_CP), a);
          a = fma4(xw.y, *reinterpret_cast<const float4*>(row + xi.y * RA_CP), a);
          a = fma4(xw.z, *reinterpret_cast<const float4*>(row + xi.z * RA_CP), a);
          a = fma4(xw.w, *reinterpret_cast<const float4*>(row + xi.w * RA_CP), a);
          *reinterpret_cast<float4*>(s.hb + (r * RA_T + cb0 + x) * RA_CP + 4 * c4) = a;
        }
        __syncthreads();
        // vertical
        if (in) {
          const int nc = min(RA_CC, c_hi - c0);
#pragma unroll
          for (int c4 = 0; c4 < RA_CC / 4; ++c4) {
            if (4 * c4 < nc) {
              const float* col = s.hb + px * RA_CP + 4 * c4;
              float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
              for (int k = 0; k < 4; ++k) a = fma4(yw[k], *reinterpret_cast<const float4*>(col + yi[k] * RA_T * RA_CP), a);
              sink(c0, c4, a);
            }
          }
        }
        __syncthreads();   // s.foot is restaged and s.hb rewritten by the next chunk
      }
      cb0 += CW;
    }
    rb0 += R;
  }
}

// source: one score grid, [h, w, ld] channels-last
struct RaGridSrc {
  const float* img;
  int w, ld;
  __device__ __forceinline__ float4 operator()(int cy, int cx, int c) const {
    return *reinterpret_cast<const float4*>(img + ((size_t)cy * w + cx) * ld + c);
  }
};

// source: a canvas of Wc columns that is never formed.  A cell is the sum of the window views that cover it, in list order from the
// first one, divided by their number (a cell that nothing covers reads 0).  A window may overhang the canvas at the bottom / right
// (multiscale): a cell that is read lies on the canvas (taps are clamped), so ry < h is ry < min(h, Hc - oy), and so along x; a
// mirrored view is mirrored over its on-canvas part.
struct RaWinSrc {
  const float* views;   // [V, h, w, ld]
  size_t view_stride;
  const int4* win;      // the usable windows (LDS), nw of them
  int nw, h, w, ld, Wc;
  // the staged window list of a canvas of Wc columns
  __device__ __forceinline__ RaWinSrc(const RaArgs& p, const RaLds& s, int Wc_)
      : views(p.src), view_stride((size_t)p.h * p.w * p.ld), win(s.win), nw(*s.nw), h(p.h), w(p.w), ld(p.ld), Wc(Wc_) {}
  __device__ __forceinline__ float4 operator()(int cy, int cx, int c) const {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int n = 0;
    for (int j = 0; j < nw; ++j) {
      const int4 wv = win[j];
      const int ry = cy - wv.y, rx = cx - wv.z;
      if (ry < 0 || ry >= h || rx < 0 || rx >= w) continue;
      const int col = (wv.w & 1) ? min(w, Wc - wv.z) - 1 - rx : rx;
      const float4 x = *reinterpret_cast<const float4*>(views + (size_t)wv.x * view_stride + ((size_t)ry * w + col) * ld + c);
      v = n ? make_float4(v.x + x.x, v.y + x.y, v.z + x.z, v.w + x.w) : x;
      ++n;
    }
    if (n > 1) {
      const float fn = (float)n;
      v = make_float4(v.x / fn, v.y / fn, v.z / fn, v.w / fn);
    }
    return v;
  }
};

// this lane's window of a list of n (n <= RA_WMAX): true when it exists and ok(window)
template <class Ok>
__device__ __forceinline__ bool ra_window(const int32_t* win, long n, int lane, Ok ok, int4& wv) {
  wv = make_int4(0, 0, 0, 0);
  if (lane >= n) return false;
  wv = *reinterpret_cast<const int4*>(win + 4 * lane);
  return ok(wv);
}

// the window list of a canvas, once per block: wave 0 keeps the windows with ok(window) in s.win, order preserved.  Call after a
// barrier (nobody still reads the old list); ends on one.
template <class Ok>
__device__ __forceinline__ void ra_stage_windows(const RaLds& s, const int32_t* win, long n, Ok ok) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int4 wv;
    const bool keep = ra_window(win, n, lane, ok, wv);
    const unsigned long long m = __ballot(keep);
    if (keep) s.win[__popcll(m & ((1ull << lane) - 1ull))] = wv;
    if (lane == 0) *s.nw = __popcll(m);
  }
  __syncthreads();
}

// sink of the argmax: the first n (1 or more) of the four channels c .. c + 3, in increasing order, strict > (the first maximum
// stays)
__device__ __forceinline__ void ra_argmax4(float& best, int& arg, int c, float4 a, int n) {
  if (a.x > best) { best = a.x; arg = c; }
  if (n > 1 && a.y > best) { best = a.y; arg = c + 1; }
  if (n > 2 && a.z > best) { best = a.z; arg = c + 2; }
  if (n > 3 && a.w > best) { best = a.w; arg = c + 3; }
}

// The end of every tile: pred, and the tile's {intersection[K], predicted[K], labelled[K]} into its slab.  After a barrier (s.foot
// is free: every walk ends on one).
// Counting rule: g is the pixel's class if it is labelled (0 <= gt < K and gt != ignore_index), else -1.  ignore_index < 0: every
// pixel of the image counts in "predicted"; >= 0: a pixel with g < 0 counts in none of the three rows (mmseg's intersect_and_union).
// WIDE: pred is int16, and [4 waves][3][K] ints do not fit at K = 1024, so the three rows take turns in one [4 waves][K] area over
// s.foot and s.hb (16 KB at K = 1024): predicted, intersection, labelled, each cleared, filled by wave_hist and summed over the
// waves in the narrow order.  The slab's layout and bytes are the narrow epilogue's.
template <bool WIDE>
__device__ __forceinline__ void ra_tile_counts(const RaArgs& p, const RaLds& s, const RaTile& t, int arg) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = p.K;
  const bool valid = t.valid;
  const size_t o = (size_t)t.pix0 + (size_t)(t.Y0 + t.py) * t.W + t.X0 + t.px;
  if (valid && p.pred) {
    if (WIDE) ((int16_t*)p.pred)[o] = (int16_t)arg;
    else ((uint8_t*)p.pred)[o] = (uint8_t)arg;
  }
  if (!p.slab) return;

  int g = -1;
  if (valid && p.gt) {
    long v;
    if (p.gt_bytes == 1) v = ((const uint8_t*)p.gt)[o];
    else if (p.gt_bytes == 4) v = ((const int32_t*)p.gt)[o];
    else v = ((const int64_t*)p.gt)[o];
    g = (v >= 0 && v < K && !(p.ignore_index >= 0 && v == p.ignore_index)) ? (int)v : -1;
  }
  int* out = p.slab + (size_t)blockIdx.x * 3 * K;
  if (WIDE) {
    int* hw = s.hist + wid * K;   // this wave's row
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int row = r == 0 ? 1 : r == 1 ? 0 : 2;   // the slab's row of this turn
      for (int i = lane; i < K; i += 64) hw[i] = 0;
      __syncthreads();
      if (r == 0) wave_hist(hw, p.ignore_index >= 0 ? g >= 0 : valid, arg, lane);
      else if (r == 1) wave_hist(hw, valid && g == arg, arg, lane);
      else wave_hist(hw, g >= 0, g, lane);
      __syncthreads();
      for (int i = tid; i < K; i += RA_THREADS)
        out[row * K + i] = ((s.hist[i] + s.hist[K + i]) + s.hist[2 * K + i]) + s.hist[3 * K + i];
      if (r < 2) __syncthreads();   // the rows are cleared again
    }
    return;
  }
  int* hw = s.hist + wid * 3 * K;   // this wave's three rows
  for (int i = lane; i < 3 * K; i += 64) hw[i] = 0;
  __syncthreads();
  wave_hist(hw + K, p.ignore_index >= 0 ? g >= 0 : valid, arg, lane);
  wave_hist(hw, valid && g == arg, arg, lane);
  wave_hist(hw + 2 * K, g >= 0, g, lane);
  __syncthreads();
  for (int i = tid; i < 3 * K; i += RA_THREADS)
    out[i] = ((s.hist[i] + s.hist[3 * K + i]) + s.hist[6 * K + i]) + s.hist[9 * K + i];
}

template <bool WIDE>
__global__ __launch_bounds__(RA_THREADS) void ra_kernel(RaArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaLds s(smem);
  RaTile t;
  if (!ra_locate<4>(p, t)) return;
  float best = -INFINITY;
  int arg = 0;
  ra_walk(s, t, p.h, p.w, p.ld, 0, p.K, RaGridSrc{p.src + (size_t)t.b * p.h * p.w * p.ld, p.w, p.ld},
          [&](int c0, int c4, float4 y) { ra_argmax4(best, arg, c0 + 4 * c4, y, p.K - c0 - 4 * c4); });
  ra_tile_counts<WIDE>(p, s, t, arg);
}

template <bool WIDE>
__global__ __launch_bounds__(RA_THREADS) void ra_win_kernel(RaArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaLds s(smem);
  RaTile t;
  if (!ra_locate<8>(p, t)) return;
  const long Hc_ = t.d[4], Wc_ = t.d[5], win0 = t.d[6], nwin = t.d[7];
  // a descriptor that does not fit the window limit or the views is not followed either
  if (Hc_ < p.h || Wc_ < p.w || Hc_ > (1L << 24) || Wc_ > (1L << 24)) return;
  if (nwin < 0 || nwin > RA_WMAX || win0 < 0 || win0 + nwin > p.n_win) return;
  const int Hc = (int)Hc_, Wc = (int)Wc_;
  // usable: the view is in range and lies on the canvas
  ra_stage_windows(s, p.win + 4 * win0, nwin, [&](int4 wv) {
    return wv.x >= 0 && wv.x < p.V && wv.y >= 0 && wv.y <= Hc - p.h && wv.z >= 0 && wv.z <= Wc - p.w;
  });
  float best = -INFINITY;
  int arg = 0;
  ra_walk(s, t, Hc, Wc, p.ld, 0, p.K, RaWinSrc(p, s, Wc),
          [&](int c0, int c4, float4 y) { ra_argmax4(best, arg, c0 + 4 * c4, y, p.K - c0 - 4 * c4); });
  ra_tile_counts<WIDE>(p, s, t, arg);
}

// counts[b][e] = sum over the image's tiles of slab[tile][e], tiles in increasing order within each of 4 strided parts, the parts
// added in order: grid (ceil(3K / 64), N), 256 threads.  DS: int64 words per descriptor, as ra_locate's
template <int DS>
__global__ __launch_bounds__(256) void ra_finish_kernel(const int64_t* desc, const int* slab, int* counts, int K, int n_tiles) {
  __shared__ int part[4][64];
  const int b = blockIdx.y, tid = threadIdx.x, q = tid >> 6;
  const int e = blockIdx.x * 64 + (tid & 63);
  const long H = desc[DS * b], W = desc[DS * b + 1], tile0 = desc[DS * b + 3];
  long nt = ((H + RA_T - 1) / RA_T) * ((W + RA_T - 1) / RA_T);
  if (H < 1 || W < 1 || tile0 < 0 || tile0 >= n_tiles) nt = 0;
  else if (tile0 + nt > n_tiles) nt = n_tiles - tile0;
  int s = 0;
  if (e < 3 * K)
    for (long i = q; i < nt; i += 4) s += slab[(size_t)(tile0 + i) * 3 * K + e];
  part[q][tid & 63] = s;
  __syncthreads();
  if (q == 0 && e < 3 * K) counts[(size_t)b * 3 * K + e] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// ---- multi-scale: several canvases per image, summed as logits or as softmax probabilities ---------------------------------
// ra_ms_kernel<MODE> (lc2is_resize_argmax_multiscale): an image is an ordered list of canvases, each with its own size and window
// list; every canvas is resized to the image's size as in ra_win_kernel and the results are combined per class before the argmax.
// The per-class sums of a pixel cannot be kept for all K classes, so the canvases are walked once per channel chunk (32
// accumulators per pixel in registers); the softmax statistics (max, 1 / sum) of every canvas at every pixel come from a first
// walk over all chunks and wait in LDS (16 canvases x 256 pixels x 8 B = 32 KB).  A window may overhang its canvas at the bottom /
// right (a scale below the crop): only its on-canvas part is read (RaWinSrc).

// a canvas row that fits the window table and the limits
__device__ __forceinline__ bool ms_canvas_ok(const RaArgs& p, const int64_t* c) {
  return c[0] >= 1 && c[0] <= (1L << 24) && c[1] >= 1 && c[1] <= (1L << 24) && c[2] >= 0 && c[3] >= 1 && c[3] <= RA_WMAX &&
         c[2] + c[3] <= p.n_win;
}

template <int MODE, bool WIDE>
__global__ __launch_bounds__(RA_THREADS) void ra_ms_kernel(RaArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaLds s(smem);
  float* s_m = s.stats;                       // PROB only: [RA_AMAX][RA_THREADS] max over the classes, per canvas and pixel
  float* s_rl = s_m + RA_AMAX * RA_THREADS;   //            [RA_AMAX][RA_THREADS] 1 / sum of exp(y - max)
  const int tid = threadIdx.x;
  const int K = p.K;
  RaTile t;
  if (!ra_locate<6>(p, t)) return;
  const long cv0 = t.d[4], ncv = t.d[5];
  // nor one that does not fit the tables or the limits: nothing is written for the image
  if (ncv < 1 || ncv > RA_AMAX || cv0 < 0 || cv0 + ncv > p.n_canv) return;
  const int A = (int)ncv;
  const int64_t* cv = p.canv + 4 * cv0;
  // usable on canvas row c: the view is in range and the origin is on the canvas
  auto usable = [&](const int64_t* c) {
    return [&p, c](int4 wv) { return wv.x >= 0 && wv.x < p.V && wv.y >= 0 && wv.y < c[0] && wv.z >= 0 && wv.z < c[1]; };
  };
  // every canvas needs a row that fits and one usable window.  Each wave looks for itself (the same loads, the same answer), so
  // the decision is the block's without a barrier.
  for (int a = 0; a < A; ++a) {
    const int64_t* c = cv + 4 * a;
    if (!ms_canvas_ok(p, c)) return;
    int4 wv;
    if (__ballot(ra_window(p.win + 4 * c[2], c[3], tid & 63, usable(c), wv)) == 0ull) return;
  }

  // the window list of canvas a, restaged when the canvas changes (the walk before it ended on a barrier)
  int staged = -1;
  auto stage = [&](int a) {
    if (a == staged) return;
    staged = a;
    const int64_t* c = cv + 4 * a;
    ra_stage_windows(s, p.win + 4 * c[2], c[3], usable(c));
  };
  // one chunk of canvas a (staged) through `sink`
  auto walk = [&](int a, int c0, auto sink) {
    const int Hc = (int)cv[4 * a], Wc = (int)cv[4 * a + 1];
    ra_walk(s, t, Hc, Wc, p.ld, c0, min(c0 + RA_CC, K), RaWinSrc(p, s, Wc), sink);
  };

  if (MODE == LC2IS_MS_PROB) {
    // pass A: the softmax statistics of every canvas at this thread's pixel, online over the chunks (valid channels only)
    for (int a = 0; a < A; ++a) {
      stage(a);
      float m = -INFINITY, l = 0.f;
      for (int c0 = 0; c0 < K; c0 += RA_CC) {
        const int nc = min(RA_CC, K - c0);
        walk(a, c0, [&](int, int c4, float4 y) {
          const bool v1 = 4 * c4 + 1 < nc, v2 = 4 * c4 + 2 < nc, v3 = 4 * c4 + 3 < nc;
          float mn = fmaxf(m, y.x);
          if (v1) mn = fmaxf(mn, y.y);
          if (v2) mn = fmaxf(mn, y.z);
          if (v3) mn = fmaxf(mn, y.w);
          l = l * __expf(m - mn) + __expf(y.x - mn);
          if (v1) l += __expf(y.y - mn);
          if (v2) l += __expf(y.z - mn);
          if (v3) l += __expf(y.w - mn);
          m = mn;
        });
      }
      s_m[a * RA_THREADS + tid] = m;
      s_rl[a * RA_THREADS + tid] = 1.f / l;
    }
  }

  // pass B: per chunk the sum over the canvases, in canvas order from the first one, then the running argmax
  float best = -INFINITY;
  int arg = 0;
  for (int c0 = 0; c0 < K; c0 += RA_CC) {
    const int nc = min(RA_CC, K - c0);
    float4 acc[RA_CC / 4];
#pragma unroll
    for (int c4 = 0; c4 < RA_CC / 4; ++c4) acc[c4] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int a = 0; a < A; ++a) {
      stage(a);
      float m = 0.f, rl = 1.f;
      if (MODE == LC2IS_MS_PROB) { m = s_m[a * RA_THREADS + tid]; rl = s_rl[a * RA_THREADS + tid]; }
      walk(a, c0, [&](int, int c4, float4 y) {
        if (MODE == LC2IS_MS_PROB)
          y = make_float4(__expf(y.x - m) * rl, __expf(y.y - m) * rl, __expf(y.z - m) * rl, __expf(y.w - m) * rl);
        const float4 sum = acc[c4];
        acc[c4] = a ? make_float4(sum.x + y.x, sum.y + y.y, sum.z + y.z, sum.w + y.w) : y;
      });
    }
    if (t.valid) {
#pragma unroll
      for (int c4 = 0; c4 < RA_CC / 4; ++c4)
        if (4 * c4 < nc) ra_argmax4(best, arg, c0 + 4 * c4, acc[c4], nc - 4 * c4);
    }
  }
  ra_tile_counts<WIDE>(p, s, t, arg);
}

// the main kernel over the tiles, then the per-image sum of the slabs if counts are wanted
template <int DS, class Kern>
int ra_launch(Kern kern, size_t lds, const RaArgs& a, int* counts, hipStream_t stream) {
  hipLaunchKernelGGL(kern, dim3((unsigned)a.n_tiles), dim3(RA_THREADS), lds, stream, a);
  const int rc = lc2is_check_launch();
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(ra_finish_kernel<DS>, dim3((3 * a.K + 63) / 64, a.N), dim3(256), 0, stream, a.desc, (const int*)a.slab, counts,
                     a.K, a.n_tiles);
  return lc2is_check_launch();
}

// the workspace of n_tiles slabs at K classes, 0 when K is outside [1, kmax]
size_t ra_workspace_bytes(long n_tiles, int K, int kmax) {
  if (n_tiles <= 0 || K <= 0 || K > kmax) return 0;
  return (size_t)n_tiles * 3 * K * sizeof(int);
}

// The three entry points behind their narrow and wide forms (WIDE: int16 pred, K up to RA_KMAX_WIDE): the argument checks in
// their order (NULL, SHAPE, UNSUPPORTED, WORKSPACE), then the launch.
template <bool WIDE>
int ra_run(const float* scores, int ld, int N, int h, int w, int K, const int64_t* desc, long n_tiles, long total_px,
           const void* gt, int gt_bytes, void* pred, int* counts, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  constexpr int KMAX = WIDE ? RA_KMAX_WIDE : RA_KMAX;
  if (!scores || !desc || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && (!gt || !workspace)) return LC2IS_ERR_NULL;
  if (N <= 0 || h <= 0 || w <= 0 || K <= 0 || ld < K || ld % 4 || ((uintptr_t)scores & 15) || n_tiles <= 0 ||
      n_tiles > 0x7fffffffL || total_px <= 0)
    return LC2IS_ERR_SHAPE;
  if (K > KMAX) return LC2IS_ERR_UNSUPPORTED;
  if (counts && gt_bytes != 1 && gt_bytes != 4 && gt_bytes != 8) return LC2IS_ERR_UNSUPPORTED;
  if (counts && workspace_bytes < ra_workspace_bytes(n_tiles, K, KMAX)) return LC2IS_ERR_WORKSPACE;
  RaArgs a = {};
  a.src = scores; a.desc = desc; a.gt = counts ? gt : nullptr; a.pred = pred; a.slab = counts ? (int*)workspace : nullptr;
  a.total_px = total_px; a.N = N; a.h = h; a.w = w; a.ld = ld; a.K = K; a.n_tiles = (int)n_tiles; a.gt_bytes = gt_bytes;
  a.ignore_index = -1;
  return ra_launch<4>(ra_kernel<WIDE>, RA_LDS, a, counts, stream);
}

template <bool WIDE>
int ra_run_windows(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N, const int32_t* win,
                   long n_win, long n_tiles, long total_px, const void* gt, int gt_bytes, int ignore_index, void* pred,
                   int* counts, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  constexpr int KMAX = WIDE ? RA_KMAX_WIDE : RA_KMAX;
  if (!views || !desc || !win || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && (!gt || !workspace)) return LC2IS_ERR_NULL;
  if (N <= 0 || V <= 0 || h <= 0 || w <= 0 || K <= 0 || ld < K || ld % 4 || ((uintptr_t)views & 15) || ((uintptr_t)win & 15) ||
      n_win <= 0 || n_tiles <= 0 || n_tiles > 0x7fffffffL || total_px <= 0 || ignore_index < -1)
    return LC2IS_ERR_SHAPE;
  if (K > KMAX) return LC2IS_ERR_UNSUPPORTED;
  if (counts && gt_bytes != 1 && gt_bytes != 4 && gt_bytes != 8) return LC2IS_ERR_UNSUPPORTED;
  if (counts && workspace_bytes < ra_workspace_bytes(n_tiles, K, KMAX)) return LC2IS_ERR_WORKSPACE;
  RaArgs a = {};
  a.src = views; a.desc = desc; a.win = win; a.gt = counts ? gt : nullptr; a.pred = pred;
  a.slab = counts ? (int*)workspace : nullptr;
  a.total_px = total_px; a.n_win = n_win; a.N = N; a.V = V; a.h = h; a.w = w; a.ld = ld; a.K = K; a.n_tiles = (int)n_tiles;
  a.gt_bytes = gt_bytes; a.ignore_index = ignore_index;
  return ra_launch<8>(ra_win_kernel<WIDE>, RA_WIN_LDS, a, counts, stream);
}

template <bool WIDE>
int ra_run_multiscale(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N, const int64_t* canv,
                      long n_canv, const int32_t* win, long n_win, long n_tiles, long total_px, const void* gt, int gt_bytes,
                      int ignore_index, int mode, void* pred, int* counts, void* workspace, size_t workspace_bytes,
                      hipStream_t stream) {
  constexpr int KMAX = WIDE ? RA_KMAX_WIDE : RA_KMAX;
  if (!views || !desc || !canv || !win || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && (!gt || !workspace)) return LC2IS_ERR_NULL;
  if (N <= 0 || V <= 0 || h <= 0 || w <= 0 || K <= 0 || ld < K || ld % 4 || ((uintptr_t)views & 15) || ((uintptr_t)win & 15) ||
      n_canv <= 0 || n_win <= 0 || n_tiles <= 0 || n_tiles > 0x7fffffffL || total_px <= 0 || ignore_index < -1 ||
      (mode != LC2IS_MS_LOGIT && mode != LC2IS_MS_PROB))
    return LC2IS_ERR_SHAPE;
  if (K > KMAX) return LC2IS_ERR_UNSUPPORTED;
  if (counts && gt_bytes != 1 && gt_bytes != 4 && gt_bytes != 8) return LC2IS_ERR_UNSUPPORTED;
  if (counts && workspace_bytes < ra_workspace_bytes(n_tiles, K, KMAX)) return LC2IS_ERR_WORKSPACE;
  RaArgs a = {};
  a.src = views; a.desc = desc; a.canv = canv; a.win = win; a.gt = counts ? gt : nullptr; a.pred = pred;
  a.slab = counts ? (int*)workspace : nullptr;
  a.total_px = total_px; a.n_canv = n_canv; a.n_win = n_win; a.N = N; a.V = V; a.h = h; a.w = w; a.ld = ld; a.K = K;
  a.n_tiles = (int)n_tiles; a.gt_bytes = gt_bytes; a.ignore_index = ignore_index;
  if (mode == LC2IS_MS_PROB) {
    static DevOnce attr_set;   // 70 KB of dynamic LDS: above the default limit (one flag per instantiation)
    if (attr_set.need()) {
      if (hipFuncSetAttribute((const void*)ra_ms_kernel<LC2IS_MS_PROB, WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)RA_MS_LDS_PROB) != hipSuccess)
        return LC2IS_ERR_LAUNCH;
      attr_set.done();
    }
    return ra_launch<6>(ra_ms_kernel<LC2IS_MS_PROB, WIDE>, RA_MS_LDS_PROB, a, counts, stream);
  }
  return ra_launch<6>(ra_ms_kernel<LC2IS_MS_LOGIT, WIDE>, RA_WIN_LDS, a, counts, stream);
}

}  // namespace

extern "C" size_t lc2is_resize_argmax_workspace_bytes(long n_tiles, int K) { return ra_workspace_bytes(n_tiles, K, RA_KMAX); }

extern "C" size_t lc2is_resize_argmax_wide_workspace_bytes(long n_tiles, int K) {
  return ra_workspace_bytes(n_tiles, K, RA_KMAX_WIDE);
}

extern "C" int lc2is_resize_argmax(const float* scores, int ld, int N, int h, int w, int K, const int64_t* desc, long n_tiles,
                                   long total_px, const void* gt, int gt_bytes, uint8_t* pred, int* counts, void* workspace,
                                   size_t workspace_bytes, lc2is_stream_t stream) {
  return ra_run<false>(scores, ld, N, h, w, K, desc, n_tiles, total_px, gt, gt_bytes, pred, counts, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

extern "C" int lc2is_resize_argmax_wide(const float* scores, int ld, int N, int h, int w, int K, const int64_t* desc,
                                        long n_tiles, long total_px, const void* gt, int gt_bytes, int16_t* pred, int* counts,
                                        void* workspace, size_t workspace_bytes, lc2is_stream_t stream) {
  return ra_run<true>(scores, ld, N, h, w, K, desc, n_tiles, total_px, gt, gt_bytes, pred, counts, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

extern "C" int lc2is_resize_argmax_windows(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                           const int32_t* win, long n_win, long n_tiles, long total_px, const void* gt,
                                           int gt_bytes, int ignore_index, uint8_t* pred, int* counts, void* workspace,
                                           size_t workspace_bytes, lc2is_stream_t stream) {
  return ra_run_windows<false>(views, ld, V, h, w, K, desc, N, win, n_win, n_tiles, total_px, gt, gt_bytes, ignore_index, pred,
                               counts, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lc2is_resize_argmax_windows_wide(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                                const int32_t* win, long n_win, long n_tiles, long total_px, const void* gt,
                                                int gt_bytes, int ignore_index, int16_t* pred, int* counts, void* workspace,
                                                size_t workspace_bytes, lc2is_stream_t stream) {
  return ra_run_windows<true>(views, ld, V, h, w, K, desc, N, win, n_win, n_tiles, total_px, gt, gt_bytes, ignore_index, pred,
                              counts, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lc2is_resize_argmax_multiscale(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                              const int64_t* canv, long n_canv, const int32_t* win, long n_win, long n_tiles,
                                              long total_px, const void* gt, int gt_bytes, int ignore_index, int mode,
                                              uint8_t* pred, int* counts, void* workspace, size_t workspace_bytes,
                                              lc2is_stream_t stream) {
  return ra_run_multiscale<false>(views, ld, V, h, w, K, desc, N, canv, n_canv, win, n_win, n_tiles, total_px, gt, gt_bytes,
                                  ignore_index, mode, pred, counts, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lc2is_resize_argmax_multiscale_wide(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc,
                                                   int N, const int64_t* canv, long n_canv, const int32_t* win, long n_win,
                                                   long n_tiles, long total_px, const void* gt, int gt_bytes, int ignore_index,
                                                   int mode, int16_t* pred, int* counts, void* workspace, size_t workspace_bytes,
                                                   lc2is_stream_t stream) {
  return ra_run_multiscale<true>(views, ld, V, h, w, K, desc, N, canv, n_canv, win, n_win, n_tiles, total_px, gt, gt_bytes,
                                 ignore_index, mode, pred, counts, workspace, workspace_bytes, (hipStream_t)stream);
}
