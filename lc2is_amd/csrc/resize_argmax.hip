// Bicubic resize of per-class scores to each image's ORIGINAL size fused with the argmax over the classes and the per-class
// confusion counts of the original-size mIoU (gfx950).
// replaces: metrics.py:61-79 (compute_gt_mIOU: F.interpolate(size=) + Softmax2d + JaccardIndex per image) and
//   metrics.py:35-42,137-143 (prepare_for_gt_metrics / original_size_interpolate, then argmax).
//
// The [K, H, W] fp32 score map of the reference (211 MB for a 683 x 512 ADE20K image at K = 151, 1.9 GB at 2048 x 1536) is never
// formed.  A block owns a 16 x 16 tile of one image's OUTPUT pixels, one thread per pixel, and keeps that pixel's running
// (max, argmax) in registers while it walks the channels in chunks of 32, in increasing order (exact ties: the lowest index wins,
// as torch.argmax).  Per chunk: the tile's low-resolution footprint is staged in LDS, a horizontal pass interpolates the tile's
// columns on every footprint row, and a vertical pass finishes each pixel.  A downscaled tile (output size below the score grid)
// reads a wider footprint: the tile is then walked in bands of rows / columns whose footprint fits RA_FMAX, chosen in the kernel
// from the same taps it uses (correct at every scale, full tiles whenever the image is upscaled by about 3 or more).
// Counts: every wave histograms its own 64 pixels in LDS (one writer per histogram: ballot + popcount per distinct class), the
// block sums its waves in a fixed order into a per-tile slab of the workspace, and ra_finish_kernel sums each image's slabs in a
// fixed order.  No read-modify-write atomics: pred and counts are bitwise reproducible and independent of the batch.
//
// ra_win_kernel (lc2is_resize_argmax_windows) is the same kernel for sliding-window evaluation: the source of an image is a canvas
// of Hc x Wc score cells that is never formed, each cell the mean of the window views that cover it (mmseg's slide_inference, with
// an optional mirrored copy of every window).  Only the footprint staging differs: a cell is summed over the image's window list
// (staged once per block in LDS) in list order and divided by the cover count.
// replaces: nothing in the reference, which scores the centre crop only (metrics.py:137-143 on one forward).
#include "common.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

constexpr int RA_T = LC2IS_RESIZE_TILE;   // output tile edge; one thread per pixel
constexpr int RA_THREADS = RA_T * RA_T;
constexpr int RA_FMAX = 10;               // footprint edge (source rows / columns) of one band
constexpr int RA_CC = 32;                 // channels per chunk
constexpr int RA_CP = RA_CC + 4;          // LDS floats per footprint cell: 16 lanes reading 16 B each across x hit distinct banks
constexpr int RA_KMAX = 192;

struct RaArgs {
  const float* scores;      // [N, h, w, ld] channels-last fp32, K valid channels
  const int64_t* desc;      // [N][4]: H, W, first pixel of the image in pred / gt, first tile
  const void* gt;           // packed like pred: uint8 / int32 / int64 (gt_bytes = 1 / 4 / 8), or null
  uint8_t* pred;            // [total_px] or null
  int* slab;                // [n_tiles][3][K] per-tile counts, or null (no counts)
  long total_px;
  int N, h, w, ld, K, n_tiles, gt_bytes;
};

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

// one wave: hist[cls] += number of its lanes with `on` and key == cls (one iteration per distinct key; the wave is the only writer)
__device__ __forceinline__ void wave_hist(int* hist, bool on, int key, int lane) {
  while (true) {
    const unsigned long long m = __ballot(on);
    if (m == 0ull) break;
    const int leader = __ffsll((unsigned long long)m) - 1;
    const int cls = __shfl(key, leader);
    const bool mine = on && key == cls;
    const unsigned long long e = __ballot(mine);
    if (lane == leader) hist[cls] += __popcll(e);
    on = on && !mine;
  }
}

__global__ __launch_bounds__(RA_THREADS) void ra_kernel(RaArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_foot = (float*)smem;                         // [RA_FMAX * RA_FMAX][RA_CP]  footprint of the band, one chunk
  float* s_hb = s_foot + RA_FMAX * RA_FMAX * RA_CP;     // [RA_FMAX][RA_T][RA_CP]     footprint rows interpolated along x
  int4* s_xi = (int4*)(s_hb + RA_FMAX * RA_T * RA_CP);  // [RA_T] x taps of the band (relative to its first column)
  float4* s_xw = (float4*)(s_xi + RA_T);                // [RA_T] x weights
  int* s_hist = (int*)smem;                             // after the channel loops: [4 waves][3][K] (aliases s_foot)

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = p.K;

  // the image of this tile: the last one whose first tile is <= blockIdx.x (desc[i][3] ascending)
  const int t = blockIdx.x;
  int lo = 0, hi = p.N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.desc[4 * mid + 3] <= t) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const long H = p.desc[4 * b], W = p.desc[4 * b + 1], pix0 = p.desc[4 * b + 2], tile0 = p.desc[4 * b + 3];
  const long tiles_x = (W + RA_T - 1) / RA_T;
  // a descriptor that does not fit the buffers is not followed (nothing outside them is read or written)
  if (H < 1 || W < 1 || t < tile0 || pix0 < 0 || pix0 + H * W > p.total_px) return;
  const long tl = t - tile0;
  const int Y0 = (int)(tl / tiles_x) * RA_T, X0 = (int)(tl % tiles_x) * RA_T;
  if (Y0 >= H) return;
  const int TH = (int)min((long)RA_T, H - Y0), TW = (int)min((long)RA_T, W - X0);
  const float sy = (float)p.h / (float)H, sx = (float)p.w / (float)W;   // torch: input_size / output_size

  const int py = tid / RA_T, px = tid % RA_T;
  const bool valid = py < TH && px < TW;
  float best = -INFINITY;
  int arg = 0;
  const float* img = p.scores + (size_t)b * p.h * p.w * p.ld;

  for (int rb0 = 0; rb0 < TH;) {
    const int R = ra_band(Y0 + rb0, TH - rb0, sy, p.h);
    const int2 ys = ra_span(Y0 + rb0, Y0 + rb0 + R - 1, sy, p.h);
    const int fy0 = ys.x, FH = ys.y - ys.x + 1;
    const bool row_in = valid && py >= rb0 && py < rb0 + R;
    int yi[4] = {0, 0, 0, 0};
    float yw[4] = {0.f, 0.f, 0.f, 0.f};
    if (row_in) {
      const Taps ty = make_taps(Y0 + py, sy, p.h, LC2IS_INTERP_BICUBIC);
#pragma unroll
      for (int k = 0; k < 4; ++k) { yi[k] = ty.idx[k] - fy0; yw[k] = ty.w[k]; }
    }
    for (int cb0 = 0; cb0 < TW;) {
      const int CW = ra_band(X0 + cb0, TW - cb0, sx, p.w);
      const int2 xs = ra_span(X0 + cb0, X0 + cb0 + CW - 1, sx, p.w);
      const int fx0 = xs.x, FW = xs.y - xs.x + 1;
      const bool in = row_in && px >= cb0 && px < cb0 + CW;
      __syncthreads();   // the previous band's last reads of s_xi / s_xw / s_hb are done
      if (tid < CW) {
        const Taps tx = make_taps(X0 + cb0 + tid, sx, p.w, LC2IS_INTERP_BICUBIC);
        s_xi[tid] = make_int4(tx.idx[0] - fx0, tx.idx[1] - fx0, tx.idx[2] - fx0, tx.idx[3] - fx0);
        s_xw[tid] = make_float4(tx.w[0], tx.w[1], tx.w[2], tx.w[3]);
      }
      for (int c0 = 0; c0 < K; c0 += RA_CC) {
        // stage the footprint's channels [c0, c0 + 32) (those at or past ld read as 0, and never reach the argmax)
        for (int i = tid; i < FH * FW * (RA_CC / 4); i += RA_THREADS) {
          const int c4 = i % (RA_CC / 4), cell = i / (RA_CC / 4);
          const int fr = cell / FW, fc = cell % FW;
          const int c = c0 + 4 * c4;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < p.ld) v = *reinterpret_cast<const float4*>(img + ((size_t)(fy0 + fr) * p.w + fx0 + fc) * p.ld + c);
          *reinterpret_cast<float4*>(s_foot + cell * RA_CP + 4 * c4) = v;
        }
        __syncthreads();
        // horizontal: s_hb[r][x] = sum_k wx[x][k] * foot[r][xi[x][k]]
        for (int i = tid; i < FH * CW * (RA_CC / 4); i += RA_THREADS) {
          const int c4 = i % (RA_CC / 4), x = (i / (RA_CC / 4)) % CW, r = i / (RA_CC / 4 * CW);
          const int4 xi = s_xi[x];
          const float4 xw = s_xw[x];
          const float* row = s_foot + r * FW * RA_CP + 4 * c4;
          float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
          a = fma4(xw.x, *reinterpret_cast<const float4*>(row + xi.x * RA_CP), a);
          a = fma4(xw.y, *reinterpret_cast<const float4*>(row + xi.y * RA_CP), a);
          a = fma4(xw.z, *reinterpret_cast<const float4*>(row + xi.z * RA_CP), a);
          a = fma4(xw.w, *reinterpret_cast<const float4*>(row + xi.w * RA_CP), a);
          *reinterpret_cast<float4*>(s_hb + (r * RA_T + cb0 + x) * RA_CP + 4 * c4) = a;
        }
        __syncthreads();
        // vertical + running argmax, channels in increasing order, strict > (the first maximum stays)
        if (in) {
          const int nc = min(RA_CC, K - c0);
          for (int c4 = 0; c4 < RA_CC / 4; ++c4) {
            if (4 * c4 >= nc) break;
            const float* col = s_hb + px * RA_CP + 4 * c4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 4; ++k) a = fma4(yw[k], *reinterpret_cast<const float4*>(col + yi[k] * RA_T * RA_CP), a);
            const int c = c0 + 4 * c4;
            if (a.x > best) { best = a.x; arg = c; }
            if (4 * c4 + 1 < nc && a.y > best) { best = a.y; arg = c + 1; }
            if (4 * c4 + 2 < nc && a.z > best) { best = a.z; arg = c + 2; }
            if (4 * c4 + 3 < nc && a.w > best) { best = a.w; arg = c + 3; }
          }
        }
        __syncthreads();   // s_foot is restaged and s_hb rewritten by the next chunk
      }
      cb0 += CW;
    }
    rb0 += R;
  }

  const size_t o = (size_t)pix0 + (size_t)(Y0 + py) * W + X0 + px;
  if (valid && p.pred) p.pred[o] = (uint8_t)arg;
  if (!p.slab) return;

  int g = -1;   // the pixel's class if it is labelled (0 <= gt < K), else -1
  if (valid && p.gt) {
    long v;
    if (p.gt_bytes == 1) v = ((const uint8_t*)p.gt)[o];
    else if (p.gt_bytes == 4) v = ((const int32_t*)p.gt)[o];
    else v = ((const int64_t*)p.gt)[o];
    g = (v >= 0 && v < K) ? (int)v : -1;
  }
  int* hw = s_hist + wid * 3 * K;   // this wave's {intersection[K], predicted[K], labelled[K]}
  for (int i = lane; i < 3 * K; i += 64) hw[i] = 0;
  __syncthreads();
  wave_hist(hw + K, valid, arg, lane);
  wave_hist(hw, valid && g == arg, arg, lane);
  wave_hist(hw + 2 * K, g >= 0, g, lane);
  __syncthreads();
  int* out = p.slab + (size_t)t * 3 * K;
  for (int i = tid; i < 3 * K; i += RA_THREADS)
    out[i] = ((s_hist[i] + s_hist[3 * K + i]) + s_hist[6 * K + i]) + s_hist[9 * K + i];
}

// counts[b][e] = sum over the image's tiles of slab[tile][e], tiles in increasing order within each of 4 strided parts, the parts
// added in order: grid (ceil(3K / 64), N), 256 threads.  DS: int64 words per descriptor (4: lc2is_resize_argmax, 8: the windowed call,
// whose first four words mean the same)
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

constexpr size_t RA_LDS = (size_t)(RA_FMAX * RA_FMAX + RA_FMAX * RA_T) * RA_CP * sizeof(float) + RA_T * (sizeof(int4) + sizeof(float4));
static_assert((size_t)RA_FMAX * RA_FMAX * RA_CP * sizeof(float) >= 4 * 3 * RA_KMAX * sizeof(int), "histograms fit the footprint");

// ---- sliding-window source: the canvas mean of the covering views ----------------------------------------------------------
constexpr int RA_WMAX = LC2IS_SLIDE_MAX_WIN;

struct RaWinArgs {
  const float* views;       // [V, h, w, ld] channels-last fp32, K valid channels: one score grid per window forward
  const int64_t* desc;      // [N][8]: H, W, first pixel, first tile (as RaArgs), Hc, Wc (canvas cells), first window, n_windows
  const int32_t* win;       // [n_win][4]: view, oy, ox (origin in canvas cells), flags (bit 0: the view is mirrored along x)
  const void* gt;
  uint8_t* pred;
  int* slab;
  long total_px, n_win;
  int N, V, h, w, ld, K, n_tiles, gt_bytes, ignore_index;
};

// A restatement of ra_kernel, not a shared body: ra_kernel has to keep the instructions it had, and a body shared through a source
// functor changes its register allocation.  Apart from the descriptor, the window list, the staging loop and the counting rule the two
// are line for line the same: a change to bands, taps or histograms goes into both (tests/test_gpu_slide.py holds the one-view case
// to ra_kernel's bits).
__global__ __launch_bounds__(RA_THREADS) void ra_win_kernel(RaWinArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_foot = (float*)smem;                         // as ra_kernel
  float* s_hb = s_foot + RA_FMAX * RA_FMAX * RA_CP;
  int4* s_xi = (int4*)(s_hb + RA_FMAX * RA_T * RA_CP);
  float4* s_xw = (float4*)(s_xi + RA_T);
  int4* s_win = (int4*)(s_xw + RA_T);                   // [RA_WMAX] the image's usable windows, in list order
  int* s_nw = (int*)(s_win + RA_WMAX);                  // their number
  int* s_hist = (int*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = p.K;

  const int t = blockIdx.x;
  int lo = 0, hi = p.N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.desc[8 * mid + 3] <= t) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const int64_t* d = p.desc + 8 * b;
  const long H = d[0], W = d[1], pix0 = d[2], tile0 = d[3], Hc_ = d[4], Wc_ = d[5], win0 = d[6], nwin = d[7];
  const long tiles_x = (W + RA_T - 1) / RA_T;
  // a descriptor that does not fit the buffers, the window limit or the views is not followed
  if (H < 1 || W < 1 || t < tile0 || pix0 < 0 || pix0 + H * W > p.total_px) return;
  if (Hc_ < p.h || Wc_ < p.w || Hc_ > (1L << 24) || Wc_ > (1L << 24)) return;
  if (nwin < 0 || nwin > RA_WMAX || win0 < 0 || win0 + nwin > p.n_win) return;
  const int Hc = (int)Hc_, Wc = (int)Wc_;
  const long tl = t - tile0;
  const int Y0 = (int)(tl / tiles_x) * RA_T, X0 = (int)(tl % tiles_x) * RA_T;
  if (Y0 >= H) return;
  const int TH = (int)min((long)RA_T, H - Y0), TW = (int)min((long)RA_T, W - X0);
  const float sy = (float)Hc / (float)H, sx = (float)Wc / (float)W;

  // the window list, once per block: wave 0 keeps the windows whose view and origin are in range, order preserved
  if (wid == 0) {
    int4 wv = make_int4(0, 0, 0, 0);
    bool ok = false;
    if (lane < nwin) {
      wv = *reinterpret_cast<const int4*>(p.win + 4 * (win0 + lane));
      ok = wv.x >= 0 && wv.x < p.V && wv.y >= 0 && wv.y <= Hc - p.h && wv.z >= 0 && wv.z <= Wc - p.w;
    }
    const unsigned long long m = __ballot(ok);
    if (ok) s_win[__popcll(m & ((1ull << lane) - 1ull))] = wv;
    if (lane == 0) *s_nw = __popcll(m);
  }
  __syncthreads();
  const int nw = *s_nw;

  const int py = tid / RA_T, px = tid % RA_T;
  const bool valid = py < TH && px < TW;
  float best = -INFINITY;
  int arg = 0;
  const size_t view_stride = (size_t)p.h * p.w * p.ld;

  for (int rb0 = 0; rb0 < TH;) {
    const int R = ra_band(Y0 + rb0, TH - rb0, sy, Hc);
    const int2 ys = ra_span(Y0 + rb0, Y0 + rb0 + R - 1, sy, Hc);
    const int fy0 = ys.x, FH = ys.y - ys.x + 1;
    const bool row_in = valid && py >= rb0 && py < rb0 + R;
    int yi[4] = {0, 0, 0, 0};
    float yw[4] = {0.f, 0.f, 0.f, 0.f};
    if (row_in) {
      const Taps ty = make_taps(Y0 + py, sy, Hc, LC2IS_INTERP_BICUBIC);
#pragma unroll
      for (int k = 0; k < 4; ++k) { yi[k] = ty.idx[k] - fy0; yw[k] = ty.w[k]; }
    }
    for (int cb0 = 0; cb0 < TW;) {
      const int CW = ra_band(X0 + cb0, TW - cb0, sx, Wc);
      const int2 xs = ra_span(X0 + cb0, X0 + cb0 + CW - 1, sx, Wc);
      const int fx0 = xs.x, FW = xs.y - xs.x + 1;
      const bool in = row_in && px >= cb0 && px < cb0 + CW;
      __syncthreads();
      if (tid < CW) {
        const Taps tx = make_taps(X0 + cb0 + tid, sx, Wc, LC2IS_INTERP_BICUBIC);
        s_xi[tid] = make_int4(tx.idx[0] - fx0, tx.idx[1] - fx0, tx.idx[2] - fx0, tx.idx[3] - fx0);
        s_xw[tid] = make_float4(tx.w[0], tx.w[1], tx.w[2], tx.w[3]);
      }
      for (int c0 = 0; c0 < K; c0 += RA_CC) {
        // stage the footprint's channels [c0, c0 + 32): each canvas cell is the sum of the views that cover it, in list order from
        // the first one, divided by their number (a cell that nothing covers reads 0)
        for (int i = tid; i < FH * FW * (RA_CC / 4); i += RA_THREADS) {
          const int c4 = i % (RA_CC / 4), cell = i / (RA_CC / 4);
          const int cy = fy0 + cell / FW, cx = fx0 + cell % FW;
          const int c = c0 + 4 * c4;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < p.ld) {
            int n = 0;
            for (int j = 0; j < nw; ++j) {
              const int4 wv = s_win[j];
              const int ry = cy - wv.y, rx = cx - wv.z;
              if (ry < 0 || ry >= p.h || rx < 0 || rx >= p.w) continue;
              const int col = (wv.w & 1) ? p.w - 1 - rx : rx;
              const float4 x = *reinterpret_cast<const float4*>(p.views + (size_t)wv.x * view_stride + ((size_t)ry * p.w + col) * p.ld + c);
              v = n ? make_float4(v.x + x.x, v.y + x.y, v.z + x.z, v.w + x.w) : x;
              ++n;
            }
            if (n > 1) {
              const float fn = (float)n;
              v = make_float4(v.x / fn, v.y / fn, v.z / fn, v.w / fn);
            }
          }
          *reinterpret_cast<float4*>(s_foot + cell * RA_CP + 4 * c4) = v;
        }
        __syncthreads();
        for (int i = tid; i < FH * CW * (RA_CC / 4); i += RA_THREADS) {
          const int c4 = i % (RA_CC / 4), x = (i / (RA_CC / 4)) % CW, r = i / (RA_CC / 4 * CW);
          const int4 xi = s_xi[x];
          const float4 xw = s_xw[x];
          const float* row = s_foot + r * FW * RA_CP + 4 * c4;
          float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
          a = fma4(xw.x, *reinterpret_cast<const float4*>(row + xi.x * RA_CP), a);
          a = fma4(xw.y, *reinterpret_cast<const float4*>(row + xi.y * RA_CP), a);
          a = fma4(xw.z, *reinterpret_cast<const float4*>(row + xi.z * RA_CP), a);
          a = fma4(xw.w, *reinterpret_cast<const float4*>(row + xi.w * RA_CP), a);
          *reinterpret_cast<float4*>(s_hb + (r * RA_T + cb0 + x) * RA_CP + 4 * c4) = a;
        }
        __syncthreads();
        if (in) {
          const int nc = min(RA_CC, K - c0);
          for (int c4 = 0; c4 < RA_CC / 4; ++c4) {
            if (4 * c4 >= nc) break;
            const float* col = s_hb + px * RA_CP + 4 * c4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 4; ++k) a = fma4(yw[k], *reinterpret_cast<const float4*>(col + yi[k] * RA_T * RA_CP), a);
            const int c = c0 + 4 * c4;
            if (a.x > best) { best = a.x; arg = c; }
            if (4 * c4 + 1 < nc && a.y > best) { best = a.y; arg = c + 1; }
            if (4 * c4 + 2 < nc && a.z > best) { best = a.z; arg = c + 2; }
            if (4 * c4 + 3 < nc && a.w > best) { best = a.w; arg = c + 3; }
          }
        }
        __syncthreads();
      }
      cb0 += CW;
    }
    rb0 += R;
  }

  const size_t o = (size_t)pix0 + (size_t)(Y0 + py) * W + X0 + px;
  if (valid && p.pred) p.pred[o] = (uint8_t)arg;
  if (!p.slab) return;

  // ignore_index < 0: every pixel counts in "predicted" (ra_kernel's rule); >= 0: a pixel whose gt is ignore_index or outside
  // [0, K) counts in none of the three rows (mmseg's intersect_and_union)
  int g = -1;
  if (valid && p.gt) {
    long v;
    if (p.gt_bytes == 1) v = ((const uint8_t*)p.gt)[o];
    else if (p.gt_bytes == 4) v = ((const int32_t*)p.gt)[o];
    else v = ((const int64_t*)p.gt)[o];
    g = (v >= 0 && v < K && !(p.ignore_index >= 0 && v == p.ignore_index)) ? (int)v : -1;
  }
  int* hw = s_hist + wid * 3 * K;
  for (int i = lane; i < 3 * K; i += 64) hw[i] = 0;
  __syncthreads();
  wave_hist(hw + K, p.ignore_index >= 0 ? g >= 0 : valid, arg, lane);
  wave_hist(hw, valid && g == arg, arg, lane);
  wave_hist(hw + 2 * K, g >= 0, g, lane);
  __syncthreads();
  int* out = p.slab + (size_t)t * 3 * K;
  for (int i = tid; i < 3 * K; i += RA_THREADS)
    out[i] = ((s_hist[i] + s_hist[3 * K + i]) + s_hist[6 * K + i]) + s_hist[9 * K + i];
}

constexpr size_t RA_WIN_LDS = RA_LDS + RA_WMAX * sizeof(int4) + 16;

// ---- multi-scale source: several canvases per image, summed as logits or as softmax probabilities --------------------------
// ra_ms_kernel<MODE> (lc2is_resize_argmax_multiscale): an image is an ordered list of canvases, each with its own size and window
// list; every canvas is resized to the image's size with ra_win_kernel's arithmetic and the results are combined per class before
// the argmax.  The per-class sums of a pixel cannot be kept for all K classes, so the canvases are walked once per channel chunk
// (32 accumulators per pixel in registers); the softmax statistics (max, 1 / sum) of every canvas at every pixel come from a
// first walk over all chunks and wait in LDS (16 canvases x 256 pixels x 8 B = 32 KB).  A window may overhang its canvas at the
// bottom / right (a scale below the crop): only its on-canvas part is read, and a mirrored view is mirrored over that part.
constexpr int RA_AMAX = LC2IS_MS_MAX_CANVAS;

struct RaMsArgs {
  const float* views;       // [V, h, w, ld] as RaWinArgs
  const int64_t* desc;      // [N][6]: H, W, first pixel, first tile (as RaArgs), first canvas, n_canvases
  const int64_t* canv;      // [n_canv][4]: Hc, Wc (canvas cells), first window, n_windows
  const int32_t* win;       // [n_win][4] as RaWinArgs
  const void* gt;
  uint8_t* pred;
  int* slab;
  long total_px, n_canv, n_win;
  int N, V, h, w, ld, K, n_tiles, gt_bytes, ignore_index;
};

// a canvas row that fits the window table and the limits
__device__ __forceinline__ bool ms_canvas_ok(const RaMsArgs& p, const int64_t* c) {
  return c[0] >= 1 && c[0] <= (1L << 24) && c[1] >= 1 && c[1] <= (1L << 24) && c[2] >= 0 && c[3] >= 1 && c[3] <= RA_WMAX &&
         c[2] + c[3] <= p.n_win;
}

// this lane's window of a checked canvas row: true when it is usable (view in range, origin on the canvas)
__device__ __forceinline__ bool ms_window(const RaMsArgs& p, const int64_t* c, int lane, int4& wv) {
  wv = make_int4(0, 0, 0, 0);
  if (lane >= c[3]) return false;
  wv = *reinterpret_cast<const int4*>(p.win + 4 * (c[2] + lane));
  return wv.x >= 0 && wv.x < p.V && wv.y >= 0 && wv.y < c[0] && wv.z >= 0 && wv.z < c[1];
}

// One channel chunk [c0, c0 + 32) of one canvas over the block's tile: ra_win_kernel's bands, staging, horizontal and vertical
// passes, statement for statement (tests/test_gpu_multiscale.py holds the one-canvas logit case to ra_win_kernel's bits), with the
// on-canvas part of an overhanging window in the staging loop.  f(c4, y) receives channels c0 + 4 * c4 .. + 3 of the thread's pixel,
// c4 a constant after unrolling; channels at or past K hold values that must not be used.  Ends on a barrier: the caller may
// restage s_win or reuse s_foot at once.
template <class F>
__device__ __forceinline__ void ms_walk(const RaMsArgs& p, float* s_foot, float* s_hb, int4* s_xi, float4* s_xw, const int4* s_win,
                                        int nw, int Hc, int Wc, long H, long W, int Y0, int X0, int TH, int TW, int c0, F&& f) {
  const int tid = threadIdx.x;
  const int py = tid / RA_T, px = tid % RA_T;
  const bool valid = py < TH && px < TW;
  const float sy = (float)Hc / (float)H, sx = (float)Wc / (float)W;
  const size_t view_stride = (size_t)p.h * p.w * p.ld;
  const int nc = min(RA_CC, p.K - c0);

  for (int rb0 = 0; rb0 < TH;) {
    const int R = ra_band(Y0 + rb0, TH - rb0, sy, Hc);
    const int2 ys = ra_span(Y0 + rb0, Y0 + rb0 + R - 1, sy, Hc);
    const int fy0 = ys.x, FH = ys.y - ys.x + 1;
    const bool row_in = valid && py >= rb0 && py < rb0 + R;
    int yi[4] = {0, 0, 0, 0};
    float yw[4] = {0.f, 0.f, 0.f, 0.f};
    if (row_in) {
      const Taps ty = make_taps(Y0 + py, sy, Hc, LC2IS_INTERP_BICUBIC);
#pragma unroll
      for (int k = 0; k < 4; ++k) { yi[k] = ty.idx[k] - fy0; yw[k] = ty.w[k]; }
    }
    for (int cb0 = 0; cb0 < TW;) {
      const int CW = ra_band(X0 + cb0, TW - cb0, sx, Wc);
      const int2 xs = ra_span(X0 + cb0, X0 + cb0 + CW - 1, sx, Wc);
      const int fx0 = xs.x, FW = xs.y - xs.x + 1;
      const bool in = row_in && px >= cb0 && px < cb0 + CW;
      __syncthreads();
      if (tid < CW) {
        const Taps tx = make_taps(X0 + cb0 + tid, sx, Wc, LC2IS_INTERP_BICUBIC);
        s_xi[tid] = make_int4(tx.idx[0] - fx0, tx.idx[1] - fx0, tx.idx[2] - fx0, tx.idx[3] - fx0);
        s_xw[tid] = make_float4(tx.w[0], tx.w[1], tx.w[2], tx.w[3]);
      }
      // stage the footprint: a cell is the sum of the on-canvas parts that cover it, in list order from the first one, divided
      // by their number.  The footprint lies on the canvas (taps are clamped), so ry < h is ry < min(h, Hc - oy), and so along x.
      for (int i = tid; i < FH * FW * (RA_CC / 4); i += RA_THREADS) {
        const int c4 = i % (RA_CC / 4), cell = i / (RA_CC / 4);
        const int cy = fy0 + cell / FW, cx = fx0 + cell % FW;
        const int c = c0 + 4 * c4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < p.ld) {
          int n = 0;
          for (int j = 0; j < nw; ++j) {
            const int4 wv = s_win[j];
            const int ry = cy - wv.y, rx = cx - wv.z;
            if (ry < 0 || ry >= p.h || rx < 0 || rx >= p.w) continue;
            const int col = (wv.w & 1) ? min(p.w, Wc - wv.z) - 1 - rx : rx;
            const float4 x = *reinterpret_cast<const float4*>(p.views + (size_t)wv.x * view_stride + ((size_t)ry * p.w + col) * p.ld + c);
            v = n ? make_float4(v.x + x.x, v.y + x.y, v.z + x.z, v.w + x.w) : x;
            ++n;
          }
          if (n > 1) {
            const float fn = (float)n;
            v = make_float4(v.x / fn, v.y / fn, v.z / fn, v.w / fn);
          }
        }
        *reinterpret_cast<float4*>(s_foot + cell * RA_CP + 4 * c4) = v;
      }
      __syncthreads();
      for (int i = tid; i < FH * CW * (RA_CC / 4); i += RA_THREADS) {
        const int c4 = i % (RA_CC / 4), x = (i / (RA_CC / 4)) % CW, r = i / (RA_CC / 4 * CW);
        const int4 xi = s_xi[x];
        const float4 xw = s_xw[x];
        const float* row = s_foot + r * FW * RA_CP + 4 * c4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        a = fma4(xw.x, *reinterpret_cast<const float4*>(row + xi.x * RA_CP), a);
        a = fma4(xw.y, *reinterpret_cast<const float4*>(row + xi.y * RA_CP), a);
        a = fma4(xw.z, *reinterpret_cast<const float4*>(row + xi.z * RA_CP), a);
        a = fma4(xw.w, *reinterpret_cast<const float4*>(row + xi.w * RA_CP), a);
        *reinterpret_cast<float4*>(s_hb + (r * RA_T + cb0 + x) * RA_CP + 4 * c4) = a;
      }
      __syncthreads();
      if (in) {
#pragma unroll
        for (int c4 = 0; c4 < RA_CC / 4; ++c4) {
          if (4 * c4 < nc) {
            const float* col = s_hb + px * RA_CP + 4 * c4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 4; ++k) a = fma4(yw[k], *reinterpret_cast<const float4*>(col + yi[k] * RA_T * RA_CP), a);
            f(c4, a);
          }
        }
      }
      __syncthreads();
      cb0 += CW;
    }
    rb0 += R;
  }
}

template <int MODE>
__global__ __launch_bounds__(RA_THREADS) void ra_ms_kernel(RaMsArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_foot = (float*)smem;                         // as ra_win_kernel
  float* s_hb = s_foot + RA_FMAX * RA_FMAX * RA_CP;
  int4* s_xi = (int4*)(s_hb + RA_FMAX * RA_T * RA_CP);
  float4* s_xw = (float4*)(s_xi + RA_T);
  int4* s_win = (int4*)(s_xw + RA_T);                   // [RA_WMAX] the usable windows of the canvas being walked, in list order
  int* s_nw = (int*)(s_win + RA_WMAX);                  // their number
  float* s_m = (float*)(s_nw + 4);                      // PROB only: [RA_AMAX][RA_THREADS] max over the classes, per canvas and pixel
  float* s_rl = s_m + RA_AMAX * RA_THREADS;             //            [RA_AMAX][RA_THREADS] 1 / sum of exp(y - max)
  int* s_hist = (int*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = p.K;

  const int t = blockIdx.x;
  int lo = 0, hi = p.N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.desc[6 * mid + 3] <= t) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const int64_t* d = p.desc + 6 * b;
  const long H = d[0], W = d[1], pix0 = d[2], tile0 = d[3], cv0 = d[4], ncv = d[5];
  const long tiles_x = (W + RA_T - 1) / RA_T;
  // a descriptor that does not fit the buffers, the tables or the limits is not followed: nothing is written for the image
  if (H < 1 || W < 1 || t < tile0 || pix0 < 0 || pix0 + H * W > p.total_px) return;
  if (ncv < 1 || ncv > RA_AMAX || cv0 < 0 || cv0 + ncv > p.n_canv) return;
  const int A = (int)ncv;
  const int64_t* cv = p.canv + 4 * cv0;
  // every canvas needs a row that fits and one usable window.  Each wave looks for itself (the same loads, the same answer), so
  // the decision is the block's without a barrier.
  for (int a = 0; a < A; ++a) {
    if (!ms_canvas_ok(p, cv + 4 * a)) return;
    int4 wv;
    if (__ballot(ms_window(p, cv + 4 * a, lane, wv)) == 0ull) return;
  }
  const long tl = t - tile0;
  const int Y0 = (int)(tl / tiles_x) * RA_T, X0 = (int)(tl % tiles_x) * RA_T;
  if (Y0 >= H) return;
  const int TH = (int)min((long)RA_T, H - Y0), TW = (int)min((long)RA_T, W - X0);

  const int py = tid / RA_T, px = tid % RA_T;
  const bool valid = py < TH && px < TW;

  // the window list of canvas a, restaged when the canvas changes: wave 0 keeps the usable windows, order preserved.  The walk
  // before it ended on a barrier, so nobody still reads the old list.
  int staged = -1;
  auto stage = [&](int a) {
    if (a == staged) return;
    staged = a;
    if (wid == 0) {
      int4 wv;
      const bool ok = ms_window(p, cv + 4 * a, lane, wv);
      const unsigned long long m = __ballot(ok);
      if (ok) s_win[__popcll(m & ((1ull << lane) - 1ull))] = wv;
      if (lane == 0) *s_nw = __popcll(m);
    }
    __syncthreads();
  };

  if (MODE == LC2IS_MS_PROB) {
    // pass A: the softmax statistics of every canvas at this thread's pixel, online over the chunks (valid channels only)
    for (int a = 0; a < A; ++a) {
      stage(a);
      float m = -INFINITY, l = 0.f;
      for (int c0 = 0; c0 < K; c0 += RA_CC) {
        const int nc = min(RA_CC, K - c0);
        ms_walk(p, s_foot, s_hb, s_xi, s_xw, s_win, *s_nw, (int)cv[4 * a], (int)cv[4 * a + 1], H, W, Y0, X0, TH, TW, c0,
                [&](int c4, float4 y) {
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

  // pass B: per chunk the sum over the canvases, in canvas order from the first one, then the running argmax as ra_win_kernel's
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
      ms_walk(p, s_foot, s_hb, s_xi, s_xw, s_win, *s_nw, (int)cv[4 * a], (int)cv[4 * a + 1], H, W, Y0, X0, TH, TW, c0,
              [&](int c4, float4 y) {
                if (MODE == LC2IS_MS_PROB)
                  y = make_float4(__expf(y.x - m) * rl, __expf(y.y - m) * rl, __expf(y.z - m) * rl, __expf(y.w - m) * rl);
                const float4 s = acc[c4];
                acc[c4] = a ? make_float4(s.x + y.x, s.y + y.y, s.z + y.z, s.w + y.w) : y;
              });
    }
    if (valid) {
#pragma unroll
      for (int c4 = 0; c4 < RA_CC / 4; ++c4) {
        if (4 * c4 < nc) {
          const float4 s = acc[c4];
          const int c = c0 + 4 * c4;
          if (s.x > best) { best = s.x; arg = c; }
          if (4 * c4 + 1 < nc && s.y > best) { best = s.y; arg = c + 1; }
          if (4 * c4 + 2 < nc && s.z > best) { best = s.z; arg = c + 2; }
          if (4 * c4 + 3 < nc && s.w > best) { best = s.w; arg = c + 3; }
        }
      }
    }
  }

  const size_t o = (size_t)pix0 + (size_t)(Y0 + py) * W + X0 + px;
  if (valid && p.pred) p.pred[o] = (uint8_t)arg;
  if (!p.slab) return;

  // counts: ra_win_kernel's rules and histograms (the last walk ended on a barrier: s_foot is free)
  int g = -1;
  if (valid && p.gt) {
    long v;
    if (p.gt_bytes == 1) v = ((const uint8_t*)p.gt)[o];
    else if (p.gt_bytes == 4) v = ((const int32_t*)p.gt)[o];
    else v = ((const int64_t*)p.gt)[o];
    g = (v >= 0 && v < K && !(p.ignore_index >= 0 && v == p.ignore_index)) ? (int)v : -1;
  }
  int* hw = s_hist + wid * 3 * K;
  for (int i = lane; i < 3 * K; i += 64) hw[i] = 0;
  __syncthreads();
  wave_hist(hw + K, p.ignore_index >= 0 ? g >= 0 : valid, arg, lane);
  wave_hist(hw, valid && g == arg, arg, lane);
  wave_hist(hw + 2 * K, g >= 0, g, lane);
  __syncthreads();
  int* out = p.slab + (size_t)t * 3 * K;
  for (int i = tid; i < 3 * K; i += RA_THREADS)
    out[i] = ((s_hist[i] + s_hist[3 * K + i]) + s_hist[6 * K + i]) + s_hist[9 * K + i];
}

constexpr size_t RA_MS_LDS_LOGIT = RA_WIN_LDS;
constexpr size_t RA_MS_LDS_PROB = RA_WIN_LDS + 2 * (size_t)RA_AMAX * RA_THREADS * sizeof(float);
static_assert(RA_MS_LDS_PROB <= 80 * 1024, "two blocks per CU");

}  // namespace

extern "C" size_t lc2is_resize_argmax_workspace_bytes(long n_tiles, int K) {
  if (n_tiles <= 0 || K <= 0 || K > RA_KMAX) return 0;
  return (size_t)n_tiles * 3 * K * sizeof(int);
}

extern "C" int lc2is_resize_argmax(const float* scores, int ld, int N, int h, int w, int K, const int64_t* desc, long n_tiles,
                                   long total_px, const void* gt, int gt_bytes, uint8_t* pred, int* counts, void* workspace,
                                   size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores || !desc || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && (!gt || !workspace)) return LC2IS_ERR_NULL;
  if (N <= 0 || h <= 0 || w <= 0 || K <= 0 || ld < K || ld % 4 || ((uintptr_t)scores & 15) || n_tiles <= 0 ||
      n_tiles > 0x7fffffffL || total_px <= 0)
    return LC2IS_ERR_SHAPE;
  if (K > RA_KMAX) return LC2IS_ERR_UNSUPPORTED;
  if (counts && gt_bytes != 1 && gt_bytes != 4 && gt_bytes != 8) return LC2IS_ERR_UNSUPPORTED;
  if (counts && workspace_bytes < lc2is_resize_argmax_workspace_bytes(n_tiles, K)) return LC2IS_ERR_WORKSPACE;
  RaArgs a;
  a.scores = scores; a.desc = desc; a.gt = counts ? gt : nullptr; a.pred = pred; a.slab = counts ? (int*)workspace : nullptr;
  a.total_px = total_px; a.N = N; a.h = h; a.w = w; a.ld = ld; a.K = K; a.n_tiles = (int)n_tiles; a.gt_bytes = gt_bytes;
  hipLaunchKernelGGL(ra_kernel, dim3((unsigned)n_tiles), dim3(RA_THREADS), RA_LDS, stream, a);
  int rc = lc2is_check_launch();
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(ra_finish_kernel<4>, dim3((3 * K + 63) / 64, N), dim3(256), 0, stream, desc, (const int*)workspace, counts, K,
                     (int)n_tiles);
  return lc2is_check_launch();
}

extern "C" int lc2is_resize_argmax_windows(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                           const int32_t* win, long n_win, long n_tiles, long total_px, const void* gt,
                                           int gt_bytes, int ignore_index, uint8_t* pred, int* counts, void* workspace,
                                           size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!views || !desc || !win || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && (!gt || !workspace)) return LC2IS_ERR_NULL;
  if (N <= 0 || V <= 0 || h <= 0 || w <= 0 || K <= 0 || ld < K || ld % 4 || ((uintptr_t)views & 15) || ((uintptr_t)win & 15) ||
      n_win <= 0 || n_tiles <= 0 || n_tiles > 0x7fffffffL || total_px <= 0 || ignore_index < -1)
    return LC2IS_ERR_SHAPE;
  if (K > RA_KMAX) return LC2IS_ERR_UNSUPPORTED;
  if (counts && gt_bytes != 1 && gt_bytes != 4 && gt_bytes != 8) return LC2IS_ERR_UNSUPPORTED;
  if (counts && workspace_bytes < lc2is_resize_argmax_workspace_bytes(n_tiles, K)) return LC2IS_ERR_WORKSPACE;
  RaWinArgs a;
  a.views = views; a.desc = desc; a.win = win; a.gt = counts ? gt : nullptr; a.pred = pred;
  a.slab = counts ? (int*)workspace : nullptr;
  a.total_px = total_px; a.n_win = n_win; a.N = N; a.V = V; a.h = h; a.w = w; a.ld = ld; a.K = K; a.n_tiles = (int)n_tiles;
  a.gt_bytes = gt_bytes; a.ignore_index = ignore_index;
  hipLaunchKernelGGL(ra_win_kernel, dim3((unsigned)n_tiles), dim3(RA_THREADS), RA_WIN_LDS, stream, a);
  int rc = lc2is_check_launch();
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(ra_finish_kernel<8>, dim3((3 * K + 63) / 64, N), dim3(256), 0, stream, desc, (const int*)workspace, counts, K,
                     (int)n_tiles);
  return lc2is_check_launch();
}

extern "C" int lc2is_resize_argmax_multiscale(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                              const int64_t* canv, long n_canv, const int32_t* win, long n_win, long n_tiles,
                                              long total_px, const void* gt, int gt_bytes, int ignore_index, int mode,
                                              uint8_t* pred, int* counts, void* workspace, size_t workspace_bytes,
                                              lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!views || !desc || !canv || !win || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && (!gt || !workspace)) return LC2IS_ERR_NULL;
  if (N <= 0 || V <= 0 || h <= 0 || w <= 0 || K <= 0 || ld < K || ld % 4 || ((uintptr_t)views & 15) || ((uintptr_t)win & 15) ||
      n_canv <= 0 || n_win <= 0 || n_tiles <= 0 || n_tiles > 0x7fffffffL || total_px <= 0 || ignore_index < -1 ||
      (mode != LC2IS_MS_LOGIT && mode != LC2IS_MS_PROB))
    return LC2IS_ERR_SHAPE;
  if (K > RA_KMAX) return LC2IS_ERR_UNSUPPORTED;
  if (counts && gt_bytes != 1 && gt_bytes != 4 && gt_bytes != 8) return LC2IS_ERR_UNSUPPORTED;
  if (counts && workspace_bytes < lc2is_resize_argmax_workspace_bytes(n_tiles, K)) return LC2IS_ERR_WORKSPACE;
  RaMsArgs a;
  a.views = views; a.desc = desc; a.canv = canv; a.win = win; a.gt = counts ? gt : nullptr; a.pred = pred;
  a.slab = counts ? (int*)workspace : nullptr;
  a.total_px = total_px; a.n_canv = n_canv; a.n_win = n_win; a.N = N; a.V = V; a.h = h; a.w = w; a.ld = ld; a.K = K;
  a.n_tiles = (int)n_tiles; a.gt_bytes = gt_bytes; a.ignore_index = ignore_index;
  if (mode == LC2IS_MS_PROB) {
    static DevOnce attr_set;   // 70 KB of dynamic LDS: above the default limit
    if (attr_set.need()) {
      if (hipFuncSetAttribute((const void*)ra_ms_kernel<LC2IS_MS_PROB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)RA_MS_LDS_PROB) != hipSuccess)
        return LC2IS_ERR_LAUNCH;
      attr_set.done();
    }
    hipLaunchKernelGGL(ra_ms_kernel<LC2IS_MS_PROB>, dim3((unsigned)n_tiles), dim3(RA_THREADS), RA_MS_LDS_PROB, stream, a);
  } else {
    hipLaunchKernelGGL(ra_ms_kernel<LC2IS_MS_LOGIT>, dim3((unsigned)n_tiles), dim3(RA_THREADS), RA_MS_LDS_LOGIT, stream, a);
  }
  int rc = lc2is_check_launch();
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(ra_finish_kernel<6>, dim3((3 * K + 63) / 64, N), dim3(256), 0, stream, desc, (const int*)workspace, counts, K,
                     (int)n_tiles);
  return lc2is_check_launch();
}
