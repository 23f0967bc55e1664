// The fused head past 192 classes (gfx950): x4 upsample + softmax cross-entropy, forward and backward, and the class map with its
// {intersection, predicted, labelled} counts, for C <= 1024 (PC-459, ADE20K-full's 847, ImageNet-S-919, a product vocabulary of a
// few hundred prompts).  replaces: what head.hip / head_argmax.hip replace, at class counts they refuse.
//
// head_ce_grp_kernel<MODE, 12, 4, OPT> (head.hip) keeps all 12 channel tiles of a pixel unit in MFMA accumulators and the whole
// footprint and its gradient mirror in LDS: 192 classes is what fits.  The kernels here keep its tile plan (16 x 16 output tiles
// shifted by 2 pixels, 4 x 4-pixel groups, one 16-pixel unit per group, two units per wave), its forward product Wm x lo and backward
// product dlogits^T x Wm on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), its turns on the LDS mirror, its per-block slabs and
// partials and a finish launch of the same summation order — and walk the class axis in CHUNKS of 192 channels, of which only one is
// in LDS at a time.  A chunk is worked in groups of four channel tiles (64 channels, the granule of ld): a ragged last chunk stages
// and multiplies only the groups that hold a class (C = 256: 12 + 4 tiles, C = 847: 4 x 12 + 8).
//
// head_ce_wide_grp_kernel<MODE>, S = 4:
//   sweep 1, chunks ascending: stage the chunk's footprint, form the logits, and keep per pixel a running maximum M and a sum of
//     exp(z - M) rescaled whenever M grows (online softmax); the label's logit is picked up from the staged footprint in the chunk
//     that holds it (one (pixel, cell quad) per lane, as in the narrow kernel).  The running pair lives in LDS ([16][16] pixels, the
//     owner wave its only reader and writer); exponents are formed as (z - M) log2(e), the difference first: it is exact where it
//     matters, and an unchanged M rescales by exactly 1, so scores of +-1e4 cost no precision.
//   then loss_i = w_y (M + ln(sum) - z_y), count_i = w_y per counted pixel (F.cross_entropy's weight; ones without).
//   sweep 2, chunks ascending (only when a gradient is wanted): restage the chunk, recompute the logits,
//     dz_k = gscale w_y (exp(z_k - M) / sum - [k == y]), transposed gradient tiles, waves taking turns on the chunk's mirror, and the
//     mirror leaves as the chunk's columns of the block's slab.  Channels at or past C are -inf in the accumulators: gradient exactly 0.
//   head_finish_wide_kernel: head_finish_kernel's fixed-order sums (tile row, footprint row, tile column, footprint column), the
//     wave passing over the channel quads 64 at a time; every one of the ld channels is written, zeros at and past C.
// head_argmax_wide_grp_kernel<MODE>, S = 4: the same chunk walk with a running (value, class) per pixel; chunks ascend and a later
//   chunk wins only with a strictly larger value, so exact ties go to the lowest class (torch.argmax); the class is clamped into
//   [0, C); pred is int16.  Counts as head_argmax_grp_kernel: wave_hist into wave-private rows [4][3][cq] — 48 KB at the cap, which
//   take the footprint's place in LDS once the walk is over — block slab, fixed-order finish.
// No label smoothing here.  NO read-modify-write atomics, LDS included: the same bytes every run.
//
// Budget (512 threads, two blocks per CU = 128 VGPRs and 80 KB of LDS per block; measured by tools/check_kernel_resources.py, see
// profiles/wide_head_cost.txt): the cross-entropy kernel's LDS is 2 x 49 x 196 floats + four [16][16] tiles = 80 928 bytes (+ 64
// static) bicubic, 43 296 bilinear; the argmax kernel's is max(footprint, count rows) + three tiles <= 52 224 bytes.  Both compile
// inside 128 registers without scratch, so two blocks per CU hold for both.
// The interpolation weights and the 16-lane row steps are head_grp.h's; the chunked work split is this file's own.
#include "common.h"
#include "head_grp.h"   // HT, HEAD_THREADS, HEAD_PAD, tap_w and the 16-lane row steps
#include "interp.h"
#include "label_hist.h"
#include "lc2is_hip.h"

namespace {

constexpr int S = 4;            // the only scale of the wide head
constexpr int G = HT / S;       // groups per tile edge
constexpr int CHUNK = 192;      // channels of the class axis in LDS at a time
constexpr int TN = CHUNK / 16;  // channel tiles of a chunk
constexpr int NG = TN / 4;      // groups of four channel tiles (64 channels)
constexpr int CS = CHUNK + HEAD_PAD;   // cell stride in LDS (floats)
constexpr int WIDE_CMAX = LC2IS_HEAD_WIDE_CMAX;
constexpr int NHW = 4;          // waves that own pixels in the argmax kernel's count phase

struct WideArgs {
  const float* lo; int ld;       // [B, h, w, ld] scores, C valid channels
  const int64_t* labels;         // [B, H, W]
  float* dlo;                    // [B, h, w, ld] gradient (every channel written by the finish launch) or null
  float* loss_sum;               // [2]: sum_i w_y (lse - z_y), sum_i w_y
  int B, h, w, H, W, C;
  long ignore_index;
  float gscale;
  float* ws_loss;                // [blocks][2] partials
  float* ws_dlo;                 // [blocks][F4 * F4][cq] footprint mirrors
  int cq;                        // channels per slab cell: C rounded up to 4
  const float* cw;               // [C] class weights (device) or null = all ones
};

struct WideArgmaxArgs {
  const float* lo; int ld;
  const int64_t* labels;         // [B, H, W] or null (pred only)
  int16_t* pred;                 // [B, H, W] or null
  int* slab;                     // [blocks][3][cq] per-tile counts or null
  int B, h, w, H, W, C, cq;
  long ignore_index;
};

// channels [c0, c0 + 64 ng) of the tile's footprint into s_lo (cell stride CS); ZERO: the same columns of the mirror cleared
template <int MODE, bool ZERO>
__device__ __forceinline__ void stage_chunk(float* s_lo, float* s_dlo, const float* lo, int ld, int b, int h, int w, int a0, int b0,
                                            int c0, int ng, int tid) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int F4 = G + NT - 1;
  const int q4 = 16 * ng;   // float4 per cell
  for (int i = tid; i < F4 * F4 * q4; i += HEAD_THREADS) {
    const int cell = i / q4, c = (i - cell * q4) * 4;
    int ry = a0 - OFF + cell / F4, rx = b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > h - 1 ? h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > w - 1 ? w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(lo + (((size_t)b * h + ry) * w + rx) * ld + c0 + c);
    if constexpr (ZERO) *reinterpret_cast<float4*>(s_dlo + cell * CS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// logits of one unit over the chunk's first ng tile groups: acc[t][r] = channel c0 + 16 t + m of pixel 4 kq + r, -inf at and past C.
// bp = s_lo + the group's first cell + m.  Tiles of groups >= ng are left untouched (and unread by every caller).
template <int NQ>
__device__ __forceinline__ void chunk_logits(f32x4_t (&acc)[TN], const float* bp, const int (&cell_off)[NQ], const float (&Af)[NQ],
                                             int ng, int c0, int C, int m) {
#pragma unroll
  for (int t = 0; t < TN; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int tg = 0; tg < NG; ++tg) {
      if (tg < ng) {   // uniform
        float bv[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) bv[tt] = bp[cell_off[q] + 16 * (4 * tg + tt)];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
          acc[4 * tg + tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Af[q], bv[tt], acc[4 * tg + tt], 0, 0, 0);
      }
    }
  }
  const float NEG = -__builtin_inff();
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    if (c0 + 16 * t + 16 > C) {   // uniform: a tile with channels past C
      if (c0 + 16 * t + m >= C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(HEAD_THREADS, 2) void head_ce_wide_grp_kernel(WideArgs p) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;   // taps per axis
  constexpr int F4 = G + NT - 1;                               // footprint edge
  constexpr int NQ = NT * NT / 4;                              // k = 4 chunks of the forward product
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_x = (p.W + S / 2 + HT - 1) / HT, tiles_y = (p.H + S / 2 + HT - 1) / HT;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int tyi = (blockIdx.x / tiles_x) % tiles_y, txi = blockIdx.x % tiles_x;
  const int a0 = G * tyi - 1, b0 = G * txi - 1;  // "floor" lo index of the tile's first group row / column
  const int Y0 = S * a0 + S / 2, X0 = S * b0 + S / 2;   // the tile's first output pixel
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_wy = (float*)(s_lab + HT * HT);       // [16][16] the label's class weight, 0 where the pixel is not counted
  float* s_mx = s_wy + HT * HT;                  // [16][16] running maximum
  float* s_sum = s_mx + HT * HT;                 // [16][16] running sum of exp(z - maximum)
  if (tid < HT * HT) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    int code = -2;
    if (Y >= 0 && X >= 0 && Y < p.H && X < p.W) {
      code = -1;
      const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
      if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
    }
    s_lab[tid] = code;
    s_wy[tid] = code >= 0 ? (p.cw ? p.cw[code] : 1.f) : 0.f;
    s_mx[tid] = -__builtin_inff();
    s_sum[tid] = 0.f;
  }

  const int m = lane & 15, kq = lane >> 4;
  constexpr float LOG2E = 1.4426950408889634f;
  const int cellm_off = ((m / NT) * F4 + m % NT) * CS + 4 * kq;   // this lane's cell / channel quad in the transposed gradient tile
  int cell_off[NQ];   // LDS float offset of the forward cell 4q + kq, relative to the group's first cell
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  // forward A: row = pixel m of the unit, k = kq -> cell 4q + kq.  Backward B of product jj: column = cell m, k = kq -> pixel 4 kq + jj
  float Af[NQ], Bb[4];
  {
    const int py_m = m / S, px_m = m % S;
#pragma unroll
    for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % NT);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int n = 4 * kq + jj;
      Bb[jj] = (m < NT * NT) ? tap_w<MODE, S>(n / S, m / NT) * tap_w<MODE, S>(n % S, m % NT) : 0.f;
    }
  }
  float loss_acc = 0.f, cnt_acc = 0.f;
  const int nch = (p.C + CHUNK - 1) / CHUNK;

  // ---- sweep 1: running maximum, rescaled sum, the label's logit ----
#pragma unroll 1
  for (int ch = 0; ch < nch; ++ch) {
    const int c0 = ch * CHUNK;
    const int ng = (min(p.C - c0, CHUNK) + 63) >> 6;
    if (ch) __syncthreads();   // the previous chunk's readers are done
    stage_chunk<MODE, false>(s_lo, s_dlo, p.lo, p.ld, b, p.h, p.w, a0, b0, c0, ng, tid);
    __syncthreads();
#pragma unroll 1
    for (int g2 = 0; g2 < 2; ++g2) {
      const int gi = 2 * wid + g2, gy = gi / G, gx = gi % G;
      const int Yb = Y0 + S * gy, Xb = X0 + S * gx;   // the group's first output pixel
      const bool active = !(Yb >= p.H || Xb >= p.W || Yb + S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
      if (!active) continue;
      const int gbase = (gy * F4 + gx) * CS;
      f32x4_t acc[TN];
      chunk_logits<NQ>(acc, s_lo + gbase + m, cell_off, Af, ng, c0, p.C, m);
      // the label's logit: this lane owns pixel m x cells {4q + kq}
      const int pix_m = (S * gy + m / S) * 16 + S * gx + m % S;
      const int lab_m = s_lab[pix_m] - c0;
      if (lab_m >= 0 && lab_m < CHUNK) {
        float zl = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) zl += Af[q] * s_lo[gbase + cell_off[q] + lab_m];
        loss_acc -= s_wy[pix_m] * zl;
      }
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int pix4 = (S * gy + kq) * 16 + S * gx;
      const f32x4_t om = *reinterpret_cast<const f32x4_t*>(s_mx + pix4);
      const f32x4_t os = *reinterpret_cast<const f32x4_t*>(s_sum + pix4);
      float mx[4], sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[r] = om[r];
#pragma unroll
      for (int tg = 0; tg < NG; ++tg) {
        if (tg < ng) {
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], acc[4 * tg + tt][r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[r] = fmaxf(row16_max(mx[r]), -3.0e38f);   // finite: a row of -inf scores makes no NaN
#pragma unroll
      for (int tg = 0; tg < NG; ++tg) {
        if (tg < ng) {
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[r] += __builtin_amdgcn_exp2f((acc[4 * tg + tt][r] - mx[r]) * LOG2E);
        }
      }
      f32x4_t nm, ns;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        nm[r] = mx[r];
        ns[r] = os[r] * __builtin_amdgcn_exp2f((om[r] - mx[r]) * LOG2E) + row16_sum(sum[r]);
      }
      if (m == 0) {
        *reinterpret_cast<f32x4_t*>(s_mx + pix4) = nm;
        *reinterpret_cast<f32x4_t*>(s_sum + pix4) = ns;
      }
    }
  }
  __syncthreads();
  // ---- loss and count: one pixel per thread of the first four waves ----
  if (tid < HT * HT && s_lab[tid] >= 0) {
    const float wy = s_wy[tid];
    loss_acc += wy * (s_mx[tid] + __logf(s_sum[tid]));
    cnt_acc += wy;
  }

  // ---- sweep 2: the gradient, chunk by chunk ----
  if (p.dlo) {
    const int q4 = p.cq >> 2;
    float* slab = p.ws_dlo + (size_t)blockIdx.x * (F4 * F4) * p.cq;
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
      const int c0 = ch * CHUNK;
      const int ng = (min(p.C - c0, CHUNK) + 63) >> 6;
      __syncthreads();   // the previous chunk's mirror has left
      stage_chunk<MODE, true>(s_lo, s_dlo, p.lo, p.ld, b, p.h, p.w, a0, b0, c0, ng, tid);
      __syncthreads();
#pragma unroll 1
      for (int g2 = 0; g2 < 2; ++g2) {
        const int gi = 2 * wid + g2, gy = gi / G, gx = gi % G;
        const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
        const bool active = !(Yb >= p.H || Xb >= p.W || Yb + S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
        const int gbase = (gy * F4 + gx) * CS;
        f32x4_t acc[TN];   // logits, then in place the transposed gradient tiles
        if (active) {
          chunk_logits<NQ>(acc, s_lo + gbase + m, cell_off, Af, ng, c0, p.C, m);
          const int pix4 = (S * gy + kq) * 16 + S * gx;
          const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + pix4);
          const f32x4_t wy4 = *reinterpret_cast<const f32x4_t*>(s_wy + pix4);
          const f32x4_t mx4 = *reinterpret_cast<const f32x4_t*>(s_mx + pix4);
          const f32x4_t sm4 = *reinterpret_cast<const f32x4_t*>(s_sum + pix4);
          float inv[4], oh[4];
          int dl[4];   // label - chunk - lane's channel offset: the one-hot sits in tile t where dl == 16 t
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool counted = lab4[r] >= 0;
            oh[r] = p.gscale * wy4[r];
            inv[r] = counted ? oh[r] / sm4[r] : 0.f;
            dl[r] = counted ? lab4[r] - c0 - m : -1;
          }
#pragma unroll
          for (int tg = 0; tg < NG; ++tg) {
            if (tg < ng) {
#pragma unroll
              for (int tt = 0; tt < 4; ++tt) {
                const int t = 4 * tg + tt;
                f32x4_t gv;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  gv[r] = __builtin_amdgcn_exp2f((acc[t][r] - mx4[r]) * LOG2E) * inv[r] - (dl[r] == 16 * t ? oh[r] : 0.f);
                f32x4_t d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) d = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[jj], Bb[jj], d, 0, 0, 0);
                acc[t] = d;   // d[r] = channel c0 + 16 t + 4 kq + r of cell m
              }
            }
          }
        }
        // the waves take turns on the mirror (head_ce_grp_kernel): plain 16-byte read-add-write, one cell per lane.  Bilinear
        // footprints are 2 x 2 cells: the groups a pass runs on waves of equal (wid >> 1) & 1 sit two cells apart, two turns do.
        constexpr int NTURN = (MODE != LC2IS_INTERP_BICUBIC) ? 2 : HEAD_THREADS / 64;
        const int my_turn = (MODE != LC2IS_INTERP_BICUBIC) ? ((wid >> 1) & 1) : wid;
        for (int turn = 0; turn < NTURN; ++turn) {
          __syncthreads();
          if (turn == my_turn && active && m < NT * NT) {
            float* dp = s_dlo + gbase + cellm_off;
#pragma unroll
            for (int tg = 0; tg < NG; ++tg) {
              if (tg < ng) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                  f32x4_t v = *reinterpret_cast<f32x4_t*>(dp + 16 * (4 * tg + tt));
                  v += acc[4 * tg + tt];
                  *reinterpret_cast<f32x4_t*>(dp + 16 * (4 * tg + tt)) = v;
                }
              }
            }
          }
        }
      }
      __syncthreads();
      // the chunk's columns of the block's slab: cells in footprint order, cq channels each, 16 bytes per lane
      const int n4 = min(16 * ng, q4 - (c0 >> 2));
      for (int i = tid; i < F4 * F4 * n4; i += HEAD_THREADS) {
        const int cell = i / n4, c = (i - cell * n4) * 4;
        *reinterpret_cast<float4*>(slab + (size_t)cell * p.cq + c0 + c) = *reinterpret_cast<const float4*>(s_dlo + cell * CS + c);
      }
    }
  }

  __shared__ float s_red[HEAD_THREADS / 64][2];
  loss_acc = wave_sum(loss_acc);
  cnt_acc = wave_sum(cnt_acc);
  if (lane == 0) { s_red[wid][0] = loss_acc; s_red[wid][1] = cnt_acc; }
  __syncthreads();
  if (tid == 0) {
    float l = 0.f, c = 0.f;
#pragma unroll
    for (int w = 0; w < HEAD_THREADS / 64; ++w) { l += s_red[w][0]; c += s_red[w][1]; }
    p.ws_loss[2 * (size_t)blockIdx.x] = l;
    p.ws_loss[2 * (size_t)blockIdx.x + 1] = c;
  }
}

// dlo[b, y, x, :] = sum of the footprint cells that map to low-res cell (y, x), over the tiles that cover it, in head_finish_kernel's
// order (tile row, footprint row, tile column, footprint column); loss_sum = sum of the blocks' partials in block order.  One wave
// per low-res cell, four cells per block; the wave passes over the ld / 4 channel quads 64 at a time.
template <int MODE>
__global__ __launch_bounds__(256) void head_finish_wide_kernel(WideArgs p, int nblk_main) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int F4 = G + NT - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && wave == 0) {
    float l = 0.f, c = 0.f;
    for (int k = lane; k < nblk_main; k += 64) { l += p.ws_loss[2 * (size_t)k]; c += p.ws_loss[2 * (size_t)k + 1]; }
    l = wave_sum(l);
    c = wave_sum(c);
    if (lane == 0) { p.loss_sum[0] = l; p.loss_sum[1] = c; }
  }
  if (!p.dlo) return;
  const long ncell = (long)p.B * p.h * p.w;
  const long cid = (long)blockIdx.x * 4 + wave;
  if (cid >= ncell) return;
  const int x = (int)(cid % p.w), y = (int)((cid / p.w) % p.h), b = (int)(cid / ((long)p.w * p.h));
  const int tiles_x = (p.W + S / 2 + HT - 1) / HT, tiles_y = (p.H + S / 2 + HT - 1) / HT;
  auto floordiv = [](int a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); };
  const int ty_lo = max(0, floordiv(y + 1 + OFF - (F4 - 1), G)), ty_hi = (y == p.h - 1) ? tiles_y - 1 : min(tiles_y - 1, (y + 1 + OFF) / G);
  const int tx_lo = max(0, floordiv(x + 1 + OFF - (F4 - 1), G)), tx_hi = (x == p.w - 1) ? tiles_x - 1 : min(tiles_x - 1, (x + 1 + OFF) / G);
  const int q4 = p.cq >> 2;
  for (int cb = 0; 4 * cb < p.ld; cb += 64) {
    const int cl = cb + lane;   // this lane's channel quad
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cl < q4) {
      for (int ty = ty_lo; ty <= ty_hi; ++ty) {
        const int by = G * ty - 1 - OFF;
        const int fy_lo = max(0, y == 0 ? 0 : y - by), fy_hi = min(F4 - 1, y == p.h - 1 ? F4 - 1 : y - by);
        for (int fy = fy_lo; fy <= fy_hi; ++fy)
          for (int tx = tx_lo; tx <= tx_hi; ++tx) {
            const int bx = G * tx - 1 - OFF;
            const int fx_lo = max(0, x == 0 ? 0 : x - bx), fx_hi = min(F4 - 1, x == p.w - 1 ? F4 - 1 : x - bx);
            const float* slab = p.ws_dlo + (((size_t)b * tiles_y + ty) * tiles_x + tx) * (F4 * F4) * p.cq;
            for (int fx = fx_lo; fx <= fx_hi; ++fx) {
              const float4 v = *reinterpret_cast<const float4*>(slab + (size_t)(fy * F4 + fx) * p.cq + 4 * cl);
              acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
          }
      }
    }
    if (4 * cl < p.ld) {   // every channel of the row is written (zeros at and past C): the caller need not clear the buffer
      float* o = p.dlo + (((size_t)b * p.h + y) * p.w + x) * p.ld + 4 * cl;
      if (4 * cl + 0 >= p.C) acc.x = 0.f;
      if (4 * cl + 1 >= p.C) acc.y = 0.f;
      if (4 * cl + 2 >= p.C) acc.z = 0.f;
      if (4 * cl + 3 >= p.C) acc.w = 0.f;
      *reinterpret_cast<float4*>(o) = acc;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(HEAD_THREADS, 2) void head_argmax_wide_grp_kernel(WideArgmaxArgs p, int lo_floats) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int F4 = G + NT - 1;
  constexpr int NQ = NT * NT / 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_x = (p.W + S / 2 + HT - 1) / HT, tiles_y = (p.H + S / 2 + HT - 1) / HT;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int tyi = (blockIdx.x / tiles_x) % tiles_y, txi = blockIdx.x % tiles_x;
  const int a0 = G * tyi - 1, b0 = G * txi - 1;
  const int Y0 = S * a0 + S / 2, X0 = S * b0 + S / 2;
  float* s_lo = (float*)smem;                    // the chunk's footprint; after the walk the count rows [NHW][3][cq] take its place
  int* s_hist = (int*)smem;
  int* s_lab = (int*)(s_lo + lo_floats);         // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  int* s_arg = s_lab + HT * HT;                  // [16][16] running class
  float* s_best = (float*)(s_arg + HT * HT);     // [16][16] running value
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
    s_arg[tid] = 0;
    s_best[tid] = -__builtin_inff();
  }

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  int cell_off[NQ];
  float Af[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
    Af[q] = tap_w<MODE, S>(m / S, (4 * q + kq) / NT) * tap_w<MODE, S>(m % S, (4 * q + kq) % NT);
  }
  const int nch = (p.C + CHUNK - 1) / CHUNK;
#pragma unroll 1
  for (int ch = 0; ch < nch; ++ch) {
    const int c0 = ch * CHUNK;
    const int ng = (min(p.C - c0, CHUNK) + 63) >> 6;
    if (ch) __syncthreads();
    stage_chunk<MODE, false>(s_lo, nullptr, p.lo, p.ld, b, p.h, p.w, a0, b0, c0, ng, tid);
    __syncthreads();
#pragma unroll 1
    for (int g2 = 0; g2 < 2; ++g2) {
      const int gi = 2 * wid + g2, gy = gi / G, gx = gi % G;
      const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
      const bool active = !(Yb >= p.H || Xb >= p.W || Yb + S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
      if (!active) continue;   // no pixel of the unit is inside the image: nothing reads its part of s_arg
      const int gbase = (gy * F4 + gx) * CS;
      f32x4_t acc[TN];
      chunk_logits<NQ>(acc, s_lo + gbase + m, cell_off, Af, ng, c0, p.C, m);
      // in-lane: channels c0 + 16 t + m, t ascending, strict > (the lowest channel of equal scores stays)
      float best[4] = {NEG, NEG, NEG, NEG};
      int arg[4] = {c0 + m, c0 + m, c0 + m, c0 + m};
#pragma unroll
      for (int tg = 0; tg < NG; ++tg) {
        if (tg < ng) {
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (acc[4 * tg + tt][r] > best[r]) { best[r] = acc[4 * tg + tt][r]; arg[r] = c0 + 16 * (4 * tg + tt) + m; }
        }
      }
      const int pix4 = (S * gy + kq) * 16 + S * gx;
      f32x4_t bv = *reinterpret_cast<const f32x4_t*>(s_best + pix4);
      i32x4_t ba = *reinterpret_cast<const i32x4_t*>(s_arg + pix4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        row16_argmax(best[r], arg[r]);
        if (best[r] > bv[r]) { bv[r] = best[r]; ba[r] = arg[r]; }   // a later chunk wins only with a strictly larger value
      }
      if (m == 0) {
        *reinterpret_cast<f32x4_t*>(s_best + pix4) = bv;
        *reinterpret_cast<i32x4_t*>(s_arg + pix4) = ba;
      }
    }
  }
  __syncthreads();   // the walk is over: s_lo is free

  // the first 256 threads own one pixel each; the other waves only help with the block's sum
  const int code = tid < HT * HT ? s_lab[tid] : -2;
  const bool inside = code != -2;
  int cls = inside ? s_arg[tid] : 0;
  cls = cls < 0 ? 0 : (cls > p.C - 1 ? p.C - 1 : cls);
  if (inside && p.pred) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    p.pred[((size_t)b * p.H + Y) * p.W + X] = (int16_t)cls;
  }
  if (!p.slab) return;
  if (wid < NHW) {
    int* hw = s_hist + wid * 3 * p.cq;   // this wave's {intersection, predicted, labelled}, which no other wave writes
    for (int i = lane; i < 3 * p.cq; i += 64) hw[i] = 0;
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

// counts[b][e] = sum over the image's tiles of slab[tile][e]: head_argmax_finish_kernel's order (tiles in increasing order within
// each of 4 strided parts, the parts added in order): grid (ceil(3C / 64), B), 256 threads.  Slab rows are cq wide, counts rows C.
__global__ __launch_bounds__(256) void head_argmax_finish_wide_kernel(const int* __restrict__ slab, int* __restrict__ counts, int C,
                                                                      int cq, int t4) {
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

// head_grp_plan's tile count and slab cell width (head.hip), S = 4
struct WidePlan { int f4, t4, cq; size_t loss_bytes, dlo_bytes, cnt_bytes; };
WidePlan wide_plan(int B, int h, int w, int C, int mode, bool want_grad) {
  WidePlan g;
  g.f4 = G + (mode == LC2IS_INTERP_BICUBIC ? 4 : 2) - 1;
  const int H = h * S, W = w * S;
  g.t4 = ((H + S / 2 + HT - 1) / HT) * ((W + S / 2 + HT - 1) / HT);
  g.cq = (C + 3) & ~3;
  g.loss_bytes = ((size_t)B * g.t4 * 2 * sizeof(float) + 255) & ~(size_t)255;
  g.dlo_bytes = want_grad ? (size_t)B * g.t4 * g.f4 * g.f4 * g.cq * sizeof(float) : 0;
  g.cnt_bytes = (size_t)B * g.t4 * 3 * g.cq * sizeof(int);
  return g;
}

bool wide_shape_ok(int B, int h, int w, int C, int ld) {
  return B > 0 && h > 0 && w > 0 && C > 0 && C <= WIDE_CMAX && ld >= C && ld <= WIDE_CMAX && ld % 64 == 0;
}
bool wide_mode_ok(int S_, int mode) { return S_ == S && (mode == LC2IS_INTERP_BICUBIC || mode == LC2IS_INTERP_BILINEAR); }

}  // namespace

extern "C" size_t lc2is_head_upsample_ce_wide_workspace_bytes(int B, int h, int w, int C, int ld, int S_, int mode, int want_grad) {
  if (!wide_shape_ok(B, h, w, C, ld) || !wide_mode_ok(S_, mode)) return 0;
  const WidePlan g = wide_plan(B, h, w, C, mode, want_grad != 0);
  return g.loss_bytes + g.dlo_bytes;
}

extern "C" int lc2is_head_upsample_ce_wide(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_sum,
                                           int B, int h, int w, int C, int S_, int mode, long ignore_index, float grad_scale,
                                           const float* class_weight, void* workspace, size_t workspace_bytes,
                                           lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !labels || !loss_sum) return LC2IS_ERR_NULL;
  if (!wide_shape_ok(B, h, w, C, ld)) return LC2IS_ERR_SHAPE;
  if (((size_t)scores_lo | (size_t)dscores_lo) & 15) return LC2IS_ERR_SHAPE;
  if (!wide_mode_ok(S_, mode)) return LC2IS_ERR_UNSUPPORTED;
  const WidePlan gp = wide_plan(B, h, w, C, mode, dscores_lo != nullptr);
  if (!workspace || ((size_t)workspace & 15) || workspace_bytes < gp.loss_bytes + gp.dlo_bytes) return LC2IS_ERR_WORKSPACE;
  WideArgs a{scores_lo, ld, labels, dscores_lo, loss_sum, B, h, w, h * S, w * S, C, ignore_index, grad_scale, (float*)workspace,
             dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr, gp.cq, class_weight};
  // the chunk's footprint, its gradient mirror, and four [16][16] tiles: labels, label weights, running maximum and sum
  const int lds = 2 * gp.f4 * gp.f4 * CS * (int)sizeof(float) + 4 * HT * HT * (int)sizeof(int);
  const long ncell = dscores_lo ? (long)B * h * w : 1;
  const int fgrid = (int)((ncell + 3) / 4);
#define LC2IS_WIDE_CE(MODE_)                                                                                                 \
  do {                                                                                                                      \
    static DevOnce attr;                                                                                                    \
    if (attr.need()) {                                                                                                      \
      if (hipFuncSetAttribute((const void*)head_ce_wide_grp_kernel<MODE_>, hipFuncAttributeMaxDynamicSharedMemorySize,      \
                              2 * 7 * 7 * CS * (int)sizeof(float) + 4 * HT * HT * (int)sizeof(int)) != hipSuccess)          \
        return LC2IS_ERR_LAUNCH;                                                                                            \
      attr.done();                                                                                                          \
    }                                                                                                                       \
    hipLaunchKernelGGL((head_ce_wide_grp_kernel<MODE_>), dim3(B * gp.t4), dim3(HEAD_THREADS), lds, stream, a);              \
    const int rc = lc2is_check_launch();                                                                                    \
    if (rc) return rc;                                                                                                      \
    hipLaunchKernelGGL((head_finish_wide_kernel<MODE_>), dim3(fgrid), dim3(256), 0, stream, a, B * gp.t4);                  \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_WIDE_CE(LC2IS_INTERP_BICUBIC);
  else LC2IS_WIDE_CE(LC2IS_INTERP_BILINEAR);
#undef LC2IS_WIDE_CE
  return lc2is_check_launch();
}

extern "C" size_t lc2is_head_upsample_argmax_wide_workspace_bytes(int B, int h, int w, int C, int S_, int mode) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > WIDE_CMAX || !wide_mode_ok(S_, mode)) return 0;
  return wide_plan(B, h, w, C, mode, false).cnt_bytes;
}

extern "C" int lc2is_head_upsample_argmax_wide(const float* scores_lo, int ld, const int64_t* labels, int16_t* pred, int32_t* counts,
                                               int B, int h, int w, int C, int S_, int mode, long ignore_index, void* workspace,
                                               size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && !labels) return LC2IS_ERR_NULL;
  if (!wide_shape_ok(B, h, w, C, ld)) return LC2IS_ERR_SHAPE;
  if ((size_t)scores_lo & 15) return LC2IS_ERR_SHAPE;
  if (!wide_mode_ok(S_, mode)) return LC2IS_ERR_UNSUPPORTED;
  const WidePlan gp = wide_plan(B, h, w, C, mode, false);
  if (counts && (!workspace || ((size_t)workspace & 15) || workspace_bytes < gp.cnt_bytes)) return LC2IS_ERR_WORKSPACE;
  WideArgmaxArgs a{scores_lo, ld, labels, pred, counts ? (int*)workspace : nullptr, B, h, w, h * S, w * S, C, gp.cq, ignore_index};
  // the chunk's footprint or, after the walk, the four waves' count rows in its place (whichever is larger), and three [16][16] tiles:
  // at most 4 * 3 * 1024 * 4 + 3072 = 52 224 bytes
  const int foot = gp.f4 * gp.f4 * CS, rows = counts ? NHW * 3 * gp.cq : 0;
  const int lo_floats = foot > rows ? foot : rows;
  const int lds = lo_floats * (int)sizeof(float) + 3 * HT * HT * (int)sizeof(int);
#define LC2IS_WIDE_AM(MODE_)                                                                                                 \
  do {                                                                                                                      \
    static DevOnce attr;                                                                                                    \
    if (attr.need()) {                                                                                                      \
      if (hipFuncSetAttribute((const void*)head_argmax_wide_grp_kernel<MODE_>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                              NHW * 3 * WIDE_CMAX * (int)sizeof(int) + 3 * HT * HT * (int)sizeof(int)) != hipSuccess)       \
        return LC2IS_ERR_LAUNCH;                                                                                            \
      attr.done();                                                                                                          \
    }                                                                                                                       \
    hipLaunchKernelGGL((head_argmax_wide_grp_kernel<MODE_>), dim3(B * gp.t4), dim3(HEAD_THREADS), lds, stream, a, lo_floats); \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_WIDE_AM(LC2IS_INTERP_BICUBIC);
  else LC2IS_WIDE_AM(LC2IS_INTERP_BILINEAR);
#undef LC2IS_WIDE_AM
  int rc = lc2is_check_launch();
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(head_argmax_finish_wide_kernel, dim3((3 * C + 63) / 64, B), dim3(256), 0, stream, (const int*)workspace, counts,
                     C, gp.cq, gp.t4);
  return lc2is_check_launch();
}
