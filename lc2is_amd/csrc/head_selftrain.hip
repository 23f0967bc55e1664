// Self-training on the fused head (gfx950): the teacher's class map with its confidence and thresholded pseudo-labels, and the
// student's cross-entropy with a per-pixel weight.
// replaces: model(inputs)["outputs"].softmax(1).max(1) >= thresh on the materialised [B,K,H,W] fp32 logits (FixMatch / ST++ /
//   DAFormer pseudo-labelling; 158 MB per 512 x 512 image at K = 151), and F.cross_entropy(..., reduction='none') * pixel_weight
//   on the same logits (DAFormer's quality weight, mmseg's weight_reduce_loss, U-Net's boundary maps), plus its autograd.
//
// head_conf_grp_kernel is a forward-only sibling of head_argmax_grp_kernel (head_argmax.hip): head_grp_plan's tiles and grid, the
// footprint staging, the unit walk and the forward product Wm x lo on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), channels at or
// past C masked to -inf.  The class is taken exactly as there (in-lane walk over the tiles, strict >, then row16_argmax: ties to the
// lowest class, a NaN never wins, the index clamped into [0, C)), so pred is byte for byte ops.head_upsample_argmax's.  The
// confidence is the winner's softmax probability, conf = 1 / sum_c exp(z_c - max): the row maximum is the argmax's own value, the
// exponent is head_ce_grp_kernel's exp2(fma(z_c, log2(e), -max log2(e))) and the 16 lanes of a row are summed with row16_sum.  That
// fma leaves the winner's own term at exp2 of a rounding residual r instead of 1 — every term carries the factor exp2(r) — so the
// numerator is the winner's term as computed, top = exp2(fma(max, ...)), not 1: conf = top / sum.  The factor cancels, and a pixel
// with one dominant class has sum == top and reaches conf == 1 exactly (1 / sum would miss a threshold of 1).  sum >= top > 0
// whenever both are numbers; a pixel where they are not (all scores -inf, a NaN, a +inf score) gets the class head_upsample_argmax
// gives it (0 for all -inf) and conf = 1 / C, the confidence of knowing nothing: conf is always finite and in (0, 1].
// The 16 results of a unit go to two [16][16] tiles in LDS beside the labels' tile (which here only marks the pixels inside the
// image); after one barrier the first 256 threads own one pixel each and write what was asked for: pred (a byte), conf (fp32),
// pseudo (int64: the class where conf >= thresh, else ignore_index).  counts: waves 0-3 take a ballot + popcount of their 64 pixels
// {kept, inside}, the block's four pairs are added in wave order into its slab [2] of the workspace and head_conf_finish_kernel sums
// each image's slabs in a fixed order.  NO read-modify-write atomics, LDS included.
//
// head_ce_pw_grp_kernel is head_ce_grp_kernel<..., OPT = true> (head.hip) with one more input, pixel_weight fp32 [B,H,W], staged as
// a [16][16] tile behind the class weights.  Per counted pixel, a1 = 1 - eps, ac = eps / C, W = sum_c w_c:
//   loss_i  = pw_i [ a1 w_y (lse - z_y) + ac (W lse - sum_c w_c z_c) ],   count_i = w_y   (NOT multiplied by pw_i)
//   dz_k    = gscale pw_i [ (a1 w_y + ac W) p_k - a1 w_y [k == y] - ac w_k ]
// The count ignores the pixel weight: the denominator of 'mean' stays this project's sum of w_y over the counted pixels, so
// pixel_weight == 1 is the existing loss, and a per-image quality weight scales that image's loss (mmseg's weight_reduce_loss)
// instead of cancelling.  Weights must be finite and >= 0 (not checked on the device: no host sync).  Every product with pw_i is a
// plain multiply of a term the unweighted kernel forms, so pw == 2^-k gives exactly 2^-k times the sums and the gradient of pw == 1.
// The turns on the LDS mirror, the slabs, the block partials and head_finish_kernel (through lc2is_head_finish_launch, head.hip)
// are the cross-entropy kernel's: no float atomics, the loss and the gradient are bitwise reproducible.
#include "common.h"
#include "head_grp.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

constexpr int NHW = 4;          // waves that own pixels after the barrier (256 pixels, 64 each)

struct ConfArgs {
  const float* lo; int ld;       // [B, h, w, ld] scores, C valid channels
  uint8_t* pred;                 // [B, H, W] or null
  float* conf;                   // [B, H, W] or null
  int64_t* pseudo;               // [B, H, W] or null
  int* slab;                     // [blocks][2] per-tile {kept, inside} or null
  int B, h, w, H, W, C;
  float thresh;
  long ignore_index;
};

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_conf_grp_kernel(ConfArgs p) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int F4 = GM::F4, NQ = GM::NQ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_cnt[NHW][2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int CS = p.ld + HEAD_PAD;
  const HeadLds L = head_grp_lds(F4, p.ld, false);
  float* s_lo = (float*)smem;
  int* s_lab = (int*)(s_lo + L.lab);             // -2 outside the image, -1 inside (there are no labels)
  int* s_arg = (int*)(s_lo + L.tail);            // [16][16] class of the pixel (read only where s_lab is not -2)
  float* s_conf = (float*)(s_arg + HT * HT);     // [16][16] its confidence
  stage_footprint<MODE, S>(s_lo, nullptr, false, p.lo, p.ld, p.h, p.w, T, tid);
  stage_labels<true>(s_lab, nullptr, T, p.H, p.W, p.C, p.ignore_index, tid);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  const float unknown = 1.f / (float)p.C;
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    const HeadUnit U = head_unit<MODE, S>(T, g2, wid, kq, CS, p.H, p.W);
    if (!U.active) continue;   // no pixel of the unit is inside the image: nothing reads its part of the tiles
    float Af[NQ];
    make_fwd_operand<MODE, S>(Af, U.prow, m, kq);
    f32x4_t acc[TN];
    fwd_product(acc, s_lo + U.gbase + m, cell_off, Af);
    // in-lane: channels 16 t + m, t ascending, strict > (the lowest channel of equal scores stays)
    float best[4] = {NEG, NEG, NEG, NEG};
    int arg[4] = {m, m, m, m};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      mask_past_c(acc[t], t, m, p.C, NEG);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (acc[t][r] > best[r]) { best[r] = acc[t][r]; arg[r] = 16 * t + m; }
    }
    i32x4_t out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      row16_argmax(best[r], arg[r]);   // every lane of the row: the row's maximum and its class
      out[r] = arg[r] < 0 ? 0 : (arg[r] > p.C - 1 ? p.C - 1 : arg[r]);
    }
    // softmax relative to the maximum, the exponent formed as in head_ce_grp_kernel (one fma per element); top = the winner's own
    // term, which that fma leaves at exp2 of a rounding residual instead of 1: it is the numerator, so the residual cancels
    float mxl[4], top[4], sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mxl[r] = -best[r] * HEAD_LOG2E;
      top[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(best[r], HEAD_LOG2E, mxl[r]));
    }
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[r] += __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], HEAD_LOG2E, mxl[r]));
    f32x4_t cf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = row16_sum(sum[r]);   // >= top: the winner's term is one of the addends, the others are >= 0
      cf[r] = (top[r] > 0.f && s >= top[r]) ? fminf(top[r] / s, 1.f) : unknown;   // (a NaN fails the comparisons)
    }
    if (m == 0) {
      const int at = (S * U.gy + U.py4) * 16 + S * U.gx + U.px4;
      *reinterpret_cast<i32x4_t*>(s_arg + at) = out;
      *reinterpret_cast<f32x4_t*>(s_conf + at) = cf;
    }
  }
  __syncthreads();

  // the first 256 threads own one pixel each
  const bool inside = tid < HT * HT && s_lab[tid] != -2;
  const int cls = inside ? s_arg[tid] : 0;
  const float cf = inside ? s_conf[tid] : 0.f;
  const bool kept = inside && cf >= p.thresh;
  if (inside) {
    const size_t at = ((size_t)T.b * p.H + (T.Y0 + (tid >> 4))) * p.W + (T.X0 + (tid & 15));
    if (p.pred) p.pred[at] = (uint8_t)cls;
    if (p.conf) p.conf[at] = cf;
    if (p.pseudo) p.pseudo[at] = kept ? (int64_t)cls : (int64_t)p.ignore_index;
  }
  if (!p.slab) return;
  if (wid < NHW) {
    const int nk = __builtin_popcountll(__ballot(kept)), ni = __builtin_popcountll(__ballot(inside));
    if (lane == 0) { s_cnt[wid][0] = nk; s_cnt[wid][1] = ni; }
  }
  __syncthreads();
  if (tid < 2) p.slab[2 * (size_t)blockIdx.x + tid] = ((s_cnt[0][tid] + s_cnt[1][tid]) + s_cnt[2][tid]) + s_cnt[3][tid];
}

// counts[b][e] = sum over the image's tiles of slab[tile][e], tiles in increasing order within each of 64 strided parts, the parts
// added in order (the shape of head_argmax_finish_kernel): grid B, 128 threads (wave e sums entry e).
__global__ __launch_bounds__(128) void head_conf_finish_kernel(const int* __restrict__ slab, int* __restrict__ counts, int t4) {
  __shared__ int part[2][64];
  const int b = blockIdx.x, e = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int* src = slab + (size_t)b * t4 * 2 + e;
  int s = 0;
  for (int i = lane; i < t4; i += 64) s += src[(size_t)i * 2];
  part[e][lane] = s;
  __syncthreads();
  if (lane == 0) {
    int tot = 0;
    for (int i = 0; i < 64; ++i) tot += part[e][i];
    counts[2 * (size_t)b + e] = tot;
  }
}

// the blocks' count slabs [blocks][2] on head_grp_plan's tiles
size_t conf_slab_bytes(const HeadGrpPlan& g, int B) { return (size_t)B * g.t4 * 2 * sizeof(int); }

// ---- cross-entropy with a per-pixel weight ----
struct CePwArgs {
  const float* lo; int ld;       // [B, h, w, ld] scores, C valid channels
  const int64_t* labels;         // [B, H, W]
  const float* pw;               // [B, H, W] pixel weights, finite and >= 0
  float* ws_loss;                // [blocks][2] loss / count partials
  float* ws_dlo;                 // [blocks][F4 * F4][cq] footprint mirrors, or null (loss only)
  int B, h, w, H, W, C, cq;
  long ignore_index;
  float gscale;
  const float* cw;               // [C] class weights (device) or null = all ones
  float eps;                     // label smoothing in [0, 1]
};

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_ce_pw_grp_kernel(CePwArgs p) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, F4 = GM::F4, NQ = GM::NQ;
  constexpr bool SUMD = GM::SUMD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int CS = p.ld + HEAD_PAD;
  const HeadLds L = head_grp_lds(F4, p.ld, true);
  const bool grad = p.ws_dlo != nullptr;
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + L.dlo;
  int* s_lab = (int*)(s_lo + L.lab);
  float* s_w = s_lo + L.tail;                    // [CMAX] class weights, zero past C
  float* s_pw = s_w + CMAX;                      // [16][16] pixel weights (read only where s_lab >= 0)
  stage_footprint<MODE, S>(s_lo, s_dlo, grad, p.lo, p.ld, p.h, p.w, T, tid);
  if (tid < HT * HT) {
    stage_label<false>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
    const int Y = T.Y0 + (tid >> 4), X = T.X0 + (tid & 15);
    s_pw[tid] = (Y >= 0 && X >= 0 && Y < p.H && X < p.W) ? p.pw[((size_t)T.b * p.H + Y) * p.W + X] : 0.f;
  }
  stage_weights(s_w, p.cw, p.C, tid);
  __syncthreads();
  const float a1 = 1.f - p.eps, ac = p.eps / (float)p.C;
  const float aw = ac * wave_sum(s_w[lane] + s_w[lane + 64] + s_w[lane + 128]);

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  const int cellm_off = make_cellm_off<MODE, S>(m, kq, CS);
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);
  // forward A: row = pixel m of the unit, k = kq -> cell 4q + kq.  Backward B of product jj: column = cell m, k = kq -> pixel 4 kq + jj
  float Af[NQ], Bb[4];
  auto make_operands = [&](int prow) {
    make_fwd_operand<MODE, S>(Af, prow, m, kq);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int n = 4 * kq + jj;
      Bb[jj] = (m < NT * NT) ? tap_w<MODE, S>(prow + n / S, m / NT) * tap_w<MODE, S>(n % S, m % NT) : 0.f;
    }
  };
  if constexpr (!SUMD) make_operands(0);
  float loss_acc = 0.f, cnt_acc = 0.f;
  f32x4_t dsum[SUMD ? TN : 1];
  if constexpr (SUMD) {
#pragma unroll
    for (int t = 0; t < TN; ++t) dsum[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  bool have_d = false;
  int gbase = 0;

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    const HeadUnit U = head_unit<MODE, S>(T, g2, wid, kq, CS, p.H, p.W);
    gbase = U.gbase;
    f32x4_t acc[TN];   // logits, then exp, then (S = 4: in place) the transposed gradient tiles
    if constexpr (!SUMD) have_d = false;
    if (U.active) {
      if constexpr (SUMD) make_operands(U.prow);
      fwd_product(acc, s_lo + gbase + m, cell_off, Af);
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int at4 = (S * U.gy + U.py4) * 16 + S * U.gx + U.px4;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + at4);
      const f32x4_t pw4 = *reinterpret_cast<const f32x4_t*>(s_pw + at4);
      {
        // the label's logit: this lane owns pixel m x cells {4q + kq}
        const int atm = (S * U.gy + U.prow + m / S) * 16 + S * U.gx + m % S;
        const int lab_m = s_lab[atm];
        if (lab_m >= 0) {
          float zl = 0.f;
#pragma unroll
          for (int q = 0; q < NQ; ++q) zl += Af[q] * s_lo[gbase + cell_off[q] + lab_m];
          loss_acc -= s_pw[atm] * (a1 * s_w[lab_m] * zl);
        }
      }
      // softmax over the channels of four pixels at once
      float mx[4] = {NEG, NEG, NEG, NEG}, sum[4] = {0.f, 0.f, 0.f, 0.f};
      float wz[4] = {0.f, 0.f, 0.f, 0.f};   // sum_c w_c z_c
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        mask_past_c(acc[t], t, m, p.C, NEG);
        const float wk = s_w[16 * t + m];   // 0 past C (and there the logit is -inf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          wz[r] += wk != 0.f ? wk * acc[t][r] : 0.f;
          mx[r] = fmaxf(mx[r], acc[t][r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // the smoothing's -(eps/C) sum_c w_c z_c, before exp overwrites the logits
        wz[r] = row16_sum(wz[r]);
        if (lab4[r] >= 0 && m == 0) loss_acc -= pw4[r] * (ac * wz[r]);
      }
      float mxl[4];
      row_max_mxl(mx, mxl);
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], HEAD_LOG2E, mxl[r]));
          acc[t][r] = e;
          sum[r] += e;
        }
      float inv[4], oh[4], pg[4];   // gradient coefficients of the softmax, the one-hot and the smoothing term, each times gscale pw
      int dl[4];                    // label - lane's channel offset: the one-hot sits in tile t where dl == 16 t
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sum[r] = row16_sum(sum[r]);
        const bool counted = lab4[r] >= 0;
        const float wy = counted ? s_w[counted ? lab4[r] : 0] : 0.f;
        const float cy = a1 * wy, cs = cy + aw;
        pg[r] = counted ? p.gscale * pw4[r] : 0.f;
        inv[r] = counted ? pg[r] * cs / sum[r] : 0.f;
        oh[r] = pg[r] * cy;
        dl[r] = counted ? lab4[r] - m : -1;
        if (counted && m == 0) {
          loss_acc += pw4[r] * (cs * (mx[r] + __logf(sum[r])));
          cnt_acc += wy;
        }
      }
      if (grad) {
        have_d = true;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const float sk = ac * s_w[16 * t + m];   // smoothing term of channel 16 t + m
          f32x4_t gv;
#pragma unroll
          for (int r = 0; r < 4; ++r) gv[r] = acc[t][r] * inv[r] - (dl[r] == 16 * t ? oh[r] : 0.f) - sk * pg[r];
          bwd_product<SUMD>(gv, Bb, t, acc, dsum);
        }
      }
    }
    if (grad && (!SUMD || g2 == 1)) {
      // the waves' turns on the mirror (head_grp.h)
      constexpr int NTURN = (S == 4 && MODE != LC2IS_INTERP_BICUBIC) ? 2 : HEAD_THREADS / 64;
      const int my_turn = (S == 4 && MODE != LC2IS_INTERP_BICUBIC) ? ((wid >> 1) & 1) : wid;
      for (int turn = 0; turn < NTURN; ++turn) {
        __syncthreads();
        if (turn == my_turn && have_d && m < NT * NT) {
          float* dp = s_dlo + gbase + cellm_off;
#pragma unroll
          for (int t = 0; t < TN; ++t) {
            f32x4_t v = *reinterpret_cast<f32x4_t*>(dp + 16 * t);
            if constexpr (SUMD) v += dsum[t]; else v += acc[t];
            *reinterpret_cast<f32x4_t*>(dp + 16 * t) = v;
          }
        }
      }
    }
  }

  // the block's [loss, count] partial and its slab: plain stores, summed in a fixed order by head_finish_kernel
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
  if (grad) store_slab<MODE, S>(s_dlo, p.ws_dlo, p.cq, CS, tid);
}

constexpr int LDS_TAIL_PW = CMAX + HT * HT;   // [CMAX] class weights, [16][16] pixel weights

}  // namespace

extern "C" size_t lc2is_head_upsample_conf_workspace_bytes(int B, int h, int w, int C, int S, int mode) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || !(S == 4 || S == 8 || S == 16)) return 0;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return 0;
  return conf_slab_bytes(head_grp_plan(B, h, w, C, S, mode, false), B);
}

extern "C" int lc2is_head_upsample_conf(const float* scores_lo, int ld, uint8_t* pred, float* conf, int64_t* pseudo,
                                        int32_t* counts, int B, int h, int w, int C, int S, int mode, float thresh,
                                        long ignore_index, void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || (!pred && !conf && !pseudo && !counts)) return LC2IS_ERR_NULL;
  if (int rc = head_grp_check(scores_lo, nullptr, thresh >= 0.f && thresh <= 1.f, B, h, w, C, ld, S, mode)) return rc;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, false);
  if (counts && !head_ws_ok(workspace, workspace_bytes, conf_slab_bytes(gp, B))) return LC2IS_ERR_WORKSPACE;
  ConfArgs a{scores_lo, ld, pred, conf, pseudo, counts ? (int*)workspace : nullptr, B, h, w, h * S, w * S, C, thresh, ignore_index};
  // the footprint, the inside / outside tile, and behind it the class tile and the confidence tile
  const int lds = head_grp_lds(gp.f4, ld, false).bytes(2 * HT * HT);
  const int rc = head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_conf_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(false, 2 * HT * HT), B * gp.t4, lds, stream, a);
  });
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(head_conf_finish_kernel, dim3(B), dim3(128), 0, stream, (const int*)workspace, counts, gp.t4);
  return lc2is_check_launch();
}

extern "C" int lc2is_head_upsample_ce_pw(const float* scores_lo, int ld, const int64_t* labels, const float* pixel_weight,
                                         float* dscores_lo, float* loss_sum, int B, int h, int w, int C, int S, int mode,
                                         long ignore_index, float grad_scale, const float* class_weight, float label_smoothing,
                                         void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !labels || !pixel_weight || !loss_sum) return LC2IS_ERR_NULL;
  if (int rc = head_grp_check(scores_lo, dscores_lo, label_smoothing >= 0.f && label_smoothing <= 1.f && grad_scale == grad_scale,
                              B, h, w, C, ld, S, mode))
    return rc;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!head_ws_ok(workspace, workspace_bytes, gp.loss_bytes + gp.dlo_bytes)) return LC2IS_ERR_WORKSPACE;
  float* ws_loss = (float*)workspace;
  float* ws_dlo = dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr;
  CePwArgs a{scores_lo, ld, labels, pixel_weight, ws_loss, ws_dlo, B, h, w, h * S, w * S, C, gp.cq, ignore_index, grad_scale,
             class_weight, label_smoothing};
  const int lds = head_grp_lds(gp.f4, ld, true).bytes(LDS_TAIL_PW);
  const int rc = head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_ce_pw_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(true, LDS_TAIL_PW), B * gp.t4, lds, stream, a);
  });
  if (rc) return rc;
  return lc2is_head_finish_launch(HeadFinishArgs{dscores_lo, loss_sum, ws_loss, ws_dlo, B, h, w, C, ld, S, mode, gp.cq, B * gp.t4},
                                  stream);
}
