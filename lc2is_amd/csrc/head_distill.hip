// Distillation on the fused head (gfx950): the per-pixel KL(teacher || student) of two upsampled low-resolution score maps and its
// gradient with respect to the student's, at a temperature.
// replaces: T*T * F.kl_div(F.log_softmax(student(inputs)["outputs"] / T, 1), F.softmax(teacher(inputs)["outputs"] / T, 1),
//   reduction='none').sum(1) on TWO materialised [B,K,H,W] fp32 logit maps (Hinton's KD as segmentation recipes apply it: mmrazor's
//   KLDivergence, the pixel-wise term of structured KD, CWD's baseline; the soft consistency of mean teacher / FixMatch / UniMatch;
//   2 x 158 MB per 512 x 512 image at K = 151), plus autograd through the student's softmax.
//
// head_kd_grp_kernel is built on head_grp.h as head_ce_pw_grp_kernel (head_selftrain.hip) is: head_grp_plan's tiles and grid, the
// footprint staging, the unit walk, the forward product Wm x lo on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), the backward
// product, the waves' turns on the LDS mirror, the slabs, the block partials and head_finish_kernel (lc2is_head_finish_launch).  The
// teacher's upsampled scores are one more forward product on a second footprint, staged behind the pixel weights.
// Per counted pixel i (labels == NULL: every pixel of the image; else label != ignore_index && 0 <= label < C), u = z / T over the
// C real channels, p = softmax(u):
//   loss_i  = pw_i T^2 sum_c p_t,c (log p_t,c - log p_s,c),   count_i = 1   (NOT multiplied by pw_i)
//   dz_s,c  = gscale pw_i T (p_s,c - p_t,c)                    (nothing flows to the teacher)
// Arithmetic.  Both softmaxes run the same instructions, head_ce_grp_kernel's exponent with the temperature folded in:
// e = exp2(fma(z, k, -max k)), k = log2(e) / T (T = 1: the cross-entropy kernel's own bits), sum = row16_sum of the in-lane sums.
// The loss stays in the log domain, on the exponents a = fma(z, k, -max k) that the two softmaxes exponentiate (log2 units):
//   KL = ln(2) sum_c e_t,c (a_t,c - a_s,c) / sum_t  -  (log sum_t - log sum_s)
// which is sum_c p_t,c (u_t,c - u_s,c) - (lse(u_t) - lse(u_s)) with each map's own shift -max k carried by both terms: log2 p_c is
// a_c - log2 sum exactly as computed, so the rounding residual of max k (3e-4 at a score of 1e4) cancels instead of biasing every
// pixel, there is no log of a rounded probability, and a teacher at 1e4 on one class does not cancel 1e4 against 1e4.  Channels
// at or past C are -inf in both maps for the maxima and the sums; their difference a_t - a_s would be -inf - -inf, so it is
// SELECTED to 0 there, not computed.  A class with p_t == 0 has e_t == 0 and a finite difference: it adds exactly 0.
// teacher == student gives equal exponents, e and sums: with
// contraction switched off for this kernel (p_s - p_t must not become fma(e_s, inv_s, -(e_t inv_t))) the loss and every dlogit are
// exactly 0.0.  Every product with pw_i is a plain multiply of a term the unweighted pixel forms: pw == 2^-k scales the sums and the
// gradient exactly.  -inf and NaN scores in real channels are unsupported (not checked on the device: no host sync).
//
// Choice: the teacher's exponentials STAY IN REGISTERS beside the student's (2 TN accumulator quads per lane, + TN more where a
// wave's two units share a group, S >= 8) — the gradient loop reads p_s and p_t of a channel tile from registers and never forms the
// teacher's product again.  LDS: student footprint, teacher footprint, gradient mirror, label tile, [16][16] pixel weights.
// From the cross-compile's kernel-resource remarks (gfx950, -O3), per instantiation family <MODE, TN, S>; NO instantiation uses
// scratch (ScratchSize 0, no spills):
//   family                  __launch_bounds__   VGPRs bicubic / bilinear by TN        dynamic LDS at the family's largest ld
//   S = 4, TN = 4 / 8       (512, 2)            93, 124 / 89, 120                     bicubic ld 128: 79 664 B (two blocks per CU)
//   S = 4, TN = 10 / 12     (512, 1)            168, 193 / 164, 188                   bicubic ld 192: 117 296 B (one block per CU)
//   S = 8,  TN = 4 .. 12    (512, 1)            142, 209, 237, 217 / 110, 156, 188, 210    bicubic ld 192: 60 848 B
//   S = 16, TN = 4 .. 12    (512, 1)            142, 204, 233, 214 / 106, 152, 184, 207    bicubic ld 192: 39 680 B
// + 64 B of static LDS (the waves' partials); no AGPRs.  <bicubic, 12, 8 / 16> would need student + teacher + the group's running
// gradient sum (3 x 48 registers) and spilled 144-156 B at 256 VGPRs: there each unit takes its own turns on the mirror instead.
// NO read-modify-write atomics, LDS included: plain-store slabs and partials, the fixed-order finish launch; the same bytes every
// run; captures into a graph.
#include "common.h"
#include "head_grp.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

struct KdArgs {
  const float* lo; const float* tlo; int ld;   // [B, h, w, ld] student / teacher scores, C valid channels
  const int64_t* labels;         // [B, H, W] or null: every pixel of the image is counted
  const float* pw;               // [B, H, W] pixel weights, finite and >= 0, or null = ones
  float* ws_loss;                // [blocks][2] loss / count partials
  float* ws_dlo;                 // [blocks][F4 * F4][cq] footprint mirrors, or null (loss only)
  int B, h, w, H, W, C, cq;
  long ignore_index;
  float temp, gscale;
};

constexpr int kd_blocks(int TN, int S) { return (S == 4 && TN <= 8) ? 2 : 1; }
// the tail behind the labels: [16][16] pixel weights, then the teacher's footprint [f4 * f4][ld + HEAD_PAD]
constexpr __host__ __device__ int kd_tail_words(int f4, int ld) { return HT * HT + f4 * f4 * (ld + HEAD_PAD); }

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, kd_blocks(TN, S)) void head_kd_grp_kernel(KdArgs p) {
#pragma clang fp contract(off)   // teacher == student must give exactly 0: p_s - p_t stays two products and one subtraction
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, F4 = GM::F4, NQ = GM::NQ;
  // S >= 8: a wave's two units are one group's and their gradient tiles are summed in registers before the turns — except at
  // TN = 12 bicubic, where student + teacher + running sum (3 x 48 registers) do not fit 256: there each unit takes its own turns
  constexpr bool SUMD = GM::SUMD && !(TN == 12 && MODE == LC2IS_INTERP_BICUBIC);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int CS = p.ld + HEAD_PAD;
  const HeadLds L = head_grp_lds(F4, p.ld, true);
  const bool grad = p.ws_dlo != nullptr;
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + L.dlo;
  int* s_lab = (int*)(s_lo + L.lab);             // -2 outside the image, -1 inside and not labelled, else the label
  float* s_pw = s_lo + L.tail;                   // [16][16] pixel weights (read only where the pixel is counted)
  float* s_tlo = s_pw + HT * HT;                 // the teacher's footprint
  stage_footprint<MODE, S>(s_lo, s_dlo, grad, p.lo, p.ld, p.h, p.w, T, tid);
  stage_footprint<MODE, S>(s_tlo, nullptr, false, p.tlo, p.ld, p.h, p.w, T, tid);
  if (tid < HT * HT) {
    stage_label<true>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
    const int Y = T.Y0 + (tid >> 4), X = T.X0 + (tid & 15);
    s_pw[tid] = (Y >= 0 && X >= 0 && Y < p.H && X < p.W) ? (p.pw ? p.pw[((size_t)T.b * p.H + Y) * p.W + X] : 1.f) : 0.f;
  }
  __syncthreads();
  const int lab_min = p.labels ? 0 : -1;         // a pixel is counted where s_lab >= lab_min
  constexpr float LN2 = 0.6931471805599453f;
  const float kexp = HEAD_LOG2E / p.temp, t2 = p.temp * p.temp, gt = p.gscale * p.temp;

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  const int cellm_off = make_cellm_off<MODE, S>(m, kq, CS);
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);
  float Af[NQ], Bb[4];
  auto make_operands = [&](int prow) {
    make_fwd_operand<MODE, S>(Af, prow, m, kq);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int n = 4 * kq + jj;
      Bb[jj] = (m < NT * NT) ? tap_w<MODE, S>(prow + n / S, m / NT) * tap_w<MODE, S>(n % S, m % NT) : 0.f;
    }
  };
  if constexpr (!GM::SUMD) make_operands(0);
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
    f32x4_t acc[TN];    // student: logits, then exp, then (S = 4: in place) the transposed gradient tiles
    f32x4_t tacc[TN];   // teacher: logits, then exp
    if constexpr (!SUMD) have_d = false;
    if (U.active) {
      if constexpr (GM::SUMD) make_operands(U.prow);
      fwd_product(acc, s_lo + gbase + m, cell_off, Af);
      fwd_product(tacc, s_tlo + gbase + m, cell_off, Af);
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int at4 = (S * U.gy + U.py4) * 16 + S * U.gx + U.px4;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + at4);
      const f32x4_t pw4 = *reinterpret_cast<const f32x4_t*>(s_pw + at4);
      // both maxima over the C real channels of four pixels at once
      float mx[4] = {NEG, NEG, NEG, NEG}, tmx[4] = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        mask_past_c(acc[t], t, m, p.C, NEG);
        mask_past_c(tacc[t], t, m, p.C, NEG);
#pragma unroll
        for (int r = 0; r < 4; ++r) { mx[r] = fmaxf(mx[r], acc[t][r]); tmx[r] = fmaxf(tmx[r], tacc[t][r]); }
      }
      float mxl[4], tmxl[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[r] = row16_max(mx[r]); tmx[r] = row16_max(tmx[r]);
        mxl[r] = -mx[r] * kexp; tmxl[r] = -tmx[r] * kexp;
      }
      // the two softmaxes by the same instructions, and sum_c e_t,c (a_t,c - a_s,c) on their exponents
      float sum[4] = {0.f, 0.f, 0.f, 0.f}, tsum[4] = {0.f, 0.f, 0.f, 0.f}, dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const bool real = 16 * t + m < p.C;   // past C both maps are -inf: the bracket is selected to 0, never formed
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float as = __builtin_fmaf(acc[t][r], kexp, mxl[r]), at = __builtin_fmaf(tacc[t][r], kexp, tmxl[r]);
          const float br = real ? at - as : 0.f;
          const float es = __builtin_amdgcn_exp2f(as), et = __builtin_amdgcn_exp2f(at);
          acc[t][r] = es; tacc[t][r] = et;
          sum[r] += es; tsum[r] += et;
          dot[r] += et * br;
        }
      }
      float inv[4], tinv[4];   // gscale pw T / sum of each map; 0 where the pixel is not counted
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sum[r] = row16_sum(sum[r]); tsum[r] = row16_sum(tsum[r]); dot[r] = row16_sum(dot[r]);
        const bool counted = lab4[r] >= lab_min;
        const float pg = counted ? gt * pw4[r] : 0.f;
        inv[r] = counted ? pg / sum[r] : 0.f;
        tinv[r] = counted ? pg / tsum[r] : 0.f;
        if (counted && m == 0) {
          const float kl = LN2 * (dot[r] / tsum[r]) - (__logf(tsum[r]) - __logf(sum[r]));
          loss_acc += pw4[r] * (t2 * kl);
          cnt_acc += 1.f;
        }
      }
      if (grad) {
        have_d = true;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          f32x4_t gv;
#pragma unroll
          for (int r = 0; r < 4; ++r) gv[r] = acc[t][r] * inv[r] - tacc[t][r] * tinv[r];
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

}  // namespace

extern "C" int lc2is_head_upsample_kd(const float* scores_lo, const float* teacher_lo, int ld, const int64_t* labels,
                                      const float* pixel_weight, float* dscores_lo, float* loss_sum, int B, int h, int w, int C,
                                      int S, int mode, long ignore_index, float temperature, float grad_scale, void* workspace,
                                      size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !teacher_lo || !loss_sum) return LC2IS_ERR_NULL;
  const bool temp_ok = temperature > 0.f && temperature < __builtin_inff();   // (a NaN fails both comparisons)
  // both score pointers and the gradient's through the one alignment test
  if (int rc = head_grp_check(scores_lo, (const void*)((size_t)teacher_lo | (size_t)dscores_lo), temp_ok && grad_scale == grad_scale,
                              B, h, w, C, ld, S, mode))
    return rc;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!head_ws_ok(workspace, workspace_bytes, gp.loss_bytes + gp.dlo_bytes)) return LC2IS_ERR_WORKSPACE;
  float* ws_loss = (float*)workspace;
  float* ws_dlo = dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr;
  KdArgs a{scores_lo, teacher_lo, ld, labels, pixel_weight, ws_loss, ws_dlo, B, h, w, h * S, w * S, C, gp.cq, ignore_index,
           temperature, grad_scale};
  const int lds = head_grp_lds(gp.f4, ld, true).bytes(kd_tail_words(gp.f4, ld));
  const int rc = head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_kd_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(true, kd_tail_words(7, CMAX)), B * gp.t4, lds,
                                                                  stream, a);
  });
  if (rc) return rc;
  return lc2is_head_finish_launch(HeadFinishArgs{dscores_lo, loss_sum, ws_loss, ws_dlo, B, h, w, C, ld, S, mode, gp.cq, B * gp.t4},
                                  stream);
}
