// Segmentation head tail: xS upsample of the per-class score map fused with softmax cross-entropy,
// forward AND backward in one pass (gfx950).
// replaces: F.interpolate(mode="bicubic", scale_factor=4) + rearrange + matmul + nn.CrossEntropyLoss
//   (reference model/model.py:41-53 + evaluate.py:68 / engine.py:94) and AuxiliaryLoss.forward
//   (model/loss.py:17-21: bilinear resize, then CE), plus their autograd.
//
// The upsample is linear with taps summing to 1, so it commutes with TextToPatch.visual and the prototype
// matmul: the host computes class scores at LOW resolution [B,h,w,Cp] (channels-last fp32,
// Cp = padded class count) with two small MFMA GEMMs and this kernel interpolates 151 channels instead of
// 768 — the [B,16384,768] tensor (25 MB/img) is never materialised.
//
// Work split: a block owns a 16x16 tile of OUTPUT pixels; the <=7x7 low-res footprint of the tile (S >= 4) is staged in LDS
// once and the gradient wrt the low-res scores is accumulated in an LDS mirror of the footprint.
//  * S = 4, 8, 16 (the headline bicubic x4 head, config 5's bilinear x4 score map, AuxiliaryLoss at 32 -> 512): the group kernels.
//    Their scheme (tiles shifted by S/2, S x S-pixel groups in units of 16 pixels, two small products on the fp32 matrix pipe,
//    waves taking turns on the LDS mirror, per-block slabs and partials) is described in head_grp.h, which also holds the pieces
//    they share; the kernels here: head_ce_grp_kernel (softmax CE, optional class weights / label smoothing), head_px_grp_kernel (per-pixel loss,
//    forward only), head_focal_grp_kernel (focal / poly-1 CE), head_sigmoid_grp_kernel (sigmoid CE / sigmoid focal),
//    head_dice_stats_grp_kernel / head_ce_dice_grp_kernel (Dice + CE).  head_finish_kernel sums the slabs and partials in a FIXED
//    order (tile row, footprint row, tile column, footprint column): no float atomics, the loss and the gradient are bitwise
//    reproducible.  (Rounds 1-4 flushed the mirror with fp32 atomics: the arrival order made the last bits of the step run-dependent.)
//  * other S (multiples of 16 from 32): head_ce_kernel — each wave walks 64 output pixels with the 64 lanes spread over CHANNELS (3 per lane, C <= 192),
//    wave reductions for the softmax, ds_add_f32 for the gradient scatter, an atomic flush (not reproducible to the last bit; no
//    configuration of the reference reaches them).
// The losses on materialised NCHW logits (the drop-in path) are loss_nchw.hip's.
#include "common.h"
#include "head_grp.h"
#include "head_loss_math.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

struct HeadArgs {
  const float* lo; int ld;       // [B, h, w, ld] scores, C valid channels
  const int64_t* labels;         // [B, H, W]
  float* dlo;                    // [B, h, w, ld] gradient accumulator (pre-zeroed) or null
  float* hi_out;                 // [B, C, H, W] upsampled scores (eval) or null
  float* loss_sum;               // [2]: sum of per-pixel losses, number of counted pixels (atomic)
  int B, h, w, H, W, C, S, mode;
  long ignore_index;
  float gscale;                  // dlo = gscale * (softmax - onehot)
  // group kernels (S = 4 / 8 / 16): per-block outputs, summed in fixed order by head_finish_kernel
  float* ws_loss;                // [blocks][2] loss / count partials
  float* ws_dlo;                 // [blocks][F4 * F4][cq] footprint mirrors
  int cq;                        // channels per slab cell: C rounded up to 4
  // class weights / label smoothing (group kernels with OPT = true only)
  const float* cw;               // [C] class weights (device) or null = all ones
  float eps;                     // label smoothing in [0, 1]
};

__device__ __forceinline__ void lds_add(float* p, float v) {
  __hip_atomic_fetch_add((__attribute__((address_space(3))) float*)LDS_PTR(p), v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int MODE>
__global__ __launch_bounds__(HEAD_THREADS) void head_ce_kernel(HeadArgs p) {
  constexpr int NTAP = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_x = (p.W + HT - 1) / HT, tiles_y = (p.H + HT - 1) / HT;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int ty = (blockIdx.x / tiles_x) % tiles_y, tx = blockIdx.x % tiles_x;
  const int Y0 = ty * HT, X0 = tx * HT;
  const float inv_scale = 1.f / (float)p.S;

  // footprint origin: lowest tap index of the tile's first row/col, highest of its last
  const Taps ty0 = make_taps(Y0, inv_scale, p.h, MODE);
  const Taps ty1 = make_taps(min(Y0 + HT - 1, p.H - 1), inv_scale, p.h, MODE);
  const Taps tx0 = make_taps(X0, inv_scale, p.w, MODE);
  const Taps tx1 = make_taps(min(X0 + HT - 1, p.W - 1), inv_scale, p.w, MODE);
  const int fy0 = ty0.idx[0], fx0 = tx0.idx[0];
  int fy1 = ty1.idx[0], fx1 = tx1.idx[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) { fy1 = max(fy1, ty1.idx[k]); fx1 = max(fx1, tx1.idx[k]); }
  const int FH = fy1 - fy0 + 1, FW = fx1 - fx0 + 1;  // <= FMAX by construction (checked on the host)

  const int Cp = p.ld;  // channel pitch in LDS == global pitch (multiple of 64 floats keeps rows bank-aligned)
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + FMAX * FMAX * Cp;
  const int fsize = FH * FW * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    const int fy = cell / FW, fx = cell % FW;
    const float4 v = *reinterpret_cast<const float4*>(
        p.lo + (((size_t)b * p.h + fy0 + fy) * p.w + fx0 + fx) * p.ld + c);
    *reinterpret_cast<float4*>(s_lo + i) = v;
    if (p.dlo) *reinterpret_cast<float4*>(s_dlo + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  // this wave's 32 pixels: rows 2*wid, 2*wid+1 of the tile, 16 columns each; lane <-> pixel for labels
  const int py_l = 2 * wid + ((lane >> 4) & 1), px_l = lane & 15;
  const int Yl = Y0 + py_l, Xl = X0 + px_l;
  int my_label = -1;
  const bool my_valid = (Yl < p.H && Xl < p.W);
  if (my_valid && p.labels) {
    const int64_t lab64 = p.labels[((size_t)b * p.H + Yl) * p.W + Xl];
    my_label = (lab64 == (int64_t)p.ignore_index || lab64 < 0 || lab64 >= p.C) ? -1 : (int)lab64;
  }

  const bool c_ok[3] = {lane < p.C, lane + 64 < p.C, lane + 128 < p.C};
  float loss_acc = 0.f, cnt_acc = 0.f;

  for (int px = 0; px < 32; ++px) {
    const int Y = Y0 + 2 * wid + (px >> 4), X = X0 + (px & 15);
    if (Y >= p.H || X >= p.W) continue;  // wave-uniform
    const int label = __builtin_amdgcn_readlane(my_label, px);   // wave-uniform lane index: v_readlane, not an LDS bpermute
    const Taps ay = make_taps(Y, inv_scale, p.h, MODE);
    const Taps ax = make_taps(X, inv_scale, p.w, MODE);
    float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NTAP; ++i) {
      const float* rowp = s_lo + ((ay.idx[i] - fy0) * FW - fx0) * Cp + lane;
#pragma unroll
      for (int j = 0; j < NTAP; ++j) {
        const float wgt = ay.w[i] * ax.w[j];
        const float* cp = rowp + ax.idx[j] * Cp;
        v[0] += wgt * cp[0];
        v[1] += wgt * cp[64];
        v[2] += wgt * cp[128];
      }
    }
    if (p.hi_out) {
      const size_t plane = (size_t)p.H * p.W;
      float* o = p.hi_out + ((size_t)b * p.C) * plane + (size_t)Y * p.W + X;
      if (c_ok[0]) o[(size_t)lane * plane] = v[0];
      if (c_ok[1]) o[(size_t)(lane + 64) * plane] = v[1];
      if (c_ok[2]) o[(size_t)(lane + 128) * plane] = v[2];
    }
    if (!p.loss_sum) continue;
    const float NEG = -__builtin_inff();
    float m = fmaxf(fmaxf(c_ok[0] ? v[0] : NEG, c_ok[1] ? v[1] : NEG), c_ok[2] ? v[2] : NEG);
    m = wave_max(m);
    float e[3];
    e[0] = c_ok[0] ? __expf(v[0] - m) : 0.f;
    e[1] = c_ok[1] ? __expf(v[1] - m) : 0.f;
    e[2] = c_ok[2] ? __expf(v[2] - m) : 0.f;
    const float ssum = wave_sum(e[0] + e[1] + e[2]);
    const bool counted = label >= 0;
    if (!counted) continue;
    const int lsel = label >> 6, llane = label & 63;
    const float vsel = lsel == 0 ? v[0] : (lsel == 1 ? v[1] : v[2]);
    const float logit_l = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vsel), llane));
    loss_acc += (m + __logf(ssum)) - logit_l;
    cnt_acc += 1.f;
    if (p.dlo) {
      const float inv = p.gscale / ssum;
      float gch[3];
      gch[0] = e[0] * inv - ((lsel == 0 && lane == llane) ? p.gscale : 0.f);
      gch[1] = e[1] * inv - ((lsel == 1 && lane == llane) ? p.gscale : 0.f);
      gch[2] = e[2] * inv - ((lsel == 2 && lane == llane) ? p.gscale : 0.f);
#pragma unroll
      for (int i = 0; i < NTAP; ++i) {
        float* rowp = s_dlo + ((ay.idx[i] - fy0) * FW - fx0) * Cp + lane;
#pragma unroll
        for (int j = 0; j < NTAP; ++j) {
          const float wgt = ay.w[i] * ax.w[j];
          float* cp = rowp + ax.idx[j] * Cp;
          if (c_ok[0]) lds_add(cp, wgt * gch[0]);
          if (c_ok[1]) lds_add(cp + 64, wgt * gch[1]);
          if (c_ok[2]) lds_add(cp + 128, wgt * gch[2]);
        }
      }
    }
  }

  __shared__ float s_red[HEAD_THREADS / 64][2];   // one pair of atomics per block (same-address atomics serialise in L2)
  if (lane == 0) { s_red[wid][0] = loss_acc; s_red[wid][1] = cnt_acc; }
  __syncthreads();
  if (p.loss_sum && tid == 0) {
    float l = 0.f, c = 0.f;
#pragma unroll
    for (int w = 0; w < HEAD_THREADS / 64; ++w) { l += s_red[w][0]; c += s_red[w][1]; }
    if (c > 0.f) {
      atomicAdd(p.loss_sum, l);
      atomicAdd(p.loss_sum + 1, c);
    }
  }
  if (p.dlo) {
    for (int i = tid; i < fsize; i += HEAD_THREADS) {
      const int cell = i / Cp, c = i % Cp;
      if (c >= p.C) continue;
      const int fy = cell / FW, fx = cell % FW;
      atomicAdd(p.dlo + (((size_t)b * p.h + fy0 + fy) * p.w + fx0 + fx) * p.ld + c, s_dlo[i]);
    }
  }
}

// ---- S = 4 / 8 / 16: the group kernels ----
// From head_grp.h in every kernel: the geometry, the tile, the label and weight staging, the slab store, and the host's LDS size
// (head_grp_lds plus the kernel's own tail below).  Its other pieces (footprint staging, unit walk, cell offsets, operands, products,
// label offsets, tile masking, row maximum) are used only in the kernels whose VGPR count and waves per SIMD they leave as they were
// in every instantiation; where a kernel keeps its own lines a comment names what moved.  The turn loop and the block partials moved
// them in every kernel that has them and are written out.  The scheme itself is described once, in head_grp.h.
constexpr int LDS_TAIL_W = CMAX;                      // [CMAX] class weights (CE with OPT, focal, sigmoid)
constexpr int LDS_TAIL_AB = 2 * CMAX;                 // [alpha | beta][CMAX] (Dice + CE, second pass)
constexpr int lds_tail_stats(int tn) { return (HEAD_THREADS / 64) * 2 * 16 * tn; }   // [waves][I | P][16 TN] (Dice statistics)

// head_ce_grp_kernel: softmax cross-entropy, forward and backward, and (eval) the upsampled scores.
// The label's logit (for the loss) is 16 x NT*NT scalars per unit: LDS reads with one (pixel, cell quad) per lane; its one-hot
// is subtracted from dlogits in the accumulator layout.
// OPT = true: class weights w and label smoothing eps (F.cross_entropy's weight / label_smoothing), W = sum_c w_c:
//   loss_i  = (1 - eps) w_y (lse - z_y) + (eps / C) (W lse - sum_c w_c z_c),   count_i = w_y
//   dz_k    = ((1 - eps) w_y + eps W / C) p_k - (1 - eps) w_y [k == y] - (eps / C) w_k
// The weights sit in LDS behind the labels (zero past C); sum_c w_c z_c is one more 16-lane row sum, taken before exp overwrites
// the logits.  OPT = false is the plain CE of the default call (its register count carries the headline step); labels may be null
// there (a scores-only call).
template <int MODE, int TN, int S, bool OPT>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_ce_grp_kernel(HeadArgs p) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, OFF = GM::OFF, F4 = GM::F4, NQ = GM::NQ;
  constexpr bool SUMD = GM::SUMD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int b = T.b, a0 = T.a0, b0 = T.b0;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;                  // cell stride in LDS (floats): the 16 cells of a group on different banks
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_w = (float*)(s_lab + HT * HT);        // OPT: [CMAX] class weights, zero past C
  // own lines: stage_footprint moved the VGPR counts of <bicubic,4,16,false>, <bicubic,4,8,false> and <bilinear,8,4,true>
  const int fsize = F4 * F4 * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    int ry = a0 - OFF + cell / F4, rx = b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > p.h - 1 ? p.h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > p.w - 1 ? p.w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(p.lo + (((size_t)b * p.h + ry) * p.w + rx) * p.ld + c);
    if (p.dlo) *reinterpret_cast<float4*>(s_dlo + cell * CS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  stage_labels<true>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
  if constexpr (OPT) {
    stage_weights(s_w, p.cw, p.C, tid);
  }
  __syncthreads();
  float a1 = 0.f, ac = 0.f, aw = 0.f;   // OPT: 1 - eps, eps / C, eps W / C
  if constexpr (OPT) {
    a1 = 1.f - p.eps;
    ac = p.eps / (float)p.C;
    aw = ac * wave_sum(s_w[lane] + s_w[lane + 64] + s_w[lane + 128]);
  }

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  const int cellm_off = make_cellm_off<MODE, S>(m, kq, CS);
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);
  // forward A: row = pixel m of the unit, k = kq -> cell 4q + kq.  Backward B of product jj: column = cell m, k = kq -> pixel 4 kq + jj
  float Af[NQ], Bb[4];
  // own lines: make_fwd_operand and a separate backward builder moved the VGPR counts of 17 of the 48 instantiations
  auto make_operands = [&](int prow) {
    const int py_m = prow + m / S, px_m = m % S;
#pragma unroll
    for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % NT);
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
    const int gy = U.gy, gx = U.gx, Yb = U.Yb, Xb = U.Xb, prow = U.prow;
    const bool active = U.active;
    gbase = U.gbase;
    f32x4_t acc[TN];   // logits, then exp, then (S = 4: in place) the transposed gradient tiles
    if constexpr (!SUMD) have_d = false;
    if (active) {
      const int py_m = prow + m / S, px_m = m % S;
      if constexpr (SUMD) make_operands(prow);   // (S = 4: one unit shape, formed once in front of the loop)
      fwd_product(acc, s_lo + gbase + m, cell_off, Af);
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int py4 = U.py4, px4 = U.px4;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
      if (p.hi_out) {
        const size_t plane = (size_t)p.H * p.W;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const int ch = 16 * t + m;
          if (ch < p.C) {
            float* o = p.hi_out + ((size_t)b * p.C + ch) * plane + (size_t)(Yb + py4) * p.W + Xb + px4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (lab4[r] != -2) o[r] = acc[t][r];
          }
        }
      }
      if (p.loss_sum) {
        // the label's logit: this lane owns pixel m x cells {4q + kq}
        const int lab_m = s_lab[(S * gy + py_m) * 16 + S * gx + px_m];
        if (lab_m >= 0) {
          if constexpr (OPT) {
            float zl = 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) zl += Af[q] * s_lo[gbase + cell_off[q] + lab_m];
            loss_acc -= a1 * s_w[lab_m] * zl;
          } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) loss_acc -= Af[q] * s_lo[gbase + cell_off[q] + lab_m];
          }
        }
        // softmax over the channels of four pixels at once
        float mx[4] = {NEG, NEG, NEG, NEG}, sum[4] = {0.f, 0.f, 0.f, 0.f};
        float wz[4] = {0.f, 0.f, 0.f, 0.f};   // OPT: sum_c w_c z_c
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          mask_past_c(acc[t], t, m, p.C, NEG);
          if constexpr (OPT) {
            const float wk = s_w[16 * t + m];   // 0 past C (and there the logit is -inf)
#pragma unroll
            for (int r = 0; r < 4; ++r) wz[r] += wk != 0.f ? wk * acc[t][r] : 0.f;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], acc[t][r]);
        }
        if constexpr (OPT) {   // the smoothing's -(eps/C) sum_c w_c z_c, before exp overwrites the logits
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            wz[r] = row16_sum(wz[r]);
            if (lab4[r] >= 0 && m == 0) loss_acc -= ac * wz[r];
          }
        }
        float mxl[4];   // -max * log2(e): exp(x - max) = exp2(fma(x, log2(e), mxl))
        row_max_mxl(mx, mxl);
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], LOG2E, mxl[r]));
            acc[t][r] = e;
            sum[r] += e;
          }
        float inv[4];
        int dl[4];   // label - lane's channel offset: the one-hot sits in tile t where dl == 16 t
        float oh[4];            // OPT: one-hot coefficient gscale (1 - eps) w_y
        unsigned cmask = 0u;    // OPT: bit r = pixel r counted
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sum[r] = row16_sum(sum[r]);
          const bool counted = lab4[r] >= 0;
          if constexpr (OPT) {
            const float wy = counted ? s_w[counted ? lab4[r] : 0] : 0.f;
            const float cy = a1 * wy, cs = cy + aw;
            inv[r] = counted ? p.gscale * cs / sum[r] : 0.f;
            dl[r] = counted ? lab4[r] - m : -1;
            oh[r] = p.gscale * cy;
            cmask |= counted ? (1u << r) : 0u;
            if (counted && m == 0) {
              loss_acc += cs * (mx[r] + __logf(sum[r]));
              cnt_acc += wy;
            }
          } else {
            inv[r] = counted ? p.gscale / sum[r] : 0.f;
            dl[r] = counted ? lab4[r] - m : -1;
            if (counted && m == 0) {
              loss_acc += mx[r] + __logf(sum[r]);
              cnt_acc += 1.f;
            }
          }
        }
        if (p.dlo) {
          have_d = true;
#pragma unroll
          for (int t = 0; t < TN; ++t) {
            f32x4_t gv;
            if constexpr (OPT) {
              const float sk = p.gscale * ac * s_w[16 * t + m];   // smoothing term of channel 16 t + m
#pragma unroll
              for (int r = 0; r < 4; ++r)
                gv[r] = acc[t][r] * inv[r] - (dl[r] == 16 * t ? oh[r] : 0.f) - ((cmask >> r) & 1u ? sk : 0.f);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) gv[r] = acc[t][r] * inv[r] - (dl[r] == 16 * t ? p.gscale : 0.f);
            }
            bwd_product<SUMD>(gv, Bb, t, acc, dsum);
          }
        }
      }
    }
    if (p.dlo && (!SUMD || g2 == 1)) {
      // the waves' turns on the mirror (head_grp.h); own lines: as a shared helper the loop moved the VGPR counts of 5 instantiations
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

  // the block's [loss, count] partial, plain stores; own lines: as a shared helper it moved the VGPR counts of 47 of 48 instantiations
  __shared__ float s_red[HEAD_THREADS / 64][2];
  loss_acc = wave_sum(loss_acc);
  cnt_acc = wave_sum(cnt_acc);
  if (lane == 0) { s_red[wid][0] = loss_acc; s_red[wid][1] = cnt_acc; }
  __syncthreads();
  if (p.loss_sum && tid == 0) {
    float l = 0.f, c = 0.f;
#pragma unroll
    for (int w = 0; w < HEAD_THREADS / 64; ++w) { l += s_red[w][0]; c += s_red[w][1]; }
    p.ws_loss[2 * (size_t)blockIdx.x] = l;
    p.ws_loss[2 * (size_t)blockIdx.x + 1] = c;
  }
  if (p.dlo) store_slab<MODE, S>(s_dlo, p.ws_dlo, p.cq, CS, tid);
}

// ---- per-pixel loss of the same head, forward only (the input of the OHEM selection, ohem.hip) ----
// The tiles, groups, units and forward product Wm x lo of the scheme, and the softmax in the accumulator layout; nothing of the
// backward: no gradient mirror in LDS, no slabs, no partials, no finish launch.  loss_px[b, Y, X] = lse - z_y in fp32 (plain CE: class
// weights and label smoothing never enter the selection), 0 where the pixel is not counted.  The label's logit is still in the
// accumulators when the maximum is taken: it is the element of tile t in the lane with dl[r] == 16 t, and one more 16-lane row sum of
// that select brings it to every lane of the row.  Lane m == 0 of a row then holds the losses of four consecutive pixels of one
// image row: one 16-byte store (S = 4: tiles start at X = -2 mod 4, the store is 8-byte aligned; a quad that crosses the image
// edge leaves pixel by pixel).
typedef float __attribute__((ext_vector_type(4), aligned(4))) f32x4_u_t;

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_px_grp_kernel(HeadArgs p, float* __restrict__ loss_px) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int G = GM::G, F4 = GM::F4, NQ = GM::NQ, UPG = GM::UPG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int b = T.b, Y0 = T.Y0, X0 = T.X0;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;
  float* s_lo = (float*)smem;
  int* s_lab = (int*)(s_lo + F4 * F4 * CS);      // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  stage_footprint<MODE, S>(s_lo, nullptr, false, p.lo, p.ld, p.h, p.w, T, tid);
  stage_labels<false>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    // own lines: head_unit moved the VGPR counts of 6 instantiations (<bicubic,10,8> lost a wave per SIMD)
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    if (!active) continue;
    const int gbase = (gy * F4 + gx) * CS;
    float Af[NQ];
    make_fwd_operand<MODE, S>(Af, prow, m, kq);
    f32x4_t acc[TN];
    fwd_product(acc, s_lo + gbase + m, cell_off, Af);
    const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
    const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
    int dl[4];
    label_offsets(dl, lab4, m, -1);
    float mx[4] = {NEG, NEG, NEG, NEG}, sum[4] = {0.f, 0.f, 0.f, 0.f}, zy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      mask_past_c(acc[t], t, m, p.C, NEG);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[r] = fmaxf(mx[r], acc[t][r]);
        zy[r] += dl[r] == 16 * t ? acc[t][r] : 0.f;
      }
    }
    float mxl[4];
    row_max_mxl(mx, mxl);
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[r] += __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], LOG2E, mxl[r]));
    f32x4_u_t out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float l = (mx[r] + __logf(row16_sum(sum[r]))) - row16_sum(zy[r]);
      out[r] = lab4[r] >= 0 ? l : 0.f;
    }
    if (m == 0) {
      float* o = loss_px + ((size_t)b * p.H + (Yb + py4)) * p.W + Xb + px4;   // (formed only where a pixel of the quad is inside)
      if (lab4[0] != -2 && lab4[3] != -2) {
        *reinterpret_cast<f32x4_u_t*>(o) = out;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (lab4[r] != -2) o[r] = out[r];
      }
    }
  }
}

// ---- focal / poly-1 cross-entropy on the same head, forward and backward in one pass ----
// For a counted pixel with label y, p = softmax, p_y its label probability, q = 1 - p_y, ce = -ln p_y, class weight w_y:
//   l      = w_y (q^gamma ce + eps1 q)                    gamma >= 0 (focal, Lin et al.), eps1 >= -1 (poly-1, Leng et al.)
//   dl/dz_j = w_y c (p_j - [j == y]),   c = q^gamma + gamma p_y q^(gamma-1) ce + eps1 p_y
// Both are functions of p_y alone, so the gradient is the CE gradient times one scalar per pixel; count = w_y as in the OPT kernel.
// The scheme is head_ce_grp_kernel's, head_finish_kernel behind it.  What differs:
//  * the loss does not split into -z_y and lse, so the label's logit meets the log-sum-exp in one lane: the accumulator element of
//    tile t in the lane with dl[r] == 16 t, one 16-lane row sum (head_px_grp_kernel's way);
//  * q = (sum of the OTHER classes' exponentials) / sum — 1 - e_y / sum and sum - e_y cancel when the label holds the maximum.  The
//    exp loop adds every class but the label's to `so`; e_y is formed once per pixel from the row-summed logit (the same bits);
//  * ce = (max - z_y) + ln(sum) is finite at p_y = 0; below q = 1/64 it is the series of -ln(1 - q), whose relative error stays
//    at fp32 rounding where ln(1 + so) has lost the small term (gamma < 1 divides ce by q);
//  * q^gamma = exp2(gamma log2 q), [gamma == 0] at q == 0; the q^(gamma-1) ce term is formed as q^gamma (ce / q), ce / q -> 1: no
//    Inf or NaN for any gamma >= 0.  A few exp2 / log2 per PIXEL; c enters inv[r] and the label's own coefficient;
//  * the label's gradient element is -c w_y q from `so`, not p_y - 1: the per-class loop is one multiply and one select.
// gamma = eps1 = 0 is the OPT kernel's weighted CE to rounding.  The two scalars travel in an argument of their own (FocalArgs,
// head_loss_math.h, with focal_coef).
template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_focal_grp_kernel(HeadArgs p, FocalArgs f) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, OFF = GM::OFF, G = GM::G, F4 = GM::F4, NQ = GM::NQ, UPG = GM::UPG;
  constexpr bool SUMD = GM::SUMD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int b = T.b, a0 = T.a0, b0 = T.b0, Y0 = T.Y0, X0 = T.X0;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_w = (float*)(s_lab + HT * HT);        // [CMAX] class weights (ones without), zero past C
  // own lines: stage_footprint moved the VGPR count of <bilinear,8,8>
  const int fsize = F4 * F4 * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    int ry = a0 - OFF + cell / F4, rx = b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > p.h - 1 ? p.h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > p.w - 1 ? p.w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(p.lo + (((size_t)b * p.h + ry) * p.w + rx) * p.ld + c);
    if (p.dlo) *reinterpret_cast<float4*>(s_dlo + cell * CS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  stage_labels<false>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
  stage_weights(s_w, p.cw, p.C, tid);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  const int cellm_off = make_cellm_off<MODE, S>(m, kq, CS);
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);
  float Af[NQ], Bb[4];
  // own lines: make_fwd_operand and a separate backward builder moved the VGPR counts of 5 of the 24 instantiations
  auto make_operands = [&](int prow) {
    const int py_m = prow + m / S, px_m = m % S;
#pragma unroll
    for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % NT);
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
    // own lines: head_unit moved the VGPR counts of 16 of the 24 instantiations
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    gbase = (gy * F4 + gx) * CS;
    f32x4_t acc[TN];   // logits, then exp, then (S = 4: in place) the transposed gradient tiles
    if constexpr (!SUMD) have_d = false;
    if (active) {
      if constexpr (SUMD) make_operands(prow);
      fwd_product(acc, s_lo + gbase + m, cell_off, Af);
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
      int dl[4];   // label - lane's channel offset: the label's class sits in tile t where dl == 16 t
      label_offsets(dl, lab4, m, -1);
      float mx[4] = {NEG, NEG, NEG, NEG}, so[4] = {0.f, 0.f, 0.f, 0.f}, zy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        mask_past_c(acc[t], t, m, p.C, NEG);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          mx[r] = fmaxf(mx[r], acc[t][r]);
          zy[r] += dl[r] == 16 * t ? acc[t][r] : 0.f;
        }
      }
      float mxl[4];   // -max * log2(e): exp(x - max) = exp2(fma(x, log2(e), mxl))
#pragma unroll
      for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); mxl[r] = -mx[r] * LOG2E; zy[r] = row16_sum(zy[r]); }
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], LOG2E, mxl[r]));
          acc[t][r] = e;
          so[r] += dl[r] == 16 * t ? 0.f : e;   // every class but the label's
        }
      float inv[4];   // gscale w_y c / sum, 0 where the pixel is not counted
      float gl[4];   // the label's own gradient element: -gscale w_y c q
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        so[r] = row16_sum(so[r]);
        const bool counted = lab4[r] >= 0;
        const float ey = counted ? __builtin_amdgcn_exp2f(__builtin_fmaf(zy[r], LOG2E, mxl[r])) : 0.f;
        const float sum = so[r] + ey;            // >= 1: the maximum's own term
        const float rs = 1.f / sum;
        const float q = so[r] * rs;
        float li;
        const float c = focal_coef(ey * rs, q, (mx[r] - zy[r]) + __logf(sum), f, &li);
        const float wy = counted ? s_w[counted ? lab4[r] : 0] : 0.f;
        inv[r] = counted ? p.gscale * wy * c * rs : 0.f;
        gl[r] = -so[r] * inv[r];
        if (counted && m == 0) {
          loss_acc += wy * li;
          cnt_acc += wy;
        }
      }
      if (p.dlo) {
        have_d = true;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          f32x4_t gv;
#pragma unroll
          for (int r = 0; r < 4; ++r) gv[r] = dl[r] == 16 * t ? gl[r] : acc[t][r] * inv[r];
          bwd_product<SUMD>(gv, Bb, t, acc, dsum);
        }
      }
    }
    // the waves take turns on the LDS mirror, as in head_ce_grp_kernel: plain 16-byte read-add-write, no LDS atomics
    if (p.dlo && (!SUMD || g2 == 1)) {
      // own lines: as a shared helper the turn loop moved the VGPR counts of <bicubic,8,16> and <bicubic,8,8>
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

  // the block's [loss, weighted count] partial and its slab: plain stores, summed in a fixed order by head_finish_kernel
  // own lines: as a shared helper the partial store moved the VGPR counts of all 24 instantiations
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
  if (p.dlo) store_slab<MODE, S>(s_dlo, p.ws_dlo, p.cq, CS, tid);
}

// ---- sigmoid cross-entropy / sigmoid focal loss on the same head: per-class binary terms, forward and backward in one pass ----
// For a counted pixel with label y and a class c < C: z the upsampled score, t = [c == y], p = sigmoid(z), p_t = t ? p : 1 - p:
//   bce   = softplus(z) - t z = -ln p_t
//   l_c   = w_c a_t (1 - p_t)^gamma bce,   a_t = alpha given ? (t ? alpha : 1 - alpha) : 1      (RetinaNet's focal loss; gamma = 0
//   l     = class_scale sum_{c < C} l_c                                                          without alpha: BCE with logits)
// No row maximum, no log-sum-exp, no coupling between the classes: everything is elementwise in the accumulator layout, and the
// pixel's loss is the sum over the TN tiles and the 16 lanes of a row.  With s = t ? -z : z (so bce = softplus(s), 1 - p_t =
// sigmoid(s) = u, p_t = sigmoid(-s) = v) both branches of the definition are one expression:
//   d l_c / dz = (t ? -1 : 1) w_c a_t u^gamma (gamma v bce + u)
// One e = exp2(-|z| log2 e) in (0, 1] serves everything (sigmoid_elem, head_loss_math.h):
//  * L = ln(1 + e): below e = 1/64 the alternating series (relative error < e^5 / 6), where 1 + e has rounded the small term away
//    — 150 of 151 classes are such negatives, and their sum is the loss; above, log2(1 + e);
//  * softplus(s) = max(s, 0) + L;  1 / (1 + e) and e / (1 + e) are the larger and the smaller of (p, 1 - p): no 1 - p;
//  * u^gamma = exp2(-gamma log2(e) softplus(-s)): ln u is never the logarithm of a rounded u, so |z| = 1e4 gives finite values for
//    every gamma >= 0; at gamma == 0 (a uniform branch) the factor is not formed at all — no 0^0, one transcendental fewer.
// Three (gamma == 0) or four quarter-rate operations per ELEMENT; the branch on gamma is uniform and taken once per tile.  Channels
// at or past C enter with z = 0 and w_c = 0: exactly 0 in loss and gradient.  count = the number of counted pixels, unweighted (the
// element-count rule of binary losses).  The scheme is head_focal_grp_kernel's; head_finish_kernel
// gathers.  Beside the element math the kernel differs in when its operands are formed (below).
template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? (TN <= 10 ? 4 : 2) : 1)) void head_sigmoid_grp_kernel(HeadArgs p, SigmoidArgs f) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, OFF = GM::OFF, G = GM::G, F4 = GM::F4, NQ = GM::NQ, UPG = GM::UPG;
  constexpr bool SUMD = GM::SUMD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int b = T.b, a0 = T.a0, b0 = T.b0, Y0 = T.Y0, X0 = T.X0;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_w = (float*)(s_lab + HT * HT);        // [CMAX] class weights (ones without), zero past C
  // own lines: stage_footprint moved the VGPR counts of <bicubic,8,8> and <bilinear,8,16>
  const int fsize = F4 * F4 * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    int ry = a0 - OFF + cell / F4, rx = b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > p.h - 1 ? p.h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > p.w - 1 ? p.w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(p.lo + (((size_t)b * p.h + ry) * p.w + rx) * p.ld + c);
    if (p.dlo) *reinterpret_cast<float4*>(s_dlo + cell * CS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  stage_labels<false>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
  stage_weights(s_w, p.cw, p.C, tid);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const int cellm_off = make_cellm_off<MODE, S>(m, kq, CS);
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);
  // The interpolation operands are formed per unit where they are used, the forward one in front of the forward product and the
  // backward one behind the element loop, from a lane index the compiler cannot see through.  At S = 4 they do not depend on the
  // unit and would be hoisted; held across the 4 TN elements, their eight registers cost the second block per CU (S = 4, TN <= 10
  // is compiled for 4 waves per SIMD = two blocks of 512 threads per CU: 126 VGPRs, no scratch; TN = 12 does not fit and keeps
  // one block per CU).
  auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
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
    // own lines: head_unit moved the VGPR counts of 10 of the 24 instantiations
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    gbase = (gy * F4 + gx) * CS;
    f32x4_t acc[TN];   // scores, then (in place) the gradient elements, then (S = 4) the transposed gradient tiles
    if constexpr (!SUMD) have_d = false;
    if (active) {
      float Af[NQ];
      {
        const int mo = opaque(m), ko = opaque(kq);
        const int py_m = prow + mo / S, px_m = mo % S;
#pragma unroll
        for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + ko) / NT) * tap_w<MODE, S>(px_m, (4 * q + ko) % NT);
      }
// own lines: fwd_product took <bilinear,10,4> from 125 to 127 VGPRs (the instantiation is built for 4 waves per SIMD)
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
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit (one row of the tile, four consecutive columns), channel
      // 16 t + m of tile t
      const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
      int dl[4];      // label - lane's channel offset: the label's class sits in tile t where dl == 16 t; -16 where not counted
      float lsum[4] = {0.f, 0.f, 0.f, 0.f};
      label_offsets(dl, lab4, m, -16);
      const bool focus = f.gamma != 0.f;   // uniform: gamma == 0 forms no (1 - p_t)^gamma — no 0^0, one transcendental fewer
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        mask_past_c(acc[t], t, m, p.C, 0.f);
        const float wc = s_w[16 * t + m];
        float li[4], g[4];
        if (focus) {   // a branch per tile
#pragma unroll
          for (int r = 0; r < 4; ++r) { g[r] = sigmoid_elem<true>(acc[t][r], dl[r] == 16 * t, f, &li[r]); }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) { g[r] = sigmoid_elem<false>(acc[t][r], dl[r] == 16 * t, f, &li[r]); }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float k = wc * (dl[r] == 16 * t ? f.cpos : f.cneg);
          lsum[r] = __builtin_fmaf(k, li[r], lsum[r]);
          acc[t][r] = k * g[r];   // (of a pixel that is not counted too: its column of the back-projection is zero)
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float lp = row16_sum(lsum[r]);   // the pixel's loss: its TN tiles in this lane, the 16 lanes of its row
        if (dl[r] > -16 && m == 0) {
          loss_acc += lp;
          cnt_acc += 1.f;
        }
      }
      if (p.dlo) {
        have_d = true;
        // pixel 4 kq + jj of the back-projection's K index is this lane's own pixel jj: gscale and the counted mask ride on Bb
        float Bz[4];
        const int mo = opaque(m), ko = opaque(kq);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int n = 4 * ko + jj;
          const float bb = (mo < NT * NT) ? tap_w<MODE, S>(prow + n / S, mo / NT) * tap_w<MODE, S>(n % S, mo % NT) : 0.f;
          Bz[jj] = dl[jj] > -16 ? bb * p.gscale : 0.f;
        }
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const f32x4_t gv = acc[t];
          bwd_product<SUMD>(gv, Bz, t, acc, dsum);
        }
      }
    }
    // the waves take turns on the LDS mirror, as in head_ce_grp_kernel: plain 16-byte read-add-write, no LDS atomics
    if (p.dlo && (!SUMD || g2 == 1)) {
      // own lines: as a shared helper the turn loop moved the VGPR count of <bilinear,8,16>
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
  // own lines: as a shared helper the partial store moved the VGPR counts of all 24 instantiations
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
  if (p.dlo) store_slab<MODE, S>(s_dlo, p.ws_dlo, p.cq, CS, tid);
}

// ---- soft Dice + cross-entropy on the same head (smp's multiclass DiceLoss / MONAI's batch=True form, combined with mean CE) ----
// Over the counted pixels V of the whole batch, p = softmax of the upsampled scores:
//   I_c = sum_{i in V, y_i = c} p_ic,  P_c = sum_{i in V} p_ic,  T_c = #{i in V: y_i = c},  U_c = P_c + T_c + s,
//   Dice = (1/C) sum_c m_c (1 - (2 I_c + s) / U_c),  m_c = [T_c > 0] (present_only) or 1;  a class with U_c = 0 adds 0.
// The gradient at one pixel needs the batch sums, so the loss takes two head passes with a small launch between them:
//   head_dice_stats_grp_kernel  forward only: per-block [I | P | T] rows and (CE sum, counted pixels) partials;
//   dice_coef_kernel            (below) sums the blocks' rows in a fixed order (fp64; counts are integers) and writes the
//                               loss block and alpha_c = 2 m_c / (C U_c), beta_c = m_c (2 I_c + s) / (C U_c^2), both times
//                               dice_weight * grad_scale, and ce_scale = ce_weight * grad_scale / n_valid;
//   head_ce_dice_grp_kernel     the shared forward + backward products with the per-pixel gradient
//                               dz_c = p_c (ce_scale + beta_c - q) - [c = y] (ce_scale + alpha_y p_y),  q = sum_k p_k beta_k - alpha_y p_y,
//                               0 where the pixel is not counted; then head_finish_kernel's fixed-order gather of the slabs.
// From head_grp.h: tile, LDS layout, staging, and the slab store of the second pass.  The unit walk, the products and the turn loop
// are these kernels' own lines: through the shared helpers their register counts moved.  No read-modify-write atomics: lane
// exchange, then LDS rows summed in wave order, then slabs summed in block order.
template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 && TN <= 10 ? 2 : 1)) void head_dice_stats_grp_kernel(HeadArgs p, DiceArgs d) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, G = GM::G, F4 = GM::F4, NQ = GM::NQ, UPG = GM::UPG;
  constexpr int NCH = 16 * TN;                   // channels the tiles cover (>= cq)
  constexpr int NW = HEAD_THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int Y0 = T.Y0, X0 = T.X0;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;
  float* s_lo = (float*)smem;
  int* s_lab = (int*)(s_lo + F4 * F4 * CS);      // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_st = (float*)(s_lab + HT * HT);       // [waves][I | P][NCH]
  __shared__ float s_ls[NW];
  stage_footprint<MODE, S>(s_lo, nullptr, false, p.lo, p.ld, p.h, p.w, T, tid);
  stage_labels<false>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  // own lines here and for the forward product: make_cell_off + fwd_product moved the VGPR counts of 3 instantiations
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  float accI[TN], accP[TN];   // channel 16 t + m over this lane's pixels
#pragma unroll
  for (int t = 0; t < TN; ++t) accI[t] = accP[t] = 0.f;
  float loss_acc = 0.f;

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    // own lines: head_unit moved the VGPR counts of 4 instantiations
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    if (!active) continue;
    const int gbase = (gy * F4 + gx) * CS;
    float Af[NQ];
    make_fwd_operand<MODE, S>(Af, prow, m, kq);
    f32x4_t acc[TN];   // logits, then exp
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
    const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
    const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
    int dl[4];
// own lines: label_offsets moved the VGPR counts of 16 of the 24 instantiations
#pragma unroll
    for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : -1;
    float mx[4] = {NEG, NEG, NEG, NEG}, sum[4] = {0.f, 0.f, 0.f, 0.f}, zy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      mask_past_c(acc[t], t, m, p.C, NEG);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[r] = fmaxf(mx[r], acc[t][r]);
        zy[r] += dl[r] == 16 * t ? acc[t][r] : 0.f;
      }
    }
    float mxl[4];
    row_max_mxl(mx, mxl);
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], LOG2E, mxl[r]));   // 0 past C
        acc[t][r] = e;
        sum[r] += e;
      }
    float inv[4];   // 1 / sum of the counted pixels, 0 elsewhere: p = e * inv adds nothing where the pixel is not counted
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = row16_sum(sum[r]);
      const float l = (mx[r] + __logf(s)) - row16_sum(zy[r]);
      const bool counted = lab4[r] >= 0;
      inv[r] = counted ? 1.f / s : 0.f;
      if (counted && m == 0) loss_acc += l;
    }
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = acc[t][r] * inv[r];
        accP[t] += pr;
        accI[t] += dl[r] == 16 * t ? pr : 0.f;
      }
  }

  // the four kq lane groups of a channel by lane exchange, the waves through LDS in wave order, the block's row as its own slab
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    accI[t] += __shfl_xor(accI[t], 16); accI[t] += __shfl_xor(accI[t], 32);
    accP[t] += __shfl_xor(accP[t], 16); accP[t] += __shfl_xor(accP[t], 32);
  }
  if (kq == 0) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      s_st[(wid * 2 + 0) * NCH + 16 * t + m] = accI[t];
      s_st[(wid * 2 + 1) * NCH + 16 * t + m] = accP[t];
    }
  }
  loss_acc = wave_sum(loss_acc);
  if (lane == 0) s_ls[wid] = loss_acc;
  __syncthreads();
  if (tid < p.cq) {   // cq <= NCH
    float I = 0.f, P = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) { I += s_st[(w * 2 + 0) * NCH + tid]; P += s_st[(w * 2 + 1) * NCH + tid]; }
    int T = 0;   // the tile's counted pixels of class tid (pixels outside the image and not-counted ones carry negative codes)
    for (int i = 0; i < HT * HT; i += 4) {
      const i32x4_t v = *reinterpret_cast<const i32x4_t*>(s_lab + i);
      T += (v[0] == tid) + (v[1] == tid) + (v[2] == tid) + (v[3] == tid);
    }
    float* row = d.ws_stat + (size_t)blockIdx.x * 3 * p.cq;
    row[tid] = I;
    row[p.cq + tid] = P;
    reinterpret_cast<int*>(row)[2 * p.cq + tid] = T;
  }
  if (wid == NW - 1) {   // (cq <= 192: the last wave holds no channel)
    int n = 0;
#pragma unroll
    for (int j = 0; j < HT * HT / 64; ++j) n += __popcll(__ballot(s_lab[64 * j + lane] >= 0));
    if (lane == 0) {
      float l = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) l += s_ls[w];
      d.ws_part[2 * (size_t)blockIdx.x] = l;
      reinterpret_cast<int*>(d.ws_part)[2 * (size_t)blockIdx.x + 1] = n;
    }
  }
}


template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_ce_dice_grp_kernel(HeadArgs p, const float* __restrict__ coef) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int NT = GM::NT, G = GM::G, F4 = GM::F4, NQ = GM::NQ, UPG = GM::UPG;
  constexpr bool SUMD = GM::SUMD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int Y0 = T.Y0, X0 = T.X0;
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);
  float* s_ab = (float*)(s_lab + HT * HT);       // [alpha | beta][CMAX], zero past C: staged once per block
  stage_footprint<MODE, S>(s_lo, s_dlo, true, p.lo, p.ld, p.h, p.w, T, tid);
  stage_labels<false>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
  if (tid < 2 * CMAX) {
    const int which = tid >= CMAX, c = tid - which * CMAX;
    s_ab[tid] = c < p.C ? coef[which * p.cq + c] : 0.f;
  }
  const float ces = coef[2 * p.cq];   // ce_weight * grad_scale / n_valid
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  const int cellm_off = ((m / NT) * F4 + m % NT) * CS + 4 * kq;
  // own lines: make_cell_off moved the VGPR counts of 5 instantiations, with fwd_product of 7
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  float Af[NQ], Bb[4];
  // own lines, as the backward product below: the shared builders and bwd_product moved the VGPR counts of 5 instantiations
  auto make_operands = [&](int prow) {
    const int py_m = prow + m / S, px_m = m % S;
#pragma unroll
    for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % NT);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int n = 4 * kq + jj;
      Bb[jj] = (m < NT * NT) ? tap_w<MODE, S>(prow + n / S, m / NT) * tap_w<MODE, S>(n % S, m % NT) : 0.f;
    }
  };
  if constexpr (!SUMD) make_operands(0);
  f32x4_t dsum[SUMD ? TN : 1];
  if constexpr (SUMD) {
#pragma unroll
    for (int t = 0; t < TN; ++t) dsum[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  bool have_d = false;
  int gbase = 0;

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    // own lines: head_unit moved the VGPR counts of 13 of the 24 instantiations
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    gbase = (gy * F4 + gx) * CS;
    f32x4_t acc[TN];   // logits, then exp, then (S = 4: in place) the transposed gradient tiles
    if constexpr (!SUMD) have_d = false;
    if (active) {
      if constexpr (SUMD) make_operands(prow);
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
      const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
      int dl[4];   // label - lane's channel offset: the one-hot sits in tile t where dl == 16 t
      label_offsets(dl, lab4, m, -1);
      float mx[4] = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        mask_past_c(acc[t], t, m, p.C, NEG);
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], acc[t][r]);
      }
      float mxl[4];
      row_max_mxl(mx, mxl);
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
      float sb[4] = {0.f, 0.f, 0.f, 0.f};   // sum_k e_k beta_k
      float ey[4] = {0.f, 0.f, 0.f, 0.f};   // e_y, picked by the one-hot select
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const float bt = s_ab[CMAX + 16 * t + m];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[t][r], LOG2E, mxl[r]));
          acc[t][r] = e;
          sum[r] += e;
          sb[r] += e * bt;
          ey[r] += dl[r] == 16 * t ? e : 0.f;
        }
      }
      float inv[4], k1[4], oh[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool counted = lab4[r] >= 0;
        inv[r] = counted ? 1.f / row16_sum(sum[r]) : 0.f;
        const float ay = s_ab[counted ? lab4[r] : 0];
        const float apy = ay * (row16_sum(ey[r]) * inv[r]);   // alpha_y p_y
        k1[r] = ces - (row16_sum(sb[r]) * inv[r] - apy);      // ce_scale - q
        oh[r] = ces + apy;
      }
      have_d = true;
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const float bt = s_ab[CMAX + 16 * t + m];
        f32x4_t gv;
#pragma unroll
        for (int r = 0; r < 4; ++r) gv[r] = (acc[t][r] * inv[r]) * (k1[r] + bt) - (dl[r] == 16 * t ? oh[r] : 0.f);
        f32x4_t dd = {0.f, 0.f, 0.f, 0.f};
        if constexpr (SUMD) dd = dsum[t];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) dd = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[jj], Bb[jj], dd, 0, 0, 0);
        if constexpr (SUMD) dsum[t] = dd; else acc[t] = dd;   // dd[r] = channel 16 t + 4 kq + r of cell m
      }
    }
    // the waves take turns to add their transposed gradient tiles to the LDS mirror (head_ce_grp_kernel's scheme, no LDS atomics)
    if (!SUMD || g2 == 1) {
      // own lines: as a shared helper the turn loop cost <bicubic,10,8> a wave per SIMD
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
  __syncthreads();
  store_slab<MODE, S>(s_dlo, p.ws_dlo, p.cq, CS, tid);
}

// One block.  Thread (slice, c) sums a quarter of the blocks' rows for class c in block order, the four slices are added in slice
// order: a fixed order, in fp64 (as optim_ctrl_update_kernel sums its partials); T and the pixel count are integers.  Thread
// (slice, 255) does the same for the (CE sum, counted pixels) partials.  coef = alpha[cq] | beta[cq] | ce_scale, 0, 0, 0.
__global__ __launch_bounds__(1024) void dice_coef_kernel(DiceCoefArgs a) {
  __shared__ double s_i[4][256], s_p[4][256];
  __shared__ long long s_t[4][256];
  __shared__ double s_dice[256];
  const int c = threadIdx.x & 255, sl = threadIdx.x >> 8;
  const int per = (a.nblk + 3) / 4;
  const int k0 = sl * per, k1 = min(a.nblk, k0 + per);
  double I = 0.0, P = 0.0;
  long long T = 0;
  if (c < a.cq) {
    for (int k = k0; k < k1; ++k) {
      const float* row = a.ws_stat + (size_t)k * 3 * a.cq;
      I += (double)row[c];
      P += (double)row[a.cq + c];
      T += reinterpret_cast<const int*>(row)[2 * a.cq + c];
    }
  } else if (c == 255) {
    for (int k = k0; k < k1; ++k) {
      I += (double)a.ws_part[2 * (size_t)k];
      T += reinterpret_cast<const int*>(a.ws_part)[2 * (size_t)k + 1];
    }
  }
  s_i[sl][c] = I; s_p[sl][c] = P; s_t[sl][c] = T;
  __syncthreads();
  const bool first = sl == 0;   // the first 256 threads finish: one per class, thread 255 for the loss
  long long n_valid = 0;
  if (first) {
    I = ((s_i[0][c] + s_i[1][c]) + s_i[2][c]) + s_i[3][c];
    P = ((s_p[0][c] + s_p[1][c]) + s_p[2][c]) + s_p[3][c];
    T = ((s_t[0][c] + s_t[1][c]) + s_t[2][c]) + s_t[3][c];
    n_valid = ((s_t[0][255] + s_t[1][255]) + s_t[2][255]) + s_t[3][255];
    const double s = (double)a.smooth, gw = (double)a.dice_weight * (double)a.grad_scale;
    double dice_c = 0.0, al = 0.0, be = 0.0;
    if (c < a.C && n_valid > 0) {
      const double U = P + (double)T + s;
      if ((!a.present_only || T > 0) && U > 0.0) {
        const double num = 2.0 * I + s;
        dice_c = 1.0 - num / U;
        al = 2.0 / ((double)a.C * U);
        be = num / ((double)a.C * U * U);
      }
    }
    s_dice[c] = dice_c;
    if (c < a.cq) {
      a.coef[c] = (float)(al * gw);
      a.coef[a.cq + c] = (float)(be * gw);
    }
    if (a.class_stats && c < a.ld_stats) {
      const bool in = c < a.C;
      a.class_stats[c] = in ? (float)I : 0.f;
      a.class_stats[a.ld_stats + c] = in ? (float)P : 0.f;
      a.class_stats[2 * a.ld_stats + c] = in ? (float)T : 0.f;
    }
  }
  __syncthreads();
  if (first && c == 255) {
    double D = 0.0;
    for (int k = 0; k < a.C; ++k) D += s_dice[k];   // class order
    D /= (double)a.C;
    const double ce = n_valid > 0 ? I / (double)n_valid : 0.0;   // (thread 255 summed the CE partials)
    a.loss_out[0] = (float)((double)a.ce_weight * ce + (double)a.dice_weight * D);
    a.loss_out[1] = (float)ce;
    a.loss_out[2] = (float)D;
    a.loss_out[3] = (float)n_valid;
    a.coef[2 * a.cq] = n_valid > 0 ? (float)((double)a.ce_weight * (double)a.grad_scale / (double)n_valid) : 0.f;
    a.coef[2 * a.cq + 1] = a.coef[2 * a.cq + 2] = a.coef[2 * a.cq + 3] = 0.f;
  }
}

// dlo[b, y, x, :] = sum of the footprint cells that map to low-res cell (y, x), over the tiles that cover it, in a fixed order;
// loss_sum = sum of the blocks' partials in block order.  One wave per low-res cell (lane = channel quad), four cells per block.
// Tile t along an axis covers the unclamped low-res indices [G t - 1 - OFF, G t - 1 - OFF + F4); indices below 0 / above n - 1 are
// the clamped taps of the image border and belong to cell 0 / n - 1.
template <int MODE, int S>
__global__ __launch_bounds__(256) void head_finish_kernel(HeadArgs p, int nblk_main) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int OFF = GM::OFF, G = GM::G, F4 = GM::F4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (p.loss_sum && blockIdx.x == 0 && wave == 0) {
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
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ty = ty_lo; ty <= ty_hi; ++ty) {
    const int by = G * ty - 1 - OFF;
    const int fy_lo = max(0, y == 0 ? 0 : y - by), fy_hi = min(F4 - 1, y == p.h - 1 ? F4 - 1 : y - by);
    for (int fy = fy_lo; fy <= fy_hi; ++fy)
      for (int tx = tx_lo; tx <= tx_hi; ++tx) {
        const int bx = G * tx - 1 - OFF;
        const int fx_lo = max(0, x == 0 ? 0 : x - bx), fx_hi = min(F4 - 1, x == p.w - 1 ? F4 - 1 : x - bx);
        const float* slab = p.ws_dlo + (((size_t)b * tiles_y + ty) * tiles_x + tx) * (F4 * F4) * p.cq;
        for (int fx = fx_lo; fx <= fx_hi; ++fx)
          if (lane < q4) {
            const float4 v = *reinterpret_cast<const float4*>(slab + (size_t)(fy * F4 + fx) * p.cq + 4 * lane);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
          }
      }
  }
  if (4 * lane < p.ld) {   // every channel of the row is written (zeros past cq): the caller need not clear the buffer
    float* o = p.dlo + (((size_t)b * p.h + y) * p.w + x) * p.ld + 4 * lane;
    if (4 * lane + 0 >= p.C) acc.x = 0.f;
    if (4 * lane + 1 >= p.C) acc.y = 0.f;
    if (4 * lane + 2 >= p.C) acc.z = 0.f;
    if (4 * lane + 3 >= p.C) acc.w = 0.f;
    *reinterpret_cast<float4*>(o) = acc;
  }
}

// ---- host side of the group kernels ----
// HeadArgs of a group-kernel call: the blocks' partials go to ws_loss, their slabs (when a gradient is wanted) to ws_slab
HeadArgs head_args(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_sum, int B, int h, int w,
                   int C, int S, int mode, long ignore_index, float grad_scale, const float* class_weight, const HeadGrpPlan& gp,
                   void* ws_loss, void* ws_slab) {
  return HeadArgs{scores_lo, ld, labels, dscores_lo, nullptr, loss_sum, B, h, w, h * S, w * S, C, S, mode, ignore_index,
                  grad_scale, (float*)ws_loss, dscores_lo ? (float*)ws_slab : nullptr, gp.cq, class_weight, 0.f};
}

// second launch: fixed-order sums of the slabs (one wave per low-res cell, four per block; fgrid blocks) and of the nblk blocks'
// loss partials
int launch_head_finish(int mode, int S, const HeadArgs& a, int nblk, int fgrid, hipStream_t stream) {
  auto fin = [&](auto M, auto S_) {
    hipLaunchKernelGGL((head_finish_kernel<M(), S_()>), dim3(fgrid), dim3(256), 0, stream, a, nblk);
    return lc2is_check_launch();
  };
  auto by_s = [&](auto M) { return S == 4 ? fin(M, HeadInt<4>{}) : (S == 8 ? fin(M, HeadInt<8>{}) : fin(M, HeadInt<16>{})); };
  return mode == LC2IS_INTERP_BICUBIC ? by_s(HeadInt<LC2IS_INTERP_BICUBIC>{}) : by_s(HeadInt<LC2IS_INTERP_BILINEAR>{});
}
// blocks of the finish launch: four low-res cells each; without a gradient only the partials are summed
int head_finish_grid(const HeadArgs& a) { return (int)(((a.dlo ? (long)a.B * a.h * a.w : 1) + 3) / 4); }
}  // namespace

int lc2is_head_finish_launch(const HeadFinishArgs& f, hipStream_t stream) {
  HeadArgs a{};   // what head_finish_kernel reads
  a.ld = f.ld; a.dlo = f.dlo; a.loss_sum = f.loss_sum;
  a.B = f.B; a.h = f.h; a.w = f.w; a.H = f.h * f.S; a.W = f.w * f.S; a.C = f.C; a.S = f.S; a.mode = f.mode;
  a.ws_loss = f.ws_loss; a.ws_dlo = f.ws_dlo; a.cq = f.cq;
  return launch_head_finish(f.mode, f.S, a, f.nblk, head_finish_grid(a), stream);
}

extern "C" size_t lc2is_head_upsample_ce_workspace_bytes(int B, int h, int w, int C, int S, int mode, int want_grad) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || !(S == 4 || S == 8 || S == 16)) return 0;   // other S: the atomic path, no workspace
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return 0;
  const HeadGrpPlan g = head_grp_plan(B, h, w, C, S, mode, want_grad != 0);
  return g.loss_bytes + g.dlo_bytes;
}

namespace {
// The CE entry differs from its siblings: scores-only calls (no labels, no loss), S >= 32 on the atomic kernel, no alignment
// check, and the smoothing range checked behind S and the mode.
int head_upsample_ce(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* scores_hi,
                     float* loss_sum, int B, int h, int w, int C, int S, int mode, long ignore_index, float grad_scale,
                     const float* class_weight, float label_smoothing, void* workspace, size_t workspace_bytes,
                     lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo) return LC2IS_ERR_NULL;
  if (!scores_hi && !loss_sum) return LC2IS_ERR_NULL;
  if ((loss_sum || dscores_lo) && !labels) return LC2IS_ERR_NULL;
  if (dscores_lo && !loss_sum) return LC2IS_ERR_NULL;
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if (S < 4 || (HT % S != 0 && S % HT != 0)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return LC2IS_ERR_SHAPE;
  // weights / smoothing only shape the loss: a scores-only call runs the plain kernel; the atomic path (S >= 32) has no such variant
  const bool opt = loss_sum && (class_weight || label_smoothing != 0.f);
  if (opt && !(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  const int H = h * S, W = w * S;
  HeadArgs a{scores_lo, ld, labels, dscores_lo, scores_hi, loss_sum, B, h, w, H, W, C, S, mode, ignore_index,
             grad_scale, nullptr, nullptr, 0, class_weight, label_smoothing};
  const int lds_bytes = 2 * FMAX * FMAX * ld * (int)sizeof(float);
  static DevOnce attr_set;
  if (attr_set.need()) {
    const int mx = 2 * FMAX * FMAX * CMAX * (int)sizeof(float);
    if (hipFuncSetAttribute((const void*)head_ce_kernel<LC2IS_INTERP_BICUBIC>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, mx) != hipSuccess ||
        hipFuncSetAttribute((const void*)head_ce_kernel<LC2IS_INTERP_BILINEAR>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, mx) != hipSuccess)
      return LC2IS_ERR_LAUNCH;
    attr_set.done();
  }
  if (S == 4 || S == 8 || S == 16) {
    const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
    const int lds = head_grp_lds(gp.f4, ld, true).bytes(opt ? LDS_TAIL_W : 0);
    if (loss_sum) {   // loss / gradient leave through per-block partials and slabs: a workspace is part of the call
      if (!head_ws_ok(workspace, workspace_bytes, gp.loss_bytes + gp.dlo_bytes)) return LC2IS_ERR_WORKSPACE;
      a.ws_loss = (float*)workspace;
      a.ws_dlo = dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr;
      a.cq = gp.cq;
    }
    const int rc = head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
      if (opt)
        return head_grp_launch<head_ce_grp_kernel<M(), TN_(), S_(), true>>(head_grp_lds_max(true, LDS_TAIL_W), B * gp.t4, lds, stream, a);
      return head_grp_launch<head_ce_grp_kernel<M(), TN_(), S_(), false>>(head_grp_lds_max(true, 0), B * gp.t4, lds, stream, a);
    });
    if (rc || !loss_sum) return rc;
    return launch_head_finish(mode, S, a, B * gp.t4, head_finish_grid(a), stream);
  }
  const int tiles = ((H + HT - 1) / HT) * ((W + HT - 1) / HT);
  if (mode == LC2IS_INTERP_BICUBIC)
    hipLaunchKernelGGL(head_ce_kernel<LC2IS_INTERP_BICUBIC>, dim3(B * tiles), dim3(HEAD_THREADS), lds_bytes,
                       stream, a);
  else
    hipLaunchKernelGGL(head_ce_kernel<LC2IS_INTERP_BILINEAR>, dim3(B * tiles), dim3(HEAD_THREADS), lds_bytes,
                       stream, a);
  return lc2is_check_launch();
}
}  // namespace

extern "C" int lc2is_head_upsample_ce(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                      float* scores_hi, float* loss_sum, int B, int h, int w, int C, int S,
                                      int mode, long ignore_index, float grad_scale, void* workspace,
                                      size_t workspace_bytes, lc2is_stream_t stream) {
  return head_upsample_ce(scores_lo, ld, labels, dscores_lo, scores_hi, loss_sum, B, h, w, C, S, mode, ignore_index,
                          grad_scale, nullptr, 0.f, workspace, workspace_bytes, stream);
}

extern "C" int lc2is_head_upsample_ce_opts(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                           float* scores_hi, float* loss_sum, int B, int h, int w, int C, int S,
                                           int mode, long ignore_index, float grad_scale, const float* class_weight,
                                           float label_smoothing, void* workspace, size_t workspace_bytes,
                                           lc2is_stream_t stream) {
  return head_upsample_ce(scores_lo, ld, labels, dscores_lo, scores_hi, loss_sum, B, h, w, C, S, mode, ignore_index,
                          grad_scale, class_weight, label_smoothing, workspace, workspace_bytes, stream);
}

extern "C" int lc2is_head_upsample_px(const float* scores_lo, int ld, const int64_t* labels, float* loss_px, int B, int h,
                                      int w, int C, int S, int mode, long ignore_index, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !labels || !loss_px) return LC2IS_ERR_NULL;
  if (int rc = head_grp_check(scores_lo, loss_px, true, B, h, w, C, ld, S, mode)) return rc;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, false);
  const HeadArgs a = head_args(scores_lo, ld, labels, nullptr, nullptr, B, h, w, C, S, mode, ignore_index, 0.f, nullptr, gp,
                               nullptr, nullptr);
  const int lds = head_grp_lds(gp.f4, ld, false).bytes(0);   // the footprint and the tile's labels
  return head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_px_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(false, 0), B * gp.t4, lds, stream, a, loss_px);
  });
}

// ---- Dice + cross-entropy: host side ----
static_assert(DICE_CMAX == CMAX, "the NCHW Dice rows and the fused head share dice_coef_kernel");
int lc2is_dice_coef_launch(const DiceCoefArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(dice_coef_kernel, dim3(1), dim3(1024), 0, stream, a);
  return lc2is_check_launch();
}

namespace {
struct DicePlan { HeadGrpPlan g; int nblk; size_t stat_bytes, part_bytes, coef_bytes; };
// workspace: [I | P | T] rows, (CE sum, count) partials, the coefficient block, then (gradient) the slabs
DicePlan dice_head_plan(int B, int h, int w, int C, int S, int mode, bool want_grad) {
  DicePlan d;
  d.g = head_grp_plan(B, h, w, C, S, mode, want_grad);
  d.nblk = B * d.g.t4;
  d.stat_bytes = dice_align((size_t)d.nblk * 3 * d.g.cq * sizeof(float));
  d.part_bytes = dice_align((size_t)d.nblk * 2 * sizeof(float));
  d.coef_bytes = dice_align((size_t)(2 * d.g.cq + 4) * sizeof(float));
  return d;
}
}  // namespace

extern "C" size_t lc2is_head_upsample_ce_dice_workspace_bytes(int B, int h, int w, int C, int S, int mode, int want_grad) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || !(S == 4 || S == 8 || S == 16)) return 0;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return 0;
  const DicePlan d = dice_head_plan(B, h, w, C, S, mode, want_grad != 0);
  return d.stat_bytes + d.part_bytes + d.coef_bytes + d.g.dlo_bytes;
}

extern "C" int lc2is_head_upsample_ce_dice(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                           float* loss_out, float* class_stats, int B, int h, int w, int C, int S, int mode,
                                           long ignore_index, float ce_weight, float dice_weight, float smooth,
                                           int present_only, float grad_scale, void* workspace, size_t workspace_bytes,
                                           lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !labels || !loss_out) return LC2IS_ERR_NULL;
  if (int rc = head_grp_check(scores_lo, dscores_lo, dice_weights_ok(ce_weight, dice_weight, smooth, grad_scale), B, h, w, C, ld, S,
                              mode))
    return rc;
  const DicePlan dp = dice_head_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!head_ws_ok(workspace, workspace_bytes, dp.stat_bytes + dp.part_bytes + dp.coef_bytes + dp.g.dlo_bytes))
    return LC2IS_ERR_WORKSPACE;
  char* wsp = (char*)workspace;
  DiceArgs da{(float*)wsp, (float*)(wsp + dp.stat_bytes)};
  float* coef = (float*)(wsp + dp.stat_bytes + dp.part_bytes);
  // no loss partials of head_finish_kernel's kind (loss_sum is null); the gradient scale rides on the coefficients
  const HeadArgs a = head_args(scores_lo, ld, labels, dscores_lo, nullptr, B, h, w, C, S, mode, ignore_index, 1.f, nullptr, dp.g,
                               nullptr, wsp + dp.stat_bytes + dp.part_bytes + dp.coef_bytes);
  const int tn = head_grp_tn(C), f4 = dp.g.f4;
  // pass 1: the footprint, the tile's labels and the waves' [I | P] rows
  int rc = head_grp_dispatch(mode, S, tn, [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_dice_stats_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(false, lds_tail_stats(12)), dp.nblk,
                                                                          head_grp_lds(f4, ld, false).bytes(lds_tail_stats(tn)),
                                                                          stream, a, da);
  });
  if (rc) return rc;
  const DiceCoefArgs ca{da.ws_stat, da.ws_part, dp.nblk, C, dp.g.cq, ce_weight, dice_weight, smooth, grad_scale,
                        present_only != 0, coef, loss_out, class_stats, ld};
  rc = lc2is_dice_coef_launch(ca, stream);
  if (rc || !dscores_lo) return rc;
  rc = head_grp_dispatch(mode, S, tn, [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_ce_dice_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(true, LDS_TAIL_AB), dp.nblk,
                                                                       head_grp_lds(f4, ld, true).bytes(LDS_TAIL_AB), stream, a,
                                                                       (const float*)coef);
  });
  if (rc) return rc;
  return launch_head_finish(mode, S, a, dp.nblk, head_finish_grid(a), stream);
}

// ---- focal / poly-1 cross-entropy, sigmoid cross-entropy / sigmoid focal loss: host side ----
namespace {
// the two entries differ in the kernel and its scalars only: launch(lds_max, nblk, lds, a) runs the loss's kernel
template <class LAUNCH>
int head_upsample_weighted(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_sum, int B, int h,
                           int w, int C, int S, int mode, long ignore_index, float grad_scale, const float* class_weight,
                           bool args_ok, void* workspace, size_t workspace_bytes, hipStream_t stream, LAUNCH&& launch) {
  if (!scores_lo || !labels || !loss_sum) return LC2IS_ERR_NULL;
  if (int rc = head_grp_check(scores_lo, dscores_lo, args_ok, B, h, w, C, ld, S, mode)) return rc;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!head_ws_ok(workspace, workspace_bytes, gp.loss_bytes + gp.dlo_bytes)) return LC2IS_ERR_WORKSPACE;
  const HeadArgs a = head_args(scores_lo, ld, labels, dscores_lo, loss_sum, B, h, w, C, S, mode, ignore_index, grad_scale,
                               class_weight, gp, workspace, (char*)workspace + gp.loss_bytes);
  // the footprint, its gradient mirror, the tile's labels and the class weights
  const int rc = launch(head_grp_lds_max(true, LDS_TAIL_W), B * gp.t4, head_grp_lds(gp.f4, ld, true).bytes(LDS_TAIL_W), a);
  if (rc) return rc;
  return launch_head_finish(mode, S, a, B * gp.t4, head_finish_grid(a), stream);
}
}  // namespace

extern "C" int lc2is_head_upsample_focal(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                         float* loss_sum, int B, int h, int w, int C, int S, int mode, long ignore_index,
                                         float grad_scale, const float* class_weight, float gamma, float poly_eps,
                                         void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const FocalArgs fa{gamma, poly_eps};
  return head_upsample_weighted(scores_lo, ld, labels, dscores_lo, loss_sum, B, h, w, C, S, mode, ignore_index, grad_scale,
                                class_weight, focal_args_ok(gamma, poly_eps), workspace, workspace_bytes, stream,
                                [&](int lds_max, int nblk, int lds, const HeadArgs& a) {
    return head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
      return head_grp_launch<head_focal_grp_kernel<M(), TN_(), S_()>>(lds_max, nblk, lds, stream, a, fa);
    });
  });
}

extern "C" int lc2is_head_upsample_sigmoid(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                           float* loss_sum, int B, int h, int w, int C, int S, int mode, long ignore_index,
                                           float grad_scale, const float* class_weight, float gamma, float alpha,
                                           float class_scale, void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const SigmoidArgs sa = sigmoid_args(gamma, alpha, class_scale);
  return head_upsample_weighted(scores_lo, ld, labels, dscores_lo, loss_sum, B, h, w, C, S, mode, ignore_index, grad_scale,
                                class_weight, sigmoid_args_ok(gamma, alpha, class_scale), workspace, workspace_bytes, stream,
                                [&](int lds_max, int nblk, int lds, const HeadArgs& a) {
    return head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
      return head_grp_launch<head_sigmoid_grp_kernel<M(), TN_(), S_()>>(lds_max, nblk, lds, stream, a, sa);
    });
  });
}

