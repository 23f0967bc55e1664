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
// once and the gradient wrt the low-res scores is accumulated in an LDS mirror of the footprint.  S = 4 / 8 / 16 (round 5): the
// mirror leaves as the block's own SLAB of a workspace (plain stores) and a second launch sums, for every low-res cell, the
// footprint cells of the tiles that cover it in a FIXED order (tile row, footprint row, tile column, footprint column); the
// blocks' loss / count partials go the same way — no float atomics, the loss and the gradient are bitwise reproducible.
// (Rounds 1-4 flushed the mirror with fp32 atomics: the arrival order made the last bits of the step run-dependent.)
// Other S keep the atomic flush (not reproducible to the last bit; no configuration of the reference reaches them).
//  * S = 4, 8, 16 (the headline bicubic x4 head, config 5's bilinear x4 score map, AuxiliaryLoss at 32 -> 512): head_ce_grp_kernel —
//    S x S-pixel groups in units of 16 pixels as two small products on the fp32 matrix pipe, softmax in the accumulator layout,
//    waves taking turns to add their gradient tiles to the LDS mirror (no LDS atomics: they retire about one lane per three
//    cycles per CU and were 90 % of the first S = 4 kernel).
//    Its siblings on the same tiles: head_px_grp_kernel (per-pixel loss, forward only), head_focal_grp_kernel (focal / poly-1 CE,
//    forward + backward), head_dice_stats_grp_kernel / head_ce_dice_grp_kernel (Dice + CE).
//  * other S (multiples of 16 from 32): head_ce_kernel — each wave walks 64 output pixels with the 64 lanes spread over CHANNELS (3 per lane, C <= 192),
//    wave reductions for the softmax, ds_add_f32 for the gradient scatter.
#include "common.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

constexpr int HT = 16;        // output tile edge
constexpr int FMAX = 8;       // max footprint edge for S >= 4 (16/S + 4 bicubic rows)
constexpr int HEAD_THREADS = 512;
constexpr int CMAX = 192;
constexpr int HEAD_PAD = 4;     // floats added to a footprint cell's LDS stride in the S = 4 kernel

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

// ---- S = 4 / 8 / 16, bicubic (S = 4: the headline configuration) or bilinear (config-5 score map, AuxiliaryLoss) ----
// The output pixels Y in [S a + S/2, S a + 3S/2) share one tap row set {a-1..a+2} (bilinear: {a, a+1}) and differ only in the
// fractional weight t = (ph + 1/2) / S, ph = 0..S-1; tiles are shifted by S/2 pixels so that they hold exactly (16/S)^2 such GROUPS
// of S x S pixels.  A group is worked in UNITS of 16 pixels (S = 4: the whole 4x4 group; S = 8: two rows of 8; S = 16: one row), two
// units per wave, and a unit is two small matrix products on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32: an exact k-ordered fp32
// fma chain at twice the plain-VALU rate, beside the VALU instead of on it):
//   logits[16 pixels][C]  = Wm[16 pixels][NT*NT cells] x lo[cells][C]            (forward,  A = weights, B = LDS footprint)
//   dlo^T [C][cells]     += dlogits^T[C][16 pixels]    x Wm[16 pixels][cells]    (backward, A = the forward's accumulators)
// Wm[pixel (py,px)][cell (i,j)] = w(py,i) * w(px,j).  The accumulator of a 16-channel tile holds, per lane, channel
// 16t + (lane & 15) of the four pixels 4 (lane >> 4) + r of the unit: the softmax over channels is an in-lane loop over the
// tiles plus four DPP steps inside a 16-lane row, for four pixels at once, and the same registers (now dlogits) are the A
// operand of the backward product once its B operand is ordered to match (k = lane >> 4 <-> pixel 4 k + jj in product jj).
// The label's logit (for the loss) is 16 x NT*NT scalars per unit: LDS reads with one (pixel, cell quad) per lane; its one-hot
// is subtracted from dlogits in the accumulator layout.
// Bilinear's clamp of the source coordinate at 0 (torch) equals clamping the tap indices because the two clamped taps coincide.
// OPT = true: class weights w and label smoothing eps (F.cross_entropy's weight / label_smoothing), W = sum_c w_c:
//   loss_i  = (1 - eps) w_y (lse - z_y) + (eps / C) (W lse - sum_c w_c z_c),   count_i = w_y
//   dz_k    = ((1 - eps) w_y + eps W / C) p_k - (1 - eps) w_y [k == y] - (eps / C) w_k
// The weights sit in LDS behind the labels (zero past C); sum_c w_c z_c is one more 16-lane row sum, taken before exp overwrites
// the logits.  OPT = false is the plain CE of the default call, untouched (its register count carries the headline step).
template <int MODE, int S> __device__ __forceinline__ float tap_w(int ph, int k) {
  const float t = ((float)ph + 0.5f) * (1.f / (float)S);
  if constexpr (MODE == LC2IS_INTERP_BICUBIC)
    return k == 0 ? cubic2(t + 1.f) : (k == 1 ? cubic1(t) : (k == 2 ? cubic1(1.f - t) : cubic2(2.f - t)));
  else
    return k == 0 ? 1.f - t : t;
}

template <int CTRL> __device__ __forceinline__ float row_dpp(float v) {   // lane permutation inside each row of 16 lanes
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, row_dpp<0xB1>(v)); v = fmaxf(v, row_dpp<0x4E>(v)); v = fmaxf(v, row_dpp<0x141>(v));
  return fmaxf(v, row_dpp<0x140>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += row_dpp<0xB1>(v); v += row_dpp<0x4E>(v); v += row_dpp<0x141>(v);
  return v + row_dpp<0x140>(v);
}

constexpr int head_grp_footprint(int mode, int S) { return HT / S + (mode == LC2IS_INTERP_BICUBIC ? 4 : 2) - 1; }

template <int MODE, int TN, int S, bool OPT>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_ce_grp_kernel(HeadArgs p) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;   // taps per axis
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;  // first tap = a - OFF
  constexpr int G = HT / S;                                    // groups per tile edge
  constexpr int F4 = G + NT - 1;                               // footprint edge
  constexpr int NQ = NT * NT / 4;                              // k = 4 chunks of the forward product
  constexpr int UPG = S * S / 16;                              // 16-pixel units per group (whole rows of the group: 16 / S rows each)
  constexpr bool SUMD = UPG > 1;                               // a wave's two units belong to one group: their gradient tiles are summed
  static_assert(S == 4 || S == 8 || S == 16, "group kernel: S x S pixel groups inside a 16 x 16 tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_x = (p.W + S / 2 + HT - 1) / HT, tiles_y = (p.H + S / 2 + HT - 1) / HT;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int tyi = (blockIdx.x / tiles_x) % tiles_y, txi = blockIdx.x % tiles_x;
  const int a0 = G * tyi - 1, b0 = G * txi - 1;  // "floor" lo index of the tile's first group row / column
  const int Y0 = S * a0 + S / 2, X0 = S * b0 + S / 2;   // the tile's first output pixel
  const int Cp = p.ld;
  const int CS = Cp + HEAD_PAD;                  // cell stride in LDS (floats): the 16 cells of a group on different banks
  float* s_lo = (float*)smem;
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_w = (float*)(s_lab + HT * HT);        // OPT: [CMAX] class weights, zero past C
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
  }
  if constexpr (OPT) {
    if (tid < CMAX) s_w[tid] = tid < p.C ? (p.cw ? p.cw[tid] : 1.f) : 0.f;
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
  const int cellm_off = ((m / NT) * F4 + m % NT) * CS + 4 * kq;   // this lane's cell / channel quad in the transposed gradient tile
  int cell_off[NQ];   // LDS float offset of the forward cell 4q + kq, relative to the group's first cell
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  // forward A: row = pixel m of the unit, k = kq -> cell 4q + kq.  Backward B of product jj: column = cell m, k = kq -> pixel 4 kq + jj
  float Af[NQ], Bb[4];
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
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;   // the group's first output pixel
    // pixel n of the unit: (py, px) inside the group
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    gbase = (gy * F4 + gx) * CS;
    f32x4_t acc[TN];   // logits, then exp, then (S = 4: in place) the transposed gradient tiles
    if constexpr (!SUMD) have_d = false;
    if (active) {
      const int py_m = prow + m / S, px_m = m % S;
      if constexpr (SUMD) make_operands(prow);   // (S = 4: one unit shape, formed once in front of the loop)
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
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
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
          if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C
            if (16 * t + m >= p.C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
          }
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
#pragma unroll
        for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); mxl[r] = -mx[r] * LOG2E; }
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
            f32x4_t d = {0.f, 0.f, 0.f, 0.f};
            if constexpr (SUMD) d = dsum[t];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) d = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[jj], Bb[jj], d, 0, 0, 0);
            if constexpr (SUMD) dsum[t] = d; else acc[t] = d;   // d[r] = channel 16 t + 4 kq + r of cell m
          }
        }
      }
    }
    // The groups of a tile overlap in every footprint cell (bicubic), and LDS float atomics retire about one LANE per three
    // cycles per CU — 2 800 lane-adds per group made them 90 % of the first S = 4 kernel.  The waves take turns instead: plain
    // 16-byte read-add-write of the transposed tiles (one cell per lane, four consecutive channels, conflict-free under the padded
    // stride).  S = 4 bilinear footprints are 2 x 2 cells: the groups a pass runs on waves of equal (wid >> 1) & 1 sit two cells
    // apart in both directions, so two turns per pass do.  S >= 8: a wave's two units are one group's, one round of turns per tile.
    if (p.dlo && (!SUMD || g2 == 1)) {
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

  // one pair of atomics per BLOCK: thousands of waves adding to the same two floats serialise in one L2 channel
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
  if (p.dlo) {   // the mirror leaves as this block's slab: cells in footprint order, cq channels each, 16 bytes per lane
    const int q4 = p.cq >> 2;
    float* slab = p.ws_dlo + (size_t)blockIdx.x * (F4 * F4) * p.cq;
    for (int i = tid; i < F4 * F4 * q4; i += HEAD_THREADS) {
      const int cell = i / q4, c = (i % q4) * 4;
      *reinterpret_cast<float4*>(slab + (size_t)cell * p.cq + c) = *reinterpret_cast<const float4*>(s_dlo + cell * CS + c);
    }
  }
}

// ---- per-pixel loss of the same head, forward only (the input of the OHEM selection, ohem.hip) ----
// head_ce_grp_kernel's tiles, groups, units and forward product Wm x lo, and its softmax in the accumulator layout; nothing of its
// backward: no gradient mirror in LDS, no slabs, no partials, no finish launch.  loss_px[b, Y, X] = lse - z_y in fp32 (plain CE: class
// weights and label smoothing never enter the selection), 0 where the pixel is not counted.  The label's logit is still in the
// accumulators when the maximum is taken: it is the element of tile t in the lane with dl[r] == 16 t, and one more 16-lane row sum of
// that select brings it to every lane of the row.  Lane m == 0 of a row then holds the losses of four consecutive pixels of one
// image row: one 16-byte store (S = 4: tiles start at X = -2 mod 4, the store is 8-byte aligned; a quad that crosses the image
// edge leaves pixel by pixel).  A kernel of its own, so that the instantiations of head_ce_grp_kernel compile to what they were.
typedef float __attribute__((ext_vector_type(4), aligned(4))) f32x4_u_t;

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_px_grp_kernel(HeadArgs p, float* __restrict__ loss_px) {
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
      const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
      if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
    }
    s_lab[tid] = code;
  }
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    if (!active) continue;
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
    const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
    const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
    int dl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : -1;
    float mx[4] = {NEG, NEG, NEG, NEG}, sum[4] = {0.f, 0.f, 0.f, 0.f}, zy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C (a counted label is below C: never selected there)
        if (16 * t + m >= p.C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[r] = fmaxf(mx[r], acc[t][r]);
        zy[r] += dl[r] == 16 * t ? acc[t][r] : 0.f;
      }
    }
    float mxl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); mxl[r] = -mx[r] * LOG2E; }
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
// Both are functions of p_y alone, so the gradient is the CE gradient times one scalar per pixel: head_ce_grp_kernel's tiles, forward
// product, softmax in the accumulator layout, transposed gradient tiles, turns on the LDS mirror, slab and partials, and
// head_finish_kernel behind it; count = w_y as in the OPT kernel.  What differs:
//  * the loss does not split into -z_y and lse, so the label's logit meets the log-sum-exp in one lane: the accumulator element of
//    tile t in the lane with dl[r] == 16 t, one 16-lane row sum (head_px_grp_kernel's way);
//  * q = (sum of the OTHER classes' exponentials) / sum — 1 - e_y / sum and sum - e_y cancel when the label holds the maximum.  The
//    exp loop adds every class but the label's to `so`; e_y is formed once per pixel from the row-summed logit (the same bits);
//  * ce = (max - z_y) + ln(sum) is finite at p_y = 0; below q = 1/64 it is the series of -ln(1 - q), whose relative error stays
//    at fp32 rounding where ln(1 + so) has lost the small term (gamma < 1 divides ce by q);
//  * q^gamma = exp2(gamma log2 q), [gamma == 0] at q == 0; the q^(gamma-1) ce term is formed as q^gamma (ce / q), ce / q -> 1: no
//    Inf or NaN for any gamma >= 0.  A few exp2 / log2 per PIXEL; c enters inv[r] and the label's own coefficient;
//  * the label's gradient element is -c w_y q from `so`, not p_y - 1: the per-class loop is one multiply and one select.
// gamma = eps1 = 0 is the OPT kernel's weighted CE to rounding.  A kernel of its own, its two scalars in an argument of their own:
// HeadArgs and the instantiations of head_ce_grp_kernel / head_px_grp_kernel compile to what they were.
struct FocalArgs { float gamma, poly_eps; };

// one pixel's focal terms from its label probability pl, q = 1 - pl (formed without cancellation) and ce_big = lse - z_y:
// returns c, *loss = q^gamma ce + eps1 q
__device__ __forceinline__ float focal_coef(float pl, float q, float ce_big, FocalArgs f, float* loss) {
  const bool small = q < 0.015625f;
  const float ser = 1.f + q * (0.5f + q * ((1.f / 3.f) + q * (0.25f + q * 0.2f)));   // -ln(1 - q) / q, q < 1/64: error < q^5 / 6
  const float cq = small ? ser : ce_big / q;   // ce / q (the division is taken only where q >= 1/64)
  const float ce = small ? q * ser : ce_big;
  float qg = 1.f;                                // q^gamma
  if (f.gamma != 0.f) qg = q > 0.f ? __builtin_amdgcn_exp2f(f.gamma * __builtin_amdgcn_logf(q)) : 0.f;
  *loss = qg * ce + f.poly_eps * q;
  return qg + f.gamma * pl * (qg * cq) + f.poly_eps * pl;
}

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_focal_grp_kernel(HeadArgs p, FocalArgs f) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int G = HT / S;
  constexpr int F4 = G + NT - 1;
  constexpr int NQ = NT * NT / 4;
  constexpr int UPG = S * S / 16;
  constexpr bool SUMD = UPG > 1;
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
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_w = (float*)(s_lab + HT * HT);        // [CMAX] class weights (ones without), zero past C
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
  if (tid < HT * HT) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    int code = -2;
    if (Y >= 0 && X >= 0 && Y < p.H && X < p.W) {
      code = -1;
      const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
      if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
    }
    s_lab[tid] = code;
  }
  if (tid < CMAX) s_w[tid] = tid < p.C ? (p.cw ? p.cw[tid] : 1.f) : 0.f;
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  const int cellm_off = ((m / NT) * F4 + m % NT) * CS + 4 * kq;
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  float Af[NQ], Bb[4];
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
      // this lane's four accumulator pixels 4 kq .. 4 kq + 3 of the unit: one row of the tile, four consecutive columns
      const int py4 = prow + (4 * kq) / S, px4 = (4 * kq) % S;
      const i32x4_t lab4 = *reinterpret_cast<const i32x4_t*>(s_lab + (S * gy + py4) * 16 + S * gx + px4);
      int dl[4];   // label - lane's channel offset: the label's class sits in tile t where dl == 16 t
#pragma unroll
      for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : -1;
      float mx[4] = {NEG, NEG, NEG, NEG}, so[4] = {0.f, 0.f, 0.f, 0.f}, zy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C (a counted label is below C: never selected there)
          if (16 * t + m >= p.C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
        }
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
          f32x4_t d = {0.f, 0.f, 0.f, 0.f};
          if constexpr (SUMD) d = dsum[t];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) d = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[jj], Bb[jj], d, 0, 0, 0);
          if constexpr (SUMD) dsum[t] = d; else acc[t] = d;   // d[r] = channel 16 t + 4 kq + r of cell m
        }
      }
    }
    // the waves take turns on the LDS mirror, as in head_ce_grp_kernel: plain 16-byte read-add-write, no LDS atomics
    if (p.dlo && (!SUMD || g2 == 1)) {
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
  if (p.dlo) {
    const int q4 = p.cq >> 2;
    float* slab = p.ws_dlo + (size_t)blockIdx.x * (F4 * F4) * p.cq;
    for (int i = tid; i < F4 * F4 * q4; i += HEAD_THREADS) {
      const int cell = i / q4, c = (i % q4) * 4;
      *reinterpret_cast<float4*>(slab + (size_t)cell * p.cq + c) = *reinterpret_cast<const float4*>(s_dlo + cell * CS + c);
    }
  }
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
// One e = exp2(-|z| log2 e) in (0, 1] serves everything:
//  * L = ln(1 + e): below e = 1/64 the alternating series (relative error < e^5 / 6), where 1 + e has rounded the small term away
//    — 150 of 151 classes are such negatives, and their sum is the loss; above, log2(1 + e);
//  * softplus(s) = max(s, 0) + L;  1 / (1 + e) and e / (1 + e) are the larger and the smaller of (p, 1 - p): no 1 - p;
//  * u^gamma = exp2(-gamma log2(e) softplus(-s)): ln u is never the logarithm of a rounded u, so |z| = 1e4 gives finite values for
//    every gamma >= 0; at gamma == 0 (a uniform branch) the factor is not formed at all — no 0^0, one transcendental fewer.
// Three (gamma == 0) or four quarter-rate operations per ELEMENT; the branch on gamma is uniform and taken once per tile.  Channels at or past C enter with z = 0 and w_c = 0: exactly 0 in
// loss and gradient.  count = the number of counted pixels, unweighted (the element-count rule of binary losses).  The tiles, LDS
// staging, products, mirror turns, partials and slabs are head_focal_grp_kernel's; head_finish_kernel gathers.  A kernel of its own
// with an argument struct of its own: HeadArgs and the existing instantiations compile to what they were.
struct SigmoidArgs { float gamma, ng2, cpos, cneg; };   // ng2 = -gamma log2(e); cpos / cneg = class_scale a_t for t = 1 / 0

// one (pixel, class) element: *l = (1 - p_t)^gamma bce, returns d *l / dz.  FOCUS = false: gamma == 0, no modulating factor
template <bool FOCUS>
__device__ __forceinline__ float sigmoid_elem(float z, bool tl, SigmoidArgs f, float* l) {
  constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
  const float s = tl ? -z : z;
  const float e = __builtin_amdgcn_exp2f(-fabsf(z) * LOG2E);
  const float ser = e * (1.f - e * (0.5f - e * ((1.f / 3.f) - e * (0.25f - e * 0.2f))));
  const float L = e < 0.015625f ? ser : LN2 * __builtin_amdgcn_logf(1.f + e);
  const float sp = fmaxf(s, 0.f) + L;               // bce
  const float big = __builtin_amdgcn_rcpf(1.f + e), sm = e * big;
  const bool pos = s >= 0.f;
  const float u = pos ? big : sm, v = pos ? sm : big;
  float lo = sp, g = u;
  if constexpr (FOCUS) {
    const float ug = __builtin_amdgcn_exp2f(f.ng2 * (fmaxf(-s, 0.f) + L));
    lo = ug * sp;
    g = ug * __builtin_fmaf(f.gamma * v, sp, u);
  }
  *l = lo;
  return tl ? -g : g;
}

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? (TN <= 10 ? 4 : 2) : 1)) void head_sigmoid_grp_kernel(HeadArgs p, SigmoidArgs f) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int G = HT / S;
  constexpr int F4 = G + NT - 1;
  constexpr int NQ = NT * NT / 4;
  constexpr int UPG = S * S / 16;
  constexpr bool SUMD = UPG > 1;
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
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);     // [16][16] pixels of the tile: -2 outside the image, -1 not counted, else label
  float* s_w = (float*)(s_lab + HT * HT);        // [CMAX] class weights (ones without), zero past C
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
  if (tid < HT * HT) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    int code = -2;
    if (Y >= 0 && X >= 0 && Y < p.H && X < p.W) {
      code = -1;
      const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
      if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
    }
    s_lab[tid] = code;
  }
  if (tid < CMAX) s_w[tid] = tid < p.C ? (p.cw ? p.cw[tid] : 1.f) : 0.f;
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const int cellm_off = ((m / NT) * F4 + m % NT) * CS + 4 * kq;
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
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
#pragma unroll
      for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : -16;
      const bool focus = f.gamma != 0.f;   // uniform: gamma == 0 forms no (1 - p_t)^gamma — no 0^0, one transcendental fewer
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C — z = 0 there, and their weight is 0
          if (16 * t + m >= p.C) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
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
          f32x4_t d = {0.f, 0.f, 0.f, 0.f};
          if constexpr (SUMD) d = dsum[t];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) d = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[jj], Bz[jj], d, 0, 0, 0);
          if constexpr (SUMD) dsum[t] = d; else acc[t] = d;   // d[r] = channel 16 t + 4 kq + r of cell m
        }
      }
    }
    // the waves take turns on the LDS mirror, as in head_ce_grp_kernel: plain 16-byte read-add-write, no LDS atomics
    if (p.dlo && (!SUMD || g2 == 1)) {
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
  if (p.dlo) {
    const int q4 = p.cq >> 2;
    float* slab = p.ws_dlo + (size_t)blockIdx.x * (F4 * F4) * p.cq;
    for (int i = tid; i < F4 * F4 * q4; i += HEAD_THREADS) {
      const int cell = i / q4, c = (i % q4) * 4;
      *reinterpret_cast<float4*>(slab + (size_t)cell * p.cq + c) = *reinterpret_cast<const float4*>(s_dlo + cell * CS + c);
    }
  }
}

// ---- soft Dice + cross-entropy on the same head (smp's multiclass DiceLoss / MONAI's batch=True form, combined with mean CE) ----
// Over the counted pixels V of the whole batch, p = softmax of the upsampled scores:
//   I_c = sum_{i in V, y_i = c} p_ic,  P_c = sum_{i in V} p_ic,  T_c = #{i in V: y_i = c},  U_c = P_c + T_c + s,
//   Dice = (1/C) sum_c m_c (1 - (2 I_c + s) / U_c),  m_c = [T_c > 0] (present_only) or 1;  a class with U_c = 0 adds 0.
// The gradient at one pixel needs the batch sums, so the loss takes two head passes with a small launch between them:
//   head_dice_stats_grp_kernel  forward only: per-block [I | P | T] rows and (CE sum, counted pixels) partials;
//   dice_coef_kernel            sums the blocks' rows in a fixed order (fp64; counts are integers) and writes the loss block and
//                               alpha_c = 2 m_c / (C U_c), beta_c = m_c (2 I_c + s) / (C U_c^2), both times dice_weight * grad_scale,
//                               and ce_scale = ce_weight * grad_scale / n_valid;
//   head_ce_dice_grp_kernel     head_ce_grp_kernel's forward + backward products with the per-pixel gradient
//                               dz_c = p_c (ce_scale + beta_c - q) - [c = y] (ce_scale + alpha_y p_y),  q = sum_k p_k beta_k - alpha_y p_y,
//                               0 where the pixel is not counted; then head_finish_kernel's fixed-order gather of the slabs.
// Kernels of their own, so that the instantiations of head_ce_grp_kernel / head_px_grp_kernel compile to what they were.  No
// read-modify-write atomics: lane exchange, then LDS rows summed in wave order, then slabs summed in block order.
struct DiceArgs {
  float* ws_stat;      // [blocks][3][cq]: I, P (fp32) and T (int32 bits) of the block's counted pixels
  float* ws_part;      // [blocks][2]: sum of the per-pixel CE (fp32), counted pixels (int32 bits)
};

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 && TN <= 10 ? 2 : 1)) void head_dice_stats_grp_kernel(HeadArgs p, DiceArgs d) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int G = HT / S;
  constexpr int F4 = G + NT - 1;
  constexpr int NQ = NT * NT / 4;
  constexpr int UPG = S * S / 16;
  constexpr int NCH = 16 * TN;                   // channels the tiles cover (>= cq)
  constexpr int NW = HEAD_THREADS / 64;
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
  float* s_st = (float*)(s_lab + HT * HT);       // [waves][I | P][NCH]
  __shared__ float s_ls[NW];
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
      const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
      if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
    }
    s_lab[tid] = code;
  }
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  constexpr float LOG2E = 1.4426950408889634f;
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  float accI[TN], accP[TN];   // channel 16 t + m over this lane's pixels
#pragma unroll
  for (int t = 0; t < TN; ++t) accI[t] = accP[t] = 0.f;
  float loss_acc = 0.f;

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    const int u = 2 * wid + g2, gi = u / UPG, rt = u % UPG, gy = gi / G, gx = gi % G;
    const int Yb = Y0 + S * gy, Xb = X0 + S * gx;
    const int prow = rt * (16 / S);
    const bool active = !(Yb + prow >= p.H || Xb >= p.W || Yb + prow + 16 / S - 1 < 0 || Xb + S - 1 < 0);  // wave-uniform
    if (!active) continue;
    const int gbase = (gy * F4 + gx) * CS;
    const int py_m = prow + m / S, px_m = m % S;
    float Af[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % NT);
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
#pragma unroll
    for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : -1;
    float mx[4] = {NEG, NEG, NEG, NEG}, sum[4] = {0.f, 0.f, 0.f, 0.f}, zy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C (a counted label is below C: never selected there)
        if (16 * t + m >= p.C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[r] = fmaxf(mx[r], acc[t][r]);
        zy[r] += dl[r] == 16 * t ? acc[t][r] : 0.f;
      }
    }
    float mxl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); mxl[r] = -mx[r] * LOG2E; }
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

// One block.  Thread (slice, c) sums a quarter of the blocks' rows for class c in block order, the four slices are added in slice
// order: a fixed order, in fp64 (as optim_ctrl_update_kernel sums its partials); T and the pixel count are integers.  Thread
// (slice, 255) does the same for the (CE sum, counted pixels) partials.  coef = alpha[cq] | beta[cq] | ce_scale, 0, 0, 0.
struct DiceCoefArgs {
  const float* ws_stat; const float* ws_part;
  int nblk, C, cq;
  float ce_weight, dice_weight, smooth, grad_scale;
  int present_only;
  float* coef;          // [2 cq + 4]
  float* loss_out;      // [4]: total, CE mean, Dice, n_valid
  float* class_stats;   // [3][ld_stats]: I, P, T (zeros past C) or null
  int ld_stats;
};

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

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_ce_dice_grp_kernel(HeadArgs p, const float* __restrict__ coef) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int G = HT / S;
  constexpr int F4 = G + NT - 1;
  constexpr int NQ = NT * NT / 4;
  constexpr int UPG = S * S / 16;
  constexpr bool SUMD = UPG > 1;
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
  float* s_dlo = s_lo + F4 * F4 * CS;
  int* s_lab = (int*)(s_dlo + F4 * F4 * CS);
  float* s_ab = (float*)(s_lab + HT * HT);       // [alpha | beta][CMAX], zero past C: staged once per block
  const int fsize = F4 * F4 * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    int ry = a0 - OFF + cell / F4, rx = b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > p.h - 1 ? p.h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > p.w - 1 ? p.w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(p.lo + (((size_t)b * p.h + ry) * p.w + rx) * p.ld + c);
    *reinterpret_cast<float4*>(s_dlo + cell * CS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid < HT * HT) {
    const int Y = Y0 + (tid >> 4), X = X0 + (tid & 15);
    int code = -2;
    if (Y >= 0 && X >= 0 && Y < p.H && X < p.W) {
      code = -1;
      const int64_t lab64 = p.labels[((size_t)b * p.H + Y) * p.W + X];
      if (lab64 != (int64_t)p.ignore_index && lab64 >= 0 && lab64 < p.C) code = (int)lab64;
    }
    s_lab[tid] = code;
  }
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
  int cell_off[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) cell_off[q] = (((4 * q + kq) / NT) * F4 + (4 * q + kq) % NT) * CS;
  float Af[NQ], Bb[4];
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
#pragma unroll
      for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : -1;
      float mx[4] = {NEG, NEG, NEG, NEG};
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        if (16 * t + 16 > p.C) {   // uniform: a tile with channels past C
          if (16 * t + m >= p.C) acc[t] = f32x4_t{NEG, NEG, NEG, NEG};
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], acc[t][r]);
      }
      float mxl[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); mxl[r] = -mx[r] * LOG2E; }
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
  {   // the mirror leaves as this block's slab: cells in footprint order, cq channels each, 16 bytes per lane
    const int q4 = p.cq >> 2;
    float* slab = p.ws_dlo + (size_t)blockIdx.x * (F4 * F4) * p.cq;
    for (int i = tid; i < F4 * F4 * q4; i += HEAD_THREADS) {
      const int cell = i / q4, c = (i % q4) * 4;
      *reinterpret_cast<float4*>(slab + (size_t)cell * p.cq + c) = *reinterpret_cast<const float4*>(s_dlo + cell * CS + c);
    }
  }
}

// dlo[b, y, x, :] = sum of the footprint cells that map to low-res cell (y, x), over the tiles that cover it, in a fixed order;
// loss_sum = sum of the blocks' partials in block order.  One wave per low-res cell (lane = channel quad), four cells per block.
// Tile t along an axis covers the unclamped low-res indices [G t - 1 - OFF, G t - 1 - OFF + F4); indices below 0 / above n - 1 are
// the clamped taps of the image border and belong to cell 0 / n - 1.
template <int MODE, int S>
__global__ __launch_bounds__(256) void head_finish_kernel(HeadArgs p, int nblk_main) {
  constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;
  constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;
  constexpr int G = HT / S;
  constexpr int F4 = G + NT - 1;
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

// ---- generic pieces for the drop-in (unfused) path -----------------------------------------------------
// softmax cross-entropy over NCHW fp32 logits: per-pixel lse + loss; backward writes dlogits NCHW.
// OPT = true: class weights cw (null = ones), label smoothing eps, per-pixel losses loss_px (null = none; 0 where not counted) and
// (backward) a per-pixel upstream gradient grad_px — the formulas of head_ce_grp_kernel's OPT variant.
struct CeOpts { const float* cw; float eps; float* loss_px; const float* grad_px; };

// ORDERED: out = per-block (loss, count) partials [gridDim.x][2], summed in a fixed order by ce_nchw_finish_kernel (the same bits
// every run).  Otherwise out = loss_sum, added into with float atomics (the workspace-less lc2is_ce_nchw_fwd / _opts entry points).
template <bool OPT, bool ORDERED>
__global__ __launch_bounds__(256) void ce_nchw_fwd_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels, float* lse,
                                                           float* out, int B, int C, size_t HW,
                                                           long ignore_index, CeOpts o) {
  const size_t total = (size_t)B * HW;
  float lacc = 0.f, cacc = 0.f;
  float wsum = 0.f;   // OPT: W = sum_c w_c
  if constexpr (OPT) {
    if (o.cw) { for (int c = 0; c < C; ++c) wsum += o.cw[c]; } else wsum = (float)C;
  }
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    float m = -__builtin_inff();
    for (int c = 0; c < C; ++c) m = fmaxf(m, base[(size_t)c * HW]);
    float s = 0.f, wz = 0.f;
    for (int c = 0; c < C; ++c) {
      const float z = base[(size_t)c * HW];
      s += __expf(z - m);
      if constexpr (OPT) wz += (o.cw ? o.cw[c] : 1.f) * z;
    }
    const float l = m + __logf(s);
    if (lse) lse[i] = l;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    if constexpr (OPT) {
      float li = 0.f;
      if (counted) {
        const float wy = o.cw ? o.cw[lab] : 1.f;
        li = (1.f - o.eps) * wy * (l - base[(size_t)lab * HW]) + (o.eps / (float)C) * (wsum * l - wz);
        lacc += li;
        cacc += wy;
      }
      if (o.loss_px) o.loss_px[i] = li;
    } else if (counted) {
      lacc += l - base[(size_t)lab * HW];
      cacc += 1.f;
    }
  }
  lacc = wave_sum(lacc);
  cacc = wave_sum(cacc);
  if constexpr (ORDERED) {
    __shared__ float red[2][4];
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = lacc;
      red[1][threadIdx.x >> 6] = cacc;
    }
    __syncthreads();
    if (threadIdx.x < 2)
      out[2 * blockIdx.x + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
  } else if ((threadIdx.x & 63) == 0 && (OPT ? lacc != 0.f || cacc != 0.f : cacc > 0.f)) {
    atomicAdd(out, lacc);
    atomicAdd(out + 1, cacc);
  }
}

// loss_sum[0..1] = the sums of ce_nchw_fwd_kernel's nblk block partials, in a fixed order (one block; overwrites loss_sum)
__global__ __launch_bounds__(256) void ce_nchw_finish_kernel(const float* __restrict__ part, int nblk, float* loss_sum) {
  float l = 0.f, c = 0.f;
  for (int k = threadIdx.x; k < nblk; k += 256) {
    l += part[2 * k];
    c += part[2 * k + 1];
  }
  l = wave_sum(l);
  c = wave_sum(c);
  __shared__ float red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = l;
    red[1][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    loss_sum[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

template <bool OPT>
__global__ __launch_bounds__(256) void ce_nchw_bwd_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ gscale_dev, float gscale,
                                                           float* dlogits, int B, int C, size_t HW,
                                                           long ignore_index, CeOpts o) {
  const size_t total = (size_t)B * HW;
  const float gs = gscale * (gscale_dev ? *gscale_dev : 1.f);
  float aw = 0.f;   // OPT: eps W / C
  if constexpr (OPT) {
    float wsum = 0.f;
    if (o.cw) { for (int c = 0; c < C; ++c) wsum += o.cw[c]; } else wsum = (float)C;
    aw = o.eps * wsum / (float)C;
  }
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    float* dbase = dlogits + b * C * HW + px;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    const float l = lse[i];
    if constexpr (OPT) {
      float cy = 0.f, cs = 0.f, g0 = 0.f;
      if (counted) {
        g0 = gs * (o.grad_px ? o.grad_px[i] : 1.f);
        cy = (1.f - o.eps) * (o.cw ? o.cw[lab] : 1.f);
        cs = cy + aw;
      }
      const float ac = o.eps / (float)C;
      for (int c = 0; c < C; ++c) {
        float g = 0.f;
        if (counted)
          g = g0 * (cs * __expf(base[(size_t)c * HW] - l) - (c == lab ? cy : 0.f) - ac * (o.cw ? o.cw[c] : 1.f));
        dbase[(size_t)c * HW] = g;
      }
    } else {
      for (int c = 0; c < C; ++c) {
        float g = 0.f;
        if (counted) g = gs * (__expf(base[(size_t)c * HW] - l) - (c == lab ? 1.f : 0.f));
        dbase[(size_t)c * HW] = g;
      }
    }
  }
}

// Focal / poly-1 CE on materialised NCHW logits (the drop-in module): head_focal_grp_kernel's per-pixel terms (focal_coef), a lane
// per pixel.  Forward: lse, the (sum of l_i, sum of w_y) block partials summed in a fixed order by ce_nchw_finish_kernel, and
// (optional) the per-pixel losses.  q is the sum of the other classes' exponentials over the full sum in both directions: the
// backward takes it from one more walk over the classes with the saved lse.  Kernels of their own: ce_nchw_*_kernel are untouched.
__global__ __launch_bounds__(256) void focal_nchw_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              float* lse, float* part, int B, int C, size_t HW, long ignore_index,
                                                              const float* __restrict__ cw, float* loss_px, FocalArgs f) {
  const size_t total = (size_t)B * HW;
  float lacc = 0.f, cacc = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    float m = -__builtin_inff();
    for (int c = 0; c < C; ++c) m = fmaxf(m, base[(size_t)c * HW]);
    float so = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = __expf(base[(size_t)c * HW] - m);
      so += (counted && c == lab) ? 0.f : e;
    }
    const float zy = counted ? base[(size_t)lab * HW] : 0.f;
    const float ey = counted ? __expf(zy - m) : 0.f;
    const float sum = so + ey;
    const float lsum = __logf(sum);
    if (lse) lse[i] = m + lsum;
    float li = 0.f;
    if (counted) {
      const float wy = cw ? cw[lab] : 1.f;
      focal_coef(ey / sum, so / sum, (m - zy) + lsum, f, &li);
      li *= wy;
      lacc += li;
      cacc += wy;
    }
    if (loss_px) loss_px[i] = li;
  }
  lacc = wave_sum(lacc);
  cacc = wave_sum(cacc);
  __shared__ float red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lacc;
    red[1][threadIdx.x >> 6] = cacc;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    part[2 * blockIdx.x + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ __launch_bounds__(256) void focal_nchw_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ lse, const float* __restrict__ gscale_dev,
                                                              float gscale, const float* __restrict__ grad_px, float* dlogits, int B,
                                                              int C, size_t HW, long ignore_index, const float* __restrict__ cw,
                                                              FocalArgs f) {
  const size_t total = (size_t)B * HW;
  const float gs = gscale * (gscale_dev ? *gscale_dev : 1.f);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    float* dbase = dlogits + b * C * HW + px;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    if (!counted) {
      for (int c = 0; c < C; ++c) dbase[(size_t)c * HW] = 0.f;
      continue;
    }
    const float l = lse[i];
    float q = 0.f;   // sum of the other classes' probabilities
    for (int c = 0; c < C; ++c) q += c == lab ? 0.f : __expf(base[(size_t)c * HW] - l);
    const float zy = base[(size_t)lab * HW];
    float li;
    const float coef = gs * (grad_px ? grad_px[i] : 1.f) * (cw ? cw[lab] : 1.f) * focal_coef(__expf(zy - l), q, l - zy, f, &li);
    for (int c = 0; c < C; ++c) dbase[(size_t)c * HW] = c == lab ? -coef * q : coef * __expf(base[(size_t)c * HW] - l);
  }
}

// Sigmoid cross-entropy / sigmoid focal loss on materialised NCHW logits (the drop-in modules): head_sigmoid_grp_kernel's element
// terms (sigmoid_elem), a lane per pixel walking its C classes.  Forward: the (sum of l_i, number of counted pixels) block partials,
// summed in a fixed order by ce_nchw_finish_kernel, and (optional) the per-pixel losses.  Nothing is saved for the backward: no lse.
__global__ __launch_bounds__(256) void sigmoid_focal_nchw_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                      float* part, int B, int C, size_t HW, long ignore_index,
                                                                      const float* __restrict__ cw, float* loss_px, SigmoidArgs f) {
  const size_t total = (size_t)B * HW;
  float lacc = 0.f, cacc = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    float li = 0.f;
    if (counted) {
      for (int c = 0; c < C; ++c) {
        float le;
        if (f.gamma != 0.f) sigmoid_elem<true>(base[(size_t)c * HW], c == lab, f, &le);
        else sigmoid_elem<false>(base[(size_t)c * HW], c == lab, f, &le);
        li = __builtin_fmaf((cw ? cw[c] : 1.f) * (c == lab ? f.cpos : f.cneg), le, li);
      }
      lacc += li;
      cacc += 1.f;
    }
    if (loss_px) loss_px[i] = li;
  }
  lacc = wave_sum(lacc);
  cacc = wave_sum(cacc);
  __shared__ float red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lacc;
    red[1][threadIdx.x >> 6] = cacc;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    part[2 * blockIdx.x + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ __launch_bounds__(256) void sigmoid_focal_nchw_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                      const float* __restrict__ gscale_dev, float gscale,
                                                                      const float* __restrict__ grad_px, float* dlogits, int B, int C,
                                                                      size_t HW, long ignore_index, const float* __restrict__ cw,
                                                                      SigmoidArgs f) {
  const size_t total = (size_t)B * HW;
  const float gs = gscale * (gscale_dev ? *gscale_dev : 1.f);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    float* dbase = dlogits + b * C * HW + px;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    if (!counted) {
      for (int c = 0; c < C; ++c) dbase[(size_t)c * HW] = 0.f;
      continue;
    }
    const float coef = gs * (grad_px ? grad_px[i] : 1.f);
    for (int c = 0; c < C; ++c) {
      float le;
      const float g = f.gamma != 0.f ? sigmoid_elem<true>(base[(size_t)c * HW], c == lab, f, &le)
                                     : sigmoid_elem<false>(base[(size_t)c * HW], c == lab, f, &le);
      dbase[(size_t)c * HW] = (coef * (cw ? cw[c] : 1.f) * (c == lab ? f.cpos : f.cneg)) * g;
    }
  }
}

// Dice + CE on materialised NCHW logits (the drop-in module): the two passes of the fused head, HBM-bound and plain, C <= CMAX.
// Pass 1: a lane owns a pixel (lse, CE); the class sums of a wave's 64 pixels are wave reductions (T: ballot popcounts) that lane 0
// adds to the wave's own LDS row; the block's rows are summed in wave order and leave as the block's slab, in the layout of
// head_dice_stats_grp_kernel: dice_coef_kernel serves both.
__global__ __launch_bounds__(256) void dice_nchw_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                               float* lse, DiceArgs d, int B, int C, int cq, size_t HW,
                                                               long ignore_index) {
  __shared__ float s_row[4][2][CMAX];
  __shared__ int s_cnt[4][CMAX];
  __shared__ float s_l[4];
  __shared__ int s_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int c = lane; c < CMAX; c += 64) { s_row[wid][0][c] = 0.f; s_row[wid][1][c] = 0.f; s_cnt[wid][c] = 0; }
  __syncthreads();
  const size_t total = (size_t)B * HW;
  float lacc = 0.f;
  int nacc = 0;   // wave-uniform
  for (size_t base = (size_t)blockIdx.x * 256; base < total; base += (size_t)gridDim.x * 256) {   // block-uniform trip count
    const size_t i = base + tid;
    const float* bp = logits;
    float l = 0.f;
    long lab = -1;
    bool counted = false;
    if (i < total) {
      const size_t b = i / HW, px = i % HW;
      bp = logits + b * C * HW + px;
      float m = -__builtin_inff();
      for (int c = 0; c < C; ++c) m = fmaxf(m, bp[(size_t)c * HW]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += __expf(bp[(size_t)c * HW] - m);
      l = m + __logf(s);
      if (lse) lse[i] = l;
      lab = (long)labels[i];
      counted = lab != ignore_index && lab >= 0 && lab < C;
      if (counted) lacc += l - bp[(size_t)lab * HW];
    }
    const unsigned long long cm = __ballot(counted);
    if (cm == 0ull) continue;   // wave-uniform
    nacc += __popcll(cm);
    for (int c = 0; c < C; ++c) {
      const float pr = counted ? __expf(bp[(size_t)c * HW] - l) : 0.f;
      const float ps = wave_sum(pr);
      const unsigned long long ym = __ballot(counted && lab == c);
      float is = 0.f;
      if (ym != 0ull) is = wave_sum(counted && lab == c ? pr : 0.f);   // wave-uniform branch
      if (lane == 0) {
        s_row[wid][1][c] += ps;
        if (ym != 0ull) { s_row[wid][0][c] += is; s_cnt[wid][c] += __popcll(ym); }
      }
    }
  }
  lacc = wave_sum(lacc);
  if (lane == 0) { s_l[wid] = lacc; s_n[wid] = nacc; }
  __syncthreads();
  if (tid < cq) {
    float* row = d.ws_stat + (size_t)blockIdx.x * 3 * cq;
    row[tid] = ((s_row[0][0][tid] + s_row[1][0][tid]) + s_row[2][0][tid]) + s_row[3][0][tid];
    row[cq + tid] = ((s_row[0][1][tid] + s_row[1][1][tid]) + s_row[2][1][tid]) + s_row[3][1][tid];
    reinterpret_cast<int*>(row)[2 * cq + tid] = ((s_cnt[0][tid] + s_cnt[1][tid]) + s_cnt[2][tid]) + s_cnt[3][tid];
  }
  if (tid == 255) {
    d.ws_part[2 * (size_t)blockIdx.x] = ((s_l[0] + s_l[1]) + s_l[2]) + s_l[3];
    reinterpret_cast<int*>(d.ws_part)[2 * (size_t)blockIdx.x + 1] = ((s_n[0] + s_n[1]) + s_n[2]) + s_n[3];
  }
}

// Pass 2: dlogits = gs * (p_c (ce_scale + beta_c - q) - [c = y] (ce_scale + alpha_y p_y)), 0 where the pixel is not counted; the
// coefficients (already times the weights and the host grad_scale) come from dice_coef_kernel's block.
__global__ __launch_bounds__(256) void dice_nchw_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                             const float* __restrict__ lse, const float* __restrict__ coef,
                                                             const float* __restrict__ gscale_dev, float gscale, float* dlogits,
                                                             int B, int C, int cq, size_t HW, long ignore_index) {
  const size_t total = (size_t)B * HW;
  const float gs = gscale * (gscale_dev ? *gscale_dev : 1.f);
  const float ces = coef[2 * cq];
  const float* alpha = coef;
  const float* beta = coef + cq;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, px = i % HW;
    const float* base = logits + b * C * HW + px;
    float* dbase = dlogits + b * C * HW + px;
    const long lab = (long)labels[i];
    const bool counted = lab != ignore_index && lab >= 0 && lab < C;
    if (!counted) {
      for (int c = 0; c < C; ++c) dbase[(size_t)c * HW] = 0.f;
      continue;
    }
    const float l = lse[i];
    float sb = 0.f;
    for (int c = 0; c < C; ++c) sb += __expf(base[(size_t)c * HW] - l) * beta[c];
    const float apy = alpha[lab] * __expf(base[(size_t)lab * HW] - l);
    const float k1 = ces - (sb - apy), oh = ces + apy;
    for (int c = 0; c < C; ++c)
      dbase[(size_t)c * HW] = gs * (__expf(base[(size_t)c * HW] - l) * (k1 + beta[c]) - (c == lab ? oh : 0.f));
  }
}

// Transposed upsample for the unfused path: dlo[b,y,x,c] = sum_{Y,X} wy(Y,y) wx(X,x) dhi[b,c,Y,X].
// grid (h, C, B), threads over x; each thread scans the <= 5S x 5S window of output pixels that can touch it.
template <int MODE>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float* __restrict__ dhi, float* dlo, int ld,
                                                            int h, int w, int C, int S) {
  const int y = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int H = h * S, W = w * S;
  const float inv_scale = 1.f / (float)S;
  const float* plane = dhi + ((size_t)b * C + c) * H * W;
  for (int x = threadIdx.x; x < w; x += 256) {
    float acc = 0.f;
    const int Y0 = max(0, S * (y - 2)), Y1 = min(H, S * (y + 3));
    const int X0 = max(0, S * (x - 2)), X1 = min(W, S * (x + 3));
    for (int Y = Y0; Y < Y1; ++Y) {
      const Taps ty = make_taps(Y, inv_scale, h, MODE);
      float wy = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) wy += (ty.idx[k] == y) ? ty.w[k] : 0.f;
      if (wy == 0.f) continue;
      float racc = 0.f;
      for (int X = X0; X < X1; ++X) {
        const Taps tx = make_taps(X, inv_scale, w, MODE);
        float wx = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) wx += (tx.idx[k] == x) ? tx.w[k] : 0.f;
        racc += wx * plane[(size_t)Y * W + X];
      }
      acc += wy * racc;
    }
    dlo[(((size_t)b * h + y) * w + x) * ld + c] = acc;
  }
}

}  // namespace

extern "C" int lc2is_upsample_bwd_nchw(const float* dhi, float* dlo, int ld, int B, int h, int w, int C, int S,
                                       int mode, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dhi || !dlo) return LC2IS_ERR_NULL;
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || ld < C || S < 1) return LC2IS_ERR_SHAPE;
  if (mode == LC2IS_INTERP_BICUBIC)
    hipLaunchKernelGGL(upsample_bwd_kernel<LC2IS_INTERP_BICUBIC>, dim3(h, C, B), dim3(256), 0, stream, dhi, dlo,
                       ld, h, w, C, S);
  else if (mode == LC2IS_INTERP_BILINEAR)
    hipLaunchKernelGGL(upsample_bwd_kernel<LC2IS_INTERP_BILINEAR>, dim3(h, C, B), dim3(256), 0, stream, dhi, dlo,
                       ld, h, w, C, S);
  else
    return LC2IS_ERR_UNSUPPORTED;
  return lc2is_check_launch();
}

namespace {
struct HeadGrpPlan { int f4, t4, cq; size_t loss_bytes, dlo_bytes; };
// the S = 4 / 8 / 16 group kernels: blocks per image, slab cell width, workspace split (loss partials first, 256-byte aligned slabs)
HeadGrpPlan head_grp_plan(int B, int h, int w, int C, int S, int mode, bool want_grad) {
  HeadGrpPlan g;
  g.f4 = head_grp_footprint(mode, S);
  const int H = h * S, W = w * S;
  g.t4 = ((H + S / 2 + HT - 1) / HT) * ((W + S / 2 + HT - 1) / HT);
  g.cq = (C + 3) & ~3;
  g.loss_bytes = ((size_t)B * g.t4 * 2 * sizeof(float) + 255) & ~(size_t)255;
  g.dlo_bytes = want_grad ? (size_t)B * g.t4 * g.f4 * g.f4 * g.cq * sizeof(float) : 0;
  return g;
}
}  // namespace

extern "C" size_t lc2is_head_upsample_ce_workspace_bytes(int B, int h, int w, int C, int S, int mode, int want_grad) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || !(S == 4 || S == 8 || S == 16)) return 0;   // other S: the atomic path, no workspace
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return 0;
  const HeadGrpPlan g = head_grp_plan(B, h, w, C, S, mode, want_grad != 0);
  return g.loss_bytes + g.dlo_bytes;
}

namespace {
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
    // channel tiles of 16 the kernel runs (tiles past C are masked): the smallest instantiation that covers C inside the row stride
    const int nt = (C + 15) / 16;
    const int tn = nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));
    const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
    const int f4 = gp.f4, t4 = gp.t4;
    const int lds4 = 2 * f4 * f4 * (ld + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) +
                     (opt ? CMAX * (int)sizeof(float) : 0);
    if (loss_sum) {   // loss / gradient leave through per-block partials and slabs: a workspace is part of the call
      if (!workspace || ((size_t)workspace & 15) || workspace_bytes < gp.loss_bytes + gp.dlo_bytes) return LC2IS_ERR_WORKSPACE;
      a.ws_loss = (float*)workspace;
      a.ws_dlo = dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr;
      a.cq = gp.cq;
    }
#define LC2IS_HEAD_GRP1(MODE_, TN_, S_, OPT_)                                                                                \
  do {                                                                                                                      \
    static DevOnce attr;                                                                                               \
    if (attr.need()) {                                                                                                            \
      if (hipFuncSetAttribute((const void*)head_ce_grp_kernel<MODE_, TN_, S_, OPT_>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                              2 * 7 * 7 * (CMAX + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) +             \
                                  (OPT_ ? CMAX * (int)sizeof(float) : 0)) != hipSuccess)                                    \
        return LC2IS_ERR_LAUNCH;                                                                                            \
      attr.done();                                                                                                          \
    }                                                                                                                       \
    hipLaunchKernelGGL((head_ce_grp_kernel<MODE_, TN_, S_, OPT_>), dim3(B * t4), dim3(HEAD_THREADS), lds4, stream, a);      \
  } while (0)
#define LC2IS_HEAD_GRP(MODE_, TN_, S_)                                                                                       \
  do {                                                                                                                      \
    if (opt) LC2IS_HEAD_GRP1(MODE_, TN_, S_, true); else LC2IS_HEAD_GRP1(MODE_, TN_, S_, false);                             \
  } while (0)
#define LC2IS_HEAD_GRP_TN(MODE_, S_)                                                                                         \
  do {                                                                                                                      \
    if (tn == 4) LC2IS_HEAD_GRP(MODE_, 4, S_); else if (tn == 8) LC2IS_HEAD_GRP(MODE_, 8, S_);                               \
    else if (tn == 10) LC2IS_HEAD_GRP(MODE_, 10, S_); else LC2IS_HEAD_GRP(MODE_, 12, S_);                                    \
  } while (0)
#define LC2IS_HEAD_GRP_S(MODE_)                                                                                              \
  do {                                                                                                                      \
    if (S == 4) LC2IS_HEAD_GRP_TN(MODE_, 4); else if (S == 8) LC2IS_HEAD_GRP_TN(MODE_, 8); else LC2IS_HEAD_GRP_TN(MODE_, 16); \
  } while (0)
    if (mode == LC2IS_INTERP_BICUBIC) LC2IS_HEAD_GRP_S(LC2IS_INTERP_BICUBIC);
    else LC2IS_HEAD_GRP_S(LC2IS_INTERP_BILINEAR);
#undef LC2IS_HEAD_GRP_S
#undef LC2IS_HEAD_GRP_TN
#undef LC2IS_HEAD_GRP
#undef LC2IS_HEAD_GRP1
    int rc = lc2is_check_launch();
    if (rc || !loss_sum) return rc;
    // second launch: fixed-order sums of the slabs (one wave per low-res cell) and of the loss partials
    const long ncell = dscores_lo ? (long)B * h * w : 1;
    const int fgrid = (int)((ncell + 3) / 4);
#define LC2IS_HEAD_FIN(MODE_, S_) hipLaunchKernelGGL((head_finish_kernel<MODE_, S_>), dim3(fgrid), dim3(256), 0, stream, a, B * t4)
    if (mode == LC2IS_INTERP_BICUBIC) { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 16); }
    else { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 16); }
#undef LC2IS_HEAD_FIN
    return lc2is_check_launch();
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

size_t ce_nchw_fwd_grid(int B, long HW) {
  size_t g = ((size_t)B * HW + 255) / 256;
  return g > 8192 ? 8192 : g;
}

// workspace != NULL: ordered sums, loss_sum overwritten; NULL: float atomics into loss_sum, which the caller clears
int ce_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px, int B, int C,
                long HW, long ignore_index, const float* class_weight, float label_smoothing, void* workspace,
                size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !loss_sum) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0) return LC2IS_ERR_SHAPE;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return LC2IS_ERR_SHAPE;
  const size_t g = ce_nchw_fwd_grid(B, HW);
  const bool ordered = workspace != nullptr;
  if (ordered && workspace_bytes < 2 * sizeof(float) * g) return LC2IS_ERR_WORKSPACE;
  float* out = ordered ? (float*)workspace : loss_sum;
  const CeOpts o{class_weight, label_smoothing, loss_px, nullptr};
  const bool opt = class_weight || label_smoothing != 0.f || loss_px;
#define LC2IS_CE_FWD(OPT_, ORD_) \
  hipLaunchKernelGGL((ce_nchw_fwd_kernel<OPT_, ORD_>), dim3((int)g), dim3(256), 0, stream, logits, labels, lse, out, B, C, \
                     (size_t)HW, ignore_index, o)
  if (ordered) {
    if (opt) LC2IS_CE_FWD(true, true); else LC2IS_CE_FWD(false, true);
  } else {
    if (opt) LC2IS_CE_FWD(true, false); else LC2IS_CE_FWD(false, false);
  }
#undef LC2IS_CE_FWD
  int rc = lc2is_check_launch();
  if (rc || !ordered) return rc;
  hipLaunchKernelGGL(ce_nchw_finish_kernel, dim3(1), dim3(256), 0, stream, out, (int)g, loss_sum);
  return lc2is_check_launch();
}

int ce_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev, float grad_scale,
                const float* grad_px, float* dlogits, int B, int C, long HW, long ignore_index, const float* class_weight,
                float label_smoothing, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !lse || !dlogits) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0) return LC2IS_ERR_SHAPE;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return LC2IS_ERR_SHAPE;
  size_t g = ((size_t)B * HW + 255) / 256;
  if (g > 8192) g = 8192;
  const CeOpts o{class_weight, label_smoothing, nullptr, grad_px};
  if (class_weight || label_smoothing != 0.f || grad_px)
    hipLaunchKernelGGL(ce_nchw_bwd_kernel<true>, dim3((int)g), dim3(256), 0, stream, logits, labels, lse, grad_scale_dev,
                       grad_scale, dlogits, B, C, (size_t)HW, ignore_index, o);
  else
    hipLaunchKernelGGL(ce_nchw_bwd_kernel<false>, dim3((int)g), dim3(256), 0, stream, logits, labels, lse, grad_scale_dev,
                       grad_scale, dlogits, B, C, (size_t)HW, ignore_index, o);
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
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if (((size_t)scores_lo | (size_t)loss_px) & 15) return LC2IS_ERR_SHAPE;
  if (!(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  const int H = h * S, W = w * S;
  HeadArgs a{scores_lo, ld, labels, nullptr, nullptr, nullptr, B, h, w, H, W, C, S, mode, ignore_index,
             0.f, nullptr, nullptr, 0, nullptr, 0.f};
  const int nt = (C + 15) / 16;
  const int tn = nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));   // head_upsample_ce's channel-tile counts
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, false);
  // the footprint and the tile's labels: at most 7 * 7 * 196 * 4 + 1024 bytes, inside the default dynamic LDS limit
  const int lds = gp.f4 * gp.f4 * (ld + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int);
#define LC2IS_HEAD_PX(MODE_, TN_, S_) \
  hipLaunchKernelGGL((head_px_grp_kernel<MODE_, TN_, S_>), dim3(B * gp.t4), dim3(HEAD_THREADS), lds, stream, a, loss_px)
#define LC2IS_HEAD_PX_TN(MODE_, S_)                                                                 \
  do {                                                                                              \
    if (tn == 4) LC2IS_HEAD_PX(MODE_, 4, S_); else if (tn == 8) LC2IS_HEAD_PX(MODE_, 8, S_);        \
    else if (tn == 10) LC2IS_HEAD_PX(MODE_, 10, S_); else LC2IS_HEAD_PX(MODE_, 12, S_);             \
  } while (0)
#define LC2IS_HEAD_PX_S(MODE_)                                                                                            \
  do {                                                                                                                    \
    if (S == 4) LC2IS_HEAD_PX_TN(MODE_, 4); else if (S == 8) LC2IS_HEAD_PX_TN(MODE_, 8); else LC2IS_HEAD_PX_TN(MODE_, 16); \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_HEAD_PX_S(LC2IS_INTERP_BICUBIC);
  else LC2IS_HEAD_PX_S(LC2IS_INTERP_BILINEAR);
#undef LC2IS_HEAD_PX_S
#undef LC2IS_HEAD_PX_TN
#undef LC2IS_HEAD_PX
  return lc2is_check_launch();
}

// ---- Dice + cross-entropy: host side ----
namespace {
struct DicePlan { HeadGrpPlan g; int nblk; size_t stat_bytes, part_bytes, coef_bytes; };
size_t dice_align(size_t n) { return (n + 255) & ~(size_t)255; }
// workspace: [I | P | T] rows, (CE sum, count) partials, the coefficient block, then (gradient) head_ce_grp_kernel's slabs
DicePlan dice_head_plan(int B, int h, int w, int C, int S, int mode, bool want_grad) {
  DicePlan d;
  d.g = head_grp_plan(B, h, w, C, S, mode, want_grad);
  d.nblk = B * d.g.t4;
  d.stat_bytes = dice_align((size_t)d.nblk * 3 * d.g.cq * sizeof(float));
  d.part_bytes = dice_align((size_t)d.nblk * 2 * sizeof(float));
  d.coef_bytes = dice_align((size_t)(2 * d.g.cq + 4) * sizeof(float));
  return d;
}
bool dice_weights_ok(float ce_weight, float dice_weight, float smooth, float grad_scale) {
  auto ok = [](float v) { return v >= 0.f && v <= 3.0e38f; };   // finite and not negative (a NaN fails both comparisons)
  return ok(ce_weight) && ok(dice_weight) && ok(smooth) && (ce_weight > 0.f || dice_weight > 0.f) && grad_scale == grad_scale;
}
int dice_nchw_grid(int B, long HW) {
  const size_t g = ((size_t)B * HW + 255) / 256;
  return (int)(g > 2048 ? 2048 : g);
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
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if (((size_t)scores_lo | (size_t)dscores_lo) & 15) return LC2IS_ERR_SHAPE;
  if (!dice_weights_ok(ce_weight, dice_weight, smooth, grad_scale)) return LC2IS_ERR_SHAPE;
  if (!(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  const DicePlan dp = dice_head_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!workspace || ((size_t)workspace & 15) ||
      workspace_bytes < dp.stat_bytes + dp.part_bytes + dp.coef_bytes + dp.g.dlo_bytes)
    return LC2IS_ERR_WORKSPACE;
  char* wsp = (char*)workspace;
  DiceArgs da{(float*)wsp, (float*)(wsp + dp.stat_bytes)};
  float* coef = (float*)(wsp + dp.stat_bytes + dp.part_bytes);
  const int H = h * S, W = w * S;
  HeadArgs a{scores_lo, ld, labels, dscores_lo, nullptr, nullptr, B, h, w, H, W, C, S, mode, ignore_index,
             1.f, nullptr, dscores_lo ? (float*)(wsp + dp.stat_bytes + dp.part_bytes + dp.coef_bytes) : nullptr, dp.g.cq,
             nullptr, 0.f};
  const int nt = (C + 15) / 16;
  const int tn = nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));   // head_upsample_ce's channel-tile counts
  const int f4 = dp.g.f4;
  // pass 1: the footprint, the tile's labels and the waves' [I | P] rows: at most 38 416 + 1 024 + 12 288 bytes of dynamic LDS
  const int lds1 = f4 * f4 * (ld + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) +
                   (HEAD_THREADS / 64) * 2 * 16 * tn * (int)sizeof(float);
  const int lds2 = 2 * f4 * f4 * (ld + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) + 2 * CMAX * (int)sizeof(float);
#define LC2IS_DICE_ST(MODE_, TN_, S_) \
  hipLaunchKernelGGL((head_dice_stats_grp_kernel<MODE_, TN_, S_>), dim3(dp.nblk), dim3(HEAD_THREADS), lds1, stream, a, da)
#define LC2IS_DICE_BW(MODE_, TN_, S_)                                                                                        \
  do {                                                                                                                      \
    static DevOnce attr;                                                                                                    \
    if (attr.need()) {                                                                                                      \
      if (hipFuncSetAttribute((const void*)head_ce_dice_grp_kernel<MODE_, TN_, S_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                              2 * 7 * 7 * (CMAX + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) +             \
                                  2 * CMAX * (int)sizeof(float)) != hipSuccess)                                             \
        return LC2IS_ERR_LAUNCH;                                                                                            \
      attr.done();                                                                                                          \
    }                                                                                                                       \
    hipLaunchKernelGGL((head_ce_dice_grp_kernel<MODE_, TN_, S_>), dim3(dp.nblk), dim3(HEAD_THREADS), lds2, stream, a, coef); \
  } while (0)
#define LC2IS_DICE_TN(K_, MODE_, S_)                                                      \
  do {                                                                                    \
    if (tn == 4) K_(MODE_, 4, S_); else if (tn == 8) K_(MODE_, 8, S_);                     \
    else if (tn == 10) K_(MODE_, 10, S_); else K_(MODE_, 12, S_);                          \
  } while (0)
#define LC2IS_DICE_S(K_, MODE_)                                                                                           \
  do {                                                                                                                    \
    if (S == 4) LC2IS_DICE_TN(K_, MODE_, 4); else if (S == 8) LC2IS_DICE_TN(K_, MODE_, 8); else LC2IS_DICE_TN(K_, MODE_, 16); \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_DICE_S(LC2IS_DICE_ST, LC2IS_INTERP_BICUBIC);
  else LC2IS_DICE_S(LC2IS_DICE_ST, LC2IS_INTERP_BILINEAR);
  int rc = lc2is_check_launch();
  if (rc) return rc;
  const DiceCoefArgs ca{da.ws_stat, da.ws_part, dp.nblk, C, dp.g.cq, ce_weight, dice_weight, smooth, grad_scale,
                        present_only != 0, coef, loss_out, class_stats, ld};
  hipLaunchKernelGGL(dice_coef_kernel, dim3(1), dim3(1024), 0, stream, ca);
  rc = lc2is_check_launch();
  if (rc || !dscores_lo) return rc;
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_DICE_S(LC2IS_DICE_BW, LC2IS_INTERP_BICUBIC);
  else LC2IS_DICE_S(LC2IS_DICE_BW, LC2IS_INTERP_BILINEAR);
#undef LC2IS_DICE_S
#undef LC2IS_DICE_TN
#undef LC2IS_DICE_BW
#undef LC2IS_DICE_ST
  rc = lc2is_check_launch();
  if (rc) return rc;
  // head_finish_kernel's fixed-order gather of the slabs (no loss partials: loss_sum is null)
  const int fgrid = (int)(((long)B * h * w + 3) / 4);
#define LC2IS_HEAD_FIN(MODE_, S_) hipLaunchKernelGGL((head_finish_kernel<MODE_, S_>), dim3(fgrid), dim3(256), 0, stream, a, dp.nblk)
  if (mode == LC2IS_INTERP_BICUBIC) { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 16); }
  else { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 16); }
#undef LC2IS_HEAD_FIN
  return lc2is_check_launch();
}

extern "C" size_t lc2is_ce_dice_nchw_workspace_bytes(int B, int C, long HW) {
  if (B <= 0 || C <= 0 || C > CMAX || HW <= 0) return 0;
  const int cq = (C + 3) & ~3;
  const size_t g = (size_t)dice_nchw_grid(B, HW);
  return dice_align(g * 3 * cq * sizeof(float)) + dice_align(g * 2 * sizeof(float));
}

extern "C" int lc2is_ce_dice_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_out,
                                      float* class_stats, float* coef, int B, int C, long HW, long ignore_index,
                                      float ce_weight, float dice_weight, float smooth, int present_only, void* workspace,
                                      size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !loss_out || !coef) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0) return LC2IS_ERR_SHAPE;
  if (!dice_weights_ok(ce_weight, dice_weight, smooth, 1.f)) return LC2IS_ERR_SHAPE;
  if (C > CMAX) return LC2IS_ERR_UNSUPPORTED;
  const int cq = (C + 3) & ~3;
  const int g = dice_nchw_grid(B, HW);
  const size_t stat_bytes = dice_align((size_t)g * 3 * cq * sizeof(float));
  if (!workspace || ((size_t)workspace & 15) || workspace_bytes < stat_bytes + dice_align((size_t)g * 2 * sizeof(float)))
    return LC2IS_ERR_WORKSPACE;
  DiceArgs da{(float*)workspace, (float*)((char*)workspace + stat_bytes)};
  hipLaunchKernelGGL(dice_nchw_stats_kernel, dim3(g), dim3(256), 0, stream, logits, labels, lse, da, B, C, cq, (size_t)HW,
                     ignore_index);
  int rc = lc2is_check_launch();
  if (rc) return rc;
  const DiceCoefArgs ca{da.ws_stat, da.ws_part, g, C, cq, ce_weight, dice_weight, smooth, 1.f, present_only != 0,
                        coef, loss_out, class_stats, C};
  hipLaunchKernelGGL(dice_coef_kernel, dim3(1), dim3(1024), 0, stream, ca);
  return lc2is_check_launch();
}

extern "C" int lc2is_ce_dice_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* coef,
                                      const float* grad_scale_dev, float grad_scale, float* dlogits, int B, int C, long HW,
                                      long ignore_index, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !lse || !coef || !dlogits) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0) return LC2IS_ERR_SHAPE;
  if (C > CMAX) return LC2IS_ERR_UNSUPPORTED;
  size_t g = ((size_t)B * HW + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(dice_nchw_bwd_kernel, dim3((int)g), dim3(256), 0, stream, logits, labels, lse, coef, grad_scale_dev,
                     grad_scale, dlogits, B, C, (C + 3) & ~3, (size_t)HW, ignore_index);
  return lc2is_check_launch();
}

extern "C" int lc2is_ce_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, int B,
                                 int C, long HW, long ignore_index, lc2is_stream_t stream) {
  return ce_nchw_fwd(logits, labels, lse, loss_sum, nullptr, B, C, HW, ignore_index, nullptr, 0.f, nullptr, 0, stream);
}

extern "C" int lc2is_ce_nchw_fwd_opts(const float* logits, const int64_t* labels, float* lse, float* loss_sum,
                                      float* loss_px, int B, int C, long HW, long ignore_index,
                                      const float* class_weight, float label_smoothing, lc2is_stream_t stream) {
  return ce_nchw_fwd(logits, labels, lse, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, label_smoothing,
                     nullptr, 0, stream);
}

extern "C" size_t lc2is_ce_nchw_fwd_workspace_bytes(int B, long HW) {
  return B > 0 && HW > 0 ? 2 * sizeof(float) * ce_nchw_fwd_grid(B, HW) : 0;
}

extern "C" int lc2is_ce_nchw_fwd_ordered(const float* logits, const int64_t* labels, float* lse, float* loss_sum,
                                         float* loss_px, int B, int C, long HW, long ignore_index,
                                         const float* class_weight, float label_smoothing, void* workspace,
                                         size_t workspace_bytes, lc2is_stream_t stream) {
  if (!workspace) return LC2IS_ERR_NULL;
  return ce_nchw_fwd(logits, labels, lse, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, label_smoothing,
                     workspace, workspace_bytes, stream);
}

extern "C" int lc2is_ce_nchw_bwd(const float* logits, const int64_t* labels, const float* lse,
                                 const float* grad_scale_dev, float grad_scale, float* dlogits, int B, int C,
                                 long HW, long ignore_index, lc2is_stream_t stream) {
  return ce_nchw_bwd(logits, labels, lse, grad_scale_dev, grad_scale, nullptr, dlogits, B, C, HW, ignore_index, nullptr,
                     0.f, stream);
}

extern "C" int lc2is_ce_nchw_bwd_opts(const float* logits, const int64_t* labels, const float* lse,
                                      const float* grad_scale_dev, float grad_scale, const float* grad_px,
                                      float* dlogits, int B, int C, long HW, long ignore_index,
                                      const float* class_weight, float label_smoothing, lc2is_stream_t stream) {
  return ce_nchw_bwd(logits, labels, lse, grad_scale_dev, grad_scale, grad_px, dlogits, B, C, HW, ignore_index,
                     class_weight, label_smoothing, stream);
}

// ---- focal / poly-1 cross-entropy: host side ----
namespace {
// gamma in [0, inf), poly_eps >= -1 and finite (a NaN fails every comparison)
bool focal_args_ok(float gamma, float poly_eps) {
  return gamma >= 0.f && gamma <= 3.0e38f && poly_eps >= -1.f && poly_eps <= 3.0e38f;
}
}  // namespace

extern "C" int lc2is_head_upsample_focal(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                         float* loss_sum, int B, int h, int w, int C, int S, int mode, long ignore_index,
                                         float grad_scale, const float* class_weight, float gamma, float poly_eps,
                                         void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !labels || !loss_sum) return LC2IS_ERR_NULL;
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if (((size_t)scores_lo | (size_t)dscores_lo) & 15) return LC2IS_ERR_SHAPE;
  if (!focal_args_ok(gamma, poly_eps)) return LC2IS_ERR_SHAPE;
  if (!(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!workspace || ((size_t)workspace & 15) || workspace_bytes < gp.loss_bytes + gp.dlo_bytes) return LC2IS_ERR_WORKSPACE;
  const int H = h * S, W = w * S;
  HeadArgs a{scores_lo, ld, labels, dscores_lo, nullptr, loss_sum, B, h, w, H, W, C, S, mode, ignore_index,
             grad_scale, (float*)workspace, dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr, gp.cq,
             class_weight, 0.f};
  const FocalArgs fa{gamma, poly_eps};
  const int nt = (C + 15) / 16;
  const int tn = nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));   // head_upsample_ce's channel-tile counts
  const int f4 = gp.f4, t4 = gp.t4;
  // the footprint, its gradient mirror, the tile's labels and the class weights (the OPT variant's layout)
  const int lds = 2 * f4 * f4 * (ld + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) + CMAX * (int)sizeof(float);
#define LC2IS_FOCAL(MODE_, TN_, S_)                                                                                          \
  do {                                                                                                                      \
    static DevOnce attr;                                                                                                    \
    if (attr.need()) {                                                                                                      \
      if (hipFuncSetAttribute((const void*)head_focal_grp_kernel<MODE_, TN_, S_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                              2 * 7 * 7 * (CMAX + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) +             \
                                  CMAX * (int)sizeof(float)) != hipSuccess)                                                 \
        return LC2IS_ERR_LAUNCH;                                                                                            \
      attr.done();                                                                                                          \
    }                                                                                                                       \
    hipLaunchKernelGGL((head_focal_grp_kernel<MODE_, TN_, S_>), dim3(B * t4), dim3(HEAD_THREADS), lds, stream, a, fa);      \
  } while (0)
#define LC2IS_FOCAL_TN(MODE_, S_)                                                                \
  do {                                                                                          \
    if (tn == 4) LC2IS_FOCAL(MODE_, 4, S_); else if (tn == 8) LC2IS_FOCAL(MODE_, 8, S_);         \
    else if (tn == 10) LC2IS_FOCAL(MODE_, 10, S_); else LC2IS_FOCAL(MODE_, 12, S_);              \
  } while (0)
#define LC2IS_FOCAL_S(MODE_)                                                                                           \
  do {                                                                                                                \
    if (S == 4) LC2IS_FOCAL_TN(MODE_, 4); else if (S == 8) LC2IS_FOCAL_TN(MODE_, 8); else LC2IS_FOCAL_TN(MODE_, 16);   \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_FOCAL_S(LC2IS_INTERP_BICUBIC);
  else LC2IS_FOCAL_S(LC2IS_INTERP_BILINEAR);
#undef LC2IS_FOCAL_S
#undef LC2IS_FOCAL_TN
#undef LC2IS_FOCAL
  int rc = lc2is_check_launch();
  if (rc) return rc;
  // second launch: head_finish_kernel's fixed-order sums of the slabs (one wave per low-res cell) and of the loss partials
  const long ncell = dscores_lo ? (long)B * h * w : 1;
  const int fgrid = (int)((ncell + 3) / 4);
#define LC2IS_HEAD_FIN(MODE_, S_) hipLaunchKernelGGL((head_finish_kernel<MODE_, S_>), dim3(fgrid), dim3(256), 0, stream, a, B * t4)
  if (mode == LC2IS_INTERP_BICUBIC) { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 16); }
  else { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 16); }
#undef LC2IS_HEAD_FIN
  return lc2is_check_launch();
}

extern "C" int lc2is_focal_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px,
                                    int B, int C, long HW, long ignore_index, const float* class_weight, float gamma,
                                    float poly_eps, void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !loss_sum || !workspace) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0 || !focal_args_ok(gamma, poly_eps)) return LC2IS_ERR_SHAPE;
  const size_t g = ce_nchw_fwd_grid(B, HW);
  if (workspace_bytes < 2 * sizeof(float) * g) return LC2IS_ERR_WORKSPACE;
  hipLaunchKernelGGL(focal_nchw_fwd_kernel, dim3((int)g), dim3(256), 0, stream, logits, labels, lse, (float*)workspace, B, C,
                     (size_t)HW, ignore_index, class_weight, loss_px, FocalArgs{gamma, poly_eps});
  int rc = lc2is_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ce_nchw_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)workspace, (int)g, loss_sum);
  return lc2is_check_launch();
}

extern "C" int lc2is_focal_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev,
                                    float grad_scale, const float* grad_px, float* dlogits, int B, int C, long HW,
                                    long ignore_index, const float* class_weight, float gamma, float poly_eps,
                                    lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !lse || !dlogits) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0 || !focal_args_ok(gamma, poly_eps)) return LC2IS_ERR_SHAPE;
  size_t g = ((size_t)B * HW + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(focal_nchw_bwd_kernel, dim3((int)g), dim3(256), 0, stream, logits, labels, lse, grad_scale_dev, grad_scale,
                     grad_px, dlogits, B, C, (size_t)HW, ignore_index, class_weight, FocalArgs{gamma, poly_eps});
  return lc2is_check_launch();
}

// ---- sigmoid cross-entropy / sigmoid focal loss: host side ----
namespace {
// gamma in [0, inf); alpha <= 1 and not a NaN (any negative value: no alpha); class_scale in (0, inf) (a NaN fails every comparison)
bool sigmoid_args_ok(float gamma, float alpha, float class_scale) {
  return gamma >= 0.f && gamma <= 3.0e38f && alpha <= 1.f && class_scale > 0.f && class_scale <= 3.0e38f;
}
SigmoidArgs sigmoid_args(float gamma, float alpha, float class_scale) {
  const bool has = !(alpha < 0.f);
  return SigmoidArgs{gamma, -gamma * 1.4426950408889634f, class_scale * (has ? alpha : 1.f), class_scale * (has ? 1.f - alpha : 1.f)};
}
}  // namespace

extern "C" int lc2is_head_upsample_sigmoid(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                           float* loss_sum, int B, int h, int w, int C, int S, int mode, long ignore_index,
                                           float grad_scale, const float* class_weight, float gamma, float alpha,
                                           float class_scale, void* workspace, size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || !labels || !loss_sum) return LC2IS_ERR_NULL;
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if (((size_t)scores_lo | (size_t)dscores_lo) & 15) return LC2IS_ERR_SHAPE;
  if (!sigmoid_args_ok(gamma, alpha, class_scale)) return LC2IS_ERR_SHAPE;
  if (!(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, dscores_lo != nullptr);
  if (!workspace || ((size_t)workspace & 15) || workspace_bytes < gp.loss_bytes + gp.dlo_bytes) return LC2IS_ERR_WORKSPACE;
  const int H = h * S, W = w * S;
  HeadArgs a{scores_lo, ld, labels, dscores_lo, nullptr, loss_sum, B, h, w, H, W, C, S, mode, ignore_index,
             grad_scale, (float*)workspace, dscores_lo ? (float*)((char*)workspace + gp.loss_bytes) : nullptr, gp.cq,
             class_weight, 0.f};
  const SigmoidArgs sa = sigmoid_args(gamma, alpha, class_scale);
  const int nt = (C + 15) / 16;
  const int tn = nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));   // head_upsample_ce's channel-tile counts
  const int f4 = gp.f4, t4 = gp.t4;
  // the footprint, its gradient mirror, the tile's labels and the class weights (the OPT variant's layout)
  const int lds = 2 * f4 * f4 * (ld + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) + CMAX * (int)sizeof(float);
#define LC2IS_SIGM(MODE_, TN_, S_)                                                                                             \
  do {                                                                                                                        \
    static DevOnce attr;                                                                                                      \
    if (attr.need()) {                                                                                                        \
      if (hipFuncSetAttribute((const void*)head_sigmoid_grp_kernel<MODE_, TN_, S_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                              2 * 7 * 7 * (CMAX + HEAD_PAD) * (int)sizeof(float) + HT * HT * (int)sizeof(int) +               \
                                  CMAX * (int)sizeof(float)) != hipSuccess)                                                   \
        return LC2IS_ERR_LAUNCH;                                                                                              \
      attr.done();                                                                                                            \
    }                                                                                                                         \
    hipLaunchKernelGGL((head_sigmoid_grp_kernel<MODE_, TN_, S_>), dim3(B * t4), dim3(HEAD_THREADS), lds, stream, a, sa);      \
  } while (0)
#define LC2IS_SIGM_TN(MODE_, S_)                                                                 \
  do {                                                                                          \
    if (tn == 4) LC2IS_SIGM(MODE_, 4, S_); else if (tn == 8) LC2IS_SIGM(MODE_, 8, S_);           \
    else if (tn == 10) LC2IS_SIGM(MODE_, 10, S_); else LC2IS_SIGM(MODE_, 12, S_);                \
  } while (0)
#define LC2IS_SIGM_S(MODE_)                                                                                          \
  do {                                                                                                              \
    if (S == 4) LC2IS_SIGM_TN(MODE_, 4); else if (S == 8) LC2IS_SIGM_TN(MODE_, 8); else LC2IS_SIGM_TN(MODE_, 16);   \
  } while (0)
  if (mode == LC2IS_INTERP_BICUBIC) LC2IS_SIGM_S(LC2IS_INTERP_BICUBIC);
  else LC2IS_SIGM_S(LC2IS_INTERP_BILINEAR);
#undef LC2IS_SIGM_S
#undef LC2IS_SIGM_TN
#undef LC2IS_SIGM
  int rc = lc2is_check_launch();
  if (rc) return rc;
  // second launch: head_finish_kernel's fixed-order sums of the slabs (one wave per low-res cell) and of the loss partials
  const long ncell = dscores_lo ? (long)B * h * w : 1;
  const int fgrid = (int)((ncell + 3) / 4);
#define LC2IS_HEAD_FIN(MODE_, S_) hipLaunchKernelGGL((head_finish_kernel<MODE_, S_>), dim3(fgrid), dim3(256), 0, stream, a, B * t4)
  if (mode == LC2IS_INTERP_BICUBIC) { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BICUBIC, 16); }
  else { if (S == 4) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 4); else if (S == 8) LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 8); else LC2IS_HEAD_FIN(LC2IS_INTERP_BILINEAR, 16); }
#undef LC2IS_HEAD_FIN
  return lc2is_check_launch();
}

extern "C" int lc2is_sigmoid_focal_nchw_fwd(const float* logits, const int64_t* labels, float* loss_sum, float* loss_px, int B,
                                            int C, long HW, long ignore_index, const float* class_weight, float gamma,
                                            float alpha, float class_scale, void* workspace, size_t workspace_bytes,
                                            lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !loss_sum || !workspace) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0 || !sigmoid_args_ok(gamma, alpha, class_scale)) return LC2IS_ERR_SHAPE;
  const size_t g = ce_nchw_fwd_grid(B, HW);
  if (workspace_bytes < 2 * sizeof(float) * g) return LC2IS_ERR_WORKSPACE;
  hipLaunchKernelGGL(sigmoid_focal_nchw_fwd_kernel, dim3((int)g), dim3(256), 0, stream, logits, labels, (float*)workspace, B, C,
                     (size_t)HW, ignore_index, class_weight, loss_px, sigmoid_args(gamma, alpha, class_scale));
  int rc = lc2is_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ce_nchw_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)workspace, (int)g, loss_sum);
  return lc2is_check_launch();
}

extern "C" int lc2is_sigmoid_focal_nchw_bwd(const float* logits, const int64_t* labels, const float* grad_scale_dev,
                                            float grad_scale, const float* grad_px, float* dlogits, int B, int C, long HW,
                                            long ignore_index, const float* class_weight, float gamma, float alpha,
                                            float class_scale, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !dlogits) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0 || !sigmoid_args_ok(gamma, alpha, class_scale)) return LC2IS_ERR_SHAPE;
  size_t g = ((size_t)B * HW + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(sigmoid_focal_nchw_bwd_kernel, dim3((int)g), dim3(256), 0, stream, logits, labels, grad_scale_dev, grad_scale,
                     grad_px, dlogits, B, C, (size_t)HW, ignore_index, class_weight, sigmoid_args(gamma, alpha, class_scale));
  return lc2is_check_launch();
}
