// The scaffolding that the group kernels of the fused head share (gfx950): head_ce_grp_kernel, head_px_grp_kernel,
// head_focal_grp_kernel, head_sigmoid_grp_kernel, head_dice_stats_grp_kernel, head_ce_dice_grp_kernel (head.hip) and
// head_argmax_grp_kernel (head_argmax.hip); head_wide.hip takes the interpolation and row primitives.  The tile, the LDS layout,
// the label / weight staging and the slab store serve every kernel; the other pieces serve the kernels whose register counts and
// occupancy they leave unchanged (head.hip says which), and the scheme all of them follow is described here, once.
//
// ---- the scheme: S = 4 / 8 / 16, bicubic (S = 4: the headline configuration) or bilinear (config-5 score map, AuxiliaryLoss) ----
// A block owns a 16x16 tile of OUTPUT pixels; the <= 7x7 low-res footprint of the tile is staged in LDS once and the gradient wrt
// the low-res scores is accumulated in an LDS mirror of the footprint.
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
// Bilinear's clamp of the source coordinate at 0 (torch) equals clamping the tap indices because the two clamped taps coincide.
//
// The groups of a tile overlap in every footprint cell (bicubic), and LDS float atomics retire about one LANE per three
// cycles per CU — 2 800 lane-adds per group made them 90 % of the first S = 4 kernel.  The waves take turns instead: plain
// 16-byte read-add-write of the transposed tiles (one cell per lane, four consecutive channels, conflict-free under the padded
// stride).  S = 4 bilinear footprints are 2 x 2 cells: the groups a pass runs on waves of equal (wid >> 1) & 1 sit two cells
// apart in both directions, so two turns per pass do.  S >= 8: a wave's two units are one group's, one round of turns per tile.
//
// The mirror leaves as the block's own SLAB of a workspace (plain stores) and head_finish_kernel sums, for every low-res cell, the
// footprint cells of the tiles that cover it in a FIXED order; the blocks' loss / count partials go the same way — no float atomics,
// the loss and the gradient are bitwise reproducible.
#pragma once
#include "common.h"
#include "interp.h"
#include "lc2is_hip.h"

#include <type_traits>

namespace {

constexpr int HT = 16;       // output tile edge
constexpr int FMAX = 8;       // max footprint edge for S >= 4 (16/S + 4 bicubic rows)
constexpr int HEAD_THREADS = 512;
constexpr int CMAX = 192;
constexpr int HEAD_PAD = 4;     // floats added to a footprint cell's LDS stride: the 16 cells of a group on different banks
constexpr float HEAD_LOG2E = 1.4426950408889634f;

constexpr int head_grp_footprint(int mode, int S) { return HT / S + (mode == LC2IS_INTERP_BICUBIC ? 4 : 2) - 1; }

// ---- geometry ----
template <int MODE, int S> struct HeadGrpGeom {
  static_assert(S == 4 || S == 8 || S == 16, "group kernel: S x S pixel groups inside a 16 x 16 tile");
  static constexpr int NT = (MODE == LC2IS_INTERP_BICUBIC) ? 4 : 2;   // taps per axis
  static constexpr int OFF = (MODE == LC2IS_INTERP_BICUBIC) ? 1 : 0;  // first tap = a - OFF
  static constexpr int G = HT / S;                                    // groups per tile edge
  static constexpr int F4 = G + NT - 1;                               // footprint edge
  static constexpr int NQ = NT * NT / 4;                              // k = 4 chunks of the forward product
  static constexpr int UPG = S * S / 16;                              // 16-pixel units per group (whole rows of the group: 16 / S rows each)
  static constexpr bool SUMD = UPG > 1;                               // a wave's two units belong to one group: their gradient tiles are summed
};

// the block's tile: image b, "floor" lo index (a0, b0) of its first group row / column, its first output pixel (Y0, X0)
struct HeadTile { int b, a0, b0, Y0, X0; };
template <int S> __device__ __forceinline__ HeadTile head_tile(int H, int W) {
  constexpr int G = HT / S;
  const int tiles_x = (W + S / 2 + HT - 1) / HT, tiles_y = (H + S / 2 + HT - 1) / HT;
  HeadTile T;
  T.b = blockIdx.x / (tiles_x * tiles_y);
  const int tyi = (blockIdx.x / tiles_x) % tiles_y, txi = blockIdx.x % tiles_x;
  T.a0 = G * tyi - 1; T.b0 = G * txi - 1;
  T.Y0 = S * T.a0 + S / 2; T.X0 = S * T.b0 + S / 2;
  return T;
}

// ---- interpolation and 16-lane row primitives ----
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
template <int CTRL> __device__ __forceinline__ int row_dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, row_dpp<0xB1>(v)); v = fmaxf(v, row_dpp<0x4E>(v)); v = fmaxf(v, row_dpp<0x141>(v));
  return fmaxf(v, row_dpp<0x140>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += row_dpp<0xB1>(v); v += row_dpp<0x4E>(v); v += row_dpp<0x141>(v);
  return v + row_dpp<0x140>(v);
}
// one exchange of (value, index) pairs: the larger value wins, equal values keep the lower index (a NaN never wins)
template <int CTRL> __device__ __forceinline__ void argmax_step(float& v, int& i) {
  const float ov = row_dpp<CTRL>(v);
  const int oi = row_dpp_i<CTRL>(i);
  const bool take = ov > v || (ov == v && oi < i);
  v = take ? ov : v;
  i = take ? oi : i;
}
__device__ __forceinline__ void row16_argmax(float& v, int& i) {   // every lane of the row ends with the row's winner
  argmax_step<0xB1>(v, i); argmax_step<0x4E>(v, i); argmax_step<0x141>(v, i); argmax_step<0x140>(v, i);
}

// ---- LDS layout ----
// Dynamic LDS of a group kernel, in 4-byte words from its start: the footprint s_lo [F4 * F4][ld + HEAD_PAD], the gradient mirror
// s_dlo of the same shape (kernels with a backward), the tile's labels s_lab [16][16], and behind them the kernel's own tail (class
// weights, Dice coefficients, statistics rows, class map + count rows).  The kernels and the host launch code both read it here.
struct HeadLds {
  int dlo, lab, tail;   // word offsets of s_dlo (= lab's when there is no mirror), s_lab and the tail
  constexpr __host__ __device__ int bytes(int tail_words) const { return (tail + tail_words) * 4; }
};
constexpr __host__ __device__ HeadLds head_grp_lds(int f4, int ld, bool has_mirror) {
  const int fp = f4 * f4 * (ld + HEAD_PAD);
  const int lab = has_mirror ? 2 * fp : fp;
  return HeadLds{fp, lab, lab + HT * HT};
}
// upper bound over every (mode, S, ld) a group kernel accepts: the 7 x 7 bicubic footprint of S = 4 at ld = CMAX
constexpr int head_grp_lds_max(bool has_mirror, int tail_words) { return head_grp_lds(7, CMAX, has_mirror).bytes(tail_words); }

// ---- staging ----
// the tile's footprint, tap indices clamped to the image, 16 bytes per lane; zero: the gradient mirror cleared beside it
template <int MODE, int S>
__device__ __forceinline__ void stage_footprint(float* s_lo, float* s_dlo, bool zero, const float* lo, int ld, int h, int w,
                                                const HeadTile& T, int tid) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int F4 = GM::F4, OFF = GM::OFF;
  const int Cp = ld, CS = Cp + HEAD_PAD;
  const int fsize = F4 * F4 * Cp;
  for (int i = tid * 4; i < fsize; i += HEAD_THREADS * 4) {
    const int cell = i / Cp, c = i % Cp;
    int ry = T.a0 - OFF + cell / F4, rx = T.b0 - OFF + cell % F4;
    ry = ry < 0 ? 0 : (ry > h - 1 ? h - 1 : ry);
    rx = rx < 0 ? 0 : (rx > w - 1 ? w - 1 : rx);
    *reinterpret_cast<float4*>(s_lo + cell * CS + c) =
        *reinterpret_cast<const float4*>(lo + (((size_t)T.b * h + ry) * w + rx) * ld + c);
    if (zero) *reinterpret_cast<float4*>(s_dlo + cell * CS + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// s_lab[16][16], one pixel per thread of the first 256: -2 outside the image, -1 not counted, else the label.
// MAYBE_NULL: labels may be null (a scores-only or pred-only call): every pixel inside the image is -1.
template <bool MAYBE_NULL>
__device__ __forceinline__ void stage_label(int* s_lab, const int64_t* labels, const HeadTile& T, int H, int W, int C,
                                            long ignore_index, int tid) {
  const int Y = T.Y0 + (tid >> 4), X = T.X0 + (tid & 15);
  int code = -2;
  if (Y >= 0 && X >= 0 && Y < H && X < W) {
    code = -1;
    if (!MAYBE_NULL || labels) {
      const int64_t lab64 = labels[((size_t)T.b * H + Y) * W + X];
      if (lab64 != (int64_t)ignore_index && lab64 >= 0 && lab64 < C) code = (int)lab64;
    }
  }
  s_lab[tid] = code;
}
template <bool MAYBE_NULL>
__device__ __forceinline__ void stage_labels(int* s_lab, const int64_t* labels, const HeadTile& T, int H, int W, int C,
                                             long ignore_index, int tid) {
  if (tid < HT * HT) stage_label<MAYBE_NULL>(s_lab, labels, T, H, W, C, ignore_index, tid);
}

// s_w[CMAX]: the class weights (ones without), zero past C
__device__ __forceinline__ void stage_weights(float* s_w, const float* cw, int C, int tid) {
  if (tid < CMAX) s_w[tid] = tid < C ? (cw ? cw[tid] : 1.f) : 0.f;
}

// ---- unit walk ----
// unit g2 (0 / 1) of wave wid: its group (gy, gx) of the tile, the group's first output pixel (Yb, Xb), the unit's first pixel row
// prow inside the group, the group's first cell in the footprint (gbase, floats), and this lane's four accumulator pixels
// 4 kq .. 4 kq + 3 of the unit: row py4 of the group, columns px4 .. px4 + 3.  active (wave-uniform): a pixel of the unit is inside.
struct HeadUnit { int gy, gx, Yb, Xb, prow, gbase, py4, px4; bool active; };
template <int MODE, int S>
__device__ __forceinline__ HeadUnit head_unit(const HeadTile& T, int g2, int wid, int kq, int CS, int H, int W) {
  using GM = HeadGrpGeom<MODE, S>;
  HeadUnit U;
  const int u = 2 * wid + g2, gi = u / GM::UPG, rt = u % GM::UPG;
  U.gy = gi / GM::G; U.gx = gi % GM::G;
  U.Yb = T.Y0 + S * U.gy; U.Xb = T.X0 + S * U.gx;
  U.prow = rt * (16 / S);
  U.active = !(U.Yb + U.prow >= H || U.Xb >= W || U.Yb + U.prow + 16 / S - 1 < 0 || U.Xb + S - 1 < 0);
  U.gbase = (U.gy * GM::F4 + U.gx) * CS;
  U.py4 = U.prow + (4 * kq) / S; U.px4 = (4 * kq) % S;
  return U;
}
// dl[r] = label - lane's channel offset: the label's class sits in tile t where dl == 16 t; `none` where the pixel is not counted
__device__ __forceinline__ void label_offsets(int (&dl)[4], const i32x4_t lab4, int m, int none) {
#pragma unroll
  for (int r = 0; r < 4; ++r) dl[r] = lab4[r] >= 0 ? lab4[r] - m : none;
}

// ---- operands and products ----
// LDS float offset of the forward cell 4q + kq, relative to the group's first cell
template <int MODE, int S, int NQ> __device__ __forceinline__ void make_cell_off(int (&cell_off)[NQ], int kq, int CS) {
  using GM = HeadGrpGeom<MODE, S>;
  static_assert(NQ == GM::NQ, "one offset per k = 4 chunk of the forward product");
#pragma unroll
  for (int q = 0; q < GM::NQ; ++q) cell_off[q] = (((4 * q + kq) / GM::NT) * GM::F4 + (4 * q + kq) % GM::NT) * CS;
}
// this lane's cell / channel quad in the transposed gradient tile
template <int MODE, int S> __device__ __forceinline__ int make_cellm_off(int m, int kq, int CS) {
  using GM = HeadGrpGeom<MODE, S>;
  return ((m / GM::NT) * GM::F4 + m % GM::NT) * CS + 4 * kq;
}
// forward A: row = pixel m of the unit, k = kq -> cell 4q + kq
template <int MODE, int S, int NQ>
__device__ __forceinline__ void make_fwd_operand(float (&Af)[NQ], int prow, int m, int kq) {
  using GM = HeadGrpGeom<MODE, S>;
  static_assert(NQ == GM::NQ, "one weight per k = 4 chunk of the forward product");
  const int py_m = prow + m / S, px_m = m % S;
#pragma unroll
  for (int q = 0; q < GM::NQ; ++q)
    Af[q] = tap_w<MODE, S>(py_m, (4 * q + kq) / GM::NT) * tap_w<MODE, S>(px_m, (4 * q + kq) % GM::NT);
}
// acc[t] = the unit's scores of channel tile t: Af x the footprint cells of the group, s_cell = s_lo + gbase + m
template <int TN, int NQ>
__device__ __forceinline__ void fwd_product(f32x4_t (&acc)[TN], const float* s_cell, const int (&cell_off)[NQ], const float (&Af)[NQ]) {
#pragma unroll
  for (int t = 0; t < TN; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float* bp = s_cell + cell_off[q];
    float bv[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) bv[t] = bp[16 * t];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Af[q], bv[t], acc[t], 0, 0, 0);
  }
}
// the transposed gradient tile of channel tile t from its dlogits gv: d[r] = channel 16 t + 4 kq + r of cell m.  SUMD: added to
// the group's running tile dsum[t]; otherwise it takes the place of acc[t]
template <bool SUMD, int TN, int ND>
__device__ __forceinline__ void bwd_product(const f32x4_t gv, const float (&Bb)[4], int t, f32x4_t (&acc)[TN], f32x4_t (&dsum)[ND]) {
  f32x4_t d = {0.f, 0.f, 0.f, 0.f};
  if constexpr (SUMD) d = dsum[t];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) d = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[jj], Bb[jj], d, 0, 0, 0);
  if constexpr (SUMD) dsum[t] = d; else acc[t] = d;
}

// ---- softmax steps ----
// a tile with channels at or past C (a uniform test first): those channels become `fill` (-inf for the softmax and the argmax,
// 0 for the sigmoid losses)
__device__ __forceinline__ void mask_past_c(f32x4_t& a, int t, int m, int C, float fill) {
  if (16 * t + 16 > C) {
    if (16 * t + m >= C) a = f32x4_t{fill, fill, fill, fill};
  }
}
// the row's maximum, and mxl = -max * log2(e): exp(x - max) = exp2(fma(x, log2(e), mxl))
__device__ __forceinline__ void row_max_mxl(float (&mx)[4], float (&mxl)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); mxl[r] = -mx[r] * HEAD_LOG2E; }
}

// ---- exit path: the slab layout is the contract with head_finish_kernel ----
// the mirror leaves as this block's slab: cells in footprint order, cq channels each, 16 bytes per lane
template <int MODE, int S> __device__ __forceinline__ void store_slab(const float* s_dlo, float* ws_dlo, int cq, int CS, int tid) {
  constexpr int F4 = HeadGrpGeom<MODE, S>::F4;
  const int q4 = cq >> 2;
  float* slab = ws_dlo + (size_t)blockIdx.x * (F4 * F4) * cq;
  for (int i = tid; i < F4 * F4 * q4; i += HEAD_THREADS) {
    const int cell = i / q4, c = (i % q4) * 4;
    *reinterpret_cast<float4*>(slab + (size_t)cell * cq + c) = *reinterpret_cast<const float4*>(s_dlo + cell * CS + c);
  }
}

// ---- host side: plan, checks, channel-tile count, dispatch, launch ----
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

// what the entry points of the group kernels check alike, behind their own null checks: shapes, the 16-byte alignment of the
// scores and of one more pointer (null passes), the loss's own scalars (args_ok), then S and the mode
int head_grp_check(const void* scores_lo, const void* aligned, bool args_ok, int B, int h, int w, int C, int ld, int S, int mode) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || ld < C || ld > CMAX || ld % 64) return LC2IS_ERR_SHAPE;
  if (((size_t)scores_lo | (size_t)aligned) & 15) return LC2IS_ERR_SHAPE;
  if (!args_ok) return LC2IS_ERR_SHAPE;
  if (!(S == 4 || S == 8 || S == 16)) return LC2IS_ERR_UNSUPPORTED;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return LC2IS_ERR_UNSUPPORTED;
  return LC2IS_OK;
}
bool head_ws_ok(const void* workspace, size_t workspace_bytes, size_t need) {
  return workspace && !((size_t)workspace & 15) && workspace_bytes >= need;
}

// channel tiles of 16 a kernel runs (tiles past C are masked): the smallest instantiation that covers C inside the row stride
inline int head_grp_tn(int C) {
  const int nt = (C + 15) / 16;
  return nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 10 ? 10 : 12));
}

template <int V> using HeadInt = std::integral_constant<int, V>;
// f(HeadInt<MODE>, HeadInt<TN>, HeadInt<S>) for the runtime (mode, S, tn); mode, S and tn are checked by the caller
template <class F> int head_grp_dispatch(int mode, int S, int tn, F&& f) {
  auto by_tn = [&](auto mode_, auto s_) {
    if (tn == 4) return f(mode_, HeadInt<4>{}, s_);
    if (tn == 8) return f(mode_, HeadInt<8>{}, s_);
    if (tn == 10) return f(mode_, HeadInt<10>{}, s_);
    return f(mode_, HeadInt<12>{}, s_);
  };
  auto by_s = [&](auto mode_) {
    if (S == 4) return by_tn(mode_, HeadInt<4>{});
    if (S == 8) return by_tn(mode_, HeadInt<8>{});
    return by_tn(mode_, HeadInt<16>{});
  };
  if (mode == LC2IS_INTERP_BICUBIC) return by_s(HeadInt<LC2IS_INTERP_BICUBIC>{});
  return by_s(HeadInt<LC2IS_INTERP_BILINEAR>{});
}

// One launch of a group kernel.  lds_max = the kernel's bound from head_grp_lds_max: past the default 64 KB limit of dynamic LDS the
// kernel's attribute is raised first, once per device and instantiation.
template <auto KERNEL, class... A>
int head_grp_launch(int lds_max, int nblk, int lds, hipStream_t stream, A... args) {
  if (lds_max > 64 * 1024) {
    static DevOnce attr;
    if (attr.need()) {
      if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess)
        return LC2IS_ERR_LAUNCH;
      attr.done();
    }
  }
  hipLaunchKernelGGL(KERNEL, dim3(nblk), dim3(HEAD_THREADS), lds, stream, args...);
  return lc2is_check_launch();
}

}  // namespace

// The finish launch of the group kernels that leave [loss, count] partials and gradient slabs (head_finish_kernel, head.hip), for
// the kernels of other translation units (head_selftrain.hip): loss_sum[2] = the nblk blocks' partials in block order, dlo
// [B, h, w, ld] = the slabs' cells in the fixed order (null: loss only).  Returns lc2is_check_launch().
struct HeadFinishArgs {
  float* dlo; float* loss_sum;
  float* ws_loss; float* ws_dlo;
  int B, h, w, C, ld, S, mode, cq, nblk;
};
__attribute__((visibility("hidden"))) int lc2is_head_finish_launch(const HeadFinishArgs& a, hipStream_t stream);
