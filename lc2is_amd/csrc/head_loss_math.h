// Element math and small argument structs that the fused head (head.hip) and the drop-in NCHW losses (loss_nchw.hip) share.
// No kernel is defined here.
#pragma once
#include "common.h"

namespace {

// ---- focal / poly-1 cross-entropy ----
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

// gamma in [0, inf), poly_eps >= -1 and finite (a NaN fails every comparison)
bool focal_args_ok(float gamma, float poly_eps) {
  return gamma >= 0.f && gamma <= 3.0e38f && poly_eps >= -1.f && poly_eps <= 3.0e38f;
}

// ---- sigmoid cross-entropy / sigmoid focal loss ----
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

// gamma in [0, inf); alpha <= 1 and not a NaN (any negative value: no alpha); class_scale in (0, inf) (a NaN fails every comparison)
bool sigmoid_args_ok(float gamma, float alpha, float class_scale) {
  return gamma >= 0.f && gamma <= 3.0e38f && alpha <= 1.f && class_scale > 0.f && class_scale <= 3.0e38f;
}
SigmoidArgs sigmoid_args(float gamma, float alpha, float class_scale) {
  const bool has = !(alpha < 0.f);
  return SigmoidArgs{gamma, -gamma * 1.4426950408889634f, class_scale * (has ? alpha : 1.f), class_scale * (has ? 1.f - alpha : 1.f)};
}

// ---- Dice + cross-entropy: the statistics rows ----
constexpr int DICE_CMAX = 192;   // classes of the [I | P | T] rows: the fused head's CMAX (head_grp.h)
struct DiceArgs {
  float* ws_stat;      // [blocks][3][cq]: I, P (fp32) and T (int32 bits) of the block's counted pixels
  float* ws_part;      // [blocks][2]: sum of the per-pixel CE (fp32), counted pixels (int32 bits)
};

size_t dice_align(size_t n) { return (n + 255) & ~(size_t)255; }
bool dice_weights_ok(float ce_weight, float dice_weight, float smooth, float grad_scale) {
  auto ok = [](float v) { return v >= 0.f && v <= 3.0e38f; };   // finite and not negative (a NaN fails both comparisons)
  return ok(ce_weight) && ok(dice_weight) && ok(smooth) && (ce_weight > 0.f || dice_weight > 0.f) && grad_scale == grad_scale;
}

}  // namespace

// The launch between the two Dice passes (dice_coef_kernel, head.hip; loss_nchw.hip calls it too): coef = alpha[cq] | beta[cq] |
// ce_scale, 0, 0, 0 from the nblk blocks' statistics rows.  Returns lc2is_check_launch().
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
__attribute__((visibility("hidden"))) int lc2is_dice_coef_launch(const DiceCoefArgs& a, hipStream_t stream);
