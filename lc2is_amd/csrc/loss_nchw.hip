// Losses on materialised NCHW fp32 logits, and the transposed upsample: the drop-in (unfused) path (gfx950).
// The fused head (head.hip) shares nothing with these kernels but the element math of head_loss_math.h.  Among themselves the
// criteria share everything but their formulas: one pixel opener (nchw_pixel), one ordered pair reduce (pair_reduce_store), one
// forward walk and one backward walk over a criterion struct (CeCrit, FocalCrit, SigmoidCrit, DiceCrit), one argument check, one
// grid rule and one launcher per direction; the cross-entropy backward keeps its own one-loop walk (see ce_nchw_bwd_kernel).  The
// helpers are forced inline, take scalars and keep the expression order the kernels had as kernels of their own: the
// evaluation loss depends on their bits.
#include "common.h"
#include "head_loss_math.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

// ---- shared pieces -------------------------------------------------------------------------------------------------------------
// pixel i of [B][HW]: its offset in the NCHW tensors (class c at off + c HW), its label, and the one definition of "counted"
struct Pixel { size_t off; const float* base; long lab; bool counted; };

__device__ __forceinline__ Pixel nchw_pixel(const float* __restrict__ logits, const int64_t* __restrict__ labels, size_t i, int C,
                                            size_t HW, long ignore_index) {
  const size_t b = i / HW, px = i % HW;
  const size_t off = b * C * HW + px;
  const long lab = (long)labels[i];
  return Pixel{off, logits + off, lab, lab != ignore_index && lab >= 0 && lab < C};
}

__device__ __forceinline__ float nchw_max(const float* base, int C, size_t HW) {
  float m = -__builtin_inff();
  for (int c = 0; c < C; ++c) m = fmaxf(m, base[(size_t)c * HW]);
  return m;
}

// dst[0..1] = the block's sums of (a, b) in a fixed order: waves, then (r0 + r1) + (r2 + r3).  Every thread of the 256 calls it.
__device__ __forceinline__ void pair_reduce_store(float a, float b, float* dst) {
  a = wave_sum(a);
  b = wave_sum(b);
  __shared__ float red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    dst[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// ---- criteria ------------------------------------------------------------------------------------------------------------------
// A criterion gives the walks: LSE (it saves / takes a per-pixel lse); fwd_open / bwd_open, its per-block prologue; stat, what the
// forward needs of EVERY pixel (St::l = the lse); term, the loss l_i of a counted pixel and *wy, what it adds to the count; grad,
// the C gradients of a counted pixel, given g0 = grad_scale * grad_scale_dev * grad_px and the pixel's lse.  PX: its forward can
// write the per-pixel losses.  The struct holds scalars only: the criterion's per-class table `cw` (class weights, null = ones;
// Dice: the coefficient block) stays a `const float* __restrict__` parameter of the kernel and is handed to each method — as a
// struct member it loses the qualifier, and its wave-uniform reads cw[c] turn from scalar into per-lane loads (a variant that
// did so, not in the tree, measured the sigmoid kernels + 45 %: the last paragraph of profiles/nchw_refactor_ab.txt).
struct NoPrologue {
  __device__ __forceinline__ float fwd_open(const float*, int) const { return 0.f; }
  __device__ __forceinline__ float bwd_open(const float*, int) const { return 0.f; }
};

// softmax cross-entropy.  OPT = true: class weights and label smoothing eps, per-pixel losses and a per-pixel upstream gradient —
// the formulas of head_ce_grp_kernel's OPT variant.
template <bool OPT>
struct CeCrit {
  static constexpr bool LSE = true, PX = OPT;
  float eps;
  struct St { float l, wz; };
  __device__ __forceinline__ float fwd_open(const float* cw, int C) const {   // OPT: W = sum_c w_c
    float wsum = 0.f;
    if constexpr (OPT) {
      if (cw) { for (int c = 0; c < C; ++c) wsum += cw[c]; } else wsum = (float)C;
    }
    return wsum;
  }
  __device__ __forceinline__ float bwd_open(const float* cw, int C) const {   // OPT: eps W / C
    return OPT ? eps * fwd_open(cw, C) / (float)C : 0.f;
  }
  __device__ __forceinline__ St stat(const float* base, const float* cw, long, bool, int C, size_t HW) const {
    const float m = nchw_max(base, C, HW);
    float s = 0.f, wz = 0.f;
    for (int c = 0; c < C; ++c) {
      const float z = base[(size_t)c * HW];
      s += __expf(z - m);
      if constexpr (OPT) wz += (cw ? cw[c] : 1.f) * z;
    }
    return St{m + __logf(s), wz};
  }
  __device__ __forceinline__ float term(const float* base, const float* cw, long lab, int C, size_t HW, St s, float wsum,
                                        float* wy) const {
    if constexpr (OPT) {
      *wy = cw ? cw[lab] : 1.f;
      return (1.f - eps) * *wy * (s.l - base[(size_t)lab * HW]) + (eps / (float)C) * (wsum * s.l - s.wz);
    } else {
      *wy = 1.f;
      return s.l - base[(size_t)lab * HW];
    }
  }
};

// Focal / poly-1 CE: head_focal_grp_kernel's per-pixel terms (focal_coef).  q is the sum of the other classes' exponentials over
// the full sum in both directions: the backward takes it from one more walk over the classes with the saved lse.
struct FocalCrit : NoPrologue {
  static constexpr bool LSE = true, PX = true;
  FocalArgs f;
  struct St { float l, m, zy, ey, so, sum, lsum; };
  __device__ __forceinline__ St stat(const float* base, const float*, long lab, bool counted, int C, size_t HW) const {
    const float m = nchw_max(base, C, HW);
    float so = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = __expf(base[(size_t)c * HW] - m);
      so += (counted && c == lab) ? 0.f : e;
    }
    const float zy = counted ? base[(size_t)lab * HW] : 0.f;
    const float ey = counted ? __expf(zy - m) : 0.f;
    const float sum = so + ey;
    const float lsum = __logf(sum);
    return St{m + lsum, m, zy, ey, so, sum, lsum};
  }
  __device__ __forceinline__ float term(const float*, const float* cw, long lab, int, size_t, St s, float, float* wy) const {
    *wy = cw ? cw[lab] : 1.f;
    float li;
    focal_coef(s.ey / s.sum, s.so / s.sum, (s.m - s.zy) + s.lsum, f, &li);
    return li * *wy;
  }
  __device__ __forceinline__ void grad(const float* base, float* dbase, const float* cw, long lab, int C, size_t HW, float l,
                                       float g0, float) const {
    float q = 0.f;   // sum of the other classes' probabilities
    for (int c = 0; c < C; ++c) q += c == lab ? 0.f : __expf(base[(size_t)c * HW] - l);
    const float zy = base[(size_t)lab * HW];
    float li;
    const float coef = g0 * (cw ? cw[lab] : 1.f) * focal_coef(__expf(zy - l), q, l - zy, f, &li);
    for (int c = 0; c < C; ++c) dbase[(size_t)c * HW] = c == lab ? -coef * q : coef * __expf(base[(size_t)c * HW] - l);
  }
};

// Sigmoid cross-entropy / sigmoid focal loss: head_sigmoid_grp_kernel's element terms (sigmoid_elem), the pixel walking its C
// classes.  The count is the number of counted pixels.  Nothing is saved for the backward: no lse.
struct SigmoidCrit : NoPrologue {
  static constexpr bool LSE = false, PX = true;
  SigmoidArgs f;
  struct St { float l; };
  __device__ __forceinline__ St stat(const float*, const float*, long, bool, int, size_t) const { return St{0.f}; }
  __device__ __forceinline__ float term(const float* base, const float* cw, long lab, int C, size_t HW, St, float,
                                        float* wy) const {
    float li = 0.f;
    for (int c = 0; c < C; ++c) {
      float le;
      if (f.gamma != 0.f) sigmoid_elem<true>(base[(size_t)c * HW], c == lab, f, &le);
      else sigmoid_elem<false>(base[(size_t)c * HW], c == lab, f, &le);
      li = __builtin_fmaf((cw ? cw[c] : 1.f) * (c == lab ? f.cpos : f.cneg), le, li);
    }
    *wy = 1.f;
    return li;
  }
  __device__ __forceinline__ void grad(const float* base, float* dbase, const float* cw, long lab, int C, size_t HW, float,
                                       float g0, float) const {
    for (int c = 0; c < C; ++c) {
      float le;
      const float g = f.gamma != 0.f ? sigmoid_elem<true>(base[(size_t)c * HW], c == lab, f, &le)
                                     : sigmoid_elem<false>(base[(size_t)c * HW], c == lab, f, &le);
      dbase[(size_t)c * HW] = (g0 * (cw ? cw[c] : 1.f) * (c == lab ? f.cpos : f.cneg)) * g;
    }
  }
};

// Dice + CE, pass 2 (its forward is dice_nchw_stats_kernel): dlogits = gs * (p_c (ce_scale + beta_c - q) - [c = y] (ce_scale +
// alpha_y p_y)); the coefficients (already times the weights and the host grad_scale) come from dice_coef_kernel's block.
struct DiceCrit {
  static constexpr bool LSE = true;
  int cq;
  __device__ __forceinline__ float bwd_open(const float* coef, int) const { return coef[2 * cq]; }   // ce_scale
  __device__ __forceinline__ void grad(const float* base, float* dbase, const float* coef, long lab, int C, size_t HW, float l,
                                       float g0, float ces) const {
    const float* alpha = coef;
    const float* beta = coef + cq;
    float sb = 0.f;
    for (int c = 0; c < C; ++c) sb += __expf(base[(size_t)c * HW] - l) * beta[c];
    const float apy = alpha[lab] * __expf(base[(size_t)lab * HW] - l);
    const float k1 = ces - (sb - apy), oh = ces + apy;
    for (int c = 0; c < C; ++c)
      dbase[(size_t)c * HW] = g0 * (__expf(base[(size_t)c * HW] - l) * (k1 + beta[c]) - (c == lab ? oh : 0.f));
  }
};

// ---- the walks -----------------------------------------------------------------------------------------------------------------
struct Sums { float loss, count; };

// a lane per pixel, grid stride: lse (where the criterion has one), the per-pixel losses (optional; 0 where not counted) and the
// lane's (sum of l_i, sum of the counts)
template <class Crit>
__device__ __forceinline__ Sums nchw_fwd_walk(const float* __restrict__ logits, const int64_t* __restrict__ labels, float* lse,
                                              float* loss_px, int B, int C, size_t HW, long ignore_index,
                                              const float* __restrict__ cw, const Crit& crit) {
  const size_t total = (size_t)B * HW;
  float lacc = 0.f, cacc = 0.f;
  const float pro = crit.fwd_open(cw, C);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const Pixel p = nchw_pixel(logits, labels, i, C, HW, ignore_index);
    const typename Crit::St s = crit.stat(p.base, cw, p.lab, p.counted, C, HW);
    if constexpr (Crit::LSE) {
      if (lse) lse[i] = s.l;
    }
    float li = 0.f;
    if (p.counted) {
      float wy;
      li = crit.term(p.base, cw, p.lab, C, HW, s, pro, &wy);
      lacc += li;
      cacc += wy;
    }
    if constexpr (Crit::PX) {
      if (loss_px) loss_px[i] = li;
    }
  }
  return Sums{lacc, cacc};
}

// part = per-block (loss, count) partials [gridDim.x][2], summed in a fixed order by ce_nchw_finish_kernel (the same bits every run)
template <class Crit>
__global__ __launch_bounds__(256) void nchw_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        float* lse, float* part, float* loss_px, int B, int C, size_t HW,
                                                        long ignore_index, const float* __restrict__ cw, Crit crit) {
  const Sums s = nchw_fwd_walk(logits, labels, lse, loss_px, B, C, HW, ignore_index, cw, crit);
  pair_reduce_store(s.loss, s.count, part + 2 * blockIdx.x);
}

// The workspace-less lc2is_ce_nchw_fwd / _opts entry points, kept for the ABI: the same walk, added into loss_sum with float
// atomics (the caller clears it; not the same bits every run).
template <bool OPT>
__global__ __launch_bounds__(256) void ce_nchw_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           float* lse, float* loss_sum, float* loss_px, int B, int C, size_t HW,
                                                           long ignore_index, const float* __restrict__ cw, CeCrit<OPT> crit) {
  const Sums s = nchw_fwd_walk(logits, labels, lse, loss_px, B, C, HW, ignore_index, cw, crit);
  const float lacc = wave_sum(s.loss), cacc = wave_sum(s.count);
  if ((threadIdx.x & 63) == 0 && (OPT ? lacc != 0.f || cacc != 0.f : cacc > 0.f)) {
    atomicAdd(loss_sum, lacc);
    atomicAdd(loss_sum + 1, cacc);
  }
}

// loss_sum[0..1] = the sums of the forward's nblk block partials, in a fixed order (one block; overwrites loss_sum)
__global__ __launch_bounds__(256) void ce_nchw_finish_kernel(const float* __restrict__ part, int nblk, float* loss_sum) {
  float l = 0.f, c = 0.f;
  for (int k = threadIdx.x; k < nblk; k += 256) {
    l += part[2 * k];
    c += part[2 * k + 1];
  }
  pair_reduce_store(l, c, loss_sum);
}

// dlogits = gs * grad_px (null = ones) * d l_i / d logits, C zeros where the pixel is not counted
template <class Crit>
__global__ __launch_bounds__(256) void nchw_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        const float* __restrict__ lse, const float* __restrict__ gscale_dev,
                                                        float gscale, const float* __restrict__ grad_px, float* dlogits, int B,
                                                        int C, size_t HW, long ignore_index, const float* __restrict__ cw,
                                                        Crit crit) {
  const size_t total = (size_t)B * HW;
  const float gs = gscale * (gscale_dev ? *gscale_dev : 1.f);
  const float pro = crit.bwd_open(cw, C);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const Pixel p = nchw_pixel(logits, labels, i, C, HW, ignore_index);
    float* dbase = dlogits + p.off;
    if (!p.counted) {
      for (int c = 0; c < C; ++c) dbase[(size_t)c * HW] = 0.f;
      continue;
    }
    float l = 0.f;
    if constexpr (Crit::LSE) l = lse[i];
    crit.grad(p.base, dbase, cw, p.lab, C, HW, l, gs * (grad_px ? grad_px[i] : 1.f), pro);
  }
}

// The cross-entropy backward stays a kernel of its own, on the shared opener and prologue: its one store loop takes the zero of a
// pixel that is not counted through a select.  Under nchw_bwd_kernel's "zeros, continue" a wave that holds both kinds of pixel
// walks two store loops, and with a few labels >= C nearly every wave does: a variant of this file that put it on the template
// measured + 25 % at (32, 151, 128, 128) (the last paragraph of profiles/nchw_refactor_ab.txt; that variant is not in the tree).
// The criteria above pay that already: their counted pixels skip a class walk of exponentials.  `cw` is deliberately NOT
// __restrict__ here: the kernel keeps the code it had before the templates, when cw was a member of an options struct.
template <bool OPT>
__global__ __launch_bounds__(256) void ce_nchw_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse, const float* __restrict__ gscale_dev,
                                                           float gscale, const float* __restrict__ grad_px, float* dlogits, int B,
                                                           int C, size_t HW, long ignore_index, const float* cw, float eps) {
  const size_t total = (size_t)B * HW;
  const float gs = gscale * (gscale_dev ? *gscale_dev : 1.f);
  const float aw = CeCrit<OPT>{eps}.bwd_open(cw, C);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const Pixel p = nchw_pixel(logits, labels, i, C, HW, ignore_index);
    float* dbase = dlogits + p.off;
    const float l = lse[i];
    if constexpr (OPT) {
      float cy = 0.f, cs = 0.f, g0 = 0.f;
      if (p.counted) {
        g0 = gs * (grad_px ? grad_px[i] : 1.f);
        cy = (1.f - eps) * (cw ? cw[p.lab] : 1.f);
        cs = cy + aw;
      }
      const float ac = eps / (float)C;
      for (int c = 0; c < C; ++c) {
        float g = 0.f;
        if (p.counted)
          g = g0 * (cs * __expf(p.base[(size_t)c * HW] - l) - (c == p.lab ? cy : 0.f) - ac * (cw ? cw[c] : 1.f));
        dbase[(size_t)c * HW] = g;
      }
    } else {
      for (int c = 0; c < C; ++c) {
        float g = 0.f;
        if (p.counted) g = gs * (__expf(p.base[(size_t)c * HW] - l) - (c == p.lab ? 1.f : 0.f));
        dbase[(size_t)c * HW] = g;
      }
    }
  }
}

// Dice + CE on materialised NCHW logits (the drop-in module): the two passes of the fused head, HBM-bound and plain, C <= DICE_CMAX.
// Pass 1: a lane owns a pixel (lse, CE); the class sums of a wave's 64 pixels are wave reductions (T: ballot popcounts) that lane 0
// adds to the wave's own LDS row; the block's rows are summed in wave order and leave as the block's slab, in the layout of
// head_dice_stats_grp_kernel: dice_coef_kernel serves both.
__global__ __launch_bounds__(256) void dice_nchw_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                               float* lse, DiceArgs d, int B, int C, int cq, size_t HW,
                                                               long ignore_index) {
  __shared__ float s_row[4][2][DICE_CMAX];
  __shared__ int s_cnt[4][DICE_CMAX];
  __shared__ float s_l[4];
  __shared__ int s_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int c = lane; c < DICE_CMAX; c += 64) { s_row[wid][0][c] = 0.f; s_row[wid][1][c] = 0.f; s_cnt[wid][c] = 0; }
  __syncthreads();
  const size_t total = (size_t)B * HW;
  const CeCrit<false> ce{0.f};
  float lacc = 0.f;
  int nacc = 0;   // wave-uniform
  for (size_t base = (size_t)blockIdx.x * 256; base < total; base += (size_t)gridDim.x * 256) {   // block-uniform trip count
    const size_t i = base + tid;
    const float* bp = logits;
    float l = 0.f;
    long lab = -1;
    bool counted = false;
    if (i < total) {
      const Pixel p = nchw_pixel(logits, labels, i, C, HW, ignore_index);
      bp = p.base;
      lab = p.lab;
      counted = p.counted;
      const CeCrit<false>::St s = ce.stat(bp, nullptr, lab, counted, C, HW);
      l = s.l;
      if (lse) lse[i] = l;
      float one;
      if (counted) lacc += ce.term(bp, nullptr, lab, C, HW, s, 0.f, &one);
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

// ---- host side: one argument check, one grid rule, one launcher per direction -----------------------------------------------------
namespace {
// the refusals every entry point opens with: `pointers` = all its required pointers are there
int nchw_args(bool pointers, int B, int C, long HW) {
  if (!pointers) return LC2IS_ERR_NULL;
  return B <= 0 || C <= 0 || HW <= 0 ? LC2IS_ERR_SHAPE : 0;
}

// a block per 256 pixels up to `cap`: 8192, 2048 for the Dice statistics (a slab per block); past it the walks stride
size_t nchw_grid(int B, long HW, size_t cap) {
  const size_t g = ((size_t)B * HW + 255) / 256;
  return g > cap ? cap : g;
}

// ordered sums: the block partials go to the workspace, ce_nchw_finish_kernel overwrites loss_sum
template <class Crit>
int nchw_fwd_launch(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px, int B, int C, long HW,
                    long ignore_index, const float* cw, void* workspace, size_t workspace_bytes, lc2is_stream_t stream_, Crit crit) {
  hipStream_t stream = (hipStream_t)stream_;
  const size_t g = nchw_grid(B, HW, 8192);
  if (workspace_bytes < 2 * sizeof(float) * g) return LC2IS_ERR_WORKSPACE;
  hipLaunchKernelGGL(nchw_fwd_kernel<Crit>, dim3((int)g), dim3(256), 0, stream, logits, labels, lse, (float*)workspace, loss_px, B,
                     C, (size_t)HW, ignore_index, cw, crit);
  int rc = lc2is_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ce_nchw_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)workspace, (int)g, loss_sum);
  return lc2is_check_launch();
}

template <class Crit>
int nchw_bwd_launch(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev, float grad_scale,
                    const float* grad_px, float* dlogits, int B, int C, long HW, long ignore_index, const float* cw,
                    lc2is_stream_t stream_, Crit crit) {
  hipLaunchKernelGGL(nchw_bwd_kernel<Crit>, dim3((int)nchw_grid(B, HW, 8192)), dim3(256), 0, (hipStream_t)stream_, logits, labels,
                     lse, grad_scale_dev, grad_scale, grad_px, dlogits, B, C, (size_t)HW, ignore_index, cw, crit);
  return lc2is_check_launch();
}

// workspace != NULL: ordered sums, loss_sum overwritten; NULL: float atomics into loss_sum, which the caller clears
int ce_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px, int B, int C,
                long HW, long ignore_index, const float* class_weight, float label_smoothing, void* workspace,
                size_t workspace_bytes, lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && loss_sum, B, C, HW)) return rc;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return LC2IS_ERR_SHAPE;
  const bool opt = class_weight || label_smoothing != 0.f || loss_px;
  if (workspace && opt)
    return nchw_fwd_launch(logits, labels, lse, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, workspace, workspace_bytes,
                           stream, CeCrit<true>{label_smoothing});
  if (workspace)
    return nchw_fwd_launch(logits, labels, lse, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, workspace, workspace_bytes,
                           stream, CeCrit<false>{label_smoothing});
  const dim3 grid((int)nchw_grid(B, HW, 8192));
  if (opt)
    hipLaunchKernelGGL(ce_nchw_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, labels, lse, loss_sum, loss_px, B, C,
                       (size_t)HW, ignore_index, class_weight, CeCrit<true>{label_smoothing});
  else
    hipLaunchKernelGGL(ce_nchw_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, labels, lse, loss_sum, loss_px, B,
                       C, (size_t)HW, ignore_index, class_weight, CeCrit<false>{label_smoothing});
  return lc2is_check_launch();
}
}  // namespace

// ---- cross-entropy ----
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
  return B > 0 && HW > 0 ? 2 * sizeof(float) * nchw_grid(B, HW, 8192) : 0;
}

extern "C" int lc2is_ce_nchw_fwd_ordered(const float* logits, const int64_t* labels, float* lse, float* loss_sum,
                                         float* loss_px, int B, int C, long HW, long ignore_index,
                                         const float* class_weight, float label_smoothing, void* workspace,
                                         size_t workspace_bytes, lc2is_stream_t stream) {
  if (!workspace) return LC2IS_ERR_NULL;
  return ce_nchw_fwd(logits, labels, lse, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, label_smoothing,
                     workspace, workspace_bytes, stream);
}

// every option null / 0: the plain kernel, as lc2is_ce_nchw_bwd
extern "C" int lc2is_ce_nchw_bwd_opts(const float* logits, const int64_t* labels, const float* lse,
                                      const float* grad_scale_dev, float grad_scale, const float* grad_px,
                                      float* dlogits, int B, int C, long HW, long ignore_index,
                                      const float* class_weight, float label_smoothing, lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && lse && dlogits, B, C, HW)) return rc;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return LC2IS_ERR_SHAPE;
  const dim3 grid((int)nchw_grid(B, HW, 8192));
  if (class_weight || label_smoothing != 0.f || grad_px)
    hipLaunchKernelGGL(ce_nchw_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, labels, lse, grad_scale_dev,
                       grad_scale, grad_px, dlogits, B, C, (size_t)HW, ignore_index, class_weight, label_smoothing);
  else
    hipLaunchKernelGGL(ce_nchw_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, labels, lse, grad_scale_dev,
                       grad_scale, grad_px, dlogits, B, C, (size_t)HW, ignore_index, class_weight, label_smoothing);
  return lc2is_check_launch();
}

extern "C" int lc2is_ce_nchw_bwd(const float* logits, const int64_t* labels, const float* lse,
                                 const float* grad_scale_dev, float grad_scale, float* dlogits, int B, int C,
                                 long HW, long ignore_index, lc2is_stream_t stream) {
  return lc2is_ce_nchw_bwd_opts(logits, labels, lse, grad_scale_dev, grad_scale, nullptr, dlogits, B, C, HW, ignore_index, nullptr,
                                0.f, stream);
}

// ---- Dice + cross-entropy ----
extern "C" size_t lc2is_ce_dice_nchw_workspace_bytes(int B, int C, long HW) {
  if (B <= 0 || C <= 0 || C > DICE_CMAX || HW <= 0) return 0;
  const int cq = (C + 3) & ~3;
  const size_t g = nchw_grid(B, HW, 2048);
  return dice_align(g * 3 * cq * sizeof(float)) + dice_align(g * 2 * sizeof(float));
}

extern "C" int lc2is_ce_dice_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_out,
                                      float* class_stats, float* coef, int B, int C, long HW, long ignore_index,
                                      float ce_weight, float dice_weight, float smooth, int present_only, void* workspace,
                                      size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = nchw_args(logits && labels && loss_out && coef, B, C, HW)) return rc;
  if (!dice_weights_ok(ce_weight, dice_weight, smooth, 1.f)) return LC2IS_ERR_SHAPE;
  if (C > DICE_CMAX) return LC2IS_ERR_UNSUPPORTED;
  const int cq = (C + 3) & ~3;
  const int g = (int)nchw_grid(B, HW, 2048);
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
  return lc2is_dice_coef_launch(ca, stream);
}

extern "C" int lc2is_ce_dice_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* coef,
                                      const float* grad_scale_dev, float grad_scale, float* dlogits, int B, int C, long HW,
                                      long ignore_index, lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && lse && coef && dlogits, B, C, HW)) return rc;
  if (C > DICE_CMAX) return LC2IS_ERR_UNSUPPORTED;
  return nchw_bwd_launch(logits, labels, lse, grad_scale_dev, grad_scale, nullptr, dlogits, B, C, HW, ignore_index, coef, stream,
                         DiceCrit{(C + 3) & ~3});
}

// ---- focal / poly-1 cross-entropy ----
extern "C" int lc2is_focal_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px,
                                    int B, int C, long HW, long ignore_index, const float* class_weight, float gamma,
                                    float poly_eps, void* workspace, size_t workspace_bytes, lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && loss_sum && workspace, B, C, HW)) return rc;
  if (!focal_args_ok(gamma, poly_eps)) return LC2IS_ERR_SHAPE;
  return nchw_fwd_launch(logits, labels, lse, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, workspace, workspace_bytes,
                         stream, FocalCrit{{}, FocalArgs{gamma, poly_eps}});
}

extern "C" int lc2is_focal_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev,
                                    float grad_scale, const float* grad_px, float* dlogits, int B, int C, long HW,
                                    long ignore_index, const float* class_weight, float gamma, float poly_eps,
                                    lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && lse && dlogits, B, C, HW)) return rc;
  if (!focal_args_ok(gamma, poly_eps)) return LC2IS_ERR_SHAPE;
  return nchw_bwd_launch(logits, labels, lse, grad_scale_dev, grad_scale, grad_px, dlogits, B, C, HW, ignore_index, class_weight,
                         stream, FocalCrit{{}, FocalArgs{gamma, poly_eps}});
}

// ---- sigmoid cross-entropy / sigmoid focal loss ----
extern "C" int lc2is_sigmoid_focal_nchw_fwd(const float* logits, const int64_t* labels, float* loss_sum, float* loss_px, int B,
                                            int C, long HW, long ignore_index, const float* class_weight, float gamma,
                                            float alpha, float class_scale, void* workspace, size_t workspace_bytes,
                                            lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && loss_sum && workspace, B, C, HW)) return rc;
  if (!sigmoid_args_ok(gamma, alpha, class_scale)) return LC2IS_ERR_SHAPE;
  return nchw_fwd_launch(logits, labels, nullptr, loss_sum, loss_px, B, C, HW, ignore_index, class_weight, workspace,
                         workspace_bytes, stream, SigmoidCrit{{}, sigmoid_args(gamma, alpha, class_scale)});
}

extern "C" int lc2is_sigmoid_focal_nchw_bwd(const float* logits, const int64_t* labels, const float* grad_scale_dev,
                                            float grad_scale, const float* grad_px, float* dlogits, int B, int C, long HW,
                                            long ignore_index, const float* class_weight, float gamma, float alpha,
                                            float class_scale, lc2is_stream_t stream) {
  if (int rc = nchw_args(logits && labels && dlogits, B, C, HW)) return rc;
  if (!sigmoid_args_ok(gamma, alpha, class_scale)) return LC2IS_ERR_SHAPE;
  return nchw_bwd_launch(logits, labels, nullptr, grad_scale_dev, grad_scale, grad_px, dlogits, B, C, HW, ignore_index, class_weight,
                         stream, SigmoidCrit{{}, sigmoid_args(gamma, alpha, class_scale)});
}
