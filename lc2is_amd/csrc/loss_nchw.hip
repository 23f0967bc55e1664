// Losses on materialised NCHW fp32 logits, and the transposed upsample: the drop-in (unfused) path (gfx950).
// The fused head (head.hip) shares nothing with these kernels but the element math of head_loss_math.h.
#include "common.h"
#include "head_loss_math.h"
#include "interp.h"
#include "lc2is_hip.h"

namespace {

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

// ---- Dice + cross-entropy ----
namespace {
int dice_nchw_grid(int B, long HW) {
  const size_t g = ((size_t)B * HW + 255) / 256;
  return (int)(g > 2048 ? 2048 : g);
}
}  // namespace

extern "C" size_t lc2is_ce_dice_nchw_workspace_bytes(int B, int C, long HW) {
  if (B <= 0 || C <= 0 || C > DICE_CMAX || HW <= 0) return 0;
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
  if (C > DICE_CMAX) return LC2IS_ERR_UNSUPPORTED;
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
  return lc2is_dice_coef_launch(ca, stream);
}

extern "C" int lc2is_ce_dice_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* coef,
                                      const float* grad_scale_dev, float grad_scale, float* dlogits, int B, int C, long HW,
                                      long ignore_index, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!logits || !labels || !lse || !coef || !dlogits) return LC2IS_ERR_NULL;
  if (B <= 0 || C <= 0 || HW <= 0) return LC2IS_ERR_SHAPE;
  if (C > DICE_CMAX) return LC2IS_ERR_UNSUPPORTED;
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

// ---- focal / poly-1 cross-entropy ----
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

// ---- sigmoid cross-entropy / sigmoid focal loss ----
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
