// The device-held optimizer path of the train step (gfx950): the step-dependent scalars (learning rate, AdamW bias
// corrections, clip coefficient, the skip verdict) live in one small control block in device memory, so a step - eager or
// replayed from a captured graph - needs no host value that changes from call to call.
//   - grad_sumsq:        pass 1 over the flat gradient arena: one fp32 sum-of-squares partial and one non-finite flag per block
//   - optim_ctrl_update: one block: global norm, clip coefficient, verdict, lr table look-up, counters, bias corrections
//   - accum_add / optim_ctrl_update_accum: gradient accumulation - the cycle's loss sum and denominator in fp64 on the device,
//                        and the control update that divides the gradient scale by that denominator
//   - sgd / adamw _ctrl: sgd_kernel / adamw_kernel of misc.hip, expression for expression, scalars read from the block
//   - ema_ctrl / swap:   the weight EMA that follows the block's verdict and counter, and the in-place exchange that evaluates it
// Every reduction has a fixed order and there is no read-modify-write atomic: results are bitwise reproducible.
#include "common.h"
#include "lc2is_hip.h"

namespace {

constexpr int SUMSQ_MAX_GRID = 4096;

inline int sumsq_grid(size_t n) {
  size_t g = (n / 4 + 255) / 256;
  if (g > (size_t)SUMSQ_MAX_GRID) g = SUMSQ_MAX_GRID;
  if (g < 1) g = 1;
  return (int)g;
}

// One lane: s += x^2 over its float4s in ascending index order (one accumulator: 4 additions per float4); amax = the largest
// |x| bit pattern seen, so "an exponent field of all ones" (inf or NaN) is amax >= 0x7f800000 - exact, and independent of the
// sum, which can overflow on finite inputs.
__device__ __forceinline__ void sumsq_acc(const float4 v, float& s, unsigned& amax) {
  s += v.x * v.x; s += v.y * v.y; s += v.z * v.z; s += v.w * v.w;
  amax = max(amax, __float_as_uint(v.x) & 0x7fffffffu);
  amax = max(amax, __float_as_uint(v.y) & 0x7fffffffu);
  amax = max(amax, __float_as_uint(v.z) & 0x7fffffffu);
  amax = max(amax, __float_as_uint(v.w) & 0x7fffffffu);
}

// Grid-stride, 16 bytes per lane; plain cached loads (the optimizer reads the buffer next).  The loop is left to the compiler:
// a hand-unrolled form with four loads a grid stride (16 MB) apart in flight per lane ran at 3.7 TB/s against 6.1 TB/s for this
// one (631 MB buffer, profiles/optim_ctrl_cost.txt).
// Block sum: the 6-level DPP tree of wave_sum, then (w0 + w1) + (w2 + w3) by lane 0.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, size_t n4, float* __restrict__ partials,
                                                          unsigned* __restrict__ flags) {
  __shared__ float wsum[4];
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  float s = 0.f;
  unsigned amax = 0u;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) sumsq_acc(g4[i], s, amax);
  const float w = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
  const int bad = __syncthreads_or(amax >= 0x7f800000u);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    flags[blockIdx.x] = bad ? 1u : 0u;
  }
}

// beta^t by squaring in fp64 (<= 64 multiplications, error far under an fp32 ulp), rounded once to fp32: what the host's
// powf(beta, t) of lc2is_adamw_step returns.
__device__ __forceinline__ float pow_uint(float beta, unsigned t) {
  double p = 1.0, b = (double)beta;
  for (; t; t >>= 1) {
    if (t & 1u) p *= b;
    b *= b;
  }
  return (float)p;
}

// One block.  Lane k sums the k-th run of consecutive partials in index order (fp64), lane 0 adds the 256 run sums in index
// order and writes the whole control block.  Shared by the two control kernels below: ACCUM = false is the per-batch update
// (the gradient scale is grad_scale, widened exactly), ACCUM = true the update that closes a gradient-accumulation cycle (the
// scale is grad_scale over the cycle's denominator, formed in fp64; lane 0 alone reads the accumulation block, after the
// barrier, and rewrites it after the control block).  A divisor of exactly 1.0 leaves (double)grad_scale as it is, so both
// instantiations then write the same bits.
template <bool ACCUM>
__device__ __forceinline__ void optim_ctrl_update_body(lc2is_optim_ctrl* ctrl, lc2is_accum_block* block, int use_denom,
                                                       const float* __restrict__ partials,
                                                       const unsigned* __restrict__ flags, int nparts,
                                                       const float* __restrict__ lr_table, int table_len, float grad_scale,
                                                       float max_norm, int skip_nonfinite, float beta1, float beta2) {
  __shared__ double run_sum[256];
  __shared__ unsigned run_bad[256];
  const int per = (nparts + 255) / 256;
  const int lo = threadIdx.x * per, hi = min(lo + per, nparts);
  double s = 0.0;
  unsigned bad = 0u;
  for (int j = lo; j < hi; ++j) {
    s += (double)partials[j];
    bad |= flags[j];
  }
  run_sum[threadIdx.x] = s;
  run_bad[threadIdx.x] = bad;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot = 0.0;
  unsigned any_bad = 0u;
  for (int k = 0; k < 256; ++k) {
    tot += run_sum[k];
    any_bad |= run_bad[k];
  }
  double scale64 = (double)grad_scale;
  double loss_sum = 0.0, denom = 0.0;
  if (ACCUM) {
    loss_sum = block->loss_sum;
    denom = block->denom;
    // every pixel of the cycle ignored: the gradient is all zeros and the scale is taken as 1 (nothing turns into a NaN)
    const double d = use_denom ? (denom > 0.0 ? denom : 1.0) : 1.0;
    scale64 = (double)grad_scale / d;
  }
  const double norm64 = scale64 * sqrt(tot);
  const float norm = (float)norm64;
  // clip_grad_norm_: min(1, max_norm / (norm + 1e-6)), from the fp64 norm and rounded once; max_norm = +inf is "no clipping",
  // exactly 1 whatever the norm holds
  float coef = 1.f;
  if (max_norm < __builtin_huge_valf()) coef = (float)fmin(1.0, (double)max_norm / (norm64 + 1e-6));
  const int finite = any_bad ? 0 : 1;
  const int apply = (finite || !skip_nonfinite) ? 1 : 0;
  const int calls = ctrl->calls;
  ctrl->lr = lr_table[min(calls, table_len - 1)];
  ctrl->calls = calls + 1;
  ctrl->finite = finite;
  ctrl->apply = apply;
  ctrl->grad_norm = norm;
  ctrl->clip_coef = coef;
  ctrl->grad_mul = (float)scale64 * coef;
  if (apply) {
    const int t = ctrl->applied + 1;
    ctrl->applied = t;
    ctrl->bc1 = 1.f - pow_uint(beta1, (unsigned)t);
    ctrl->bc2 = 1.f - pow_uint(beta2, (unsigned)t);
  } else {
    ctrl->skipped = ctrl->skipped + 1;
  }
  if (ACCUM) {   // the cycle is closed: its mean (0 / 0 = NaN where nothing counted, torch's mean) and count stay readable
    block->last_loss = (float)(use_denom ? loss_sum / denom : loss_sum);
    block->last_denom = (float)denom;
    block->loss_sum = 0.0;
    block->denom = 0.0;
    block->micro = 0;
  }
}

__global__ __launch_bounds__(256) void optim_ctrl_update_kernel(lc2is_optim_ctrl* ctrl, const float* __restrict__ partials,
                                                                 const unsigned* __restrict__ flags, int nparts,
                                                                 const float* __restrict__ lr_table, int table_len,
                                                                 float grad_scale, float max_norm, int skip_nonfinite,
                                                                 float beta1, float beta2) {
  optim_ctrl_update_body<false>(ctrl, nullptr, 0, partials, flags, nparts, lr_table, table_len, grad_scale, max_norm,
                                skip_nonfinite, beta1, beta2);
}

__global__ __launch_bounds__(256) void optim_ctrl_update_accum_kernel(lc2is_optim_ctrl* ctrl, lc2is_accum_block* block,
                                                                       int use_denom, const float* __restrict__ partials,
                                                                       const unsigned* __restrict__ flags, int nparts,
                                                                       const float* __restrict__ lr_table, int table_len,
                                                                       float grad_scale, float max_norm, int skip_nonfinite,
                                                                       float beta1, float beta2) {
  optim_ctrl_update_body<true>(ctrl, block, use_denom, partials, flags, nparts, lr_table, table_len, grad_scale, max_norm,
                               skip_nonfinite, beta1, beta2);
}

// One micro-batch of a gradient-accumulation cycle: the head's [sum of losses, (weighted) count] joins the cycle's fp64 sums
// (fp32 stops counting exactly at 2^24 labels).  One lane, plain loads and stores, no atomics: the block is written by this
// launch and read by the next one on the same stream.
__global__ __launch_bounds__(64) void accum_add_kernel(lc2is_accum_block* block, const float* __restrict__ loss2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  block->loss_sum = block->loss_sum + (double)loss2[0];
  block->denom = block->denom + (double)loss2[1];
  block->micro = block->micro + 1;
}

// sgd_kernel of misc.hip with lr and the gradient multiplier read from the control block; `reverse` walks the arena from its
// end (element-wise: the same bits either way).
__global__ __launch_bounds__(256) void sgd_ctrl_kernel(float* p, const float* __restrict__ g, float* mom, size_t n4,
                                                        const lc2is_optim_ctrl* __restrict__ ctrl, float momentum, float wd,
                                                        int reverse) {
  if (!ctrl->apply) return;
  const float lr = ctrl->lr, gscale = ctrl->grad_mul;
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (size_t)gridDim.x * 256) {
    const size_t i = reverse ? n4 - 1 - j : j;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float d[4] = {gv.x * gscale + wd * pv.x, gv.y * gscale + wd * pv.y, gv.z * gscale + wd * pv.z,
                  gv.w * gscale + wd * pv.w};
    if (mom) {
      float4 mv = reinterpret_cast<float4*>(mom)[i];
      mv.x = momentum * mv.x + d[0]; mv.y = momentum * mv.y + d[1];
      mv.z = momentum * mv.z + d[2]; mv.w = momentum * mv.w + d[3];
      reinterpret_cast<float4*>(mom)[i] = mv;
      d[0] = mv.x; d[1] = mv.y; d[2] = mv.z; d[3] = mv.w;
    }
    pv.x -= lr * d[0]; pv.y -= lr * d[1]; pv.z -= lr * d[2]; pv.w -= lr * d[3];
    reinterpret_cast<float4*>(p)[i] = pv;
  }
}

__global__ __launch_bounds__(256) void adamw_ctrl_kernel(float* p, const float* __restrict__ g, float* m, float* v, size_t n4,
                                                          const lc2is_optim_ctrl* __restrict__ ctrl, float b1, float b2,
                                                          float eps, float wd, int reverse) {
  if (!ctrl->apply) return;
  const float lr = ctrl->lr, gscale = ctrl->grad_mul, bc1 = ctrl->bc1, bc2 = ctrl->bc2;
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (size_t)gridDim.x * 256) {
    const size_t i = reverse ? n4 - 1 - j : j;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = gp[k] * gscale;
      pp[k] *= (1.f - lr * wd);
      mp[k] = b1 * mp[k] + (1.f - b1) * gg;
      vp[k] = b2 * vp[k] + (1.f - b2) * gg * gg;
      const float denom = sqrtf(vp[k]) / sqrtf(bc2) + eps;
      pp[k] -= (lr / bc1) * (mp[k] / denom);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// Parameter groups: sgd_ctrl_kernel / adamw_ctrl_kernel, expression for expression, with lr = ctrl->lr * group.lr_scale (one fp32
// multiplication) and wd = group.weight_decay, the group being that of the 64-element granule the lane's float4 lies in
// (gmap: one byte per granule; float4 i lies in granule i >> 4, so 16 consecutive lanes share a byte).  The group table
// (<= 255 entries of 8 bytes) is staged in LDS once per block.  An id that names no table entry - 255 is the reserved one - makes
// the 16 lanes of the granule skip it: no load, no store.
__device__ __forceinline__ void stage_groups(float2* tab, const lc2is_param_group* __restrict__ groups, int ngroups) {
  if ((int)threadIdx.x < ngroups) {
    const lc2is_param_group e = groups[threadIdx.x];
    tab[threadIdx.x] = make_float2(e.lr_scale, e.weight_decay);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void sgd_groups_kernel(float* p, const float* __restrict__ g, float* mom, size_t n4,
                                                          const lc2is_optim_ctrl* __restrict__ ctrl,
                                                          const uint8_t* __restrict__ gmap,
                                                          const lc2is_param_group* __restrict__ groups, int ngroups,
                                                          float momentum, int reverse) {
  __shared__ float2 tab[256];
  if (!ctrl->apply) return;   // (uniform over the grid: no lane is left waiting at the barrier below)
  stage_groups(tab, groups, ngroups);
  const float lr0 = ctrl->lr, gscale = ctrl->grad_mul;
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (size_t)gridDim.x * 256) {
    const size_t i = reverse ? n4 - 1 - j : j;
    const unsigned gid = gmap[i >> 4];
    if (gid >= (unsigned)ngroups) continue;
    const float2 grp = tab[gid];
    const float lr = lr0 * grp.x, wd = grp.y;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float d[4] = {gv.x * gscale + wd * pv.x, gv.y * gscale + wd * pv.y, gv.z * gscale + wd * pv.z,
                  gv.w * gscale + wd * pv.w};
    if (mom) {
      float4 mv = reinterpret_cast<float4*>(mom)[i];
      mv.x = momentum * mv.x + d[0]; mv.y = momentum * mv.y + d[1];
      mv.z = momentum * mv.z + d[2]; mv.w = momentum * mv.w + d[3];
      reinterpret_cast<float4*>(mom)[i] = mv;
      d[0] = mv.x; d[1] = mv.y; d[2] = mv.z; d[3] = mv.w;
    }
    pv.x -= lr * d[0]; pv.y -= lr * d[1]; pv.z -= lr * d[2]; pv.w -= lr * d[3];
    reinterpret_cast<float4*>(p)[i] = pv;
  }
}

__global__ __launch_bounds__(256) void adamw_groups_kernel(float* p, const float* __restrict__ g, float* m, float* v, size_t n4,
                                                            const lc2is_optim_ctrl* __restrict__ ctrl,
                                                            const uint8_t* __restrict__ gmap,
                                                            const lc2is_param_group* __restrict__ groups, int ngroups,
                                                            float b1, float b2, float eps, int reverse) {
  __shared__ float2 tab[256];
  if (!ctrl->apply) return;
  stage_groups(tab, groups, ngroups);
  const float lr0 = ctrl->lr, gscale = ctrl->grad_mul, bc1 = ctrl->bc1, bc2 = ctrl->bc2;
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (size_t)gridDim.x * 256) {
    const size_t i = reverse ? n4 - 1 - j : j;
    const unsigned gid = gmap[i >> 4];
    if (gid >= (unsigned)ngroups) continue;
    const float2 grp = tab[gid];
    const float lr = lr0 * grp.x, wd = grp.y;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = gp[k] * gscale;
      pp[k] *= (1.f - lr * wd);
      mp[k] = b1 * mp[k] + (1.f - b1) * gg;
      vp[k] = b2 * vp[k] + (1.f - b2) * gg * gg;
      const float denom = sqrtf(vp[k]) / sqrtf(bc2) + eps;
      pp[k] -= (lr / bc1) * (mp[k] / denom);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// Exponential moving average of the parameters, held next to them: e += w * (p - e), evaluated as one fma on the difference
// (torch's lerp form for small weights).  Geometry and early return of sgd_ctrl_kernel.  An element whose bits already equal the
// parameter's keeps them through a select, not through arithmetic: -0 + w * 0 is +0, inf - inf is a NaN, and a NaN would come
// back with another payload.  That is what keeps the EMA of frozen / unreached parameters and of the alignment padding
// bit-identical to the arena without a granule map.
// The weight: `w` as the host rounded it from 1 - decay in fp64; under warm-up max(w, 9 / (10 + j)) for the j-th EMA update
// (TF's decay = min(decay, (1 + j) / (10 + j))), from wave-uniform values in fp64, rounded once.
// Plain cached loads (the optimizer has just written p) and plain stores; no atomics, no LDS, no scratch.
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
  const float r = fmaf(w, p - e, e);
  return __float_as_uint(p) == __float_as_uint(e) ? e : r;
}

__global__ __launch_bounds__(256) void ema_ctrl_kernel(float* __restrict__ e, const float* __restrict__ p, size_t n4,
                                                        const lc2is_optim_ctrl* __restrict__ ctrl, float w, int warmup,
                                                        int every, int reverse) {
  if (!ctrl->apply) return;
  const int u = ctrl->applied;
  if (u % every != 0) return;
  if (warmup) w = fmaxf(w, (float)(9.0 / (10.0 + (double)(u / every))));
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (size_t)gridDim.x * 256) {
    const size_t i = reverse ? n4 - 1 - j : j;
    float4 ev = reinterpret_cast<float4*>(e)[i];
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    ev.x = ema_lerp(ev.x, pv.x, w); ev.y = ema_lerp(ev.y, pv.y, w);
    ev.z = ema_lerp(ev.z, pv.z, w); ev.w = ema_lerp(ev.w, pv.w, w);
    reinterpret_cast<float4*>(e)[i] = ev;
  }
}

// In-place exchange of two equal-length, non-overlapping buffers, 16 bytes per lane, as integers: every bit pattern survives.
__global__ __launch_bounds__(256) void swap_f32_kernel(uint4* __restrict__ a, uint4* __restrict__ b, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const uint4 av = a[i], bv = b[i];
    a[i] = bv;
    b[i] = av;
  }
}

inline int ew_grid(size_t work_items) {
  size_t g = (work_items + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int lc2is_grad_sumsq_blocks(size_t n) { return (n == 0 || n % 4) ? 0 : sumsq_grid(n); }

extern "C" size_t lc2is_grad_sumsq_workspace_bytes(size_t n) {
  return (n == 0 || n % 4) ? 0 : (size_t)sumsq_grid(n) * (sizeof(float) + sizeof(unsigned));
}

extern "C" int lc2is_grad_sumsq(const float* grads, size_t n, void* workspace, size_t workspace_bytes,
                                lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!grads || !workspace) return LC2IS_ERR_NULL;
  if (n == 0 || n % 4 || !aligned16(grads) || ((uintptr_t)workspace & 3u)) return LC2IS_ERR_SHAPE;
  if (workspace_bytes < lc2is_grad_sumsq_workspace_bytes(n)) return LC2IS_ERR_WORKSPACE;
  const int grid = sumsq_grid(n);
  float* partials = (float*)workspace;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(256), 0, stream, grads, n / 4, partials,
                     (unsigned*)(partials + grid));
  return lc2is_check_launch();
}

extern "C" int lc2is_optim_ctrl_update(lc2is_optim_ctrl* ctrl, const float* partials, const unsigned int* flags,
                                       int nparts, const float* lr_table, int table_len, float grad_scale,
                                       float max_norm, int skip_nonfinite, float beta1, float beta2,
                                       lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctrl || !partials || !flags || !lr_table) return LC2IS_ERR_NULL;
  if (nparts < 1 || nparts > SUMSQ_MAX_GRID || table_len < 1 || !(max_norm > 0.f) || !(grad_scale > 0.f) ||
      !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || ((uintptr_t)ctrl & 3u))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(optim_ctrl_update_kernel, dim3(1), dim3(256), 0, stream, ctrl, partials, flags, nparts, lr_table,
                     table_len, grad_scale, max_norm, skip_nonfinite, beta1, beta2);
  return lc2is_check_launch();
}

extern "C" int lc2is_accum_add(lc2is_accum_block* block, const float* loss2, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!block || !loss2) return LC2IS_ERR_NULL;
  if (((uintptr_t)block & 7u) || ((uintptr_t)loss2 & 3u)) return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(accum_add_kernel, dim3(1), dim3(64), 0, stream, block, loss2);
  return lc2is_check_launch();
}

extern "C" int lc2is_optim_ctrl_update_accum(lc2is_optim_ctrl* ctrl, lc2is_accum_block* block, int use_denom,
                                             const float* partials, const unsigned int* flags, int nparts,
                                             const float* lr_table, int table_len, float grad_scale, float max_norm,
                                             int skip_nonfinite, float beta1, float beta2, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctrl || !block || !partials || !flags || !lr_table) return LC2IS_ERR_NULL;
  if (nparts < 1 || nparts > SUMSQ_MAX_GRID || table_len < 1 || !(max_norm > 0.f) || !(grad_scale > 0.f) ||
      !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || ((uintptr_t)ctrl & 3u) ||
      ((uintptr_t)block & 7u) || (use_denom != 0 && use_denom != 1))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(optim_ctrl_update_accum_kernel, dim3(1), dim3(256), 0, stream, ctrl, block, use_denom, partials, flags,
                     nparts, lr_table, table_len, grad_scale, max_norm, skip_nonfinite, beta1, beta2);
  return lc2is_check_launch();
}

extern "C" int lc2is_sgd_step_ctrl(float* params, const float* grads, float* momentum_buf, size_t n,
                                   const lc2is_optim_ctrl* ctrl, float momentum, float weight_decay, int reverse,
                                   lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!params || !grads || !ctrl) return LC2IS_ERR_NULL;
  if (n == 0 || n % 4) return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(sgd_ctrl_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, params, grads, momentum_buf, n / 4,
                     ctrl, momentum, weight_decay, reverse);
  return lc2is_check_launch();
}

extern "C" int lc2is_adamw_step_ctrl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                                     const lc2is_optim_ctrl* ctrl, float beta1, float beta2, float eps,
                                     float weight_decay, int reverse, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !ctrl) return LC2IS_ERR_NULL;
  if (n == 0 || n % 4) return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(adamw_ctrl_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq,
                     n / 4, ctrl, beta1, beta2, eps, weight_decay, reverse);
  return lc2is_check_launch();
}

// The granule map holds n / 64 bytes, so n must be whole granules.  16-byte alignment (one float4 per lane) is what is enforced;
// the arena gives 256, which puts every granule on a 256-byte line of its own.
extern "C" int lc2is_sgd_step_groups(float* params, const float* grads, float* momentum_buf, size_t n,
                                     const lc2is_optim_ctrl* ctrl, const uint8_t* granule_group,
                                     const lc2is_param_group* groups, int ngroups, float momentum, int reverse,
                                     lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!params || !grads || !ctrl || !granule_group || !groups) return LC2IS_ERR_NULL;
  if (n == 0 || n % LC2IS_GROUP_GRANULE || ngroups < 1 || ngroups > LC2IS_MAX_PARAM_GROUPS || !aligned16(params) ||
      !aligned16(grads) || !aligned16(momentum_buf))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(sgd_groups_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, params, grads, momentum_buf, n / 4, ctrl,
                     granule_group, groups, ngroups, momentum, reverse);
  return lc2is_check_launch();
}

extern "C" int lc2is_adamw_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                                       const lc2is_optim_ctrl* ctrl, const uint8_t* granule_group,
                                       const lc2is_param_group* groups, int ngroups, float beta1, float beta2, float eps,
                                       int reverse, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !ctrl || !granule_group || !groups) return LC2IS_ERR_NULL;
  if (n == 0 || n % LC2IS_GROUP_GRANULE || ngroups < 1 || ngroups > LC2IS_MAX_PARAM_GROUPS || !aligned16(params) ||
      !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(adamw_groups_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq, n / 4,
                     ctrl, granule_group, groups, ngroups, beta1, beta2, eps, reverse);
  return lc2is_check_launch();
}

extern "C" int lc2is_ema_update_ctrl(float* ema, const float* params, size_t n, const lc2is_optim_ctrl* ctrl,
                                     float one_minus_decay, int warmup, int every, int reverse, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ema || !params || !ctrl) return LC2IS_ERR_NULL;
  if (n == 0 || n % 4 || !aligned16(ema) || !aligned16(params) || ((uintptr_t)ctrl & 3u) ||
      !(one_minus_decay > 0.f && one_minus_decay <= 1.f) || every < 1)
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(ema_ctrl_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, ema, params, n / 4, ctrl, one_minus_decay,
                     warmup, every, reverse);
  return lc2is_check_launch();
}

extern "C" int lc2is_swap_f32(float* a, float* b, size_t n, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !b) return LC2IS_ERR_NULL;
  if (n == 0 || n % 4 || !aligned16(a) || !aligned16(b)) return LC2IS_ERR_SHAPE;
  const uintptr_t lo = (uintptr_t)(a < b ? a : b), hi = (uintptr_t)(a < b ? b : a);
  if (hi - lo < n * sizeof(float)) return LC2IS_ERR_SHAPE;   // the two ranges overlap (a == b included)
  hipLaunchKernelGGL(swap_f32_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, stream, reinterpret_cast<uint4*>(a),
                     reinterpret_cast<uint4*>(b), n / 4);
  return lc2is_check_launch();
}
