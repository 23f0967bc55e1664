// Mixed-sample augmentation on the device: ClassMix (DACS, DAFormer) and CutMix (CPS, UniMatch) of a destination and a source batch,
// the step between the teacher's pseudo-labels and the student's step in self-training.  Two launches, nothing but device memory
// decides the result, so the pair captures into a graph and a replay draws again from the epoch / key tensors.
//   * mix_select_kernel: one block per output sample writes its plan row (mode, source row, cutmix box, chosen-class bitmap) and
//     an info row.  Classmix finds the classes of the source label map as LDS flags, ranks their (draw, class) pairs by counting
//     smaller pairs and forms the bitmap by ballot: no read-modify-write atomic anywhere.
//   * mix_apply_kernel: one launch for pixels, labels and weights (label cells are extra blocks of the same grid, as in
//     aug_apply_kernel).  HBM-bound: 3 * 16-byte loads of the CHOSEN side and 3 * 16-byte stores per lane; the mask is one source
//     label (8 bytes, shared by the r rows of a cell and cached) and one bitmap word from LDS per pixel quad.
// The exact definition is in include/lc2is_hip.h; tests/mix_ref.py restates it in numpy (every output is a select: bit for bit).
// The RNG and aug_div live in aug_rng.h; the launcher's overlap predicate (lc2is_bytes_overlap) in common.h.
#include "common.h"
#include "aug_rng.h"
#include "lc2is_hip.h"

namespace {

constexpr int MIX_P = LC2IS_MIX_PLAN_WORDS;
constexpr int MIX_BM = LC2IS_MIX_BITMAP;
constexpr int MIX_BM_WORDS = LC2IS_MIX_MAX_CLASSES / 32;
constexpr int MS_THREADS = LC2IS_MIX_MAX_CLASSES;   // lane tid holds class tid
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_UNROLL = 4;                        // independent 8-byte loads in flight per lane
static_assert(MIX_BM + MIX_BM_WORDS == MIX_P && MS_WAVES * 2 == MIX_BM_WORDS, "plan row layout");

__device__ __forceinline__ int mix_mulshift(unsigned u24, long long n) {   // uniform in [0, n), n <= 2^24
  return (int)(((unsigned long long)u24 * (unsigned long long)n) >> 24);
}

__global__ __launch_bounds__(MS_THREADS) void mix_select_kernel(const int64_t* __restrict__ src_lab, int Bs,
                                                                 const int64_t* __restrict__ src_index,
                                                                 const int64_t* __restrict__ keys, const int32_t* __restrict__ epoch,
                                                                 const lc2is_mix_config cfg, int L, int32_t* __restrict__ plan,
                                                                 int32_t* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) unsigned s_draw[MS_THREADS];   // presence flags first, then the draws of the present classes
  __shared__ unsigned s_bm[MIX_BM_WORDS];
  __shared__ int s_cnt[MS_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int32_t* row = plan + (size_t)b * MIX_P;
  int32_t* irow = info + (size_t)b * 4;
  const long long srow = src_index ? (long long)src_index[b] : (long long)b;
  const int LL = L * L;
  if (srow < 0 || srow >= Bs) {   // block-uniform: the empty mask
    if (tid < MIX_P) row[tid] = 0;
    if (tid < 4) irow[tid] = tid == 0 ? -1 : 0;
    return;
  }
  const unsigned h = aug_key(cfg.seed_lo, cfg.seed_hi, *epoch, (long long)keys[b]) ^ LC2IS_MIX_STREAM;
  if (cfg.mode != LC2IS_MIX_CLASSMIX) {   // block-uniform: cutmix draws one box, none draws nothing
    if (tid >= MIX_BM && tid < MIX_P) row[tid] = 0;
    if (tid == 0) {
      int top = 0, left = 0, bh = 0, bw = 0;
      if (cfg.mode == LC2IS_MIX_CUTMIX) {
        const long long a = cfg.area_lo1024 + mix_mulshift(aug_u24(h, 0), (long long)cfg.area_hi1024 - cfg.area_lo1024 + 1);
        long long hmin = (a * L + 1023) >> 10;
        hmin = hmin < 1 ? 1 : hmin;
        bh = (int)hmin + mix_mulshift(aug_u24(h, 1), L - hmin + 1);
        long long w = (2 * a * L * L + 1024ll * bh) / (2048ll * bh);
        bw = (int)(w < 1 ? 1 : (w > L ? L : w));
        top = mix_mulshift(aug_u24(h, 2), L - bh + 1);
        left = mix_mulshift(aug_u24(h, 3), L - bw + 1);
      }
      row[0] = cfg.mode; row[1] = (int)srow; row[2] = top; row[3] = left; row[4] = bh; row[5] = bw; row[6] = 0; row[7] = 0;
      irow[0] = 0; irow[1] = 0; irow[2] = bh * bw; irow[3] = LL;
    }
    return;
  }

  // ---- classmix: the classes present in the source map ----
  const int64_t* map = src_lab + (size_t)srow * LL;
  const int K = cfg.n_classes;
  s_draw[tid] = 0u;
  __syncthreads();
  for (int base = 0; base < LL; base += MS_THREADS * MS_UNROLL) {   // block-uniform trip count
    long long v[MS_UNROLL];
#pragma unroll
    for (int e = 0; e < MS_UNROLL; ++e) {
      const int cell = base + e * MS_THREADS + tid;
      v[e] = cell < LL ? (long long)map[cell] : -1ll;
    }
#pragma unroll
    for (int e = 0; e < MS_UNROLL; ++e)
      if ((unsigned long long)v[e] < (unsigned long long)K && v[e] != cfg.ignore_index && v[e] != cfg.exclude_label)
        s_draw[v[e]] = 1u;   // same-value plain stores: the order of arrival does not matter
  }
  __syncthreads();
  const bool present = s_draw[tid] != 0u;   // (only flags below K were set)
  const unsigned d = aug_u24(h, 16u + (unsigned)tid);
  const int n_wave = __popcll(__ballot(present));
  __syncthreads();   // every flag is read: the array takes the draws
  s_draw[tid] = present ? d : 0xFFFFFFFFu;   // an absent class is smaller than nobody (a draw is below 2^24)
  if (lane == 0) s_cnt[wid] = n_wave;
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int w = 0; w < MS_WAVES; ++w) n += s_cnt[w];
  const int n_chosen = (n + 1) >> 1;
  int rank = 0;
  if (wid * 64 < K) {   // wave-uniform; classes K .. round-up-to-4 hold 0xFFFFFFFF
    for (int c = 0; c < K; c += 4) {
      const i32x4_t q = *(const i32x4_t*)&s_draw[c];   // one address per wave: a broadcast read
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned o = (unsigned)q[e];
        rank += (o < d || (o == d && c + e < tid)) ? 1 : 0;
      }
    }
  }
  const bool chosen = present && rank < n_chosen;
  const unsigned long long bal = __ballot(chosen);
  if (lane == 0) {
    s_bm[2 * wid] = (unsigned)bal;
    s_bm[2 * wid + 1] = (unsigned)(bal >> 32);
    row[MIX_BM + 2 * wid] = (int)(unsigned)bal;
    row[MIX_BM + 2 * wid + 1] = (int)(unsigned)(bal >> 32);
  }
  __syncthreads();   // the bitmap is complete; s_cnt has been read by every lane

  // ---- masked cells: ballot + popcount per wave, the waves' counts added in wave order ----
  int cnt = 0;   // wave-uniform
  for (int base = 0; base < LL; base += MS_THREADS * MS_UNROLL) {
    long long v[MS_UNROLL];
#pragma unroll
    for (int e = 0; e < MS_UNROLL; ++e) {
      const int cell = base + e * MS_THREADS + tid;
      v[e] = cell < LL ? (long long)map[cell] : -1ll;
    }
#pragma unroll
    for (int e = 0; e < MS_UNROLL; ++e) {
      const bool in = (unsigned long long)v[e] < (unsigned long long)LC2IS_MIX_MAX_CLASSES;
      const unsigned c = in ? (unsigned)v[e] : 0u;
      cnt += __popcll(__ballot(in && ((s_bm[c >> 5] >> (c & 31u)) & 1u)));
    }
  }
  if (lane == 0) s_cnt[wid] = cnt;
  __syncthreads();
  if (tid == 0) {
    int masked = 0;
#pragma unroll
    for (int w = 0; w < MS_WAVES; ++w) masked += s_cnt[w];
    row[0] = LC2IS_MIX_CLASSMIX; row[1] = (int)srow; row[2] = 0; row[3] = 0; row[4] = 0; row[5] = 0; row[6] = n; row[7] = n_chosen;
    irow[0] = n; irow[1] = n_chosen; irow[2] = masked; irow[3] = LL;
  }
}

struct MixPlan {   // block-uniform: one sample per blockIdx.y
  int mode, top, left, bh, bw;
  size_t srow;
};
__device__ __forceinline__ MixPlan mix_plan(const int32_t* __restrict__ prow, int Bs) {
  MixPlan p;
  p.mode = prow[0];
  const int srow = prow[1];
  if ((unsigned)srow >= (unsigned)Bs || (p.mode != LC2IS_MIX_CLASSMIX && p.mode != LC2IS_MIX_CUTMIX)) p.mode = LC2IS_MIX_NONE;
  p.srow = p.mode == LC2IS_MIX_NONE ? 0 : (size_t)srow;
  p.top = prow[2]; p.left = prow[3]; p.bh = prow[4]; p.bw = prow[5];
  return p;
}
// Is cell (ci, cj) of this sample masked?  (ci, cj inside the L x L grid: the one read is inside the source map)
__device__ __forceinline__ bool mix_cell(const MixPlan& p, const int64_t* __restrict__ smap, const unsigned* s_bm, int ci, int cj,
                                         int L) {
  if (p.mode == LC2IS_MIX_CLASSMIX) {
    const long long v = smap[ci * L + cj];
    const bool in = (unsigned long long)v < (unsigned long long)LC2IS_MIX_MAX_CLASSES;
    const unsigned c = in ? (unsigned)v : 0u;
    return in && ((s_bm[c >> 5] >> (c & 31u)) & 1u);
  }
  // cutmix (unsigned compare: top <= ci < top + bh); mode NONE: nothing
  return p.mode == LC2IS_MIX_CUTMIX && (unsigned)(ci - p.top) < (unsigned)p.bh && (unsigned)(cj - p.left) < (unsigned)p.bw;
}

// QUAD: r % 4 == 0, the four pixels of a lane lie in one cell
template <bool QUAD>
__global__ __launch_bounds__(256) void mix_apply_kernel(const float* __restrict__ dst_px, const int64_t* __restrict__ dst_lab,
                                                         const float* __restrict__ dst_pw, const float* __restrict__ src_px,
                                                         const int64_t* __restrict__ src_lab, const float* __restrict__ src_pw,
                                                         int Bs, const int32_t* __restrict__ plan, int S, int L, int img_blocks,
                                                         float* __restrict__ out_px, int64_t* __restrict__ out_lab,
                                                         float* __restrict__ out_pw) {
  __shared__ unsigned s_bm[MIX_BM_WORDS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int32_t* prow = plan + (size_t)b * MIX_P;
  const MixPlan p = mix_plan(prow, Bs);
  if (p.mode == LC2IS_MIX_CLASSMIX) {   // block-uniform
    if (tid < MIX_BM_WORDS) s_bm[tid] = (unsigned)prow[MIX_BM + tid];
    __syncthreads();
  }
  const int LL = L * L;
  const int64_t* smap = src_lab + p.srow * LL;

  if ((int)blockIdx.x >= img_blocks) {   // ---- label and weight cells ----
    const int cell = ((int)blockIdx.x - img_blocks) * 256 + tid;
    if (cell >= LL) return;
    int cj;
    const int ci = aug_div(cell, L, __builtin_amdgcn_rcpf((float)L), cj);
    const size_t di = (size_t)b * LL + cell, si = p.srow * LL + cell;
    if (mix_cell(p, smap, s_bm, ci, cj, L)) {
      out_lab[di] = src_lab[si];
      out_pw[di] = src_pw ? src_pw[si] : 1.0f;
    } else {
      out_lab[di] = dst_lab[di];
      out_pw[di] = dst_pw ? dst_pw[di] : 1.0f;
    }
    return;
  }

  // ---- pixels: 4 consecutive x per lane, all 3 channels, from the chosen side only ----
  const int W4 = S >> 2, r = S / L;
  const int q = (int)blockIdx.x * 256 + tid;
  if (q >= S * W4) return;
  int jq, rem;
  const int i = aug_div(q, W4, __builtin_amdgcn_rcpf((float)W4), jq);
  const int j0 = jq * 4;
  const float rr = __builtin_amdgcn_rcpf((float)r);
  const int ci = aug_div(i, r, rr, rem);
  const size_t plane = (size_t)S * S;
  const size_t doff = ((size_t)b * 3 * S + i) * S + j0, soff = (p.srow * 3 * S + i) * S + j0;
  float* out = out_px + doff;
  if (QUAD) {
    const bool m = mix_cell(p, smap, s_bm, ci, aug_div(j0, r, rr, rem), L);
    const float* from = m ? src_px + soff : dst_px + doff;
#pragma unroll
    for (int c = 0; c < 3; ++c) *(f32x4_t*)(out + c * plane) = *(const f32x4_t*)(from + c * plane);
    return;
  }
  bool m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = mix_cell(p, smap, s_bm, ci, aug_div(j0 + k, r, rr, rem), L);
  if (m[0] == m[1] && m[0] == m[2] && m[0] == m[3]) {
    const float* from = m[0] ? src_px + soff : dst_px + doff;
#pragma unroll
    for (int c = 0; c < 3; ++c) *(f32x4_t*)(out + c * plane) = *(const f32x4_t*)(from + c * plane);
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4_t v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (m[k] ? src_px + soff : dst_px + doff)[c * plane + k];
    *(f32x4_t*)(out + c * plane) = v;
  }
}

}  // namespace

extern "C" int lc2is_mix_select(const int64_t* src_lab, int Bs, const int64_t* src_index, const int64_t* keys, int B,
                                const int32_t* epoch, const lc2is_mix_config* cfg, int L, int32_t* plan, int32_t* info,
                                lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!src_lab || !keys || !epoch || !cfg || !plan || !info) return LC2IS_ERR_NULL;
  if (B <= 0 || Bs <= 0 || L <= 0 || L > LC2IS_AUG_MAX_SIDE || cfg->n_classes < 1 || cfg->n_classes > LC2IS_MIX_MAX_CLASSES ||
      cfg->area_lo1024 < 1 || cfg->area_hi1024 < cfg->area_lo1024 || cfg->area_hi1024 > 1024 || ((uintptr_t)src_lab & 7) ||
      ((uintptr_t)keys & 7) || ((uintptr_t)src_index & 7) || ((uintptr_t)plan & 3) || ((uintptr_t)info & 3) || ((uintptr_t)epoch & 3))
    return LC2IS_ERR_SHAPE;
  if (cfg->mode != LC2IS_MIX_NONE && cfg->mode != LC2IS_MIX_CLASSMIX && cfg->mode != LC2IS_MIX_CUTMIX) return LC2IS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mix_select_kernel, dim3(B), dim3(MS_THREADS), 0, stream, src_lab, Bs, src_index, keys, epoch, *cfg, L, plan,
                     info);
  return lc2is_check_launch();
}

extern "C" int lc2is_mix_apply(const float* dst_px, const int64_t* dst_lab, const float* dst_pw, const float* src_px,
                               const int64_t* src_lab, const float* src_pw, int Bs, const int32_t* plan, int B, int S, int L,
                               float* out_px, int64_t* out_lab, float* out_pw, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dst_px || !dst_lab || !src_px || !src_lab || !plan || !out_px || !out_lab || !out_pw) return LC2IS_ERR_NULL;
  if (B <= 0 || B > 65535 || Bs <= 0 || S < 4 || S > LC2IS_AUG_MAX_SIDE || (S & 3) || L <= 0 || S % L ||
      (((uintptr_t)dst_px | (uintptr_t)src_px | (uintptr_t)out_px) & 15) ||
      (((uintptr_t)dst_lab | (uintptr_t)src_lab | (uintptr_t)out_lab) & 7) ||
      (((uintptr_t)dst_pw | (uintptr_t)src_pw | (uintptr_t)out_pw | (uintptr_t)plan) & 3))
    return LC2IS_ERR_SHAPE;
  const size_t px = (size_t)3 * S * S * sizeof(float), cells = (size_t)L * L;
  if (lc2is_bytes_overlap(out_px, B * px, dst_px, B * px) || lc2is_bytes_overlap(out_px, B * px, src_px, Bs * px) ||
      lc2is_bytes_overlap(out_lab, B * cells * 8, dst_lab, B * cells * 8) || lc2is_bytes_overlap(out_lab, B * cells * 8, src_lab, Bs * cells * 8) ||
      lc2is_bytes_overlap(out_pw, B * cells * 4, dst_pw, B * cells * 4) || lc2is_bytes_overlap(out_pw, B * cells * 4, src_pw, Bs * cells * 4))
    return LC2IS_ERR_SHAPE;
  const int img_blocks = (S * (S >> 2) + 255) / 256, lab_blocks = (int)((cells + 255) / 256);
  const dim3 grid(img_blocks + lab_blocks, B), block(256);
  if ((S / L) % 4 == 0)
    hipLaunchKernelGGL(mix_apply_kernel<true>, grid, block, 0, stream, dst_px, dst_lab, dst_pw, src_px, src_lab, src_pw, Bs, plan, S,
                       L, img_blocks, out_px, out_lab, out_pw);
  else
    hipLaunchKernelGGL(mix_apply_kernel<false>, grid, block, 0, stream, dst_px, dst_lab, dst_pw, src_px, src_lab, src_pw, Bs, plan, S,
                       L, img_blocks, out_px, out_lab, out_pw);
  return lc2is_check_launch();
}
