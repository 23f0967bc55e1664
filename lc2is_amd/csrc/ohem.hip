// Online hard example mining: exact k-th largest per-pixel loss on the device, and the relabelling (gfx950).
// replaces: mmseg's OHEMPixelSampler (threshold form) / HRNet's OhemCrossEntropy — softmax, gather, torch.sort over every pixel of
//   the batch, `p < max(p_sorted[k], thresh)` — restated in loss space (include/lc2is_hip.h states the rule).
//
// ohem_select is a most-significant-digit radix select over the monotone uint32 image of the fp32 loss bits, four 8-bit digits:
//   ohem_hist_kernel<FIRST>   pass 0 reads loss_px + labels and writes the keys (0 = not valid: no valid key is 0, see ohem_key), the
//                             later passes read the keys alone (4 bytes per pixel); every pass counts the histogram of its digit over
//                             the valid keys that match the prefix found so far
//   ohem_pick_kernel          one block: sums the blocks' histogram rows, finds the digit that holds rank k, extends the prefix
//   ohem_apply_kernel         labels_out = label where valid and loss > L_eff, ignore_index elsewhere
// No read-modify-write atomic anywhere, LDS included.  The histogram of 64 keys (one per lane) is 8 ballots of the digit bits; lane
// j ANDs bits 2..7 (or their complements, by j's own bits) with the "counted" ballot and splits the result four ways by bits 0..1:
// four popcounts give it the counts of bins 4j..4j+3 for these 64 keys, accumulated in four registers.  The waves of a block leave
// their 256 counts in LDS rows of their own (plain stores), 256 lanes add the rows, the block's row leaves as plain stores to a
// workspace slab.  Integer counts: any order is exact, the same bytes every run.
// Grid as grad_sumsq_kernel's: grid-stride, 16 bytes of loss / keys per lane; blocks of 1024 lanes and at most 512 of them, so
// that the slab the one-block pick launch reads stays at 0.5 MB.
#include "common.h"
#include "lc2is_hip.h"

namespace {

constexpr int OH_THREADS = 1024;
constexpr int OH_WAVES = OH_THREADS / 64;
constexpr int OH_MAX_BLOCKS = 512;
constexpr int OH_BINS = 256;
constexpr size_t OH_STATE_BYTES = 64;
constexpr size_t OH_SLAB_BYTES = (size_t)OH_MAX_BLOCKS * OH_BINS * sizeof(unsigned);

struct OhemState {
  unsigned prefix;     // the digits found so far, in place
  unsigned krem;       // rank still to descend inside the keys that match the prefix
  long long n_valid;
  long long k;         // -1: nothing valid, no rank is searched
};

// Monotone image of the fp32 order: negative values complemented, the others with the sign bit set; -0 < +0 (a total order
// consistent with <).  A NaN of either sign maps to the top key, above +inf, so a non-finite loss is the first rank, not hidden.
// Key 0 would be the bits 0xffffffff, a NaN: no valid pixel has it, and it marks the pixels that are not valid.
__device__ __forceinline__ unsigned ohem_key(float v) {
  const unsigned u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ohem_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool ohem_valid(long long lab, long ignore_index, int C) {
  return lab != (long long)ignore_index && lab >= 0 && lab < (long long)C;
}

template <bool FIRST>
__global__ __launch_bounds__(OH_THREADS) void ohem_hist_kernel(const float* __restrict__ loss, const int64_t* __restrict__ labels,
                                                                unsigned* __restrict__ keys, long n, int C, long ignore_index,
                                                                const OhemState* __restrict__ st, int shift,
                                                                unsigned* __restrict__ slab) {
  __shared__ unsigned s_hist[OH_WAVES][OH_BINS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long nq = (n + 3) >> 2;
  unsigned prefix = 0u, pmask = 0u;
  if constexpr (!FIRST) {
    prefix = st->prefix;
    pmask = ~0u << (shift + 8);   // (shift <= 16 here)
  }
  unsigned long long xm[6];   // bit t of this lane's bin group clear: the complement of ballot t + 2 is wanted
#pragma unroll
  for (int t = 0; t < 6; ++t) xm[t] = ((lane >> t) & 1) ? 0ull : ~0ull;
  unsigned c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;

  for (long base = (long)blockIdx.x * OH_THREADS; base < nq; base += (long)gridDim.x * OH_THREADS) {   // block-uniform trip count
    const long q = base + tid;
    const long i0 = 4 * q;
    unsigned key[4] = {0u, 0u, 0u, 0u};
    if (i0 + 3 < n) {
      if constexpr (FIRST) {
        const float4 v = *reinterpret_cast<const float4*>(loss + i0);
        const longlong2 la = *reinterpret_cast<const longlong2*>(labels + i0);
        const longlong2 lb = *reinterpret_cast<const longlong2*>(labels + i0 + 2);
        key[0] = ohem_valid(la.x, ignore_index, C) ? ohem_key(v.x) : 0u;
        key[1] = ohem_valid(la.y, ignore_index, C) ? ohem_key(v.y) : 0u;
        key[2] = ohem_valid(lb.x, ignore_index, C) ? ohem_key(v.z) : 0u;
        key[3] = ohem_valid(lb.y, ignore_index, C) ? ohem_key(v.w) : 0u;
        *reinterpret_cast<uint4*>(keys + i0) = make_uint4(key[0], key[1], key[2], key[3]);
      } else {
        const uint4 kv = *reinterpret_cast<const uint4*>(keys + i0);
        key[0] = kv.x; key[1] = kv.y; key[2] = kv.z; key[3] = kv.w;
      }
    } else {   // the ragged last quad (and the lanes past it: nothing counted)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < n) {
          if constexpr (FIRST) {
            key[e] = ohem_valid(labels[i0 + e], ignore_index, C) ? ohem_key(loss[i0 + e]) : 0u;
            keys[i0 + e] = key[e];
          } else {
            key[e] = keys[i0 + e];
          }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool counted = key[e] != 0u && ((key[e] ^ prefix) & pmask) == 0u;
      const unsigned long long M = __ballot(counted);
      if (M == 0ull) continue;   // wave-uniform: after pass 0 most batches of 64 hold no key of the prefix
      const unsigned d = key[e] >> shift;
      unsigned long long b[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) b[t] = __ballot((d >> t) & 1u);
      unsigned long long mh = M;
#pragma unroll
      for (int t = 0; t < 6; ++t) mh &= b[t + 2] ^ xm[t];
      c0 += __popcll(mh & ~b[1] & ~b[0]);
      c1 += __popcll(mh & ~b[1] & b[0]);
      c2 += __popcll(mh & b[1] & ~b[0]);
      c3 += __popcll(mh & b[1] & b[0]);
    }
  }
  *reinterpret_cast<uint4*>(&s_hist[wid][4 * lane]) = make_uint4(c0, c1, c2, c3);
  __syncthreads();
  if (tid < OH_BINS) {
    unsigned s = 0u;
#pragma unroll
    for (int w = 0; w < OH_WAVES; ++w) s += s_hist[w][tid];
    slab[(size_t)blockIdx.x * OH_BINS + tid] = s;
  }
}

// One block.  Lane (j, part) sums bin j over the blocks of its part; 256 lanes then hold the bin totals and the number of counted keys
// in the bins above theirs; the one lane whose bin holds rank krem extends the prefix.  first: the totals of pass 0 are n_valid, and k
// is formed; last: the prefix is the pivot's key, and *info is written.
__global__ __launch_bounds__(OH_THREADS) void ohem_pick_kernel(OhemState* st, const unsigned* __restrict__ slab, int nblk, int shift,
                                                                int first, int last, long min_kept_total, float loss_thresh,
                                                                lc2is_ohem_info* info) {
  __shared__ unsigned s_part[OH_THREADS / OH_BINS][OH_BINS];
  __shared__ unsigned s_cnt[OH_BINS];
  const int tid = threadIdx.x, j = tid & (OH_BINS - 1), part = tid / OH_BINS;
  unsigned s = 0u;
  for (int b = part; b < nblk; b += OH_THREADS / OH_BINS) s += slab[(size_t)b * OH_BINS + j];
  s_part[part][j] = s;
  __syncthreads();
  if (tid < OH_BINS) s_cnt[tid] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
  __syncthreads();
  const bool binlane = tid < OH_BINS;   // (whole waves; the others only keep the barrier below company)
  unsigned above = 0u, total = 0u;
  if (binlane)
    for (int i = 0; i < OH_BINS; ++i) {
      const unsigned c = s_cnt[i];
      total += c;
      above += i > tid ? c : 0u;
    }
  long long n_valid, k;
  unsigned prefix, krem;
  if (first) {
    n_valid = (long long)total;
    k = (long long)min_kept_total < n_valid - 1 ? (long long)min_kept_total : n_valid - 1;
    prefix = 0u;
    krem = k >= 0 ? (unsigned)k : 0u;
  } else {
    n_valid = st->n_valid; k = st->k; prefix = st->prefix; krem = st->krem;
  }
  __syncthreads();   // every lane has read the state before one of them writes it
  if (!binlane) return;
  const unsigned cnt = s_cnt[tid];
  const bool hit = k >= 0 && above <= krem && krem - above < cnt;   // at most one lane: the bins partition the counted keys
  if (hit) {
    prefix |= (unsigned)tid << shift;
    st->prefix = prefix; st->krem = krem - above; st->n_valid = n_valid; st->k = k;
  } else if (k < 0 && tid == 0 && first) {
    st->prefix = 0u; st->krem = 0u; st->n_valid = n_valid; st->k = k;
  }
  if (last && (hit || (k < 0 && tid == 0))) {
    const float L = k >= 0 ? ohem_unkey(prefix) : __builtin_inff();
    info->n_valid = n_valid;
    info->k = k;
    info->L = L;
    info->L_eff = fminf(L, loss_thresh);
  }
}

// labels_out = label where the pixel is valid and its loss exceeds L_eff (IEEE, strict), ignore_index elsewhere.
__global__ __launch_bounds__(256) void ohem_apply_kernel(const float* __restrict__ loss, const int64_t* __restrict__ labels,
                                                          int64_t* __restrict__ labels_out, long n, int C, long ignore_index,
                                                          const lc2is_ohem_info* __restrict__ info) {
  const float leff = info->L_eff;
  const long nq = (n + 3) >> 2;
  const long long ign = (long long)ignore_index;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long i0 = 4 * q;
    if (i0 + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(loss + i0);
      longlong2 la = *reinterpret_cast<const longlong2*>(labels + i0);
      longlong2 lb = *reinterpret_cast<const longlong2*>(labels + i0 + 2);
      la.x = (ohem_valid(la.x, ignore_index, C) && v.x > leff) ? la.x : ign;
      la.y = (ohem_valid(la.y, ignore_index, C) && v.y > leff) ? la.y : ign;
      lb.x = (ohem_valid(lb.x, ignore_index, C) && v.z > leff) ? lb.x : ign;
      lb.y = (ohem_valid(lb.y, ignore_index, C) && v.w > leff) ? lb.y : ign;
      *reinterpret_cast<longlong2*>(labels_out + i0) = la;
      *reinterpret_cast<longlong2*>(labels_out + i0 + 2) = lb;
    } else {
      for (long i = i0; i < n; ++i) {
        const long long lab = labels[i];
        labels_out[i] = (ohem_valid(lab, ignore_index, C) && loss[i] > leff) ? lab : ign;
      }
    }
  }
}

bool ohem_n_ok(long n) { return n >= 1 && n < (1L << 31); }

}  // namespace

extern "C" size_t lc2is_ohem_select_workspace_bytes(long n) {
  if (!ohem_n_ok(n)) return 0;
  return OH_STATE_BYTES + OH_SLAB_BYTES + (((size_t)n * sizeof(unsigned) + 15) & ~(size_t)15);
}

extern "C" int lc2is_ohem_select(const float* loss_px, const int64_t* labels, int64_t* labels_out, long n, int C,
                                 long ignore_index, float loss_thresh, long min_kept_total, void* info, void* workspace,
                                 size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!loss_px || !labels || !labels_out || !info || !workspace) return LC2IS_ERR_NULL;
  if (!ohem_n_ok(n) || C < 1 || min_kept_total < 0 || !(loss_thresh >= 0.f)) return LC2IS_ERR_SHAPE;
  if ((((size_t)loss_px | (size_t)labels | (size_t)labels_out | (size_t)workspace) & 15) || ((size_t)info & 7)) return LC2IS_ERR_SHAPE;
  if (workspace_bytes < lc2is_ohem_select_workspace_bytes(n)) return LC2IS_ERR_WORKSPACE;
  OhemState* st = (OhemState*)workspace;
  unsigned* slab = (unsigned*)((char*)workspace + OH_STATE_BYTES);
  unsigned* keys = (unsigned*)((char*)workspace + OH_STATE_BYTES + OH_SLAB_BYTES);
  lc2is_ohem_info* inf = (lc2is_ohem_info*)info;
  const long nq = (n + 3) >> 2;
  const long want = (nq + OH_THREADS - 1) / OH_THREADS;
  const int grid = (int)(want < OH_MAX_BLOCKS ? want : OH_MAX_BLOCKS);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (pass == 0)
      hipLaunchKernelGGL(ohem_hist_kernel<true>, dim3(grid), dim3(OH_THREADS), 0, stream, loss_px, labels, keys, n, C,
                         ignore_index, st, shift, slab);
    else
      hipLaunchKernelGGL(ohem_hist_kernel<false>, dim3(grid), dim3(OH_THREADS), 0, stream, loss_px, labels, keys, n, C,
                         ignore_index, st, shift, slab);
    hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(OH_THREADS), 0, stream, st, slab, grid, shift, pass == 0, pass == 3,
                       min_kept_total, loss_thresh, inf);
  }
  const long awant = (nq + 255) / 256;
  const int agrid = (int)(awant < 4096 ? awant : 4096);
  hipLaunchKernelGGL(ohem_apply_kernel, dim3(agrid), dim3(256), 0, stream, loss_px, labels, labels_out, n, C, ignore_index, inf);
  return lc2is_check_launch();
}
