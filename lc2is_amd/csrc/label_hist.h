// Atomics-free histogram of uint8 labels (gfx950, wave64), shared by aug_crop_select_kernel and label_hist_kernel (augment.hip);
// at the end wave_hist, the same scheme on int keys for the class counts of resize_argmax.hip and head_argmax.hip.
// Every wave owns one row of LH_BINS counts in LDS, which no other wave writes.  The lanes of the wave that hold the same label
// are merged before the add: the first lane still to be served is the leader, its label is broadcast (v_readlane), one ballot
// finds the lanes that match, and the leader alone does a plain `row[v] += popcount`; the loop ends when every lane is served.
// Label maps are piecewise constant, so 64 neighbouring pixels hold one or two labels and the loop runs once or twice; 64 different
// labels cost 64 rounds and are still exact.  One wave's LDS operations complete in order, so the add of one round (or call) is seen
// by the next, whichever lane issues it.  The rows are added in a fixed order (lh_block_sum): integer counts, the same bytes every
// run.  No read-modify-write atomic, in LDS or in global memory.
#pragma once
#include "common.h"

constexpr int LH_BINS = 256;

// Zero this wave's row (4 bins per lane).  The caller keeps other waves from reading the row meanwhile (a barrier after lh_block_sum).
__device__ __forceinline__ void lh_wave_clear(unsigned* row) {
  *reinterpret_cast<uint4*>(row + 4 * (threadIdx.x & 63)) = make_uint4(0u, 0u, 0u, 0u);
}

// Count label v (0..255) of every lane with `counted` into this wave's row.  Call with the whole wave converged (all 64 lanes
// reach the call together); every value that steers the loop is a ballot, hence wave-uniform.
__device__ __forceinline__ void lh_wave_add(unsigned* row, unsigned v, bool counted) {
  const int lane = threadIdx.x & 63;
  v &= LH_BINS - 1;   // the leader always matches itself: every round serves at least one lane
  unsigned long long todo = __ballot(counted);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const unsigned lv = (unsigned)__builtin_amdgcn_readlane((int)v, leader);
    const unsigned long long same = __ballot(counted && v == lv);
    if (lane == leader) row[lv] += (unsigned)__popcll(same);
    todo &= ~same;
  }
}

// Bin `bin` summed over the block's `waves` rows (rows[w * LH_BINS + bin]), in wave order.  After a __syncthreads().
__device__ __forceinline__ unsigned lh_block_sum(const unsigned* rows, int waves, int bin) {
  unsigned s = 0u;
  for (int w = 0; w < waves; ++w) s += rows[w * LH_BINS + bin];
  return s;
}

// The same leader scheme on int keys with the bin count left to the caller (resize_argmax.hip, head_argmax.hip):
// hist[cls] += number of this wave's lanes with `on` and key == cls.  One iteration per distinct key; the wave is the only writer.
__device__ __forceinline__ void wave_hist(int* hist, bool on, int key, int lane) {
  while (true) {
    const unsigned long long m = __ballot(on);
    if (m == 0ull) break;
    const int leader = __ffsll((unsigned long long)m) - 1;
    const int cls = __shfl(key, leader);
    const bool mine = on && key == cls;
    const unsigned long long e = __ballot(mine);
    if (lane == leader) hist[cls] += __popcll(e);
    on = on && !mine;
  }
}
