// Class map and {intersection, predicted, labelled} counts of the fused head at its own output size (gfx950), forward only.
// replaces: model(inputs)["outputs"].argmax(1) — a second forward that materialises the [B,K,H,W] fp32 logits (158 MB per 512 x 512
//   image at K = 151) — followed by mmseg's accuracy() / intersect_and_union() on the training batch (decode.acc_seg, train mIoU).
//
// head_argmax_grp_kernel is the argmax sibling of head_px_grp_kernel (head.hip): head_grp_plan's tiles and grid, the same S x S-pixel
// groups in units of 16 pixels, the same footprint staging and the same forward product Wm x lo on the fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32), channels at or past C masked to -inf in the accumulators.  Nothing of the softmax: the accumulator of
// channel tile t holds, per lane, channel 16 t + (lane & 15) of four pixels, so the argmax over the channels is an in-lane walk over
// the tiles (ascending, strict >: the first maximum stays) and four row_dpp steps that combine (value, index) pairs inside a row of 16
// lanes — the larger value wins, equal values keep the lower index: torch.argmax's tie rule.  The index is clamped into [0, C): a NaN
// score may pick any class but never indexes outside a histogram row; a pixel whose scores are all -inf gets class 0.
// The 16 results of a unit go to a [16][16] tile in LDS beside the labels' tile; after one barrier the first 256 threads own one pixel
// each (as in the kernels of resize_argmax.hip): pred[b, Y, X] leaves as a byte, and waves 0-3 count their 64 pixels into wave-private
// LDS rows [3][cq] with wave_hist (label_hist.h: ballot + popcount, one plain add per distinct class, the wave the only writer).
// Counting rule (the loss's own, and mmseg's): a pixel counts iff label != ignore_index && 0 <= label < C; it adds to
// predicted[pred] and labelled[label], and to intersection[pred] when pred == label; any other pixel adds to none of the three.
// The block sums its four waves in wave order into its own slab [3][cq] of the workspace and head_argmax_finish_kernel sums each
// image's slabs in a fixed order.  NO read-modify-write atomics, LDS included: integer counts, the same bytes every run.
// The tiles, the staging, the unit walk, the forward product and the row steps are head_grp.h's; the kernel's own: the argmax walk,
// the class tile and the counts.
#include "common.h"
#include "head_grp.h"
#include "interp.h"
#include "label_hist.h"
#include "lc2is_hip.h"

namespace {

constexpr int NHW = 4;          // waves that own pixels after the barrier (256 pixels, 64 each)

struct ArgmaxArgs {
  const float* lo; int ld;       // [B, h, w, ld] scores, C valid channels
  const int64_t* labels;         // [B, H, W] or null (pred only)
  uint8_t* pred;                 // [B, H, W] or null
  int* slab;                     // [blocks][3][cq] per-tile counts or null
  int B, h, w, H, W, C, cq;
  long ignore_index;
};

template <int MODE, int TN, int S>
__global__ __launch_bounds__(HEAD_THREADS, (S == 4 ? 2 : 1)) void head_argmax_grp_kernel(ArgmaxArgs p) {
  using GM = HeadGrpGeom<MODE, S>;
  constexpr int F4 = GM::F4, NQ = GM::NQ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const HeadTile T = head_tile<S>(p.H, p.W);
  const int CS = p.ld + HEAD_PAD;
  const HeadLds L = head_grp_lds(F4, p.ld, false);
  float* s_lo = (float*)smem;
  int* s_lab = (int*)(s_lo + L.lab);
  int* s_arg = (int*)(s_lo + L.tail);            // [16][16] class of the pixel (read only where s_lab is not -2)
  int* s_hist = s_arg + HT * HT;                 // counts wanted: [NHW waves][intersection | predicted | labelled][cq]
  stage_footprint<MODE, S>(s_lo, nullptr, false, p.lo, p.ld, p.h, p.w, T, tid);
  if (tid < HT * HT) {
    stage_label<true>(s_lab, p.labels, T, p.H, p.W, p.C, p.ignore_index, tid);
    if (p.slab) {   // this wave's rows, which no other wave writes
      int* hw = s_hist + wid * 3 * p.cq;
      for (int i = lane; i < 3 * p.cq; i += 64) hw[i] = 0;
    }
  }
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const float NEG = -__builtin_inff();
  int cell_off[NQ];
  make_cell_off<MODE, S>(cell_off, kq, CS);

#pragma unroll 1
  for (int g2 = 0; g2 < 2; ++g2) {
    const HeadUnit U = head_unit<MODE, S>(T, g2, wid, kq, CS, p.H, p.W);
    if (!U.active) continue;   // no pixel of the unit is inside the image: nothing reads its part of s_arg
    float Af[NQ];
    make_fwd_operand<MODE, S>(Af, U.prow, m, kq);
    f32x4_t acc[TN];
    fwd_product(acc, s_lo + U.gbase + m, cell_off, Af);
    // in-lane: channels 16 t + m, t ascending, strict > (the lowest channel of equal scores stays)
    float best[4] = {NEG, NEG, NEG, NEG};
    int arg[4] = {m, m, m, m};
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      mask_past_c(acc[t], t, m, p.C, NEG);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (acc[t][r] > best[r]) { best[r] = acc[t][r]; arg[r] = 16 * t + m; }
    }
    i32x4_t out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      row16_argmax(best[r], arg[r]);
      out[r] = arg[r] < 0 ? 0 : (arg[r] > p.C - 1 ? p.C - 1 : arg[r]);
    }
    if (m == 0) *reinterpret_cast<i32x4_t*>(s_arg + (S * U.gy + U.py4) * 16 + S * U.gx + U.px4) = out;
  }
  __syncthreads();

  // the first 256 threads own one pixel each; the other waves only help with the block's sum
  const int code = tid < HT * HT ? s_lab[tid] : -2;
  const bool inside = code != -2;
  const int cls = inside ? s_arg[tid] : 0;
  if (inside && p.pred) {
    const int Y = T.Y0 + (tid >> 4), X = T.X0 + (tid & 15);
    p.pred[((size_t)T.b * p.H + Y) * p.W + X] = (uint8_t)cls;
  }
  if (!p.slab) return;
  if (wid < NHW) {
    int* hw = s_hist + wid * 3 * p.cq;   // this wave's {intersection, predicted, labelled}
    const bool counted = code >= 0;
    wave_hist(hw + p.cq, counted, cls, lane);
    wave_hist(hw, counted && cls == code, cls, lane);
    wave_hist(hw + 2 * p.cq, counted, code, lane);
  }
  __syncthreads();
  const int n = 3 * p.cq;
  int* o = p.slab + (size_t)blockIdx.x * n;
  for (int i = tid; i < n; i += HEAD_THREADS) o[i] = ((s_hist[i] + s_hist[n + i]) + s_hist[2 * n + i]) + s_hist[3 * n + i];
}

// counts[b][e] = sum over the image's tiles of slab[tile][e], tiles in increasing order within each of 4 strided parts, the parts
// added in order (the shape of ra_finish_kernel): grid (ceil(3C / 64), B), 256 threads.  Slab rows are cq wide, counts rows C.
__global__ __launch_bounds__(256) void head_argmax_finish_kernel(const int* __restrict__ slab, int* __restrict__ counts, int C, int cq,
                                                                 int t4) {
  __shared__ int part[4][64];
  const int b = blockIdx.y, tid = threadIdx.x, q = tid >> 6;
  const int e = blockIdx.x * 64 + (tid & 63);
  int s = 0;
  if (e < 3 * C) {
    const int k = e / C, c = e - k * C;
    const int* src = slab + (size_t)b * t4 * 3 * cq + k * cq + c;
    for (int i = q; i < t4; i += 4) s += src[(size_t)i * 3 * cq];
  }
  part[q][tid & 63] = s;
  __syncthreads();
  if (q == 0 && e < 3 * C) counts[(size_t)b * 3 * C + e] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// the blocks' count slabs [blocks][3][cq] on head_grp_plan's tiles
size_t argmax_slab_bytes(const HeadGrpPlan& g, int B) { return (size_t)B * g.t4 * 3 * g.cq * sizeof(int); }

}  // namespace

extern "C" size_t lc2is_head_upsample_argmax_workspace_bytes(int B, int h, int w, int C, int S, int mode) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || C > CMAX || !(S == 4 || S == 8 || S == 16)) return 0;
  if (mode != LC2IS_INTERP_BICUBIC && mode != LC2IS_INTERP_BILINEAR) return 0;
  return argmax_slab_bytes(head_grp_plan(B, h, w, C, S, mode, false), B);
}

extern "C" int lc2is_head_upsample_argmax(const float* scores_lo, int ld, const int64_t* labels, uint8_t* pred, int32_t* counts,
                                          int B, int h, int w, int C, int S, int mode, long ignore_index, void* workspace,
                                          size_t workspace_bytes, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!scores_lo || (!pred && !counts)) return LC2IS_ERR_NULL;
  if (counts && !labels) return LC2IS_ERR_NULL;
  if (int rc = head_grp_check(scores_lo, nullptr, true, B, h, w, C, ld, S, mode)) return rc;
  const HeadGrpPlan gp = head_grp_plan(B, h, w, C, S, mode, false);
  if (counts && !head_ws_ok(workspace, workspace_bytes, argmax_slab_bytes(gp, B))) return LC2IS_ERR_WORKSPACE;
  const int H = h * S, W = w * S;
  ArgmaxArgs a{scores_lo, ld, labels, pred, counts ? (int*)workspace : nullptr, B, h, w, H, W, C, gp.cq, ignore_index};
  // the footprint, the labels' tile, and behind it the class tile and the four waves' rows
  const int lds = head_grp_lds(gp.f4, ld, false).bytes(HT * HT + (counts ? NHW * 3 * gp.cq : 0));
  const int rc = head_grp_dispatch(mode, S, head_grp_tn(C), [&](auto M, auto TN_, auto S_) {
    return head_grp_launch<head_argmax_grp_kernel<M(), TN_(), S_()>>(head_grp_lds_max(false, HT * HT + NHW * 3 * CMAX), B * gp.t4, lds,
                                                                      stream, a);
  });
  if (rc || !counts) return rc;
  hipLaunchKernelGGL(head_argmax_finish_kernel, dim3((3 * C + 63) / 64, B), dim3(256), 0, stream, (const int*)workspace, counts, C,
                     gp.cq, gp.t4);
  return lc2is_check_launch();
}
