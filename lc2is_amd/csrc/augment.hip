// Train-time augmentation on the device (the `transform` hook of data/dataset.py:144-149, which the reference
// leaves to the host): random rescale + crop + horizontal flip + photometric jitter of a whole batch, cut from a pool of decoded
// uint8 images that lives in HBM straight into the step's pixel_values [B,3,S,S] fp32 and label [B,L,L] int64.
//   * aug_params_kernel: one thread per sample draws the sample's parameters from a counter-based RNG keyed by
//     (seed, epoch, dataset index, draw number) and folds the photometric steps into one 3x3 matrix + offset.
//   * aug_apply_kernel: one launch for the batch, images and labels together (label cells are extra blocks of the same grid).
//     HBM-bound by its 3 * 16-byte stores per lane; the source taps are unaligned 8-byte reads (two neighbouring HWC pixels) that
//     neighbouring lanes take from neighbouring bytes.  Source coordinates are exact integers: the quotient of at most 4096 comes
//     from one fp32 multiply by a reciprocal and an integer correction instead of hipcc's ~35-instruction udiv.
//   * aug_crop_select_kernel (optional, between the two): the class-ratio re-draw of mmseg's RandomCrop(cat_max_ratio).  One block
//     per sample counts the label cells aug_apply would write for each candidate origin and replaces the row's (top, left).
//   * label_hist_kernel: per-image class counts of the pool's label maps, for class weights.  Both count with label_hist.h.
// The exact definition is in include/lc2is_hip.h; tests/augment_ref.py and tests/catcrop_ref.py restate it in numpy (integers bit
// for bit).  The counter RNG, aug_div and the colour steps live in aug_rng.h; the colour map's load and apply and the label cell's rule
// (aug_cell_pos, aug_cell_src), which the apply and the crop-select kernel share, in view_common.h.
#include "common.h"
#include "aug_rng.h"
#include "view_common.h"
#include "label_hist.h"
#include "lc2is_hip.h"

namespace {

constexpr int AUG_P = LC2IS_AUG_PARAM_WORDS;

__global__ __launch_bounds__(64) void aug_params_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ keys, int B,
                                                         const int32_t* __restrict__ epoch, const lc2is_aug_image* __restrict__ desc,
                                                         long n_images, const lc2is_aug_config cfg, int32_t* __restrict__ params) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int32_t* row = params + (size_t)b * AUG_P;
  const long long slot = slots[b];
  int H = 0, W = 0;
  if (slot >= 0 && slot < n_images) { H = desc[slot].H; W = desc[slot].W; }
  if (H < 1 || W < 1 || H > LC2IS_AUG_MAX_SIDE || W > LC2IS_AUG_MAX_SIDE) {
#pragma unroll
    for (int e = 0; e < AUG_P; ++e) row[e] = 0;
    return;
  }
  const unsigned h = aug_key(cfg.seed_lo, cfg.seed_hi, *epoch, keys ? (long long)keys[b] : slot);
  const int S = cfg.crop_size;
  // integers in integer arithmetic only (64-bit products of a 24-bit uniform)
  const long long r = cfg.ratio_lo1024 +
                      (long long)(((unsigned long long)aug_u24(h, 0) * (unsigned long long)(cfg.ratio_hi1024 - cfg.ratio_lo1024 + 1)) >> 24);
  const long long t = ((long long)cfg.base_size * r + 512) >> 10;
  const long long s = H < W ? H : W;
  long long nh = (2 * (long long)H * t + s) / (2 * s), nw = (2 * (long long)W * t + s) / (2 * s);
  nh = nh < 1 ? 1 : (nh > LC2IS_AUG_MAX_RESIZED ? LC2IS_AUG_MAX_RESIZED : nh);
  nw = nw < 1 ? 1 : (nw > LC2IS_AUG_MAX_RESIZED ? LC2IS_AUG_MAX_RESIZED : nw);
  const long long fh = nh > S ? nh - S : 0, fw = nw > S ? nw - S : 0;
  row[LC2IS_AUG_NH] = (int)nh;
  row[LC2IS_AUG_NW] = (int)nw;
  row[LC2IS_AUG_TOP] = (int)(((unsigned long long)aug_u24(h, 1) * (unsigned long long)(fh + 1)) >> 24);
  row[LC2IS_AUG_LEFT] = (int)(((unsigned long long)aug_u24(h, 2) * (unsigned long long)(fw + 1)) >> 24);
  row[LC2IS_AUG_FLIP] = aug_u24(h, 3) < cfg.flip_thr ? 1 : 0;

  // photometric steps folded into rgb' = M rgb + o (0..255 scale); one clamp, in aug_apply
  float M[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, o[3] = {0.f, 0.f, 0.f};
  if (aug_u24(h, 4) < cfg.photo_thr[0]) {
    const float d = aug_range(aug_u24(h, 5), -cfg.brightness_delta, cfg.brightness_delta);
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] += d;
  }
  if (aug_u24(h, 6) < cfg.photo_thr[1]) {
    const float c = aug_range(aug_u24(h, 7), cfg.contrast_lo, cfg.contrast_hi);
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] *= c;
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] *= c;
  }
  if (aug_u24(h, 8) < cfg.photo_thr[2]) {
    aug_saturation(aug_range(aug_u24(h, 9), cfg.saturation_lo, cfg.saturation_hi), M, o);
  }
  if (aug_u24(h, 10) < cfg.photo_thr[3]) {
    const float a = aug_range(aug_u24(h, 11), -cfg.hue_delta, cfg.hue_delta);
    aug_hue(cosf(a), sinf(a), M, o);
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) row[LC2IS_AUG_M + e] = __builtin_bit_cast(int, M[e]);
#pragma unroll
  for (int e = 0; e < 3; ++e) row[LC2IS_AUG_O + e] = __builtin_bit_cast(int, o[e]);
#pragma unroll
  for (int e = LC2IS_AUG_O + 3; e < AUG_P; ++e) row[e] = 0;
}

__device__ __forceinline__ int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct AugSample {   // block-uniform: one sample per blockIdx.y
  bool valid;
  int H, W, nh, nw, top, left, flip;
  long long img_off, lab_off;
};
__device__ __forceinline__ AugSample aug_sample(const lc2is_aug_image* __restrict__ desc, long n_images,
                                                const int64_t* __restrict__ slots, const int32_t* __restrict__ prow,
                                                size_t img_bytes, size_t lab_bytes) {
  AugSample s;
  const long long slot = slots[blockIdx.y];
  s.valid = slot >= 0 && slot < n_images;
  const lc2is_aug_image d = s.valid ? desc[slot] : lc2is_aug_image{0, 0, 0, 0};
  s.H = d.H; s.W = d.W; s.img_off = d.img_off; s.lab_off = d.lab_off;
  s.nh = prow[LC2IS_AUG_NH]; s.nw = prow[LC2IS_AUG_NW];
  s.top = prow[LC2IS_AUG_TOP]; s.left = prow[LC2IS_AUG_LEFT]; s.flip = prow[LC2IS_AUG_FLIP];
  s.valid = s.valid && s.H >= 1 && s.W >= 1 && s.H <= LC2IS_AUG_MAX_SIDE && s.W <= LC2IS_AUG_MAX_SIDE && s.nh >= 1 && s.nw >= 1 &&
            s.nh <= LC2IS_AUG_MAX_RESIZED && s.nw <= LC2IS_AUG_MAX_RESIZED && s.img_off >= 0 && s.lab_off >= 0 &&
            (unsigned long long)s.img_off + (unsigned long long)s.H * s.W * 3 + 5 <= img_bytes &&
            (unsigned long long)s.lab_off + (unsigned long long)s.H * s.W <= lab_bytes;
  return s;
}

__device__ __forceinline__ i32x2_t aug_load8(const unsigned char* p) {   // unaligned: one global_load_dwordx2
  i32x2_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ float aug_byte(i32x2_t v, int k) {   // byte k of the 8 (k constant after unrolling)
  return (float)(((unsigned)(k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 0xffu);
}

__global__ __launch_bounds__(256) void aug_apply_kernel(const unsigned char* __restrict__ img, size_t img_bytes,
                                                         const unsigned char* __restrict__ lab, size_t lab_bytes,
                                                         const lc2is_aug_image* __restrict__ desc, long n_images,
                                                         const int64_t* __restrict__ slots, const int32_t* __restrict__ params,
                                                         int S, int L, int img_blocks, const lc2is_aug_norm norm, long pad_label,
                                                         float* __restrict__ out_img, int64_t* __restrict__ out_lab) {
  const int b = blockIdx.y;
  const int32_t* prow = params + (size_t)b * AUG_P;
  const AugSample s = aug_sample(desc, n_images, slots, prow, img_bytes, lab_bytes);
  const int dy = 2 * s.nh, dx = 2 * s.nw;
  const float rdy = __builtin_amdgcn_rcpf((float)dy), rdx = __builtin_amdgcn_rcpf((float)dx);

  if ((int)blockIdx.x >= img_blocks) {   // ---- label cells ----
    const int cell = ((int)blockIdx.x - img_blocks) * 256 + threadIdx.x;
    if (cell >= L * L) return;
    int cj;
    const int ci = aug_div(cell, L, __builtin_amdgcn_rcpf((float)L), cj);
    int yr, xr, ys, xs;
    long v = pad_label;
    if (aug_cell_pos(s.valid, ci, cj, S / L, S, s.top, s.left, s.flip, s.nh, s.nw, yr, xr)) {
      aug_cell_src(yr, xr, s.H, s.W, dy, dx, rdy, rdx, ys, xs);
      v = lab[s.lab_off + (long long)ys * s.W + xs];
    }
    out_lab[((size_t)b * L + ci) * L + cj] = v;
    return;
  }

  // ---- image: 4 consecutive output x per lane, all 3 channels ----
  const int W4 = S >> 2;
  const int p = (int)blockIdx.x * 256 + threadIdx.x;
  if (p >= S * W4) return;
  int jq;
  const int i = aug_div(p, W4, __builtin_amdgcn_rcpf((float)W4), jq);
  const int j0 = jq * 4;
  float* dst = out_img + ((size_t)b * 3 * S + i) * S + j0;
  const size_t plane = (size_t)S * S;
  const int yr = (int)((unsigned)s.top + (unsigned)i);
  const bool row_in = s.valid && (unsigned)yr < (unsigned)s.nh;
  if (!__builtin_amdgcn_ballot_w64(row_in)) {   // the whole wave is padding (wave-uniform branch)
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) *(f32x4_t*)(dst + c * plane) = z;
    return;
  }
  // s.valid holds from here on (it is block-uniform and part of row_in); every coordinate is clamped into the image, so the reads
  // are in bounds also for the lanes that turn out to be padding
  const int H = s.H, W = s.W;
  int ry;
  const int ny = aug_clampi((2 * aug_clampi(yr, 0, s.nh - 1) + 1) * H - s.nh, 0, dy * (H - 1));
  const int y0 = aug_div(ny, dy, rdy, ry);
  const int y1 = y0 + 1 < H ? y0 + 1 : H - 1;
  const float fy = (float)ry * rdy;
  const unsigned char* base = img + s.img_off;
  const unsigned char* r0 = base + (size_t)y0 * W * 3;
  const unsigned char* r1 = base + (size_t)y1 * W * 3;

  i32x2_t t0[4], t1[4];
  float fx[4];
  bool in[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = j0 + k;
    const int xr = (int)((unsigned)s.left + (unsigned)(s.flip ? S - 1 - j : j));
    in[k] = row_in && (unsigned)xr < (unsigned)s.nw;
    int rx;
    const int nx = aug_clampi((2 * aug_clampi(xr, 0, s.nw - 1) + 1) * W - s.nw, 0, dx * (W - 1));
    const int x0 = aug_div(nx, dx, rdx, rx);
    fx[k] = (float)rx * rdx;   // 0 at x0 == W - 1, where the second pixel of the read lies past the row and has no weight
    t0[k] = aug_load8(r0 + 3 * x0);
    t1[k] = aug_load8(r1 + 3 * x0);
  }
  const ColourMap km = colour_load(prow, LC2IS_AUG_M);

  f32x4_t out[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p00 = aug_byte(t0[k], c), p01 = aug_byte(t0[k], 3 + c), p10 = aug_byte(t1[k], c), p11 = aug_byte(t1[k], 3 + c);
      const float h0 = p00 + fx[k] * (p01 - p00), h1 = p10 + fx[k] * (p11 - p10);
      a[c] = h0 + fy * (h1 - h0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = (colour_apply(km, a, c) * (1.0f / 255.0f) - norm.mean[c]) * norm.inv_std[c];
      out[c][k] = in[k] ? v : 0.f;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) *(f32x4_t*)(dst + c * plane) = out[c];   // plain (write-back) stores: patchify reads them next
}

// ---- class-ratio crop re-draw (mmseg RandomCrop(cat_max_ratio)) and the per-image label histogram ----
// Both count uint8 labels with the wave histogram of label_hist.h: no read-modify-write atomic, the same bytes every run.
constexpr int LH_THREADS = 1024;
constexpr int LH_WAVES = LH_THREADS / 64;
constexpr int LH_UNROLL = 4;   // independent one-byte loads in flight per lane

struct LabSample {   // block-uniform
  bool valid;
  int H, W;
  long long lab_off;
};
__device__ __forceinline__ LabSample lab_sample(const lc2is_aug_image* __restrict__ desc, long n_images, long long slot,
                                                size_t lab_bytes) {
  LabSample s;
  s.valid = slot >= 0 && slot < n_images;
  const lc2is_aug_image d = s.valid ? desc[slot] : lc2is_aug_image{0, 0, 0, 0};
  s.H = d.H; s.W = d.W; s.lab_off = d.lab_off;
  s.valid = s.valid && s.H >= 1 && s.W >= 1 && s.H <= LC2IS_AUG_MAX_SIDE && s.W <= LC2IS_AUG_MAX_SIDE && s.lab_off >= 0 &&
            (unsigned long long)s.lab_off + (unsigned long long)s.H * s.W <= lab_bytes;
  return s;
}

// One block per sample walks the candidates in order and leaves at the first accepted one.  Per candidate: every lane gathers
// LH_UNROLL label cells per round (aug_cell_pos / aug_cell_src: the cells aug_apply_kernel's label branch writes), the waves count them in
// their LDS rows, 256 lanes add the rows in wave order and four waves reduce n = sum, m = max, d = classes present; the verdict
// d > 1 && m * 1024 < ratio1024 * n is block-uniform.  Lane 0 writes the chosen (top, left) into the row and {t*, n, m, d} to info.
__global__ __launch_bounds__(LH_THREADS) void aug_crop_select_kernel(const unsigned char* __restrict__ lab, size_t lab_bytes,
                                                                      const lc2is_aug_image* __restrict__ desc, long n_images,
                                                                      const int64_t* __restrict__ slots, const int64_t* __restrict__ keys,
                                                                      const int32_t* __restrict__ epoch, unsigned seed_lo,
                                                                      unsigned seed_hi, int S, int L, int ratio1024, int ignore_label,
                                                                      int tries, int32_t* params, int32_t* info) {
  __shared__ unsigned s_hist[LH_WAVES * LH_BINS];
  __shared__ unsigned s_red[LH_BINS / 64][3];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int32_t* row = params + (size_t)b * AUG_P;
  int32_t* irow = info ? info + (size_t)b * 4 : nullptr;
  const long long slot = slots[b];
  const LabSample s = lab_sample(desc, n_images, slot, lab_bytes);
  const int nh = row[LC2IS_AUG_NH], nw = row[LC2IS_AUG_NW], flip = row[LC2IS_AUG_FLIP];
  int top = row[LC2IS_AUG_TOP], left = row[LC2IS_AUG_LEFT];   // candidate 0: the row's own draw
  if (!(s.valid && nh >= 1 && nw >= 1 && nh <= LC2IS_AUG_MAX_RESIZED && nw <= LC2IS_AUG_MAX_RESIZED)) {   // block-uniform
    if (tid == 0 && irow) { irow[0] = -1; irow[1] = 0; irow[2] = 0; irow[3] = 0; }
    return;
  }
  const unsigned h = aug_key(seed_lo, seed_hi, *epoch, keys ? (long long)keys[b] : slot);
  const unsigned long long fh1 = (unsigned long long)(nh > S ? nh - S : 0) + 1, fw1 = (unsigned long long)(nw > S ? nw - S : 0) + 1;
  const int q = S / L, LL = L * L, H = s.H, W = s.W;
  const int dy = 2 * nh, dx = 2 * nw;
  const float rL = __builtin_amdgcn_rcpf((float)L), rdy = __builtin_amdgcn_rcpf((float)dy), rdx = __builtin_amdgcn_rcpf((float)dx);
  const unsigned char* src = lab + s.lab_off;
  unsigned* mine = s_hist + wid * LH_BINS;
  int pick = tries;
  unsigned pn = 0u, pm = 0u, pd = 0u;
  for (int t = 0; t < tries; ++t) {
    if (t > 0) {
      top = (int)(((unsigned long long)aug_u24(h, 10u + 2u * t) * fh1) >> 24);
      left = (int)(((unsigned long long)aug_u24(h, 11u + 2u * t) * fw1) >> 24);
    }
    lh_wave_clear(mine);
    for (int base = 0; base < LL; base += LH_THREADS * LH_UNROLL) {   // block-uniform trip count
      unsigned v[LH_UNROLL];
      bool counted[LH_UNROLL];
#pragma unroll
      for (int e = 0; e < LH_UNROLL; ++e) {
        int cell = base + e * LH_THREADS + tid;
        bool in = cell < LL;
        cell = in ? cell : 0;
        int cj;
        const int ci = aug_div(cell, L, rL, cj);
        int yr, xr;
        in = aug_cell_pos(in, ci, cj, q, S, top, left, flip, nh, nw, yr, xr);   // outside: padding, not counted
        v[e] = 0u;
        if (in) {
          int ys, xs;
          aug_cell_src(yr, xr, H, W, dy, dx, rdy, rdx, ys, xs);
          v[e] = src[(long long)ys * W + xs];
        }
        counted[e] = in && (int)v[e] != ignore_label;
      }
#pragma unroll
      for (int e = 0; e < LH_UNROLL; ++e) lh_wave_add(mine, v[e], counted[e]);
    }
    __syncthreads();
    if (wid < LH_BINS / 64) {   // whole waves: lane tid holds class tid
      const unsigned nc = lh_block_sum(s_hist, LH_WAVES, tid);
      unsigned sum = nc, mx = nc;
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        sum += (unsigned)__shfl_xor((int)sum, off);
        const unsigned o = (unsigned)__shfl_xor((int)mx, off);
        mx = o > mx ? o : mx;
      }
      const unsigned present = (unsigned)__popcll(__ballot(nc > 0u));
      if (lane == 0) { s_red[wid][0] = sum; s_red[wid][1] = mx; s_red[wid][2] = present; }
    }
    __syncthreads();   // the rows are read: the next candidate may clear them; s_red is written again only after its first barrier
    unsigned n = 0u, m = 0u, d = 0u;
#pragma unroll
    for (int w = 0; w < LH_BINS / 64; ++w) {
      n += s_red[w][0];
      m = s_red[w][1] > m ? s_red[w][1] : m;
      d += s_red[w][2];
    }
    if (d > 1u && (long long)m * 1024 < (long long)ratio1024 * (long long)n) {   // block-uniform
      pick = t; pn = n; pm = m; pd = d;
      break;
    }
  }
  if (pick == tries) {   // none accepted: one more draw, taken unchecked
    top = (int)(((unsigned long long)aug_u24(h, 10u + 2u * tries) * fh1) >> 24);
    left = (int)(((unsigned long long)aug_u24(h, 11u + 2u * tries) * fw1) >> 24);
  }
  if (tid == 0) {
    row[LC2IS_AUG_TOP] = top;
    row[LC2IS_AUG_LEFT] = left;
    if (irow) { irow[0] = pick; irow[1] = (int)pn; irow[2] = (int)pm; irow[3] = (int)pd; }
  }
}

// One block per image, block-stride over its H * W labels: a wave reads 64 neighbouring bytes per load, LH_UNROLL loads in flight.
__global__ __launch_bounds__(LH_THREADS) void label_hist_kernel(const unsigned char* __restrict__ lab, size_t lab_bytes,
                                                                 const lc2is_aug_image* __restrict__ desc, long n_images,
                                                                 const int64_t* __restrict__ slots, int32_t* __restrict__ counts) {
  __shared__ unsigned s_hist[LH_WAVES * LH_BINS];
  const int b = blockIdx.x, tid = threadIdx.x, wid = tid >> 6;
  int32_t* out = counts + (size_t)b * LH_BINS;
  const LabSample s = lab_sample(desc, n_images, slots[b], lab_bytes);
  if (!s.valid) {   // block-uniform
    if (tid < LH_BINS) out[tid] = 0;
    return;
  }
  const int n = s.H * s.W;   // <= 2^24
  const unsigned char* src = lab + s.lab_off;
  unsigned* mine = s_hist + wid * LH_BINS;
  lh_wave_clear(mine);
  for (int base = 0; base < n; base += LH_THREADS * LH_UNROLL) {   // block-uniform trip count
    unsigned v[LH_UNROLL];
    bool in[LH_UNROLL];
#pragma unroll
    for (int e = 0; e < LH_UNROLL; ++e) {
      const int p = base + e * LH_THREADS + tid;
      in[e] = p < n;
      v[e] = in[e] ? (unsigned)src[p] : 0u;
    }
#pragma unroll
    for (int e = 0; e < LH_UNROLL; ++e) lh_wave_add(mine, v[e], in[e]);
  }
  __syncthreads();
  if (tid < LH_BINS) out[tid] = (int)lh_block_sum(s_hist, LH_WAVES, tid);
}

}  // namespace

extern "C" int lc2is_aug_params(const int64_t* slots, const int64_t* keys, int B, const int32_t* epoch, const lc2is_aug_image* desc,
                                long n_images, const lc2is_aug_config* cfg, int32_t* params, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!slots || !epoch || !desc || !cfg || !params) return LC2IS_ERR_NULL;
  if (B <= 0 || n_images <= 0 || cfg->crop_size <= 0 || cfg->crop_size > LC2IS_AUG_MAX_SIDE || cfg->base_size <= 0 ||
      cfg->base_size > 65536 || cfg->ratio_lo1024 < 1 || cfg->ratio_hi1024 < cfg->ratio_lo1024 || cfg->ratio_hi1024 > (1 << 20) ||
      cfg->flip_thr > (1u << 24))
    return LC2IS_ERR_SHAPE;
  for (int e = 0; e < 4; ++e)
    if (cfg->photo_thr[e] > (1u << 24)) return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(aug_params_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, slots, keys, B, epoch, desc, n_images, *cfg, params);
  return lc2is_check_launch();
}

extern "C" int lc2is_aug_apply(const uint8_t* img, size_t img_bytes, const uint8_t* lab, size_t lab_bytes,
                               const lc2is_aug_image* desc, long n_images, const int64_t* slots, const int32_t* params, int B, int S,
                               int L, const lc2is_aug_norm* norm, long pad_label, float* out_img, int64_t* out_lab,
                               lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!img || !lab || !desc || !slots || !params || !norm || !out_img || !out_lab) return LC2IS_ERR_NULL;
  if (B <= 0 || B > 65535 || n_images <= 0 || S <= 0 || S > LC2IS_AUG_MAX_SIDE || (S & 3) || L <= 0 || S % L ||
      ((uintptr_t)out_img & 15) || ((uintptr_t)out_lab & 7) || ((uintptr_t)params & 3) || ((uintptr_t)desc & 7))
    return LC2IS_ERR_SHAPE;
  const int img_blocks = (S * (S >> 2) + 255) / 256, lab_blocks = (L * L + 255) / 256;
  hipLaunchKernelGGL(aug_apply_kernel, dim3(img_blocks + lab_blocks, B), dim3(256), 0, stream, img, img_bytes, lab, lab_bytes, desc,
                     n_images, slots, params, S, L, img_blocks, *norm, pad_label, out_img, out_lab);
  return lc2is_check_launch();
}

extern "C" int lc2is_aug_crop_select(const uint8_t* lab, size_t lab_bytes, const lc2is_aug_image* desc, long n_images,
                                     const int64_t* slots, const int64_t* keys, int B, const int32_t* epoch, const lc2is_aug_config* cfg,
                                     int32_t* params, int L, int ratio1024, int ignore_label, int tries, int32_t* info,
                                     lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!lab || !desc || !slots || !epoch || !cfg || !params) return LC2IS_ERR_NULL;
  const int S = cfg->crop_size;
  if (B <= 0 || n_images <= 0 || S <= 0 || S > LC2IS_AUG_MAX_SIDE || L <= 0 || S % L || ratio1024 < 1 || ratio1024 > 1023 ||
      ignore_label < -1 || ignore_label > 255 || tries < 1 || tries > LC2IS_AUG_MAX_TRIES || ((uintptr_t)params & 3) ||
      ((uintptr_t)info & 3) || ((uintptr_t)desc & 7))
    return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(aug_crop_select_kernel, dim3(B), dim3(LH_THREADS), 0, stream, lab, lab_bytes, desc, n_images, slots, keys, epoch,
                     cfg->seed_lo, cfg->seed_hi, S, L, ratio1024, ignore_label, tries, params, info);
  return lc2is_check_launch();
}

extern "C" int lc2is_label_histogram(const uint8_t* lab, size_t lab_bytes, const lc2is_aug_image* desc, long n_images,
                                     const int64_t* slots, int B, int32_t* counts, lc2is_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!lab || !desc || !slots || !counts) return LC2IS_ERR_NULL;
  if (B <= 0 || n_images <= 0 || ((uintptr_t)counts & 3) || ((uintptr_t)desc & 7)) return LC2IS_ERR_SHAPE;
  hipLaunchKernelGGL(label_hist_kernel, dim3(B), dim3(LH_THREADS), 0, stream, lab, lab_bytes, desc, n_images, slots, counts);
  return lc2is_check_launch();
}
