/* lc2is_hip.h — C ABI of liblc2is_hip.so, the MI355X (gfx950) kernels behind the LC2IS hot path.
 *
 * The reference (AntoineBlanot/LC2IS) has no FFI layer: its hot path is PyTorch / transformers operator
 * calls inside nn.Module.forward.  Each entry point below replaces one such operator
 * call (forward or its autograd backward); the citation after "replaces:" is the reference call site
 * (paths relative to the reference root; "hf:" = transformers/models/clip/modeling_clip.py, "torch:" =
 * torch/nn).  INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes; no torch types.  All pointers are DEVICE pointers unless noted.
 *   - bf16 tensors are raw uint16 bit patterns (void* here); fp32 tensors are float*.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, allocates
 *     nothing, keeps no global mutable state; workspaces are caller-owned.
 *   - return value: 0 = launched; negative = refused before any launch (LC2IS_ERR_*).  Never throws.
 *   - row-major 2-D operands carry an explicit leading dimension (elements).
 */
#ifndef LC2IS_HIP_H
#define LC2IS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC2IS_ACT_NONE 0
#define LC2IS_ACT_QUICK_GELU 1  /* x*sigmoid(1.702x), hf:activations.py:122-123                      */
#define LC2IS_ACT_RELU 2        /* F.relu default of model/decoder.py:11                                */
#define LC2IS_ACT_DQUICK_GELU 3 /* backward: acc * quick_gelu'(aux_in)                                  */
#define LC2IS_ACT_DRELU 4       /* backward: acc * (aux_in > 0)                                          */
#define LC2IS_ACT_QUICK_GELU_GRAD 5 /* forward: out = quick_gelu(z), aux_out = quick_gelu'(z) (bf16) — saves the
                                      backward's transcendentals; pair with LC2IS_ACT_MUL_AUX            */
#define LC2IS_ACT_MUL_AUX 6     /* backward: acc * aux_in (aux_in = the derivative saved by code 5)     */
#define LC2IS_ACT_GELU_ERF 7    /* exact GELU 0.5x(1+erf(x/sqrt2)), hf:activations.py "gelu" (Swin MLP) */
#define LC2IS_ACT_DGELU_ERF 8   /* backward: acc * gelu'(aux_in)                                         */
#define LC2IS_ACT_ADD_AUX 9     /* acc + bias + aux_in: the residual add of a bf16 residual stream (`x + out_proj(..)`,
                                   `x + fc2(..)` of hf CLIPEncoderLayer.forward:362-383), fp32 add, one rounding */

#define LC2IS_INTERP_BICUBIC 0  /* F.interpolate(mode="bicubic", align_corners=False), A = -0.75, border clamp */
#define LC2IS_INTERP_BILINEAR 1 /* F.interpolate(mode="bilinear", align_corners=False)                          */

typedef void* lc2is_stream_t; /* hipStream_t */

/* Base addresses of the dense hot-path operands (lc2is_gemm_nt_* / gemm_tn_* / colsum, layernorm, attention, dropout_rows, swin_attn).
 * The kernels issue 8- and 16-byte accesses; the `ld %` rules of an entry point make every ROW as aligned as the first, so the
 * base has to be:
 *   - bf16 rows with ld % 8 == 0: 16 bytes;  bf16 rows of an entry that admits ld % 4 == 0, with such an ld: 8 bytes;
 *   - fp32 rows (ld % 4 == 0): 16 bytes;
 *   - vectors without an ld: 16 bytes where the kernel reads them as float4 (bias of the NT GEMMs, gamma / beta), else 4 (db,
 *     dgamma / dbeta, mean / rstd, lse, delta, kbias, the Swin bias tables).
 * A pointer below its rule is refused with LC2IS_ERR_SHAPE, next to the ld checks, before any launch.  NULL passes (optional
 * operands are tested for NULL elsewhere). */
#define LC2IS_MISALIGNED(p, bytes) ((p) != NULL && ((uintptr_t)(p) & ((uintptr_t)(bytes) - 1u)) != 0)
#define LC2IS_MISALIGNED_BF16(p, ld) LC2IS_MISALIGNED(p, ((ld) % 8) ? 8 : 16)
#define LC2IS_MISALIGNED_F32(p) LC2IS_MISALIGNED(p, 16)

/* One fp32 master weight [N,K] (contiguous) and its bf16 shadows; see lc2is_shadow_refresh. */
typedef struct {
  const void* src; /* fp32 [N,K]                                               */
  void* dst;       /* bf16 [N, ld_dst]  row-major copy (forward GEMM operand), may be NULL */
  void* dstT;      /* bf16 [K, ld_dstT] transposed copy (dgrad GEMM operand), may be NULL  */
  int N, K, ld_dst, ld_dstT;
  int tile_start;  /* exclusive prefix sum of ceil(N/64)*ceil(K/64) over the table          */
  int flags;       /* bit 0: dst is fp32 and receives a plain copy (fused bias vectors); dstT unused     */
} lc2is_shadow_desc;

/* ABI / build identification: returns a static string "lc2is_hip <abi> gfx950". Host memory. */
const char* lc2is_version(void);

/* Compute units the GEMM tile planners may count on (0 = all 256, the default).  The large-tile kernels run one block per CU and
 * their plans are whole rounds of the CUs; a CU held by another queue's kernel for the duration (RCCL's channels while gradients
 * are reduced under the backward pass) would turn "exactly one round" into two.  With a budget n the persistent kernels launch n
 * blocks and every round count is taken over n CUs.  Process-wide.  The NT GEMM plans are bitwise equal under any budget; the
 * weight-gradient plans (lc2is_gemm_tn_bf16 / _grouped) choose their M-split count from it, i.e. the ORDER of their fp32 partial
 * sums: their results move in the last bits with the budget (each call reads the budget once and is reproducible for a given value).
 * replaces: nothing in the reference (torch DDP leaves this to the vendor GEMM library's heuristics). */
int lc2is_set_cu_budget(int ncu);
int lc2is_get_cu_budget(void);

/* ---- dense layers ------------------------------------------------------------------------------
 * out[M,N] = epi(A[M,K] · W[N,K]^T + bias[N]) (+ resid[M,N]); K % 64 == 0, N % 4 == 0.
 * act: QUICK_GELU/RELU apply after bias and (if aux_out) store the pre-activation as bf16;
 *      DQUICK_GELU/DRELU multiply by the activation derivative at aux_in (saved pre-activation /
 *      saved relu output) — used by the dgrad of fc1 / linear1.
 * Either or both of out_bf16 / out_f32 may be given.  tile_cfg 0 = auto (the plan: exact rounds of 256x256 or 256x384 tiles over
 * the chip's 256 CUs, persistent form for bf16 outputs, the <= 64 ragged rows of B x 1025-token inputs computed inside the same
 * launch); a non-zero tile_cfg forces one kernel for tests and A/B (1-3 register-staged 128x128 / 256x128 / 64x64, 4 / 6 LDS-DMA
 * 256x256 / 128x128, 15 persistent 256x256, 16 = 256x384 [N % 384 == 0, no activation, fp32-only or bf16-only output], 17 = row
 * kernel for M <= 64) and returns LC2IS_ERR_UNSUPPORTED where that kernel does not take the problem.  Every plan gives bitwise the
 * same result as tile_cfg 4.
 * replaces: nn.Linear.forward at hf:CLIPAttention.forward (q/k/v/out_proj), hf:CLIPMLP.forward,
 *   torch:nn/functional.py multi_head_attention_forward in/out projections, DecoderLayer linear1/2
 *   (model/decoder.py:9-21), TextToPatch.forward (model/text_patch.py:14-19),
 *   torch.matmul(feature_v, feature_t.T) (model/model.py:50), and — with W^T shadows — their dgrads. */
int lc2is_gemm_nt_bf16(const void* A, int lda, const void* W, int ldw, const float* bias,
                       const float* resid, int ldr, const void* aux_in, int ldx, void* out_bf16, int ldo,
                       float* out_f32, int ldf, void* aux_out, int ldy, int M, int N, int K, int act,
                       int tile_cfg, lc2is_stream_t stream);

/* The plan lc2is_gemm_nt_bf16 runs for the same arguments under the present CU budget, without launching anything (no GPU is
 * needed; pointers are only tested for NULL).  A plan is one or two launches: kernel `cfg` over rows [row0, row0 + rows) with
 * `tail_rows` further ragged rows computed inside that launch; the records tile [0, M).  off_* are the bytes by which the
 * launch's pointers lie past the caller's (0 for an absent one).  Returns the number of records (at most `cap` are written) or
 * the error code lc2is_gemm_nt_bf16 would return.  All NT kernels give bitwise the same output, so this is the only way a test
 * can see which one the dispatch picks. */
typedef struct {
  int cfg, row0, rows, tail_rows;
  int staged_epi; /* epilogue through LDS: 0 no, 1 bf16 traffic, 2 fp32-only output */
  long long off_a, off_resid, off_aux_in, off_out_bf16, off_out_f32, off_aux_out;
} lc2is_gemm_nt_launch;
int lc2is_gemm_nt_plan(const void* A, int lda, const void* W, int ldw, const float* bias, const float* resid, int ldr,
                       const void* aux_in, int ldx, void* out_bf16, int ldo, float* out_f32, int ldf, void* aux_out, int ldy,
                       int M, int N, int K, int act, int tile_cfg, lc2is_gemm_nt_launch* out, int cap);

/* The residual-stream GEMM and the LayerNorm that follows it in ONE launch (round 5): out_f32 = A.W^T + bias (+ resid) as
 * lc2is_gemm_nt_bf16 writes it, and ln_out = bf16((out_f32 - mean) * rstd * gamma + beta) per row over the N columns (mean, rstd
 * fp32 [M], may be NULL).  N = 384 or 768, M >= 256; runs on 256x384 tiles whose two column tiles exchange their row statistics
 * (two-pass variance, halves combined in a fixed order: reproducible) through `xchg` (>= lc2is_gemm_nt_ln_xchg_bytes, 8-byte
 * aligned, ALL ZERO before the first call; the kernel leaves it all zero again — one buffer per stream that may run such a launch).
 * The <= 64 ragged rows of B x 1025-token inputs are computed inside the launch and normalised by a small second launch.
 * Returns LC2IS_ERR_UNSUPPORTED for shapes it does not take: call lc2is_gemm_nt_bf16 and lc2is_layernorm_fwd instead.
 * replaces: out_proj / fc2 + residual add followed by layer_norm2 / the next layer's layer_norm1 in hf:CLIPEncoderLayer.forward
 *   (modeling_clip.py:362-383), reached from model/encoder.py:29-30. */
size_t lc2is_gemm_nt_ln_xchg_bytes(int M, int N);
int lc2is_gemm_nt_ln_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, const float* resid, int ldr,
                          float* out_f32, int ldf, const float* gamma, const float* beta, float eps, void* ln_out, int ldl,
                          float* mean, float* rstd, void* xchg, size_t xchg_bytes, int M, int N, int K, lc2is_stream_t stream);

/* Strided-batched plain product, ONE launch: for b < batch, out[b][M,N] = A[b][M,K] · W[b][N,K]^T (no bias / activation);
 * stride_* are ELEMENT strides between consecutive problems (stride_a, stride_w multiples of 8, outputs multiples of 4).
 * replaces: torch.einsum('bchw,bkc->bkhw', visual, text) with per-image class embeddings (reference
 *   model/final.py:355, model/model.py:161,210, model/ftn.py:60) and, on transposed operands, its backward. */
int lc2is_gemm_nt_bf16_batched(const void* A, int lda, long stride_a, const void* W, int ldw, long stride_w,
                               void* out_bf16, int ldo, long stride_ob, float* out_f32, int ldf, long stride_of,
                               int M, int N, int K, int batch, lc2is_stream_t stream);

/* dW[N,K] (fp32) = dY[M,N]^T · X[M,K]  (weight gradient of out = X·W^T), reduced over M.
 * The M range is cut into `splits` slabs (workspace = splits*N*K fp32) summed by a second launch, so
 * the result is bitwise reproducible.  accumulate != 0 adds into dW instead of overwriting.
 * db (optional, fp32 [N]): the bias gradient colsum(dY), fused (one extra ones-fragment MFMA per tile).
 * N % 8 == 0 and K % 8 == 0.   replaces: autograd of the nn.Linear calls above. */
size_t lc2is_gemm_tn_workspace_bytes(int M, int N, int K);
int lc2is_gemm_tn_bf16(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, float* db, int M,
                       int N, int K, int accumulate, void* workspace, size_t workspace_bytes,
                       lc2is_stream_t stream);

/* The plan lc2is_gemm_tn_bf16 runs for densely packed operands of this shape under the present CU budget and overrides
 * (LC2IS_GEMM_TN_CFG), without launching anything: no GPU is needed.  The split count fixes the order of the fp32 partial sums,
 * so this plan decides result bits, not only speed.  Returns the code the launcher would return for the shape. */
typedef struct {
  int big;        /* kernel form: 1 = 256x256 LDS-DMA tiles, 0 = 128x128 register-staged tiles */
  int ntn, ntk;   /* output tiles along N and K */
  int splits;     /* ranges the M rows are cut into; > 1: each writes a slab, a second launch sums them in order */
  int chunk;      /* rows per range, a multiple of 64 */
  int grid;       /* blocks of the main launch = ntn * ntk * splits */
  int red_grid;   /* slab blocks of the reduce launch, 0 when splits == 1 (a db adds ceil(N / 256) blocks behind them) */
  long long workspace_bytes;   /* = lc2is_gemm_tn_workspace_bytes(M, N, K) */
} lc2is_tn_plan;
int lc2is_gemm_tn_plan(int M, int N, int K, lc2is_tn_plan* out);

/* Grouped form: up to LC2IS_TN_GROUP_MAX weight gradients (one transformer layer — q, k, v, out-proj, fc1, fc2, each the
 * autograd of an nn.Linear call listed above — or a whole tower's: 12 layers = 72 problems = 1296 output tiles, scheduled as
 * full-length blocks plus a few finely split problems that fill the last round of CUs) in ONE grid and one ordered-reduce
 * launch.  Up to 16 problems travel as kernel arguments.  More than 16: the descriptor table is uploaded into the front of the
 * workspace (one small H2D copy on `stream` from a pinned host image).  Such a call can be captured into a hipGraph: the copy
 * becomes a memcpy node that re-reads its host image at every replay, so a captured call gets an image of its own that the
 * library keeps for the graph (see lc2is_release_captured_tables below).  N and K multiples of 8; a group whose N and K are all
 * multiples of 256 runs on the 256x256 LDS-DMA tiles, any other (the Swin blocks) on 128x128 tiles.  Same results contract: fp32,
 * bitwise reproducible, db (optional) = column sums of dY, `accumulate` adds to dW / db. */
#define LC2IS_TN_GROUP_MAX 128
typedef struct lc2is_tn_problem {
  const void* dY; const void* X; float* dW; float* db;
  int ldy, ldx, ldw, M, N, K, accumulate;
} lc2is_tn_problem;
size_t lc2is_gemm_tn_grouped_workspace_bytes(const lc2is_tn_problem* problems, int n);
int lc2is_gemm_tn_grouped(const lc2is_tn_problem* problems, int n, void* workspace, size_t workspace_bytes,
                          lc2is_stream_t stream);

/* The plan lc2is_gemm_tn_grouped runs for the same problems under the present CU budget, without launching anything (no GPU is
 * needed; pointers are only tested for NULL): a summary and one record per problem in GRID order (at most `cap` are written).
 * Returns the code the launcher would return for the problems (LC2IS_ERR_NULL also for a missing `summary` / `recs`). */
typedef struct {
  int small;      /* 1: 128x128 register-staged body (some N or K off the 256 grid), 0: 256x256 LDS-DMA body */
  int table;      /* 1: descriptors uploaded into the front of the workspace (n > 16), 0: passed as kernel arguments */
  int grid, red_grid;          /* blocks of the main and of the reduce launch (0: no reduce launch) */
  long long workspace_bytes;   /* = lc2is_gemm_tn_grouped_workspace_bytes(problems, n), table_bytes included */
  long long table_bytes;
} lc2is_tn_group_plan;
typedef struct {
  int index;                    /* of the problem in the caller's list */
  int ntn, ntk, splits, chunk;  /* as in lc2is_tn_plan */
  int blk_end, red_end;         /* exclusive ends of the problem's block ranges in the main and the reduce grid */
  int red_blocks;               /* slab blocks among its reduce blocks (the rest sum the bias partials) */
  long long slab_offset, bias_offset;   /* bytes from the start of the workspace; -1: written straight to dW / db (or no db) */
} lc2is_tn_group_rec;
int lc2is_gemm_tn_grouped_plan(const lc2is_tn_problem* problems, int n, lc2is_tn_group_plan* summary, lc2is_tn_group_rec* recs,
                               int cap);

/* The pinned host image of a CAPTURED lc2is_gemm_tn_grouped call of more than 16 problems belongs to the graph that captured it
   and must outlive it; the library holds it until told otherwise.  lc2is_release_captured_tables frees
   every such image (returns how many): call it once ALL graphs captured so far have been destroyed.  Per-graph ownership:
   lc2is_captured_tables_mark() before and after a capture brackets the images that capture registered, and
   lc2is_release_captured_tables_range(first, last) frees exactly those once that graph is destroyed (lc2is_amd.step.TrainStep
   does, when a captured step is released or captured again) — other live graphs keep theirs.  Slots are never reused or
   removed (a released slot stays empty), so marks stay valid across either release call; the global release is for
   tear-down only — it also frees images of graphs that are still alive.  No reference counterpart (host-side resource
   management). */
int lc2is_release_captured_tables(void);
int lc2is_captured_tables_mark(void);
int lc2is_release_captured_tables_range(int first, int last);

/* db[N] (fp32) = column sums of dY[M,N] (bias gradient). workspace >= lc2is_colsum_workspace_bytes. */
size_t lc2is_colsum_workspace_bytes(int M, int N);
int lc2is_colsum_bf16(const void* dY, int ldy, float* db, int M, int N, int accumulate, void* workspace,
                      size_t workspace_bytes, lc2is_stream_t stream);

/* ---- LayerNorm -----------------------------------------------------------------------------------
 * y = (x - mean)/sqrt(var + eps) * gamma + beta over the last dim C (C % 4 == 0, C <= 2048);
 * x fp32 [M,C] (the residual stream is kept in fp32), y bf16; mean/rstd fp32 [M] saved for backward
 * (may be NULL in inference).  gamma/beta fp32, beta may be NULL (torch 2.10 bias=False drift).
 * replaces: nn.LayerNorm.forward at hf:CLIPEncoderLayer.forward:362-383, pre_layrnorm / final_layer_norm,
 *   norm1-3 of torch TransformerDecoderLayer (model/decoder.py:9). */
int lc2is_layernorm_fwd(const void* x, int ldx, int x_is_bf16, const float* gamma, const float* beta, void* y_bf16,
                        int ldy, float* y_f32, int ldyf, float* mean, float* rstd, int M, int C, float eps,
                        lc2is_stream_t stream);

/* dx = LN'(dy) (+ dres), written as fp32 and/or bf16; dgamma/dbeta accumulated over rows through
 * `workspace` (>= lc2is_layernorm_bwd_workspace_bytes) and a second launch (deterministic).
 * dy is bf16 [M,C] (the dgrad GEMM's output) or, if dy_f32 != NULL, fp32. */
size_t lc2is_layernorm_bwd_workspace_bytes(int M, int C);
int lc2is_layernorm_bwd(const void* dy_bf16, int lddy, const float* dy_f32, int lddyf, const void* x,
                        int ldx, int x_is_bf16, const float* gamma, const float* mean, const float* rstd,
                        const void* dres, int lddres, int dres_is_bf16, float* dx_f32, int lddx, void* dx_bf16,
                        int lddxb, float* dgamma, float* dbeta, int accumulate, int M, int C, void* workspace,
                        size_t workspace_bytes, lc2is_stream_t stream);

/* Deferred parameter gradients: a lc2is_layernorm_bwd call with dgamma == dbeta == NULL leaves its per-block partial
 * sums in `workspace` — lc2is_layernorm_bwd_partials(M, C) rows of [dgamma partial (C) | dbeta partial (C)] — and
 * lc2is_ln_partials_reduce sums the partials of up to LC2IS_LN_PARTIALS_MAX such calls in ONE launch (fixed-order sums:
 * bit-identical to the per-call second launch).  Items must not share an output vector (-> LC2IS_ERR_UNSUPPORTED).
 * replaces: the weight.grad / bias.grad accumulation of every nn.LayerNorm of a tower's backward (autograd of
 *   hf:CLIPEncoderLayer.forward:362-383; 50 latency-bound 13-us launches per train step become two). */
#define LC2IS_LN_PARTIALS_MAX 64
typedef struct {
  const float* partials; /* the workspace of the lc2is_layernorm_bwd call */
  float* dgamma;         /* [C] or NULL */
  float* dbeta;          /* [C] or NULL */
  int nparts;            /* lc2is_layernorm_bwd_partials(M, C) of that call */
  int C;
  int accumulate;        /* 0: overwrite, 1: add to the vectors */
} lc2is_ln_partials;
int lc2is_layernorm_bwd_partials(int M, int C);
int lc2is_ln_partials_reduce(const lc2is_ln_partials* items, int n, lc2is_stream_t stream);

/* ---- attention -----------------------------------------------------------------------------------
 * O[b,s,h,:] = softmax_k( scale * Q[b,s,h,:]·K[b,k,h,:] + kbias[b,k] (+ causal) ) · V[b,k,h,:]
 * Q/K/V/O are token-major 2-D views: row (b*S + s), head h in columns [h*D,(h+1)*D), row stride ld*
 * (elements) — Q, K, V may alias one packed projection buffer.  D in {64, 96, 128}.  Every ld* is a multiple of 8 (16-byte
 * row chunks: the operands by LDS-DMA, O and dQ by 16-byte stores), except lddk / lddv, which may be multiples of 4 (8-byte stores).
 * kbias: fp32 [B,Sk] additive key bias in natural-log units, NULL = none.  Per key it is any finite value or -inf
 * (masked); 0 / -inf is key_padding_mask / attention_mask, and the masked keys may be any subset, not only a suffix.
 * +inf and NaN are not allowed.  causal != 0 adds the lower-triangular mask (requires Sq == Sk).
 * lse2 (optional, fp32 [B,H,Sq]): log2-domain log-sum-exp of the scaled, biased, masked scores, saved for backward.
 * Empty rows: a query row with no visible key (every key -inf, the causal mask included) gives O = 0 and lse2 = -inf;
 * the backward gives that row dQ = 0 and takes nothing from it into dK / dV.  This deliberately differs from torch,
 * whose softmax over an all -inf row is NaN.
 * Masked keys: their dK / dV rows are 0, and their K / V rows do not influence any output — provided they are finite
 * (a masked probability is an exact 0, and 0 * NaN or 0 * Inf is NaN here as in torch).
 * tests/test_gpu_attention_masks.py holds all of this row by row against fp64.
 * replaces: hf:modeling_clip.py:259-277 eager_attention_forward (+ :298-335), and the attention core of
 *   torch:nn/functional.py multi_head_attention_forward used by model/decoder.py:9-21. */
int lc2is_attention_fwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                        int ldo, float* lse2, const float* kbias, int B, int H, int Sq, int Sk, int D,
                        float scale, int causal, lc2is_stream_t stream);

/* Backward of lc2is_attention_fwd: dQ, dK, dV (bf16, same 2-D strided views as Q/K/V — they may alias one
 * packed dQKV buffer) from dO, the forward's O and lse2.  `delta` is fp32 [B,H,Sq] scratch (rowsum(dO*O)).
 * kbias / causal as in the forward (the same values must be passed); empty rows and masked keys as stated there.
 * Two launches (dQ; then dK/dV), no atomics: bitwise reproducible.
 * replaces: autograd of the attention cores above (reference engine.py:100 loss.backward()). */
int lc2is_attention_bwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv,
                        const void* O, int ldo, const void* dO, int lddo, void* dQ, int lddq, void* dK,
                        int lddk, void* dV, int lddv, const float* lse2, float* delta, const float* kbias,
                        int B, int H, int Sq, int Sk, int D, float scale, int causal, lc2is_stream_t stream);

/* The same two operators with dropout on the attention probabilities (training mode of torch's
 * multi_head_attention_forward, dropout_p = the layer's `dropout`: torch:nn/functional.py:6206, reached from
 * PromptLayer model/decoder.py:24-28, the SR layers model/hierarchical.py:174-225 / model/decoder.py:113-134 and
 * nn.TransformerDecoderLayer at model/ftn.py:135).  No mask is stored: keep(seed, row=(b*H+h)*Sq+q, col=key) is a
 * counter-based hash evaluated in the forward and again in both backward kernels (csrc/common.h); survivors are scaled
 * by 1/(1-p).  The stream is this library's, not torch's Philox stream; lc2is_dropout_mask exports it for tests. */
int lc2is_attention_fwd_dropout(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                                int ldo, float* lse2, const float* kbias, int B, int H, int Sq, int Sk, int D,
                                float scale, int causal, float p_drop, unsigned long long seed, lc2is_stream_t stream);
int lc2is_attention_bwd_dropout(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv,
                                const void* O, int ldo, const void* dO, int lddo, void* dQ, int lddq, void* dK,
                                int lddk, void* dV, int lddv, const float* lse2, float* delta, const float* kbias,
                                int B, int H, int Sq, int Sk, int D, float scale, int causal, float p_drop,
                                unsigned long long seed, lc2is_stream_t stream);

/* ---- dropout / drop-path (training mode), mask never materialised ------------------------------------------------
 * dropout_rows_f32: y[m][c] = resid[m][c] + keep * x[m][c] / (1-p)   (resid optional; fp32 and / or bf16 output).
 *   rows_per_sample == 0: one Bernoulli(1-p) decision per element, coordinate (m, c) — nn.Dropout on a branch output
 *   (dropout1/2/3 of torch's Transformer layers) and, applied to a gradient with the forward's seed, its backward.
 *   rows_per_sample > 0: one decision per SAMPLE (row m belongs to sample m / rows_per_sample) — hf SwinDropPath
 *   (modeling_swin.py:280-302) and its backward.
 * dropout_rows_bf16: the same per-element form on bf16 (the dropout between activation and linear2).
 * dropout_mask: out[r][c] = keep(seed, r, c) as bytes — test / debug export of the decisions, never on the product path. */
int lc2is_dropout_rows_f32(const float* x, int ldx, const float* resid, int ldr, float* y32, int ldy, void* y16,
                           int ldy16, int M, int C, int rows_per_sample, float p, unsigned long long seed,
                           lc2is_stream_t stream);
int lc2is_dropout_rows_bf16(const void* x, int ldx, void* y, int ldy, int M, int C, float p, unsigned long long seed,
                            lc2is_stream_t stream);
int lc2is_dropout_mask(unsigned char* out, long rows, int cols, float p, unsigned long long seed, lc2is_stream_t stream);


/* ---- glue (all single-pass, HBM-bound) --------------------------------------------------------------
 * Refresh every bf16 weight shadow from the fp32 master copy in ONE launch: `descs` is a DEVICE array of
 * ndesc descriptors ordered by tile_start; total_tiles = sum of tile counts.  K % 4 == 0 always, N % 4 == 0
 * when dstT != NULL.  Several descriptors may target sub-blocks of one fused buffer (q/k/v -> [3C,C]). */
int lc2is_shadow_refresh(const lc2is_shadow_desc* descs, int ndesc, int total_tiles, lc2is_stream_t stream);
int lc2is_cast_f32_bf16(const float* src, int ld_src, void* dst_bf16, int ld_dst, int M, int C,
                        lc2is_stream_t stream);
int lc2is_transpose_bf16(const void* src, int ld_src, void* dst, int ld_dst, int R, int C,
                         lc2is_stream_t stream);
/* batch of `batch` such transposes in one launch; stride_* = elements between consecutive matrices. */
int lc2is_transpose_bf16_batched(const void* src, int ld_src, long stride_src, void* dst, int ld_dst, long stride_dst,
                                 int R, int C, int batch, lc2is_stream_t stream);

/* ViT patch embedding operand: out[(b*G*G + gy*G + gx)][c*p*p + i*p + j] = pixels[b][c][gy*p+i][gx*p+j]
 * (bf16, G = H / patch, trailing pixels dropped like a stride-p conv); columns [3*p*p, ld_out) are zeroed.
 * replaces: nn.Conv2d(3, C, patch, stride=patch, bias=False) im2col at hf:modeling_clip.py:202-218. */
int lc2is_patchify(const float* pixels, void* out_bf16, int ld_out, int B, int H, int W, int patch,
                   lc2is_stream_t stream);
/* x[b,0] = cls + pos[0]; x[b,1+p] = patch[b*P+p] + pos[1+p]   (hf:modeling_clip.py:211-217) and backward. */
int lc2is_vit_embed_fwd(const float* patch, int ld_patch, const float* cls, const float* pos, float* x,
                        int ldx, int B, int P, int C, lc2is_stream_t stream);
int lc2is_vit_embed_bwd(const float* dx, int ldx, float* dpos, float* dcls, void* dpatch_bf16, int ld_dpatch,
                        int B, int P, int C, int accumulate, lc2is_stream_t stream);
/* x[b*L+l] = token_embedding[ids[b,l]] + position_embedding[l]  (hf CLIPTextEmbeddings.forward) and
 * backward (dtok via fp32 atomics into a caller-zeroed/running [vocab,C] gradient). */
int lc2is_text_embed_fwd(const int64_t* ids, const float* tok, const float* pos, float* x, int ldx, int B,
                         int L, int C, int vocab, lc2is_stream_t stream);
/* dtok (zeros or the running gradient) += per-token sums in row order, no atomics: bitwise reproducible */
int lc2is_text_embed_bwd(const int64_t* ids, const float* dx, int ldx, float* dtok, float* dpos, int B, int L,
                         int C, int vocab, int accumulate, lc2is_stream_t stream);
/* dst[b, dst_off+s, :] = src[b, src_off+s, :], s < n (fp32 rows of C, optional bf16 copy): drops / re-inserts
 * the CLS token (`last_hidden_state[:, 1:, :]`, model/encoder.py:30). */
int lc2is_rows_copy_f32(const float* src, int S_src, int src_off, float* dst_f32, void* dst_bf16, int S_dst,
                        int dst_off, int B, int n, int C, lc2is_stream_t stream);
/* the same from bf16 rows (a bf16 residual stream): widened into dst_f32 and / or copied into dst_bf16 */
int lc2is_rows_copy_bf16(const void* src, int S_src, int src_off, float* dst_f32, void* dst_bf16, int S_dst,
                         int dst_off, int B, int n, int C, lc2is_stream_t stream);

/* Fused optimizer step over the flat fp32 parameter arena (n % 4 == 0).  g is multiplied by grad_scale
 * (1/world_size for DP).  SGD: torch.optim.SGD semantics (momentum_buf may be NULL); AdamW: torch.optim.AdamW.
 * replaces: optimizer.step() at engine.py:101. */
int lc2is_sgd_step(float* params, const float* grads, float* momentum_buf, size_t n, float lr, float momentum,
                   float weight_decay, float grad_scale, lc2is_stream_t stream);
int lc2is_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                     lc2is_stream_t stream);

/* ---- segmentation head tail ------------------------------------------------------------------------
 * scores_lo: fp32 channels-last [B,h,w,ld] (C valid classes, ld in {64,128,192}); output grid H = h*S,
 * W = w*S.  Computes upsample(mode) -> softmax CE against labels[B,H,W] (int64):
 *   loss_sum[0] = sum of per-pixel losses, loss_sum[1] = number of counted pixels;
 *   dscores_lo (optional, same layout) = grad_scale * U^T (softmax - onehot);
 *   scores_hi (optional) = upsampled scores as NCHW fp32 [B,C,H,W] (the reference's `outputs`).
 * S in {4, 8, 16} (every configuration of the reference): NO float atomics — the blocks' loss partials and gradient
 *   footprints go to `workspace` (>= lc2is_head_upsample_ce_workspace_bytes, 16-byte aligned; required whenever loss_sum is
 *   given) and a second launch sums them in a fixed order: loss and gradient are bitwise reproducible; loss_sum and every
 *   element of dscores_lo (all ld channels) are OVERWRITTEN, no clearing by the caller.
 * other S (multiples of 16 from 32): one launch that ADDS into loss_sum / dscores_lo with fp32 atomics (the caller clears
 *   both; results differ in the last bits from run to run); no workspace (the size query returns 0).
 * replaces: model/model.py:41-53 (bicubic x4 + TextToPatch.visual + prototype matmul, commuted), CE at
 *   engine.py:94, AuxiliaryLoss (model/loss.py:17-21, bilinear). */
size_t lc2is_head_upsample_ce_workspace_bytes(int B, int h, int w, int C, int S, int mode, int want_grad);
int lc2is_head_upsample_ce(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                           float* scores_hi, float* loss_sum, int B, int h, int w, int C, int S, int mode,
                           long ignore_index, float grad_scale, void* workspace, size_t workspace_bytes,
                           lc2is_stream_t stream);
/* lc2is_head_upsample_ce with F.cross_entropy's class weights and label smoothing (S in {4, 8, 16}):
 * class_weight: device fp32 [C] or NULL (all ones); label_smoothing eps in [0, 1] (else LC2IS_ERR_SHAPE).  With w, W = sum_c w_c,
 *   loss_sum[0] = sum_i (1-eps) w_y (lse - z_y) + (eps/C) (W lse - sum_c w_c z_c), loss_sum[1] = sum_i w_y (the weighted count of
 *   the mean), dscores_lo = grad_scale * U^T (((1-eps) w_y + eps W/C) softmax - (1-eps) w_y onehot - (eps/C) w).
 * NULL weights with eps = 0 (or no loss_sum) is exactly lc2is_head_upsample_ce; other S with options: LC2IS_ERR_UNSUPPORTED.
 * replaces: nn.CrossEntropyLoss(weight=w, label_smoothing=eps) at engine.py:94 and AuxiliaryLoss(weight, label_smoothing)
 *   (model/loss.py:14-21), fused as above. */
int lc2is_head_upsample_ce_opts(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo,
                                float* scores_hi, float* loss_sum, int B, int h, int w, int C, int S, int mode,
                                long ignore_index, float grad_scale, const float* class_weight, float label_smoothing,
                                void* workspace, size_t workspace_bytes, lc2is_stream_t stream);
/* Transposed upsample (autograd of F.interpolate) for the unfused path: dhi NCHW fp32 [B,C,h*S,w*S] ->
 * dlo channels-last fp32 [B,h,w,ld] (columns >= C untouched). */
int lc2is_upsample_bwd_nchw(const float* dhi, float* dlo, int ld, int B, int h, int w, int C, int S, int mode,
                            lc2is_stream_t stream);
/* Plain nn.CrossEntropyLoss on NCHW fp32 logits (the unfused drop-in path): forward saves per-pixel lse,
 * backward writes dlogits = grad_scale * (*grad_scale_dev) * (softmax - onehot). */
int lc2is_ce_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, int B, int C,
                      long HW, long ignore_index, lc2is_stream_t stream);
int lc2is_ce_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev,
                      float grad_scale, float* dlogits, int B, int C, long HW, long ignore_index,
                      lc2is_stream_t stream);
/* The same with class weights (device fp32 [C] or NULL), label smoothing eps in [0, 1] and reduction="none": the per-pixel
 * terms of lc2is_head_upsample_ce_opts.  Forward: loss_sum[0] = sum of the per-pixel losses, loss_sum[1] = sum of w_y (the
 * caller clears both), loss_px (optional, [B,HW]) = per-pixel loss, 0 where not counted.  Backward: dlogits = grad_scale *
 * (*grad_scale_dev) * grad_px[i] (grad_px optional, [B,HW]; NULL = 1) * dloss_i/dlogits.
 * replaces: nn.CrossEntropyLoss(weight, reduction, label_smoothing) (torch: nn/modules/loss.py CrossEntropyLoss.forward) and its
 *   autograd, on materialised NCHW logits. */
int lc2is_ce_nchw_fwd_opts(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px,
                           int B, int C, long HW, long ignore_index, const float* class_weight, float label_smoothing,
                           lc2is_stream_t stream);
int lc2is_ce_nchw_bwd_opts(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev,
                           float grad_scale, const float* grad_px, float* dlogits, int B, int C, long HW,
                           long ignore_index, const float* class_weight, float label_smoothing,
                           lc2is_stream_t stream);
/* lc2is_ce_nchw_fwd_opts with ordered sums (class_weight NULL, label_smoothing 0 and loss_px NULL: lc2is_ce_nchw_fwd): every
 * block writes its (loss, count) partial to the workspace, lc2is_ce_nchw_fwd_workspace_bytes(B, HW) bytes, and a second launch
 * sums them in a fixed order into loss_sum (overwritten, no clearing), so the sums are the same bits every run.  The two entry
 * points above add into loss_sum with float atomics, whose arrival order changes the last bits from run to run. */
size_t lc2is_ce_nchw_fwd_workspace_bytes(int B, long HW);
int lc2is_ce_nchw_fwd_ordered(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px,
                              int B, int C, long HW, long ignore_index, const float* class_weight, float label_smoothing,
                              void* workspace, size_t workspace_bytes, lc2is_stream_t stream);

/* ---- multi-scale decoder glue (BASELINE config 5; all channels-last token tensors [B, h*w, C]) --------
 * bilinear xS upsample (align_corners=False) forward / backward.
 * replaces: rearrange + F.interpolate(mode="bilinear", scale_factor=S) + rearrange at
 *   model/hierarchical.py:103-109,146-149,166-170, model/decoder.py:66-72,106-109, model/ftn.py:113,155. */
int lc2is_bilinear_up_fwd(const float* in, float* out_f32, void* out_bf16, int B, int h, int w, int C, int S,
                          lc2is_stream_t stream);
int lc2is_bilinear_up_bwd(const float* dout, float* din_f32, void* din_bf16, int B, int h, int w, int C, int S,
                          int accumulate, lc2is_stream_t stream);
/* Spatial-reduction conv operand: out[(b,y,x)][(2i+j)*C + c] = in[(b,2y+i,2x+j)][c] (bf16); scatter != 0 applies
 * the inverse map (its backward).  replaces: the im2col of Conv2d(d, d, kernel_size=2, stride=2) in
 *   SRTransformer*._sa_block (model/hierarchical.py:191,214; model/decoder.py:124). */
int lc2is_sr_gather(const void* src_bf16, void* dst_bf16, int B, int h, int w, int C, int scatter,
                    lc2is_stream_t stream);
/* Backward of the gather accumulated onto an fp32 gradient stream: dst[(b,2y+i,2x+j)][c] += src[(b,y,x)][(2i+j)*C+c]. */
int lc2is_sr_scatter_add_f32(const void* src_bf16, float* dst_f32, int B, int h, int w, int C, lc2is_stream_t stream);
/* y = x / max(||x||_2, eps) over the last dim (F.normalize, model/final.py:353-354) and its backward. */
int lc2is_l2norm_fwd(const float* x, float* y_f32, void* y_bf16, float* inv_norm, int M, int C, float eps,
                     lc2is_stream_t stream);
int lc2is_l2norm_bwd(const float* dy, const float* x, const float* inv_norm, float* dx, int M, int C, float eps,
                     lc2is_stream_t stream);
/* out = a + b (+ c) (+ d)  — torch.stack(...).sum(0) of model/hierarchical.py:128-129. */
int lc2is_add_n(const float* a, const float* b, const float* c, const float* d, float* out_f32, void* out_bf16,
                size_t n, lc2is_stream_t stream);

/* ---- Swin backbone (model/encoder.py:121-131 -> hf:models/swin/modeling_swin.py) ---------------------------------
 * rows_gather: dst[r][0:cols] = (map[r] >= 0 ? src[map[r]][0:cols] : 0) (+ add[r][0:cols]); src/dst fp32 or bf16
 *   (flags), add fp32.  With host-built index maps this is pad + cyclic shift + window partition
 *   (modeling_swin.py:546-550), window reverse + un-shift + un-pad + residual add (:558-567), the patch-merging 2x2
 *   concat (:318-321) and each of their backwards (inverse maps). */
int lc2is_rows_gather(const void* src, int ld_src, int src_bf16, void* dst, int ld_dst, int dst_bf16, const int* map,
                      const float* add, int ld_add, int rows, int cols, lc2is_stream_t stream);
/* Window attention (modeling_swin.py:373-398,428-465): qkv [nwin*S, 3C] bf16 (q | k | v, head h at columns 32h),
 *   S = ws*ws <= 64, head_dim 32, bias [nH,S,S] fp32 = relative position bias; for shift > 0 the cyclic-shift region
 *   mask (-100 across regions, :584-607) is derived from the window index (win_per_img windows per image, nwx per
 *   row, padded grid Hp x Wp).  out [nwin*S, C] bf16, lse [nwin,nH,S].  Backward writes dqkv and the bias gradient
 *   dbias [nH,S,S] (summed over windows in a fixed order; workspace from the _workspace_bytes call). */
int lc2is_swin_attn_fwd(const void* qkv, int ld, void* out, int ldo, float* lse, const float* bias, int nwin,
                        int win_per_img, int nwx, int Hp, int Wp, int ws, int shift, int nH, int C, float scale,
                        lc2is_stream_t stream);
size_t lc2is_swin_attn_bwd_workspace_bytes(int nwin, int ws, int nH);
int lc2is_swin_attn_bwd(const void* qkv, int ld, const void* o, int ld_o, const void* dout, int lddo, const float* lse,
                        const float* bias, void* dqkv, int lddq, float* dbias, int accumulate_dbias, int nwin,
                        int win_per_img, int nwx, int Hp, int Wp, int ws, int shift, int nH, int C, float scale,
                        void* workspace, size_t workspace_bytes, lc2is_stream_t stream);

/* gradient of the relative_position_bias_table [T = (2 ws - 1)^2, nH] from dbias [nH, S*S]: dtable[t][h] = sum of
 * dbias[h][p] over the pairs p = positions[offsets[t] .. offsets[t+1]) (the inverse of relative_position_index,
 * modeling_swin.py:350-383), added in list order.  replaces: autograd of `table[index]` (index_put_ with accumulate). */
int lc2is_swin_bias_table_grad(const float* dbias, const int* offsets, const int* positions, float* dtable, int nH, int SS,
                               int T, int accumulate, lc2is_stream_t stream);

/* ---- preprocessing in front of the path (evaluate.py:58-61, data/collator.py:82-91; Pillow inside transformers'
 * CLIPFeatureExtractor) — byte / integer work, bit-exact against Pillow --------------------------------------------
 * resample_u8: one separable 8-bit pass of PIL's ImagingResample over an HWC uint8 image along `axis` (1 = width,
 *   0 = height): out = clip8((1<<21 + sum_t in[first+t] * kk[o][t]) >> 22) with bounds[o] = (first, count) and the
 *   22-bit fixed-point coefficients built on the host as Resample.c precompute_coeffs / normalize_coeffs_8bpc do.
 * gather2d_u8: dst[y][x][c] = src[yi[y]][xi[x]][c] (nearest resize, Geometry.c ImagingScaleAffine index vectors).
 * crop_lut: S x S crop at (top,left) + 256-entry lookup: uint8 HWC -> float32 CHW via lut_f32[C][256] (x/255 and
 *   (x-mean)/std folded in with the reference's float ops) and / or channel 0 -> int64 via lut_i64[256] (labels). */
int lc2is_resample_u8(const void* src_u8, int H, int W, int C, void* dst_u8, int out_size, int axis, const int* bounds,
                      const int* kk, int ksize, lc2is_stream_t stream);
int lc2is_gather2d_u8(const void* src_u8, int H, int W, int C, void* dst_u8, int out_h, int out_w, const int* yi,
                      const int* xi, lc2is_stream_t stream);
int lc2is_crop_lut(const void* src_u8, int H, int W, int C, int top, int left, int S, const float* lut_f32,
                   float* dst_f32, const int64_t* lut_i64, int64_t* dst_i64, lc2is_stream_t stream);

/* ---- remaining losses (model/loss.py) and the parity metric (metrics.py) on channels-last scores ----------
 * rows_ce: softmax-CE over the K contiguous classes of each of M rows: loss_sum[0] += sum of per-row losses,
 *   lse[M] (optional), dx (optional) (+)= grad_scale * (softmax - onehot).  A row whose label lies outside [0, K)
 *   adds nothing to loss_sum or dx.  ContrastiveLoss.loss_visual (model/loss.py:59) — also usable for any [M,K] logits.
 * cols_ce: ContrastiveLoss.loss_textual (model/loss.py:58): x viewed [B,H,W,K], log-softmax over H (dim 1 — what
 *   nn.CrossEntropyLoss does with the reference's one-hot float targets), loss_sum[0] += sum over (b,w,k) columns;
 *   dx += grad_scale * d/dx; labels outside [0, K) match no class. */
int lc2is_rows_ce(const float* x, const int64_t* labels, float* lse, float* loss_sum, float* dx, float grad_scale,
                  int M, int K, int accumulate_dx, lc2is_stream_t stream);
int lc2is_cols_ce(const float* x, const int64_t* labels, float* loss_sum, float* dx, float grad_scale, int B, int H,
                  int W, int K, lc2is_stream_t stream);
/* NPairLoss.forward before its reduction (model/loss.py:30-35): res[i] = sum_p pos_ip / (pos_ip + sum_q neg_iq). */
int lc2is_npair(const float* x, const float* x_pos, const float* x_neg, float* res, int n, int n_pos, int n_neg, int d,
                lc2is_stream_t stream);
/* Its backward: dres [n] = gradient of res; workspace = n * (n_pos + 1) floats.  Fixed summation order. */
int lc2is_npair_bwd(const float* x, const float* x_pos, const float* x_neg, const float* dres, float* dx, float* dx_pos,
                    float* dx_neg, float* workspace, int n, int n_pos, int n_neg, int d, lc2is_stream_t stream);
/* compute_mIOU's confusion counts (metrics.py:82-102): counts[b] = {intersection[K], predicted[K], labelled[K]} (int32,
 * caller-zeroed) from NCHW scores at the upsampled size and the nearest-x S labels. */
int lc2is_miou_counts(const float* scores_hi, const int64_t* labels_lo, int* counts, int B, int K, int H, int W, int S,
                      lc2is_stream_t stream);

/* ---- original-size prediction and mIoU --------------------------------------------------------------------------------
 * Per image b of a batch: bicubic resize of scores[b] (channels-last fp32 [N,h,w,ld], K valid channels, ld % 4 == 0, ld >= K,
 * 16-byte aligned) to its own size H_b x W_b (any size >= 1: torch's upsample_bicubic2d with align_corners=False and an explicit
 * size: scale h / H, A = -0.75, taps clamped), then the argmax over the K channels (exact ties: the lowest index) — without
 * forming the [K,H,W] score map.
 *   desc: DEVICE int64 [N][4] = {H_b, W_b, first pixel of image b in pred / gt, first tile of image b}; the images are packed
 *     row-major one after the other (total_px pixels), image b has ceil(H_b/16) * ceil(W_b/16) tiles of LC2IS_RESIZE_TILE^2
 *     pixels, first tiles ascending from 0 (n_tiles in all).  A descriptor that does not fit total_px / n_tiles is not followed.
 *   pred (optional): uint8 [total_px], the argmax.
 *   counts (optional): int32 [N][3][K] = {intersection, predicted, labelled} per class, OVERWRITTEN (no clearing): every pixel
 *     counts in "predicted", "labelled" and "intersection" only where 0 <= gt < K (lc2is_miou_counts' rule).  Needs gt (packed
 *     like pred; gt_bytes = 1: uint8, 4: int32, 8: int64) and workspace (>= lc2is_resize_argmax_workspace_bytes(n_tiles, K)
 *     = n_tiles * 3 * K * 4 bytes: per-tile counts, summed per image in a fixed order by a second launch; no atomics, bitwise
 *     reproducible).
 * K > 192 or another gt_bytes: LC2IS_ERR_UNSUPPORTED.
 * replaces: metrics.py:61-79 (compute_gt_mIOU: F.interpolate(size=) + Softmax2d + JaccardIndex) and metrics.py:35-42,137-143
 *   (prepare_for_gt_metrics / original_size_interpolate, then argmax). */
#define LC2IS_RESIZE_TILE 16
size_t lc2is_resize_argmax_workspace_bytes(long n_tiles, int K);
int lc2is_resize_argmax(const float* scores, int ld, int N, int h, int w, int K, const int64_t* desc, long n_tiles,
                        long total_px, const void* gt, int gt_bytes, uint8_t* pred, int* counts, void* workspace,
                        size_t workspace_bytes, lc2is_stream_t stream);

/* ---- sliding-window evaluation: window-mean resize + argmax -----------------------------------------------------------
 * lc2is_resize_argmax with another source.  Image b is resized from a canvas of Hc_b x Wc_b score cells that is never formed:
 * a canvas cell is the mean of the window views that cover it (mmseg's slide_inference on the score-cell grid, logits averaged).
 *   views: channels-last fp32 [V,h,w,ld], K valid channels, ld % 4 == 0, ld >= K, 16-byte aligned: one score grid per window
 *     forward.
 *   desc: DEVICE int64 [N][8] = {H_b, W_b, first pixel, first tile (all four as in lc2is_resize_argmax), Hc_b, Wc_b, first
 *     window of image b in win, its number of windows}.
 *   win: DEVICE int32 [n_win][4] = {view index, oy, ox, flags}, 16-byte aligned; the origin is in canvas cells; flags bit 0: the
 *     view is mirrored along x (view column j is canvas column ox + w - 1 - j).
 *   Canvas cell (cy, cx), channel c: the fp32 sum over the image's windows, in list order and starting from the first one that
 *     covers the cell, divided (IEEE fp32 division) by their number; a cell that no window covers reads 0.  The output pixel is
 *     torch's bicubic resize of that canvas (align_corners=False, explicit size, scale Hc / H, Wc / W), then the argmax, the
 *     per-wave histograms and per-tile slabs of lc2is_resize_argmax (same workspace: lc2is_resize_argmax_workspace_bytes).
 *   Every descriptor value is range-checked on the device: a window whose view is outside [0, V) or whose origin is outside
 *     [0, Hc - h] x [0, Wc - w] is skipped; an image with more than LC2IS_SLIDE_MAX_WIN windows, a window range outside
 *     [0, n_win], Hc < h or Wc < w is not followed: its pred pixels are left as they were and its counts are UNDEFINED (its
 *     slabs are not written; lc2is_resize_argmax treats a descriptor it does not follow the same way).  Nothing outside the
 *     buffers is read or written.
 *   ignore_index: -1 = lc2is_resize_argmax's counting rule (every pixel counts in "predicted"); >= 0 = mmseg's rule: a pixel
 *     whose gt equals ignore_index or lies outside [0, K) counts in none of the three rows.
 * Error codes as lc2is_resize_argmax (ignore_index < -1: LC2IS_ERR_SHAPE).  No atomics: bitwise reproducible, batch independent.
 * replaces: nothing in the reference, which scores the centre crop only (metrics.py:137-143 original_size_interpolate of one
 *   forward); this is the slide mode of the published ADE20K protocol on top of the same resize + argmax. */
#define LC2IS_SLIDE_MAX_WIN 64
int lc2is_resize_argmax_windows(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                const int32_t* win, long n_win, long n_tiles, long total_px, const void* gt, int gt_bytes,
                                int ignore_index, uint8_t* pred, int* counts, void* workspace, size_t workspace_bytes,
                                lc2is_stream_t stream);

/* ---- multi-scale + flip evaluation: several canvases per image, summed before the argmax --------------------------------
 * lc2is_resize_argmax_windows with a list of canvases per image (one per scale, or per scale and flip): every canvas is the
 * window mean of lc2is_resize_argmax_windows, resized to the image's size H_b x W_b with the same arithmetic; the resized
 * canvases y_0, y_1, ... are combined per class and the argmax (first maximum), counts and workspace are those of
 * lc2is_resize_argmax_windows.  Neither a canvas nor a [K,H,W] map is formed.
 *   views, win: as lc2is_resize_argmax_windows; all canvases of all images index the one views tensor.
 *   desc: DEVICE int64 [N][6] = {H_b, W_b, first pixel, first tile (all four as in lc2is_resize_argmax), first canvas of image b
 *     in canv, its number of canvases (1 to LC2IS_MS_MAX_CANVAS)}.
 *   canv: DEVICE int64 [n_canv][4] = {Hc, Wc (canvas cells, each 1 to 2^24), first window of the canvas in win, its number of
 *     windows (1 to LC2IS_SLIDE_MAX_WIN)}.
 *   A canvas may be smaller than a view: a window is usable when 0 <= oy < Hc and 0 <= ox < Wc, and only its on-canvas part,
 *     vh = min(h, Hc - oy) rows by vw = min(w, Wc - ox) columns from the view's top-left, is read.  A mirrored view (flags bit 0)
 *     is mirrored over that part: view column j < vw is canvas column ox + vw - 1 - j.
 *   mode: LC2IS_MS_LOGIT: s[c] = y_0[c] + y_1[c] + ..., in canvas order from y_0 (one canvas: lc2is_resize_argmax_windows'
 *     bits).  LC2IS_MS_PROB: s[c] = sum_a exp(y_a[c] - m_a) / l_a with m_a = max_c y_a[c], l_a = sum_c exp(y_a[c] - m_a) over the
 *     K valid channels, in canvas order: the softmax of every canvas summed (mmseg's aug_test).  exp is the hardware exp2 path
 *     (relative error of the order of 1e-6).
 *   Every descriptor value is range-checked on the device: an unusable window (view outside [0, V), origin off the canvas) is
 *     skipped; an image whose canvas range lies outside [0, n_canv], with no or more than LC2IS_MS_MAX_CANVAS canvases, or with a
 *     canvas whose size or window range does not fit or that has no usable window, is not followed: its pred pixels are left
 *     as they were and its counts are UNDEFINED.  Nothing outside the buffers is read or written.
 * Error codes as lc2is_resize_argmax_windows; another mode: LC2IS_ERR_SHAPE.  No atomics: bitwise reproducible, batch
 * independent.
 * replaces: nothing in the reference (centre crop only, metrics.py:137-143); this is the "ms+flip" row of the published ADE20K
 *   protocol on top of the same resize + argmax. */
#define LC2IS_MS_MAX_CANVAS 16
#define LC2IS_MS_LOGIT 0
#define LC2IS_MS_PROB 1
int lc2is_resize_argmax_multiscale(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                   const int64_t* canv, long n_canv, const int32_t* win, long n_win, long n_tiles,
                                   long total_px, const void* gt, int gt_bytes, int ignore_index, int mode, uint8_t* pred,
                                   int* counts, void* workspace, size_t workspace_bytes, lc2is_stream_t stream);

/* ---- the three resize + argmax entries past 192 classes ----------------------------------------------------------------
 * lc2is_resize_argmax, lc2is_resize_argmax_windows and lc2is_resize_argmax_multiscale for 1 <= K <= LC2IS_RESIZE_WIDE_KMAX
 * classes (PC-459, ADE20K-full's 847, ImageNet-S-919).  Every argument, descriptor, device-side range check, counting rule
 * (ignore_index) and mode is that of the narrow entry of the same name, with two differences:
 *   pred (optional): int16 [total_px], packed as the narrow pred (a class index does not fit uint8 past 255).
 *   workspace: >= lc2is_resize_argmax_wide_workspace_bytes(n_tiles, K) = n_tiles * 3 * K * 4 bytes for 1 <= K <= 1024 (0
 *     otherwise): the same dense per-tile slabs {intersection[K], predicted[K], labelled[K]}, summed per image by the same
 *     second launch in the same order.  A slab is 12 KB per 16 x 16 tile at K = 1024; one 683 x 512 image (1376 tiles) at
 *     K = 847 needs 14 MB, one 2048 x 1536 image (12288 tiles) 125 MB.  (The [K,H,W] fp32 score map that is never formed
 *     would be 1.18 GB and 10.6 GB.)
 * Per class the arithmetic is the narrow kernels' (same taps, fma order, window-mean order and canvas order), the argmax is
 * the first maximum and the counts are exact integers: with K <= 192 a wide call returns the narrow call's pred values and
 * count bytes, only slower in its count epilogue (the three rows of a tile's counts take turns in LDS: [4 waves][K] ints, 16 KB
 * at K = 1024, inside the footprint area; the multiscale PROB kernel keeps its 70 KB and two blocks per CU).
 * A descriptor that does not fit is not followed, as in the narrow entries: its pred pixels are left as they were, its counts
 * are UNDEFINED, nothing outside the buffers is read or written.
 * Error codes and their order as the narrow entries: LC2IS_ERR_NULL, LC2IS_ERR_SHAPE, LC2IS_ERR_UNSUPPORTED (K > 1024 or
 * another gt_bytes), LC2IS_ERR_WORKSPACE.  No atomics: bitwise reproducible, batch independent.
 * replaces: as the narrow entries; the reference has no vocabulary past 151 classes. */
#define LC2IS_RESIZE_WIDE_KMAX 1024
size_t lc2is_resize_argmax_wide_workspace_bytes(long n_tiles, int K);
int lc2is_resize_argmax_wide(const float* scores, int ld, int N, int h, int w, int K, const int64_t* desc, long n_tiles,
                             long total_px, const void* gt, int gt_bytes, int16_t* pred, int* counts, void* workspace,
                             size_t workspace_bytes, lc2is_stream_t stream);
int lc2is_resize_argmax_windows_wide(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                     const int32_t* win, long n_win, long n_tiles, long total_px, const void* gt,
                                     int gt_bytes, int ignore_index, int16_t* pred, int* counts, void* workspace,
                                     size_t workspace_bytes, lc2is_stream_t stream);
int lc2is_resize_argmax_multiscale_wide(const float* views, int ld, int V, int h, int w, int K, const int64_t* desc, int N,
                                        const int64_t* canv, long n_canv, const int32_t* win, long n_win, long n_tiles,
                                        long total_px, const void* gt, int gt_bytes, int ignore_index, int mode,
                                        int16_t* pred, int* counts, void* workspace, size_t workspace_bytes,
                                        lc2is_stream_t stream);

/* ---- the device-held optimizer path (optim.hip) -----------------------------------------------------------------------
 * The scalars of an optimizer step that change from call to call live in this block in DEVICE memory (48 bytes, 4-byte
 * aligned, all zero before the first step), so a step needs no host value that differs between calls and can be replayed
 * from a captured graph.  Only lc2is_optim_ctrl_update (and its _accum form) writes it: plain vector stores from one lane of
 * its one block. */
typedef struct {
  int32_t calls;    /* iterations seen: indexes the lr table (the reference advances its scheduler every iteration)        */
  int32_t applied;  /* updates actually applied: AdamW's t                                                                 */
  int32_t skipped;  /* steps skipped for a non-finite gradient so far                                                      */
  int32_t finite;   /* this step: 1 = every gradient element was finite (exponent bits, not the sum)                       */
  float grad_norm;  /* this step: global L2 norm of grad_scale * g; +inf where the fp32 sum of squares overflowed          */
  float clip_coef;  /* this step: min(1, max_norm / (grad_norm + 1e-6)); exactly 1 for max_norm = +inf                     */
  float lr;         /* this step: lr_table[min(calls before this step, table_len - 1)]                                     */
  float bc1, bc2;   /* this step: 1 - beta1^applied, 1 - beta2^applied (kept from the last applied step on a skip)         */
  float grad_mul;   /* this step: grad_scale * clip_coef, what the _ctrl optimizers multiply g by                          */
  int32_t apply;    /* this step: 1 = the _ctrl optimizers update; 0 = they return before touching memory                  */
  int32_t reserved;
} lc2is_optim_ctrl;

/* Pass 1 over the flat gradient: per-block fp32 partial sums of squares and per-block "saw an inf or NaN" flags (from the
 * exponent bits: exact, whatever the sum does).  n % 4 == 0, grads 16-byte aligned.  The grid is a function of n alone:
 * lc2is_grad_sumsq_blocks(n) = min(4096, ceil(n / 1024)) blocks of 256 lanes, grid-stride, 16 bytes per lane, one fp32
 * accumulator per lane in ascending index order, then a fixed 8-level tree per block.  workspace (4-byte aligned,
 * >= lc2is_grad_sumsq_workspace_bytes(n) = 8 * blocks) receives fp32 partials[blocks] followed by uint32 flags[blocks].
 * No atomics: bitwise reproducible.  Plain cached loads (the optimizer reads the buffer next).
 * replaces: the gradient inspection of GradScaler.step (engine.py:89-91, `scaler.step(optimizer)` skips on inf / NaN) and the
 *   norm of torch.nn.utils.clip_grad_norm_ (the reference does not clip). */
int lc2is_grad_sumsq_blocks(size_t n);
size_t lc2is_grad_sumsq_workspace_bytes(size_t n);
int lc2is_grad_sumsq(const float* grads, size_t n, void* workspace, size_t workspace_bytes, lc2is_stream_t stream);

/* One small launch between pass 1 and the optimizer.  Sums partials[0:nparts] in fp64 in index order (256 consecutive runs,
 * run sums added in index order), ORs the flags, and writes into *ctrl:
 *   grad_norm = grad_scale * sqrt(sum), clip_coef (max_norm > 0; +inf = no clipping), finite,
 *   lr = lr_table[min(calls, table_len - 1)] (DEVICE fp32 table: entry i is the rate of call i + 1, the last one is held), calls += 1,
 *   then if finite or !skip_nonfinite: apply = 1, applied += 1, bc1 / bc2 = 1 - beta^applied; else apply = 0, skipped += 1.
 * replaces: lr_scheduler.step() at engine.py:103-104 (the host tabulates the scheduler), GradScaler's skip decision
 *   (engine.py:89-91), clip_grad_norm_'s coefficient, and the host-side bias corrections of lc2is_adamw_step. */
int lc2is_optim_ctrl_update(lc2is_optim_ctrl* ctrl, const float* partials, const unsigned int* flags, int nparts,
                            const float* lr_table, int table_len, float grad_scale, float max_norm, int skip_nonfinite,
                            float beta1, float beta2, lc2is_stream_t stream);

/* Gradient accumulation: N micro-batches per optimizer update with the EXACT large-batch mean.  The head writes the gradient
 * of the SUM of the pixel losses and returns [sum of losses, (weighted) count]; the arena accumulates those sums over the
 * cycle, and this block in DEVICE memory (32 bytes, 8-byte aligned, all zero before the first cycle) holds the cycle's
 * denominator, so the update divides by the count of ALL pixels of the cycle - not the mean of micro-batch means, which
 * weights the pixels of sparsely labelled crops more heavily than the large batch would.  fp64 sums: fp32 stops counting
 * exactly at 2^24, which 32 micro-batches of 524 288 labels reach.  Written by one lane in plain stores, no atomics; read by the
 * next launch on the same stream. */
typedef struct {
  double loss_sum;   /* open cycle: sum over its micro-batches of loss2[0]                                                  */
  double denom;      /* open cycle: sum over its micro-batches of loss2[1]                                                  */
  int32_t micro;     /* open cycle: micro-batches added so far                                                              */
  int32_t reserved;
  float last_loss;   /* last closed cycle: loss_sum / denom (use_denom; NaN when denom == 0), or loss_sum                   */
  float last_denom;  /* last closed cycle: its denom                                                                        */
} lc2is_accum_block;

/* loss_sum += (double)loss2[0], denom += (double)loss2[1], micro += 1.  loss2: DEVICE fp32 [2] as lc2is_head_upsample_ce
 * returns it.  One lane of one block.  block 8-byte aligned, loss2 4-byte aligned (else LC2IS_ERR_SHAPE).
 * replaces: nothing in the reference, which calls optimizer.step() after every batch (engine.py:89-101); stands in for the
 *   `loss = loss / accum_steps` of the usual accumulation loop, which cannot give the large batch's mean over non-ignored pixels. */
int lc2is_accum_add(lc2is_accum_block* block, const float* loss2, lc2is_stream_t stream);

/* lc2is_optim_ctrl_update for the call that closes an accumulation cycle: the same kernel body with the gradient scale
 *   scale64 = (double)grad_scale / d,  d = use_denom ? (block->denom > 0 ? block->denom : 1.0) : 1.0
 * wherever lc2is_optim_ctrl_update uses grad_scale: grad_norm = scale64 * sqrt(sum), grad_mul = (float)scale64 * clip_coef.
 * Then it writes the block: last_loss = use_denom ? loss_sum / denom : loss_sum, last_denom = denom, and loss_sum, denom and
 * micro are zeroed for the next cycle.  With use_denom == 0, or denom == 1.0, *ctrl receives the very bits
 * lc2is_optim_ctrl_update writes.  use_denom in {0, 1}, block 8-byte aligned, everything else as lc2is_optim_ctrl_update.
 * replaces: nothing in the reference (engine.py:89-101 steps after every batch); the per-update scheduler step, skip decision
 *   and clip coefficient of lc2is_optim_ctrl_update, taken once per cycle on the accumulated gradient. */
int lc2is_optim_ctrl_update_accum(lc2is_optim_ctrl* ctrl, lc2is_accum_block* block, int use_denom, const float* partials,
                                  const unsigned int* flags, int nparts, const float* lr_table, int table_len,
                                  float grad_scale, float max_norm, int skip_nonfinite, float beta1, float beta2,
                                  lc2is_stream_t stream);

/* lc2is_sgd_step / lc2is_adamw_step with lr, bc1, bc2 and the gradient multiplier (grad_scale * clip_coef) read from *ctrl;
 * with ctrl->apply == 0 they return before touching params or any state buffer.  The same expressions: with clip_coef == 1 and
 * a constant table lc2is_sgd_step_ctrl gives the bits of lc2is_sgd_step.  reverse != 0 walks the arena from its end.
 * replaces: optimizer.step() at engine.py:101 as `scaler.step(optimizer)` runs it (engine.py:89-91). */
int lc2is_sgd_step_ctrl(float* params, const float* grads, float* momentum_buf, size_t n, const lc2is_optim_ctrl* ctrl,
                        float momentum, float weight_decay, int reverse, lc2is_stream_t stream);
int lc2is_adamw_step_ctrl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                          const lc2is_optim_ctrl* ctrl, float beta1, float beta2, float eps, float weight_decay,
                          int reverse, lc2is_stream_t stream);

/* Parameter groups: the _ctrl optimizers in ONE launch over the whole arena with a learning-rate factor and a weight decay per
 * group.  The arena is cut into granules of LC2IS_GROUP_GRANULE = 64 elements (every parameter of ParamArena starts on one);
 * granule_group (DEVICE, n / 64 bytes) names the group of each granule, groups (DEVICE, ngroups entries) holds the constants.
 * Per element: lr = ctrl->lr * lr_scale (one fp32 multiplication), weight_decay the group's, everything else - grad_mul, bc1,
 * bc2, apply, reverse - as lc2is_sgd_step_ctrl / lc2is_adamw_step_ctrl, expression for expression: a range updated here has the
 * bits the _ctrl entry gives on that range with ctrl->lr set to the product.  A granule whose id is >= ngroups - 255 is the
 * reserved spelling - is SKIPPED: nothing of it is loaded or stored (torch.optim leaving a parameter without a gradient alone).
 * n % 64 == 0, 1 <= ngroups <= LC2IS_MAX_PARAM_GROUPS = 255, buffers 16-byte aligned.  No atomics; independent of the grid.
 * replaces: optimizer.step() at engine.py:101 for an optimizer built with torch.optim param_groups. */
#define LC2IS_GROUP_GRANULE 64
#define LC2IS_MAX_PARAM_GROUPS 255
#define LC2IS_GROUP_SKIP 255
typedef struct {
  float lr_scale;     /* multiplies ctrl->lr; 0 = the group's parameters keep their bits (moments / momentum still advance) */
  float weight_decay; /* in place of the weight_decay argument of the _ctrl entries                                        */
} lc2is_param_group;
int lc2is_sgd_step_groups(float* params, const float* grads, float* momentum_buf, size_t n, const lc2is_optim_ctrl* ctrl,
                          const uint8_t* granule_group, const lc2is_param_group* groups, int ngroups, float momentum,
                          int reverse, lc2is_stream_t stream);
int lc2is_adamw_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                            const lc2is_optim_ctrl* ctrl, const uint8_t* granule_group, const lc2is_param_group* groups,
                            int ngroups, float beta1, float beta2, float eps, int reverse, lc2is_stream_t stream);

/* Weight EMA held on the device, following the control block: with ctrl->apply == 0 (a skipped step), or ctrl->applied % every
 * != 0, the launch returns before touching memory; otherwise, per element, ema += w * (params - ema), one fma on the difference.
 *   w = one_minus_decay: 1 - decay formed in fp64 ON THE HOST and rounded once (1.f - 0.9999f would be off by 3e-4 relative);
 *   warmup != 0: the j-th EMA update (j = applied / every, 1-based) takes max(w, 9 / (10 + j)), i.e. TF's decay
 *     min(decay, (1 + j) / (10 + j)), formed in fp64 and rounded once.
 * An element whose bits equal the parameter's keeps its bits exactly (+-0, denormals, infinities and NaN payloads included): the
 * EMA of parameters that never move, and of the arena's alignment padding, stays bit-identical to them.
 * n % 4 == 0, n > 0, both buffers 16-byte aligned, 0 < one_minus_decay <= 1, every >= 1 (else LC2IS_ERR_SHAPE).  Same grid and
 * walk (reverse != 0: from the end; the same bits) as lc2is_sgd_step_ctrl.  No atomics, element-wise: bitwise reproducible.
 * replaces: nothing in the reference, which keeps no averaged weights; stands in for torch.optim.swa_utils.AveragedModel with
 *   get_ema_multi_avg_fn (a second model and a torch._foreach_lerp_ over every parameter tensor per step) / timm's ModelEmaV3. */
int lc2is_ema_update_ctrl(float* ema, const float* params, size_t n, const lc2is_optim_ctrl* ctrl, float one_minus_decay,
                          int warmup, int every, int reverse, lc2is_stream_t stream);

/* Exchanges the contents of two fp32 buffers of n elements in place, bit for bit (NaN payloads and -0.0 survive).  n % 4 == 0,
 * n > 0, both 16-byte aligned, the ranges disjoint (else LC2IS_ERR_SHAPE).  Evaluating with the EMA weights is "swap, evaluate,
 * swap back": every pointer - parameter views, a captured graph's arguments - stays where it was, and nothing is allocated.
 * replaces: nothing in the reference; stands in for the store() / copy_to() / restore() of EMA helpers (torch._foreach_copy_ three
 *   times through a temporary of the model's size), or evaluating torch.optim.swa_utils.AveragedModel.module, a second model. */
int lc2is_swap_f32(float* a, float* b, size_t n, lc2is_stream_t stream);

/* ---- train-time augmentation on the device: random rescale + crop + horizontal flip + photometric jitter, one launch per batch ----
 * replaces: the `transform` hook of the training dataset (data/dataset.py:144-149: one random transform applied to the image and
 *   to the label under a shared RNG state), which the reference leaves to the host.  Here the decoded uint8 pixels live on the
 *   device (an image pool), and two launches cut a whole augmented batch into the pixel_values / label tensors of the step.
 * Image pool: one packed uint8 buffer of HWC pixels, one of HW labels, and a descriptor per image.  The 8 bytes that follow the last
 *   pixel of an image must be readable (img_off + 3*H*W + 5 <= img_bytes): a tap is fetched as one unaligned 8-byte read. */
typedef struct {
  int64_t img_off;  /* byte offset of the image's first pixel in the image buffer */
  int64_t lab_off;  /* byte offset of the label map in the label buffer           */
  int32_t H, W;     /* 1 .. LC2IS_AUG_MAX_SIDE                                    */
} lc2is_aug_image;
#define LC2IS_AUG_MAX_SIDE 4096
#define LC2IS_AUG_MAX_RESIZED 262143 /* nh, nw <= this: (2 * n + 1) * 4096 fits int32                                           */
#define LC2IS_AUG_PARAM_WORDS 20     /* one row of the parameter table, 32-bit words:                                          */
#define LC2IS_AUG_NH 0               /*   int32 nh, nw: the size the image is resized to                                       */
#define LC2IS_AUG_NW 1
#define LC2IS_AUG_TOP 2              /*   int32 top, left: the crop's origin in the resized image                              */
#define LC2IS_AUG_LEFT 3
#define LC2IS_AUG_FLIP 4             /*   int32 flip: 1 = mirrored left-right                                                  */
#define LC2IS_AUG_M 5                /*   fp32 M[3][3] row-major and fp32 o[3]: rgb' = clamp(M rgb + o, 0, 255) on the 0..255 scale */
#define LC2IS_AUG_O 14               /*   words 17..19: 0                                                                      */
typedef struct {
  uint32_t seed_lo, seed_hi;      /* the 64-bit seed                                                                           */
  int32_t crop_size, base_size;   /* S; the short edge is resized to base_size * ratio                                         */
  int32_t ratio_lo1024, ratio_hi1024; /* the ratio's range in 1/1024 units (512, 2048 = 0.5 .. 2.0), lo <= hi                  */
  uint32_t flip_thr;              /* round(p * 2^24): flip iff u24 < flip_thr                                                  */
  uint32_t photo_thr[4];          /* the same for brightness, contrast, saturation, hue; all 0 = identity colour               */
  float brightness_delta;         /* b in [-delta, delta], added on the 0..255 scale                                           */
  float contrast_lo, contrast_hi; /* c: every channel is multiplied by c                                                      */
  float saturation_lo, saturation_hi; /* s: rgb' = s rgb + (1 - s) grey, grey = 0.299 r + 0.587 g + 0.114 b                    */
  float hue_delta;                /* h in [-delta, delta] RADIANS: rotation about the grey axis (1, 1, 1)                      */
} lc2is_aug_config;
typedef struct {
  float mean[3], inv_std[3];      /* out_c = (v * (1/255) - mean_c) * inv_std_c, inv_std_c = 1 / std_c rounded to fp32 once    */
} lc2is_aug_norm;

/* aug_params_kernel, one thread per sample b < B: reads slot = slots[b] (the image's row in `desc`), key = keys ? keys[b] : slot (the
 * DATASET index the random numbers are drawn for; it differs from the slot only when the pool holds a transient batch), *epoch,
 * desc[slot].(H, W), and writes row b of params [B][LC2IS_AUG_PARAM_WORDS].  Every random number is a pure function of
 * (seed, *epoch, key, draw number k):  h = mix32(lo32(key) + seed_lo); h = mix32(h ^ (hi32(key) + seed_hi));
 * h = mix32(h ^ (epoch * 0x9E3779B9 + 0x85EBCA6B));  u24(k) = mix32(h + k * 0x9E3779B9) >> 8  (mix32 = lowbias32, uint32 wrap-around),
 * so an image gets the same augmentation in an epoch whatever its batch, position, rank or batch size, and a captured launch draws
 * new parameters on replay once the DEVICE arrays slots / keys / epoch hold new values.  Draws, integers in integer arithmetic only:
 *   k=0  r = ratio_lo1024 + ((u24 * (ratio_hi1024 - ratio_lo1024 + 1)) >> 24);  t = (base_size * r + 512) >> 10;  s = min(H, W);
 *        nh = min(max(1, (2*H*t + s) / (2*s)), LC2IS_AUG_MAX_RESIZED), nw the same with W
 *   k=1  top = (u24 * (max(nh - S, 0) + 1)) >> 24      k=2  left the same with nw      k=3  flip = u24 < flip_thr
 *   k=4,6,8,10  step on iff u24 < photo_thr[0..3];  k=5,7,9,11  its value lo + (hi - lo) * (u24 * 2^-24) in fp32
 * Colour: M = I, o = 0, then for each step that is on, in this order: brightness o += b; contrast M, o *= c; saturation
 * (M, o) = A (M, o) with A = s I + (1 - s) 1 w^T; hue (M, o) = R (M, o) with R the rotation by h about (1, 1, 1) / sqrt(3).  ONE
 * clamp to [0, 255] follows in aug_apply, none between the steps.  slot outside [0, n_images) or H, W outside
 * 1..LC2IS_AUG_MAX_SIDE: the row is all zeros, which aug_apply renders as padding.  No atomics. */
int lc2is_aug_params(const int64_t* slots, const int64_t* keys, int B, const int32_t* epoch, const lc2is_aug_image* desc,
                     long n_images, const lc2is_aug_config* cfg /* HOST */, int32_t* params, lc2is_stream_t stream);

/* aug_apply_kernel, ONE launch for the batch: grid.y = B samples, grid.x = image blocks followed by label blocks (256 lanes; an
 * image lane makes 4 consecutive output x of all 3 channels: three 16-byte write-back stores, patchify reads the tensor next).
 * out_img fp32 [B][3][S][S] (16-byte aligned), out_lab int64 [B][L][L]; S % 4 == 0, S % L == 0, q = S / L, S <= 4096, B <= 65535.
 * Output pixel (i, j) looks at resized-image pixel yr = top + i, xr = left + (flip ? S-1-j : j).  Outside [0,nh) x [0,nw) the image
 * value is 0.0 (the mean colour after normalisation) and the label is pad_label.  Inside, exact in int32:
 *   ny = clamp((2*yr+1)*H - nh, 0, 2*nh*(H-1)); y0 = ny / (2*nh); fy = float(ny - y0*2*nh) / float(2*nh); y1 = min(y0+1, H-1);
 *   the same for x; a = lerp(lerp(p00, p01, fx), lerp(p10, p11, fx), fy) per channel in fp32 (lerp(a, b, f) = a + f * (b - a));
 *   v = clamp(M a + o, 0, 255); out_c = (v * (1/255) - mean_c) * inv_std_c.
 *   = F.interpolate(size=(nh, nw), mode="bilinear", align_corners=False) + zero pad + crop + flip + colour + normalise.
 * Label cell (i, j) is the label at output pixel (i*q + q/2, j*q + q/2): source ys = ((2*yr+1)*H) / (2*nh), xs likewise
 *   (mode="nearest-exact"), passed through as int64.
 * A sample whose slot, descriptor (sides, offsets against img_bytes / lab_bytes) or nh / nw is out of range is rendered as padding:
 * nothing outside the two buffers is read whatever the tables hold.  No atomics, no LDS; bitwise reproducible. */
int lc2is_aug_apply(const uint8_t* img, size_t img_bytes, const uint8_t* lab, size_t lab_bytes, const lc2is_aug_image* desc,
                    long n_images, const int64_t* slots, const int32_t* params, int B, int S, int L,
                    const lc2is_aug_norm* norm /* HOST */, long pad_label, float* out_img, int64_t* out_lab,
                    lc2is_stream_t stream);

/* aug_crop_select_kernel, an OPTIONAL launch between lc2is_aug_params and lc2is_aug_apply: the class-ratio re-draw of the crop
 * origin.  One block per sample b < B reads row b of params and the pool's label map and overwrites the row's LC2IS_AUG_TOP /
 * LC2IS_AUG_LEFT words with the selected candidate; every other word of the row stays.  S = cfg->crop_size, S % L == 0, q = S / L.
 * Integers only: the result is exact.
 *   Candidates: candidate 0 is the (top, left) already in the row (draws k = 1, 2); for t = 1 .. tries (1 <= tries <=
 *     LC2IS_AUG_MAX_TRIES)   top_t = (u24(10 + 2t) * (max(nh - S, 0) + 1)) >> 24,  left_t = (u24(11 + 2t) * (max(nw - S, 0) + 1)) >> 24
 *     with the sample hash of lc2is_aug_params (cfg's seed, *epoch, key = keys ? keys[b] : slots[b]): draws 12 .. 31.
 *   Counted for candidate t: exactly the L x L label cells lc2is_aug_apply would write for (nh, nw, top_t, left_t, flip of the
 *     row) - cell (i, j) looks at output pixel (i*q + q/2, j*q + q/2), the same yr, xr (flip included) and nearest-exact ys, xs.  A
 *     cell outside [0, nh) x [0, nw) is padding and is not counted, whatever pad_label will be; a cell whose label equals
 *     ignore_label (0 .. 255, or -1 for none) is not counted.  n_c per class c, n = sum n_c, m = max n_c, d = #{c : n_c > 0}.
 *   Verdict: candidate t is accepted iff d > 1 && m * 1024 < ratio1024 * n (64-bit), ratio1024 = round(cat_max_ratio * 1024) in
 *     1 .. 1023: mmseg's `len(cnt) > 1 and max(cnt) / sum(cnt) < cat_max_ratio`, on the labels the loss will see (mmseg counts the
 *     full-resolution crop; the cells are q * q times fewer reads).
 *   Selection: candidates 0 .. tries-1 are checked in order and the first accepted one is taken; if none is, candidate `tries` is
 *     taken unchecked (mmseg draws once more after its last failed check in the same way).
 *   info (may be NULL): int32 [B][4] = {t*, n, m, d} of the chosen candidate, {tries, 0, 0, 0} when none was accepted.
 * A slot outside [0, n_images), a descriptor whose sides or lab_off do not fit lab_bytes, or nh / nw outside
 * 1 .. LC2IS_AUG_MAX_RESIZED (the all-zero row lc2is_aug_params writes for a bad slot included): the row is left untouched, info =
 * {-1, 0, 0, 0}, and nothing outside the buffers is read.  The class counts are a wave-merged LDS histogram (csrc/label_hist.h):
 * NO read-modify-write atomics, LDS included; bitwise reproducible; device values only, so a captured launch selects afresh on replay.
 * Errors: LC2IS_ERR_NULL (lab, desc, slots, epoch, cfg, params); LC2IS_ERR_SHAPE (B, n_images < 1, S % L, ratio1024, ignore_label or
 * tries out of range, params / info not 4-byte or desc not 8-byte aligned).
 * replaces: mmseg's RandomCrop(cat_max_ratio=0.75) - np.unique over every candidate crop of the label map, on the host. */
#define LC2IS_AUG_MAX_TRIES 10
int lc2is_aug_crop_select(const uint8_t* lab, size_t lab_bytes, const lc2is_aug_image* desc, long n_images, const int64_t* slots,
                          const int64_t* keys, int B, const int32_t* epoch, const lc2is_aug_config* cfg /* HOST */, int32_t* params,
                          int L, int ratio1024, int ignore_label, int tries, int32_t* info, lc2is_stream_t stream);

/* label_hist_kernel, one block per row b < B with a block-stride loop: counts[b][v] (int32 [B][256], OVERWRITTEN) = the number of
 * pixels of image slots[b] whose label is v.  Sides are at most LC2IS_AUG_MAX_SIDE, so a count stays below 2^24 + 1.  The same range
 * checks as above (slot, sides, lab_off against lab_bytes): a bad row gives all zeros and reads nothing.  The same wave-merged LDS
 * histogram: no atomics, exact.  Errors: LC2IS_ERR_NULL; LC2IS_ERR_SHAPE (B, n_images < 1, counts not 4-byte or desc not 8-byte aligned).
 * replaces: np.bincount / torch.bincount over every label map of the training split, the input of median-frequency (Eigen &
 *   Fergus) or ENet class weights for nn.CrossEntropyLoss(weight=). */
int lc2is_label_histogram(const uint8_t* lab, size_t lab_bytes, const lc2is_aug_image* desc, long n_images, const int64_t* slots,
                          int B, int32_t* counts, lc2is_stream_t stream);

/* ---- mixed-sample augmentation on the device: ClassMix and CutMix of two batches, two launches ------------------------
 * Output sample b < B is destination sample b with the masked region replaced by source sample s = src_index[b] (NULL: s = b) of a
 * source batch of Bs samples; a batch is pixels fp32 [.,3,S,S], labels int64 [.,L,L] and per-pixel loss weights fp32 [.,L,L] or NULL
 * (= ones).  S % 4 == 0, S % L == 0, r = S / L >= 1, S <= LC2IS_AUG_MAX_SIDE.  The mask lives on the L x L label cells; pixel (y, x)
 * belongs to cell (y / r, x / r).  The outputs are SELECTS, never blends:
 *   out_px = mask ? src_px : dst_px (all three channels), out_lab = mask ? src_lab : dst_lab, out_pw = mask ? src_pw : dst_pw,
 * only the chosen side of an element is read, so a NaN / infinity on the other side does not reach the output.  The outputs may
 * alias neither input; the source batch may be the destination batch itself (ClassMix within a batch, src_index = a roll).
 * Random numbers: h = the sample hash of lc2is_aug_params for (cfg's seed, *epoch, keys[b]) XOR LC2IS_MIX_STREAM, u24(k) as there:
 * a mixer and a TrainAugment with the same seed share no draw, a sample's mask depends on (seed, epoch, key, its source label map)
 * only, and a captured launch pair draws again on replay from the DEVICE epoch / keys / src_index.
 * Mask, by cfg->mode:
 *   LC2IS_MIX_CLASSMIX: the classes PRESENT in the source map src_lab[s] are the labels v with 0 <= v < n_classes, v != ignore_index,
 *     v != exclude_label (-1: none; ADE20K's label 0, the pad label, is the usual value); 1 <= n_classes <= LC2IS_MIX_MAX_CLASSES.
 *     With n present, the CHOSEN set is the ceil(n / 2) present classes c with the smallest pairs (u24(16 + c), c) - ties of the
 *     24-bit draw break by class id: a uniformly random subset of fixed size, DACS's randperm(n)[:(n + n % 2) / 2].  A cell is
 *     masked iff its source label is chosen; n = 0 gives the empty mask.
 *   LC2IS_MIX_CUTMIX, one box, integers only (64-bit products):
 *     a = area_lo1024 + ((u24(0) * (area_hi1024 - area_lo1024 + 1)) >> 24)      the box's share of the area in 1/1024 units
 *     hmin = max(1, ceil(a * L / 1024));  bh = hmin + ((u24(1) * (L - hmin + 1)) >> 24)
 *     bw = clamp((2 * a * L * L + 1024 * bh) / (2 * 1024 * bh), 1, L)            a * L * L / (1024 * bh), rounded
 *     top = (u24(2) * (L - bh + 1)) >> 24;  left = (u24(3) * (L - bw + 1)) >> 24
 *     cell (i, j) is masked iff top <= i < top + bh && left <= j < left + bw.  1 <= area_lo1024 <= area_hi1024 <= 1024 (default
 *     256, 512).  The aspect is uniform in the box HEIGHT; CutMix-Seg's is log-uniform in the aspect ratio.
 *   LC2IS_MIX_NONE: the empty mask.
 * replaces: DACS / DAFormer's ClassMix (torch.unique per image - a host read -, randperm, a broadcast compare, three blends by a
 *   float mask) and the CutMix of CPS / UniMatch / French et al. (numpy box draws on the host, slice assignment per image). */
#define LC2IS_MIX_NONE 0
#define LC2IS_MIX_CLASSMIX 1
#define LC2IS_MIX_CUTMIX 2
#define LC2IS_MIX_MAX_CLASSES 1024
#define LC2IS_MIX_STREAM 0x4D495831u /* "MIX1" */
#define LC2IS_MIX_PLAN_WORDS 40      /* one plan row, int32: {mode, source row, top, left, bh, bw, classes present, classes chosen}, */
#define LC2IS_MIX_BITMAP 8           /*   then the chosen-class bitmap: class c is bit c % 32 of word LC2IS_MIX_BITMAP + c / 32     */
typedef struct {
  uint32_t seed_lo, seed_hi;          /* the 64-bit seed                                              */
  int32_t mode;                       /* LC2IS_MIX_*                                                  */
  int32_t n_classes;                  /* classmix: 1 .. LC2IS_MIX_MAX_CLASSES                         */
  int64_t ignore_index, exclude_label;/* classmix: labels that are never present (exclude: -1 = none) */
  int32_t area_lo1024, area_hi1024;   /* cutmix: the box's area share in 1/1024 units                 */
} lc2is_mix_config;

/* mix_select_kernel, one block of 1024 lanes per output sample b < B: writes row b of plan int32 [B][LC2IS_MIX_PLAN_WORDS] and of
 * info int32 [B][4] = {classes present, classes chosen, masked cells, L * L}.  Classmix: presence is recorded as flags in LDS
 * (same-value plain stores), a class's rank is the count of smaller pairs among the present classes, the bitmap words are wave
 * ballots, the masked cells are counted by ballot + popcount and summed in a fixed order; top .. bw are 0.  Cutmix: the box, the two
 * class counts and the bitmap are 0, masked cells = bh * bw.  NO read-modify-write atomics, LDS included; bitwise reproducible.
 * A source row outside [0, Bs): the plan row is all zeros (mode NONE: the empty mask, nothing of the source is read, by
 * lc2is_mix_apply neither) and info = {-1, 0, 0, 0}.
 * Errors, in this order, from the arguments alone: LC2IS_ERR_NULL (src_lab, keys, epoch, cfg, plan, info); LC2IS_ERR_SHAPE (B, Bs < 1,
 * L outside 1 .. LC2IS_AUG_MAX_SIDE, n_classes or the area range out of range, src_lab / keys / src_index not 8-byte, plan / info /
 * epoch not 4-byte aligned); LC2IS_ERR_UNSUPPORTED (a mode that is none of the three). */
int lc2is_mix_select(const int64_t* src_lab, int Bs, const int64_t* src_index, const int64_t* keys, int B, const int32_t* epoch,
                     const lc2is_mix_config* cfg /* HOST */, int L, int32_t* plan, int32_t* info, lc2is_stream_t stream);

/* mix_apply_kernel, ONE launch for pixels, labels and weights: grid.y = B samples, grid.x = pixel blocks followed by label-cell
 * blocks (256 lanes; a pixel lane makes 4 consecutive x of all 3 channels with 16-byte loads and stores and ONE mask lookup when
 * r % 4 == 0; otherwise a float4 can straddle two cells and the lane selects per element, with 16-byte loads where its four masks
 * agree).  Reads the plan rows lc2is_mix_select wrote; a row whose mode is none of CLASSMIX / CUTMIX or whose source row lies outside
 * [0, Bs) gives the destination sample, and whatever a row holds nothing outside the batches is read.  dst_pw / src_pw may be NULL
 * (ones).  Ideal traffic: one read and one write of [B,3,S,S] plus the label and weight maps.  No atomics; bitwise reproducible.
 * Errors, in this order: LC2IS_ERR_NULL (dst_px, dst_lab, src_px, src_lab, plan, out_px, out_lab, out_pw); LC2IS_ERR_SHAPE (B outside
 * 1 .. 65535, Bs < 1, S outside 4 .. LC2IS_AUG_MAX_SIDE, S % 4, L < 1, S % L, pixels not 16-byte, labels not 8-byte, weights / plan
 * not 4-byte aligned, an output that overlaps an input). */
int lc2is_mix_apply(const float* dst_px, const int64_t* dst_lab, const float* dst_pw, const float* src_px, const int64_t* src_lab,
                    const float* src_pw, int Bs, const int32_t* plan, int B, int S, int L, float* out_px, int64_t* out_lab,
                    float* out_pw, lc2is_stream_t stream);

/* ---- strong photometric views on the device: colour jitter, random greyscale, Gaussian blur; two launches --------------
 * The student's view in self-training (FixMatch, UniMatch, CPS, DACS, DAFormer): the SAME geometry as the view the teacher
 * labelled, another and stronger colour, made from the normalised fp32 batch [B,3,S,S] (before or after the mix).  Per sample b, from
 * row b of a parameter table int32 [B][LC2IS_STRONG_PARAM_WORDS] (fp32 fields as bit patterns):
 *   word LC2IS_STRONG_FLAGS   bit 0 (LC2IS_STRONG_COLOUR): the colour map (M, o) is not the identity and is applied;
 *                             bit 1 (LC2IS_STRONG_GREY): greyscale was drawn (recorded; it is folded into M, o, and implies bit 0);
 *                             bit 2 (LC2IS_STRONG_BLUR): the blur is applied
 *   word LC2IS_STRONG_R       int32 R, the blur's radius, 0 .. LC2IS_STRONG_MAX_RADIUS
 *   word LC2IS_STRONG_SIGMA   fp32 sigma
 *   words LC2IS_STRONG_M ..   fp32 M[3][3] row-major, then LC2IS_STRONG_O .. fp32 o[3]: rgb' = clamp(M rgb + o, 0, 255), 0..255 scale
 *   words LC2IS_STRONG_W ..   fp32 w[0 .. 8], the blur's taps (w[k] weighs the pixels at distance k); entries past R are 0
 *   words 24 .. 31            0
 * Random numbers: h = the sample hash of lc2is_aug_params for (cfg's seed, *epoch, keys[b]) XOR LC2IS_STRONG_STREAM, u24(k) as there: a
 * StrongAugment, a TrainAugment and a SampleMix with one seed share no draw; a sample's view depends on (seed, epoch, key) only, and a
 * captured launch pair draws again on replay from the DEVICE epoch / keys.  Draws (a value is drawn whether its switch is on or not):
 *   k=0  jitter group on iff u24 < jitter_thr
 *   k=1..4  brightness b in [-brightness_delta, brightness_delta] (0..255 scale), contrast c, saturation s, hue h (radians), each
 *           lo + (hi - lo) * (u24 * 2^-24) in fp32
 *   k=5  grey on iff u24 < gray_thr        k=6  blur on iff u24 < blur_thr
 *   k=7  sigma = fma(sigma_hi - sigma_lo, u24 * 2^-24, sigma_lo) in fp32 (the difference rounded, then ONE rounding), 0 < sigma_lo <=
 *        sigma_hi <= 2.0;  R = min(LC2IS_STRONG_MAX_RADIUS, ceil(4 * sigma))
 * Colour: M = I, o = 0; with the jitter group on ALL FOUR steps of lc2is_aug_params in its order and linear form: brightness o += b;
 * contrast M, o *= c; saturation (M, o) = A (M, o), A = s I + (1 - s) 1 w^T; hue (M, o) = R (M, o), R the rotation by h about
 * (1, 1, 1) / sqrt(3).  Grey on then applies (M, o) = A (M, o) with A = 1 w^T, w = (0.299, 0.587, 0.114).  ONE clamp to [0, 255]
 * follows in strong_apply, none between the steps: intermediate values outside the range are carried, not cut - the project's
 * deliberate difference from torchvision's ColorJitter, which clips after every step.
 * Blur taps: w_k = exp(-k^2 / (2 sigma^2)) / (w_0 + 2 sum_{k=1..R} w_k) for k = 0 .. R, formed in fp32 in the params kernel. */
#define LC2IS_STRONG_MAX_RADIUS 8
#define LC2IS_STRONG_STREAM 0x53545231u /* "STR1" */
#define LC2IS_STRONG_PARAM_WORDS 32
#define LC2IS_STRONG_FLAGS 0
#define LC2IS_STRONG_R 1
#define LC2IS_STRONG_SIGMA 2
#define LC2IS_STRONG_M 3
#define LC2IS_STRONG_O 12
#define LC2IS_STRONG_W 15
#define LC2IS_STRONG_COLOUR 1
#define LC2IS_STRONG_GREY 2
#define LC2IS_STRONG_BLUR 4
typedef struct {
  uint32_t seed_lo, seed_hi;                /* the 64-bit seed                                                           */
  uint32_t jitter_thr, gray_thr, blur_thr;  /* round(p * 2^24): on iff u24 < thr                                         */
  float brightness_delta;                   /* b in [-delta, delta], added on the 0..255 scale                           */
  float contrast_lo, contrast_hi;           /* c: every channel is multiplied by c                                       */
  float saturation_lo, saturation_hi;       /* s: rgb' = s rgb + (1 - s) grey                                            */
  float hue_delta;                          /* h in [-delta, delta] RADIANS                                              */
  float sigma_lo, sigma_hi;                 /* 0 < sigma_lo <= sigma_hi <= 2.0                                           */
  float mean[3], std[3], inv_std[3];        /* the batch's normalisation; inv_std_c = 1 / std_c rounded to fp32 once     */
} lc2is_strong_config;

/* strong_params_kernel, one thread per sample b < B: writes row b of params as defined above.  No atomics.
 * Errors, in this order, from the arguments alone: LC2IS_ERR_NULL (keys, epoch, cfg, params); LC2IS_ERR_SHAPE (B < 1, a threshold above
 * 2^24, a sigma range that is not 0 < lo <= hi <= 2.0, keys not 8-byte, epoch / params not 4-byte aligned).
 * replaces: the host-side draws of torchvision's ColorJitter.get_params / RandomGrayscale / GaussianBlur.get_params (torch.rand,
 *   torch.empty(1).uniform_(sigma_min, sigma_max) per image) and the Gaussian kernel each image's sigma is turned into. */
int lc2is_strong_params(const int64_t* keys, int B, const int32_t* epoch, const lc2is_strong_config* cfg /* HOST */, int32_t* params,
                        lc2is_stream_t stream);

/* strong_apply_kernel, ONE launch for the batch: grid.y = B samples, grid.x = tiles of 32 rows x 64 columns; in / out fp32
 * [B][3][S][S].  Sample b, as row b of params says (only the words named here are read; bit 1 of the flags is not acted on):
 *   flags == 0: out = in BIT FOR BIT (NaN payloads included): no de-normalise / re-normalise round trip.
 *   colour (bit 0):  v_c = 255 * (x_c * std_c + mean_c);  v' = clamp(M v + o, 0, 255)  (fminf(fmaxf(., 0), 255): a NaN becomes 0);
 *     after the blur, if any:  out_c = (v'_c * (1/255) - mean_c) * inv_std_c   (lc2is_aug_apply's last line).
 *   blur (bit 2):  a separable blur with the row's w[0 .. R] on v' (directly on x when colour is off), rows first, then columns:
 *     t(y, x) = w_0 v'(y, x) + sum_{k=1..R} w_k (v'(y, rho(x - k)) + v'(y, rho(x + k))),  u(y, x) the same over y on t, with the
 *     border reflected without repeating the edge: rho(i) = -i for i < 0, 2 (S - 1) - i for i >= S (torch's "reflect"; S >= 12 > R).
 *     Taps past R are not read, whatever the row's w holds there.
 *   A row whose R lies outside 0 .. LC2IS_STRONG_MAX_RADIUS or whose flag word has a bit above bit 2 is rendered as the copy.  Every
 *   index is reflected and then clamped into the image: whatever a row holds, nothing outside `in` is read.
 * Samples without blur stream: 16-byte loads and stores, no LDS traffic.  With blur the colour-mapped tile plus a halo of R is staged
 * in LDS once per block (colour at staging time, not per tap) and both passes run from LDS; 57 KB of LDS per block, two blocks per
 * CU.  The branch is block-uniform (one sample per grid.y).  No atomics, no scratch; bitwise reproducible; a sample's output does not
 * depend on B or on its position in the batch.  Ideal traffic: one read and one write of [B,3,S,S].
 * Errors, in this order, from the arguments alone: LC2IS_ERR_NULL (in, params, cfg, out); LC2IS_ERR_SHAPE (B outside 1 .. 65535, S
 * outside 12 .. LC2IS_AUG_MAX_SIDE, S % 4, in / out not 16-byte or params not 4-byte aligned, in and out overlapping: the blur reads a
 * halo, so the call cannot run in place).
 * replaces: ColorJitter + RandomGrayscale + GaussianBlur applied to the normalised batch: de-normalise, a per-sample 3x3 product
 *   (einsum), clamp, F.pad(mode="reflect") + a grouped conv2d with per-sample kernels, re-normalise - several passes over the batch. */
int lc2is_strong_apply(const float* in, const int32_t* params, const lc2is_strong_config* cfg /* HOST */, int B, int S, float* out,
                       lc2is_stream_t stream);

/* ---- geometric views on the device: a random affine warp per sample, the labels follow; two launches -------------------
 * Rotation, isotropic scale, shear, translation and horizontal flip of a batch: pixels fp32 [B,3,S,S] bilinear, labels int64 [B,L,L]
 * and per-pixel loss weights fp32 [B,L,L] nearest, all three under the SAME map.  Out-of-frame image taps take cfg->fill (normalised
 * units; 0.0 is the mean colour), out-of-frame label cells take cfg->ignore_index and their weights 0.0.  The map goes from OUTPUT to
 * SOURCE and is held as integers, so every index and every fraction is exact.  Row b of a parameter table int32
 * [B][LC2IS_GEO_PARAM_WORDS]:
 *   word LC2IS_GEO_FLAGS      bit 0 (LC2IS_GEO_WARP): the map is not the identity or the flip; bit 1 (LC2IS_GEO_FLIP): flipped
 *   words LC2IS_GEO_M ..      m00 m01 m10 m11 in Q16 (LC2IS_GEO_ONE = 65536 = 1.0)
 *   words LC2IS_GEO_T ..      tx ty in Q16, as a fraction of the side
 *   words LC2IS_GEO_REC ..    the fp32 bit patterns of theta, s, phi, fx, fy as drawn: recorded for the reader, lc2is_geo_apply does not
 *                             read them
 *   words 12 .. 15            0
 * The map, for output element (y, x) of a map of side n (n = S for pixels, n = L for label cells), all in int64:
 *   u = 2x + 1 - n,  v = 2y + 1 - n,   U = m00 u + m01 v + 2 tx n,   V = m10 u + m11 v + 2 ty n
 * Pixels:  X = U + (S - 1) 65536;  x0 = X >> 17 (floor);  fx = (X & 0x1FFFF) 2^-17;  Y, y0, fy likewise from V.  The taps are
 *   (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1); a tap outside [0, S)^2 is fill_c.
 *   out = lerp(lerp(p00, p01, fx), lerp(p10, p11, fx), fy),  lerp(a, b, f) = a + f (b - a)  (lc2is_aug_apply's form), in fp32.
 *   When a fraction is 0 the near tap is SELECTED and the far tap is not read: a NaN next door does not spread, and the identity,
 *   the flip, quarter turns and whole-pixel shifts are bit-exact copies of their source elements.
 *   This is F.grid_sample(x, F.affine_grid(theta, align_corners=False), "bilinear", "zeros", align_corners=False) with
 *   theta = [[m00, m01, 2 tx], [m10, m11, 2 ty]] / 65536 (and fill = 0).
 * Label cells and weights:  xs = (U + L 65536) >> 17,  ys = (V + L 65536) >> 17  (the nearest cell centre, ties upwards); a cell
 *   inside [0, L)^2 takes lab[ys][xs] and pw[ys][xs], a cell outside takes ignore_index and 0.0.
 * Random numbers: h = the sample hash of lc2is_aug_params for (cfg's seed, *epoch, keys[b]) XOR LC2IS_GEO_STREAM, u24(k) as there: a
 * GeometricAugment, a StrongAugment, a SampleMix and a TrainAugment with one seed share no draw; a sample's map depends on (seed,
 * epoch, key) only, and a captured launch pair draws again on replay from the DEVICE epoch / keys.  Draws (a value is drawn whether
 * its switch is on or not), each fp32 value fma(hi - lo, u24 * 2^-24, lo): the difference rounded to fp32, then ONE rounding (what
 * aug_range's lo + (hi - lo) * t compiles to; written out here so that tx, ty can be restated exactly):
 *   k=0  warp on iff u24 < warp_thr                 k=1  theta in [-rotate, rotate] radians
 *   k=2  s in [scale_lo, scale_hi], uniform         k=3  phi in [-shear, shear] radians
 *   k=4, 5  fx, fy in [-translate, translate]       k=6  flip on iff u24 < flip_thr, independent of k=0
 * With warp on, in fp32:  M = (1/s) R(theta) H(phi),  R = [[cos, -sin], [sin, cos]],  H = [[1, tan phi], [0, 1]],
 *   m.. = (int)rintf(M.. * 65536),  t. = (int)rintf(f. * 65536);  otherwise M = I, t = 0.  Flip then negates column 0 (m00, m10).
 *   s > 1 magnifies.  With this M the content turns counter-clockwise: [[0, -1], [1, 0]] gives torch.rot90(x, 1, (-2, -1)).
 * Limits of the config: 0 <= rotate <= pi, 0.25 <= scale_lo <= scale_hi <= 4, 0 <= shear <= pi / 4, 0 <= translate <= 0.5 (the fp32
 * neighbours of pi and pi / 4 included), thresholds <= 2^24; they keep |m..| <= LC2IS_GEO_MAX_M = 8 * 65536. */
#define LC2IS_GEO_STREAM 0x47454F31u /* "GEO1" */
#define LC2IS_GEO_PARAM_WORDS 16
#define LC2IS_GEO_FLAGS 0
#define LC2IS_GEO_M 1
#define LC2IS_GEO_T 5
#define LC2IS_GEO_REC 7
#define LC2IS_GEO_WARP 1
#define LC2IS_GEO_FLIP 2
#define LC2IS_GEO_ONE 65536
#define LC2IS_GEO_MAX_M 524288
#define LC2IS_GEO_MAX_T 65536
#define LC2IS_GEO_MIN_SIDE 8
typedef struct {
  uint32_t seed_lo, seed_hi;      /* the 64-bit seed                                                   */
  uint32_t warp_thr, flip_thr;    /* round(p * 2^24): on iff u24 < thr                                 */
  float rotate;                   /* theta in [-rotate, rotate] RADIANS, rotate <= pi                  */
  float scale_lo, scale_hi;       /* s: 0.25 <= scale_lo <= scale_hi <= 4                              */
  float shear;                    /* phi in [-shear, shear] RADIANS, shear <= pi / 4                   */
  float translate;                /* fx, fy in [-translate, translate] of the side, translate <= 0.5   */
  float fill[3];                  /* out-of-frame colour per channel, NORMALISED units                 */
  int64_t ignore_index;           /* out-of-frame label                                                */
} lc2is_geo_config;

/* geo_params_kernel, one thread per sample b < B: writes row b of params as defined above.  No atomics.
 * Errors, in this order, from the arguments alone: LC2IS_ERR_NULL (keys, epoch, cfg, params); LC2IS_ERR_SHAPE (B < 1, a config outside
 * the limits above, keys not 8-byte, epoch / params not 4-byte aligned).
 * replaces: the host-side draws of torchvision's RandomAffine.get_params / RandomHorizontalFlip and mmseg's RandomRotate (one
 *   torch.empty(1).uniform_ or np.random call per value and image) and the 2 x 3 theta each image's draw is turned into. */
int lc2is_geo_params(const int64_t* keys, int B, const int32_t* epoch, const lc2is_geo_config* cfg /* HOST */, int32_t* params,
                     lc2is_stream_t stream);

/* geo_apply_kernel, ONE launch for pixels, labels and weights: grid.y = B samples, grid.x = pixel blocks followed by label-cell
 * blocks (256 lanes), the layout of mix_apply_kernel.  in_lab / in_pw may be NULL: that map is then neither read nor written (its
 * out pointer is ignored); with both NULL there are no label-cell blocks (L is still checked).  Sample b, as row b of params says
 * (only words 0 .. 6 are read):
 *   flags == 0, whatever the other words hold: the COPY of the sample - pixels, labels and weights bit for bit (NaN payloads too).
 *   a flag bit above bit 1, an |m..| > LC2IS_GEO_MAX_M or a |t.| > LC2IS_GEO_MAX_T: rendered as the copy as well.
 *   otherwise (bit 0 or bit 1 set): the map of words 1 .. 6 as defined above.  The two bits are not told apart: a flip is the map
 *   m = (-65536, 0, 0, 65536).
 * Every 64-bit index is clamped into [-2, n] before it is narrowed and every tap is bounds-checked: whatever a row holds, nothing
 * outside the inputs is read.
 * Copy rows stream: a block moves 512 consecutive pixel quads of all three channels with 16-byte loads and stores, no index
 * arithmetic (the later half of the sample's blocks has nothing to do).  Mapped rows: a block makes a 32 x 32 output tile; a lane
 * makes 4 consecutive x of all three channels and writes three 16-byte stores.  A wave's patch is 32 columns x 8 rows (strong_apply's
 * is 64 x 4): each of its store instructions still fills whole 128-byte lines, and its rotated footprint is squarer, so at 45
 * degrees it spans about 28 source rows of 2 lines each where the 64 x 4 patch spans 48 rows of 2 - 3 lines.  The taps come from one
 * of two places, chosen per block (block-uniform):
 *   staged: the block forms the source bounding box of its tile from the tile's four corners (the map is affine, so the extreme
 *     near taps belong to corners; + 1 for the far taps), clips it to the image and widens it to whole quads; when the box holds at
 *     most 4096 words per channel (48 KB of LDS, three blocks per CU) it is staged once with 16-byte loads and every tap is an LDS
 *     read.  Up to a 2 x zoom-out at any angle fits (45 degrees at scale 0.8: 60 x 64); at S <= 64 everything fits.
 *   direct: a larger box (zooming far out: scale 0.25 reads 128 x 128) is not staged; the taps are predicated 4-byte gathers from
 *     global memory.  The arithmetic is the same: both forms give the same bits.
 * Label cells are one per lane (8-byte / 4-byte accesses) in every case.  The branches are block-uniform (one sample per grid.y).
 * No atomics, no scratch; bitwise reproducible; a sample's output depends neither on B nor on its position in the batch.  Ideal
 * traffic: one read and one write of [B,3,S,S] plus the label and weight maps.
 * Errors, in this order, from the arguments alone: LC2IS_ERR_NULL (in_px, params, cfg, out_px; out_lab with in_lab given; out_pw
 * with in_pw given); LC2IS_ERR_SHAPE (B outside 1 .. 65535, S outside LC2IS_GEO_MIN_SIDE .. LC2IS_AUG_MAX_SIDE, S % 4, L < 1, S % L, a
 * config outside the limits, pixels not 16-byte, labels not 8-byte, weights / params not 4-byte aligned, an output that overlaps
 * its input).
 * replaces: torchvision's RandomAffine / mmseg's RandomRotate on a device batch - F.affine_grid, F.grid_sample(bilinear) on the
 *   pixels, F.grid_sample(nearest) on float copies of labels and weights, an in-frame mask and torch.where for the fill colour, the
 *   ignore label and the zero weight: several full-size temporaries, and no exact definition at cell edges. */
int lc2is_geo_apply(const float* in_px, const int64_t* in_lab, const float* in_pw, const int32_t* params,
                    const lc2is_geo_config* cfg /* HOST */, int B, int S, int L, float* out_px, int64_t* out_lab, float* out_pw,
                    lc2is_stream_t stream);

/* geo_scores_kernel, ONE launch: a teacher's low-resolution score map follows the student's geometric view (the soft-teacher step
 * under a geometric view: the teacher saw the weak view, the student sees the warped one, and the per-pixel KL needs the teacher's
 * scores at the student's grid positions), with an optional weight map at label resolution.  The FORWARD direction only: the same
 * output-to-source map as lc2is_geo_apply.
 *   in_scores / out_scores  fp32 [B][g][g][ld], i.e. [B*g*g, ld] channel-last as the head's scores are held; ALL ld columns are
 *                           treated alike (padding columns are warped like the rest; their content is nobody's business)
 *   params                  the table [B][LC2IS_GEO_PARAM_WORDS] of lc2is_geo_params; only words 0 .. 6 are read
 *   in_tw / out_tw          fp32 [B][L][L], looked at only with want_tw != 0; in_tw may be NULL
 * Rows are told apart exactly as lc2is_geo_apply tells them apart: flags == 0, a flag bit above bit 1, an |m..| > LC2IS_GEO_MAX_M
 * or a |t.| > LC2IS_GEO_MAX_T give the COPY of the sample, bit for bit (NaN payloads too); otherwise the map of words 1 .. 6.
 * Scores of a mapped row, output cell (y, x): the map above for a map of side n = g, all in int64:
 *   u = 2x + 1 - g,  v = 2y + 1 - g,   U = m00 u + m01 v + 2 tx g,   V = m10 u + m11 v + 2 ty g
 *   X = U + (g - 1) 65536;  Xc = min(max(X, 0), (g - 1) 2^17);  x0 = Xc >> 17;  fxi = Xc & 0x1FFFF;  fx = fxi 2^-17;
 *   Y, Yc, y0, fyi, fy likewise from V.
 *   The position is clamped BEFORE it is split into index and fraction: an out-of-frame cell selects the border cell (fraction
 *   0) with no arithmetic, and every tap that is read lies inside the sample.  Taps and order are lc2is_geo_apply's pixel rule, per
 *   column, in fp32:
 *     top = fxi ? p00 + fx (p01 - p00) : p00;   bot = fxi ? p10 + fx (p11 - p10) : p10;   out = fyi ? top + fy (bot - top) : top
 *   with p00 = in[y0][x0], p01 = in[y0][x0+1], p10 = in[y0+1][x0], p11 = in[y0+1][x0+1]; a far tap whose fraction is 0 is not read:
 *   the identity, the flip, quarter and half turns and whole-cell shifts move bits, and a NaN next door does not spread.
 *   This is F.grid_sample(x, F.affine_grid(theta, align_corners=False), "bilinear", padding_mode="border", align_corners=False)
 *   with theta = [[m00, m01, 2 tx], [m10, m11, 2 ty]] / 65536 on the [B, ld, g, g] view of the scores.
 *   Border, not a fill value: the head upsamples these scores bicubically, so a fill would leak into in-frame pixels next to the
 *   edge; border values are plausible scores, and the mask below takes the out-of-frame pixels out of the loss.
 * Weight map, want_tw != 0: lc2is_geo_apply's cell rule at side L: xs = (U + L 65536) >> 17, ys = (V + L 65536) >> 17 with U, V for
 *   n = L; a cell inside [0, L)^2 takes in_tw[ys][xs], or 1.0f when in_tw is NULL (out_tw is then the IN-FRAME MASK); a cell outside
 *   takes 0.0f.  A copy row copies in_tw, or writes ones.  With want_tw == 0 neither weight pointer is touched (L is not checked).
 * Layout: grid.y = B samples, grid.x = score blocks followed by weight-cell blocks (256 lanes), the branches block-uniform (one
 * sample per grid.y).  A score block of a mapped row owns a 4 x 4 patch of output cells, so that neighbouring cells share their taps
 * in cache; a lane owns a float4 column group of a cell: four 16-byte loads at most and one 16-byte store along the channel axis,
 * the lanes of a cell reading whole rows of 4 ld bytes.  A copy row streams: block k moves the 4 ld quads after quad 4 ld k of the
 * sample with 16-byte loads and stores and no index arithmetic.  Weight cells are one per lane (4-byte accesses).  No LDS, no
 * atomics, no scratch; bitwise reproducible; a sample's output depends neither on B nor on its position in the batch.  Every
 * 64-bit index is range-checked before it is narrowed: whatever a row holds, nothing outside the inputs is read.  Ideal traffic:
 * one read and one write of the scores plus the weight map.
 * Errors, in this order, from the arguments alone: LC2IS_ERR_NULL (in_scores, params, out_scores; out_tw with want_tw);
 * LC2IS_ERR_SHAPE (B outside 1 .. 65535, g outside 1 .. 512, ld outside 4 .. 1024, ld % 4; with want_tw: L < 1,
 * L > LC2IS_AUG_MAX_SIDE, L % g; scores not 16-byte, weights / params not 4-byte aligned; an output that overlaps its input).
 * replaces: scores.view(B, g, g, ld).permute(0, 3, 1, 2), a theta built from the table (on the host: a read-back that breaks graph
 *   capture), F.affine_grid, F.grid_sample(bilinear, border), permute back and contiguous(); for the mask F.grid_sample(nearest) of
 *   the weights or of ones and a torch.where - several temporaries of the scores' size, and no exact definition at cell edges. */
int lc2is_geo_scores(const float* in_scores, const float* in_tw, const int32_t* params, int B, int g, int ld, int L, int want_tw,
                     float* out_scores, float* out_tw, lc2is_stream_t stream);

/* ---- online hard example mining (OHEM): the loss over the pixels the model currently gets wrong ----------------------
 * Rule, in loss space: a pixel is valid iff label != ignore_index && 0 <= label < C; l_i = lse_i - z_{i,y_i} (plain CE, fp32);
 * k = min(min_kept_total, n_valid - 1); L = the valid loss of rank k (0-based, descending); L_eff = fminf(L, loss_thresh) with
 * loss_thresh = fp32(-log(thresh)) formed in fp64 by the caller; a valid pixel is KEPT iff l_i > L_eff (IEEE, strict: the pivot
 * and its ties are dropped).  labels_out = label where kept, ignore_index elsewhere; the OHEM loss is the existing criterion on
 * labels_out.
 * replaces: mmseg's OHEMPixelSampler with a threshold / HRNet's OhemCrossEntropy (softmax, gather, sort, p < max(p_sorted[k],
 *   thresh)) — torch.sort / topk over every pixel of the batch.
 *
 * lc2is_head_upsample_px: the forward half of lc2is_head_upsample_ce alone, S in {4, 8, 16} (else LC2IS_ERR_UNSUPPORTED): the same
 * upsample products and softmax, one launch, no workspace, no gradient; loss_px fp32 [B,H,W] (16-byte aligned) receives l_i, 0
 * where the pixel is not valid.  Bitwise reproducible.
 * replaces: F.interpolate + F.cross_entropy(reduction="none") in front of the sampler. */
int lc2is_head_upsample_px(const float* scores_lo, int ld, const int64_t* labels, float* loss_px, int B, int h, int w, int C,
                           int S, int mode, long ignore_index, lc2is_stream_t stream);

/* The 24-byte block lc2is_ohem_select writes.  n_valid = 0: k = -1, L = +inf (nothing exceeds the pivot of an empty set). */
typedef struct {
  int64_t n_valid;   /* valid pixels                                                  */
  int64_t k;         /* min(min_kept_total, n_valid - 1)                              */
  float L;           /* the valid loss of rank k, descending                          */
  float L_eff;       /* fminf(L, loss_thresh): kept iff l_i > L_eff                   */
} lc2is_ohem_info;

/* Exact k-th largest on the device and the relabelling, over n = B*H*W values (1 <= n < 2^31), no host read, capturable.
 * Most-significant-digit radix select, four 8-bit digits of the monotone uint32 image of the fp32 bits (sign-flipped; a NaN of
 * either sign orders above +inf; -0 below +0).  Pass 0 reads loss_px + labels and writes the keys (0 = not valid) to the
 * workspace; every pass counts the digit histogram of the keys that match the prefix found so far — 8 wave ballots of the digit
 * bits, lane j combines them into the counts of bins 4j..4j+3 in registers — and a one-block launch sums the blocks' rows and
 * picks the digit; the last launch writes labels_out and *info.  NO read-modify-write atomics, LDS included; the counts are
 * integers: the same bytes every run.  loss_px, labels, labels_out, workspace: 16-byte aligned (else LC2IS_ERR_SHAPE);
 * workspace >= lc2is_ohem_select_workspace_bytes(n) = 4 n + a fixed 0.5 MB of histogram rows (a pure host function; 0 for a
 * refused n).  loss_thresh >= 0, min_kept_total >= 0, C >= 1 (else LC2IS_ERR_SHAPE).  info: lc2is_ohem_info on the device.
 * replaces: the sort / topk of the samplers named above. */
size_t lc2is_ohem_select_workspace_bytes(long n);
int lc2is_ohem_select(const float* loss_px, const int64_t* labels, int64_t* labels_out, long n, int C, long ignore_index,
                      float loss_thresh, long min_kept_total, void* info, void* workspace, size_t workspace_bytes,
                      lc2is_stream_t stream);

/* ---- soft Dice + cross-entropy (a region loss beside the per-pixel ones) ----------------------------------------------
 * p_i = softmax of the class scores at pixel i; V = the counted pixels (label != ignore_index && 0 <= label < C, inside the
 * image: the rule of the CE head).  Per class over the whole batch of the call:
 *   I_c = sum_{i in V, y_i = c} p_ic,   P_c = sum_{i in V} p_ic,   T_c = #{i in V : y_i = c},   U_c = P_c + T_c + smooth,
 *   Dice = (1/C) sum_c m_c (1 - (2 I_c + smooth) / U_c),  m_c = [T_c > 0] if present_only else 1  (a class with U_c = 0 adds 0),
 *   loss = ce_weight * CE_mean + dice_weight * Dice,       CE_mean = the plain mean CE over V.
 * present_only != 0 is segmentation_models_pytorch's multiclass DiceLoss, present_only = 0 MONAI's DiceLoss(softmax, batch=True).
 * Gradient: dDice/dz_ic = p_ic (beta_c - alpha_y [c = y] - q_i), q_i = sum_k p_ik beta_k - alpha_y p_iy, alpha_c = 2 m_c / (C U_c),
 * beta_c = m_c (2 I_c + smooth) / (C U_c^2): it needs the batch sums, so every call is a statistics pass, a one-block launch
 * that sums the blocks' rows in a fixed order (fp64; T and the pixel count are integers) and writes a device coefficient block,
 * and (gradient) a second pass.  Nothing is read on the host; the chain captures into a graph.  NO read-modify-write atomics:
 * loss, statistics and gradient are the same bytes every run.
 * loss_out fp32 [4] = {loss, CE_mean, Dice, n_valid}; with no counted pixel all four and the gradient are 0 (nothing is NaN).
 * ce_weight, dice_weight, smooth: finite and >= 0, the two weights not both 0 (else LC2IS_ERR_SHAPE).
 * replaces: smp.losses.DiceLoss(mode="multiclass") / monai.losses.DiceLoss(softmax=True, batch=True) + nn.CrossEntropyLoss on
 *   the upsampled logits (mmseg's [CrossEntropyLoss, DiceLoss] decode-head recipes), plus their autograd.
 *
 * lc2is_head_upsample_ce_dice: on the fused head of lc2is_head_upsample_ce (scores_lo fp32 [B,h,w,ld] channels-last, the xS
 * upsample never materialised), S in {4, 8, 16} (else LC2IS_ERR_UNSUPPORTED), C <= ld <= 192, ld % 64 == 0.  dscores_lo (NULL:
 * forward only, two launches) receives grad_scale * d loss / d scores_lo — the gradient of the scalar loss, not of a sum; all ld
 * channels are overwritten.  class_stats: fp32 [3][ld] = I, P, T (zeros past C) or NULL.  workspace: 16-byte aligned,
 * >= lc2is_head_upsample_ce_dice_workspace_bytes(...) (a pure host function; 0 for a call that would be refused). */
size_t lc2is_head_upsample_ce_dice_workspace_bytes(int B, int h, int w, int C, int S, int mode, int want_grad);
int lc2is_head_upsample_ce_dice(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_out,
                                float* class_stats, int B, int h, int w, int C, int S, int mode, long ignore_index,
                                float ce_weight, float dice_weight, float smooth, int present_only, float grad_scale,
                                void* workspace, size_t workspace_bytes, lc2is_stream_t stream);

/* The same loss on materialised NCHW fp32 logits [B,C,HW] (the drop-in criterion), C <= 192 (else LC2IS_ERR_UNSUPPORTED).
 * _fwd: lse fp32 [B,HW] (or NULL), loss_out fp32 [4], class_stats fp32 [3][C] or NULL, and coef — fp32 [2 * cq + 4], cq = C rounded
 * up to 4: alpha[cq] * dice_weight, beta[cq] * dice_weight, ce_weight / n_valid — which the caller keeps for _bwd.
 * _bwd: dlogits = grad_scale * (*grad_scale_dev, NULL = 1) * d loss / d logits; every element is written.
 * replaces: the same criteria applied to model(inputs)["outputs"] (evaluate.py:68, engine.py:94,150), plus their autograd. */
size_t lc2is_ce_dice_nchw_workspace_bytes(int B, int C, long HW);
int lc2is_ce_dice_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_out, float* class_stats,
                           float* coef, int B, int C, long HW, long ignore_index, float ce_weight, float dice_weight,
                           float smooth, int present_only, void* workspace, size_t workspace_bytes, lc2is_stream_t stream);
int lc2is_ce_dice_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* coef,
                           const float* grad_scale_dev, float grad_scale, float* dlogits, int B, int C, long HW,
                           long ignore_index, lc2is_stream_t stream);

/* ---- class map and accuracy / IoU counts of the fused head at its own output size ------------------------------------------
 * lc2is_head_upsample_argmax: the forward product of lc2is_head_upsample_ce alone (scores_lo fp32 [B,h,w,ld] channels-last, 16-byte
 * aligned, C <= ld <= 192, ld % 64 == 0, S in {4, 8, 16}, else LC2IS_ERR_UNSUPPORTED), then the argmax over the C classes of every
 * output pixel in the accumulators: exact ties go to the lowest class (torch.argmax), a pixel whose scores are all -inf gets class
 * 0, and the class is clamped into [0, C) (a NaN score may pick any class).  The xS map is never materialised.
 *   pred   uint8 [B,H,W] or NULL: the class map, every pixel written.
 *   counts int32 [B][3][C] or NULL: per image {intersection, predicted, labelled}.  A pixel counts iff label != ignore_index &&
 *          0 <= label < C (the rule of the CE head, and mmseg's); a counted pixel adds to predicted[pred] and labelled[label], and
 *          to intersection[pred] when pred == label; any other pixel adds to none of the three.  Needs labels (int64 [B,H,W]) and
 *          a 16-byte aligned workspace >= lc2is_head_upsample_argmax_workspace_bytes(...) (a pure host function; 0 for a call that
 *          would be refused): B * tiles * 3 * cq int32 slabs, cq = C rounded up to 4, summed per image in a fixed order by a second
 *          launch.  Every element of counts is overwritten.
 * pred and counts both NULL, or counts without labels: LC2IS_ERR_NULL.  A pred-only call takes no workspace (and labels may be NULL).
 * NO read-modify-write atomics, LDS included; the same bytes every run; captures into a graph.
 * replaces: model(inputs)["outputs"].argmax(1) on the materialised [B,K,H,W] logits of a second forward, and mmseg's accuracy() /
 *   intersect_and_union() on it (decode.acc_seg, the running train mIoU). */
size_t lc2is_head_upsample_argmax_workspace_bytes(int B, int h, int w, int C, int S, int mode);
int lc2is_head_upsample_argmax(const float* scores_lo, int ld, const int64_t* labels, uint8_t* pred, int32_t* counts, int B, int h,
                               int w, int C, int S, int mode, long ignore_index, void* workspace, size_t workspace_bytes,
                               lc2is_stream_t stream);

/* ---- focal and poly-1 cross-entropy (the focusing per-pixel losses) ----------------------------------------------------------
 * For a counted pixel i (label != ignore_index && 0 <= label < C: the rule of the CE head) with label y, p = softmax of its class
 * scores, q = 1 - p_y, ce = -ln p_y and class weight w_y (class_weight: device fp32 [C], the per-class alpha, or NULL = ones):
 *   l_i      = w_y (q^gamma ce + poly_eps q)                                 gamma = 0, poly_eps = 0: the weighted CE
 *   dl_i/dz_j = w_y c (p_j - [j == y]),   c = q^gamma + gamma p_y q^(gamma-1) ce + poly_eps p_y
 * gamma in [0, inf), poly_eps in [-1, inf), both finite (else LC2IS_ERR_SHAPE).  q is formed from the other classes' exponentials,
 * not as 1 - p_y; q == 0 gives q^gamma = [gamma == 0] and a zero q^(gamma-1) ce term, p_y == 0 a finite ce: nothing is Inf or NaN.
 * loss_sum[0] = sum_i l_i, loss_sum[1] = sum_i w_y (the denominator of this project's mean, as lc2is_head_upsample_ce_opts; kornia
 * and MONAI divide by the number of pixels instead).
 * replaces: kornia.losses.FocalLoss / monai.losses.FocalLoss(use_softmax=True) / mmseg's FocalLoss on softmax logits, and PolyLoss's
 *   Poly1CrossEntropyLoss, composed from torch ops on model(inputs)["outputs"] (engine.py:94), plus their autograd.
 *
 * lc2is_head_upsample_focal: on the fused head of lc2is_head_upsample_ce (scores_lo fp32 [B,h,w,ld] channels-last, 16-byte aligned,
 * C <= ld <= 192, ld % 64 == 0, else LC2IS_ERR_SHAPE; S in {4, 8, 16} and a known mode, else LC2IS_ERR_UNSUPPORTED), one forward +
 * backward launch and the fixed-order finish launch.  dscores_lo (NULL: loss only) = grad_scale * U^T (sum_i dl_i/dz), all ld
 * channels overwritten.  workspace: 16-byte aligned, >= lc2is_head_upsample_ce_workspace_bytes(B, h, w, C, S, mode, dscores_lo !=
 * NULL) (else LC2IS_ERR_WORKSPACE).  Refusals in the order NULL, SHAPE, UNSUPPORTED, WORKSPACE.  NO read-modify-write atomics, LDS
 * included: the same bytes every run; captures into a graph. */
int lc2is_head_upsample_focal(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_sum, int B,
                              int h, int w, int C, int S, int mode, long ignore_index, float grad_scale,
                              const float* class_weight, float gamma, float poly_eps, void* workspace, size_t workspace_bytes,
                              lc2is_stream_t stream);
/* The same loss on materialised NCHW fp32 logits [B,C,HW] (the drop-in criterion).  _fwd: lse fp32 [B,HW] (or NULL), loss_sum[2]
 * overwritten through ordered block partials (workspace >= lc2is_ce_nchw_fwd_workspace_bytes(B, HW)), loss_px (optional, [B,HW]) =
 * l_i, 0 where not counted.  _bwd: dlogits = grad_scale * (*grad_scale_dev, NULL = 1) * grad_px[i] (NULL = 1) * dl_i/dlogits from
 * _fwd's lse; every element is written.
 * replaces: the same criteria on model(inputs)["outputs"] with reduction 'mean' / 'sum' / 'none', plus their autograd. */
int lc2is_focal_nchw_fwd(const float* logits, const int64_t* labels, float* lse, float* loss_sum, float* loss_px, int B, int C,
                         long HW, long ignore_index, const float* class_weight, float gamma, float poly_eps, void* workspace,
                         size_t workspace_bytes, lc2is_stream_t stream);
int lc2is_focal_nchw_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_scale_dev,
                         float grad_scale, const float* grad_px, float* dlogits, int B, int C, long HW, long ignore_index,
                         const float* class_weight, float gamma, float poly_eps, lc2is_stream_t stream);

/* ---- sigmoid cross-entropy and sigmoid focal loss (the per-class binary losses) ----------------------------------------------
 * For a counted pixel i (label != ignore_index && 0 <= label < C: the rule of the CE head) with label y and a class c < C, z = z_ic
 * the class score, t = [c == y], p = sigmoid(z), p_t = t ? p : 1 - p, class weight w_c (class_weight: device fp32 [C], the weight of
 * class c's binary term, or NULL = ones):
 *   bce       = softplus(z) - t z                                  ( = -ln p_t )
 *   l_ic      = w_c a_t (1 - p_t)^gamma bce,   a_t = alpha given ? (t ? alpha : 1 - alpha) : 1
 *   dl_ic/dz  = w_c a_t ( t ? (1-p)^gamma (gamma p ln p - (1-p)) : p^gamma (p - gamma (1-p) ln(1-p)) )
 *   l_i       = class_scale * sum_{c<C} l_ic
 * gamma in [0, inf) and finite; alpha <= 1, any negative value = no alpha, not a NaN; class_scale in (0, inf) and finite (else
 * LC2IS_ERR_SHAPE).  gamma = 0 without alpha is binary cross-entropy with logits on one-hot targets; gamma > 0 is RetinaNet's focal
 * loss elementwise.  ln p and ln(1 - p) are -softplus(-z) and -softplus(z), never the logarithm of a rounded p: z = +-1e4 gives
 * finite losses and gradients for every gamma; at gamma = 0 the modulating factor is not formed (no 0^0).  No softmax: the classes
 * of a pixel do not compete, and the gradient of a class depends on its own score alone.
 * loss_sum[0] = sum_i l_i, loss_sum[1] = the NUMBER of counted pixels, unweighted and exact: the mean of a binary loss divides by a
 * count of elements (torch's and mmseg's rule), not by a weight sum as this project's softmax cross-entropy does.  class_scale = 1 / C
 * makes loss_sum[0] / loss_sum[1] torch's elementwise mean over counted pixels x C; class_scale = 1 the per-pixel mean of the
 * class sums.
 * replaces: torch.nn.BCEWithLogitsLoss on one-hot targets / mmseg's CrossEntropyLoss(use_sigmoid=True), and
 *   torchvision.ops.sigmoid_focal_loss / mmseg's FocalLoss, composed from torch ops on model(inputs)["outputs"] (engine.py:94), plus
 *   their autograd.
 *
 * lc2is_head_upsample_sigmoid: on the fused head of lc2is_head_upsample_ce (scores_lo fp32 [B,h,w,ld] channels-last, 16-byte
 * aligned, C <= ld <= 192, ld % 64 == 0, else LC2IS_ERR_SHAPE; S in {4, 8, 16} and a known mode, else LC2IS_ERR_UNSUPPORTED), one
 * forward + backward launch and the fixed-order finish launch.  dscores_lo (NULL: loss only) = grad_scale * U^T (sum_i dl_i/dz), all
 * ld channels overwritten, exactly 0 at and past C.  workspace: 16-byte aligned, >= lc2is_head_upsample_ce_workspace_bytes(B, h, w,
 * C, S, mode, dscores_lo != NULL) (else LC2IS_ERR_WORKSPACE).  Refusals in the order NULL, SHAPE, UNSUPPORTED, WORKSPACE.  NO
 * read-modify-write atomics, LDS included: the same bytes every run; captures into a graph. */
int lc2is_head_upsample_sigmoid(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_sum, int B,
                                int h, int w, int C, int S, int mode, long ignore_index, float grad_scale,
                                const float* class_weight, float gamma, float alpha, float class_scale, void* workspace,
                                size_t workspace_bytes, lc2is_stream_t stream);
/* The same loss on materialised NCHW fp32 logits [B,C,HW] (the drop-in criteria).  _fwd: loss_sum[2] overwritten through ordered
 * block partials (workspace >= lc2is_ce_nchw_fwd_workspace_bytes(B, HW)), loss_px (optional, [B,HW]) = l_i, 0 where not counted.
 * _bwd: dlogits = grad_scale * (*grad_scale_dev, NULL = 1) * grad_px[i] (NULL = 1) * dl_i/dlogits; nothing saved by _fwd is needed
 * (no lse); every element is written.
 * replaces: the same criteria on model(inputs)["outputs"] with reduction 'mean' / 'sum' / 'none', plus their autograd. */
int lc2is_sigmoid_focal_nchw_fwd(const float* logits, const int64_t* labels, float* loss_sum, float* loss_px, int B, int C, long HW,
                                 long ignore_index, const float* class_weight, float gamma, float alpha, float class_scale,
                                 void* workspace, size_t workspace_bytes, lc2is_stream_t stream);
int lc2is_sigmoid_focal_nchw_bwd(const float* logits, const int64_t* labels, const float* grad_scale_dev, float grad_scale,
                                 const float* grad_px, float* dlogits, int B, int C, long HW, long ignore_index,
                                 const float* class_weight, float gamma, float alpha, float class_scale, lc2is_stream_t stream);

/* ---- the fused head past 192 classes: cross-entropy, class map and counts for C <= 1024 ------------------------------------
 * The entry points above keep every class of a pixel in registers and the whole footprint in LDS, and stop at 192 classes.  These
 * two walk the class axis in chunks of 192 channels (the tile plan, products and summation orders are lc2is_head_upsample_ce's):
 * 1 <= C <= ld <= LC2IS_HEAD_WIDE_CMAX, ld % 64 == 0 (ld need not be the smallest pad), scores_lo fp32 [B,h,w,ld] channels-last,
 * 16-byte aligned, else LC2IS_ERR_SHAPE; S == 4 and a known mode, else LC2IS_ERR_UNSUPPORTED.  C <= 192 is accepted (the narrow
 * entry points are the faster ones there).  The [B,C,H,W] map is never materialised.
 *
 * lc2is_head_upsample_ce_wide: lc2is_head_upsample_ce_opts with label_smoothing = 0.  Two sweeps over the chunks — an online
 * softmax (running maximum, rescaled sum, the label's logit), then the gradient with the logits formed again — and the fixed-order
 * finish launch.  loss_sum[0] = sum_i w_y (lse_i - z_iy), loss_sum[1] = sum_i w_y over the counted pixels (label != ignore_index &&
 * 0 <= label < C); class_weight: device fp32 [C] or NULL (all ones).  dscores_lo (NULL: loss only, one sweep) = grad_scale * U^T
 * (w_y (softmax - onehot)), all ld channels overwritten, exactly 0 at and past C.  workspace: 16-byte aligned, >=
 * lc2is_head_upsample_ce_wide_workspace_bytes(B, h, w, C, ld, S, mode, dscores_lo != NULL) = B * tiles * 2 floats rounded up to 256
 * bytes + (gradient wanted) B * tiles * f^2 * cq floats, tiles = ceil((4h + 2) / 16) * ceil((4w + 2) / 16), f = 7 bicubic / 5 bilinear,
 * cq = C rounded up to 4 (else LC2IS_ERR_WORKSPACE).
 * lc2is_head_upsample_argmax_wide: lc2is_head_upsample_argmax with pred int16 [B,H,W]; the running (value, class) of a pixel is
 * replaced only by a strictly larger value of a later chunk, so exact ties go to the lowest class.  counts int32 [B][3][C] needs
 * labels and a workspace >= lc2is_head_upsample_argmax_wide_workspace_bytes(...) = B * tiles * 3 * cq int32; a pred-only call takes
 * no workspace (and labels may be NULL).
 * Both: refusals in the order NULL, SHAPE, UNSUPPORTED, WORKSPACE, from the arguments alone, before any launch; the workspace queries
 * are pure host functions, 0 for a call that would be refused.  NO read-modify-write atomics, LDS included: the same bytes every
 * run; captures into a graph.
 * replaces: F.interpolate(scale_factor=4) + nn.CrossEntropyLoss(weight=) and .argmax(1) + intersect_and_union() on the [B,K,H,W]
 *   logits of an open-vocabulary class set (PC-459, ADE20K-full 847, ImageNet-S-919), plus their autograd. */
#define LC2IS_HEAD_WIDE_CMAX 1024
size_t lc2is_head_upsample_ce_wide_workspace_bytes(int B, int h, int w, int C, int ld, int S, int mode, int want_grad);
int lc2is_head_upsample_ce_wide(const float* scores_lo, int ld, const int64_t* labels, float* dscores_lo, float* loss_sum, int B,
                                int h, int w, int C, int S, int mode, long ignore_index, float grad_scale,
                                const float* class_weight, void* workspace, size_t workspace_bytes, lc2is_stream_t stream);
size_t lc2is_head_upsample_argmax_wide_workspace_bytes(int B, int h, int w, int C, int S, int mode);
int lc2is_head_upsample_argmax_wide(const float* scores_lo, int ld, const int64_t* labels, int16_t* pred, int32_t* counts, int B,
                                    int h, int w, int C, int S, int mode, long ignore_index, void* workspace,
                                    size_t workspace_bytes, lc2is_stream_t stream);

/* ---- distillation on the fused head: per-pixel KL(teacher || student) of two upsampled score maps ---------------------------
 * On the fused head of lc2is_head_upsample_ce: scores_lo (student) and teacher_lo fp32 [B,h,w,ld] channels-last with the same ld,
 * both 16-byte aligned, C <= ld <= 192, ld % 64 == 0, temperature T finite and > 0 (else LC2IS_ERR_SHAPE); S in {4, 8, 16} and a
 * known mode (else LC2IS_ERR_UNSUPPORTED).  Refusals in the order NULL, SHAPE, UNSUPPORTED, WORKSPACE, from the arguments alone,
 * before any launch.  Neither xS map is materialised.
 * Counted pixels: labels == NULL: every pixel of the image; else int64 [B,H,W] and the pixels with label != ignore_index &&
 * 0 <= label < C (the labelled region: crop padding stays out).  pixel_weight: fp32 [B,H,W], finite and >= 0 (documented, not
 * checked on the device), or NULL (ones).  Per counted pixel i, u = z / T over the C real channels, p = softmax(u):
 *   loss_i  = pw_i T^2 sum_c p_t,c (log p_t,c - log p_s,c),   count_i = 1  (NOT multiplied by pw_i)
 *   dz_s,c  = grad_scale pw_i T (p_s,c - p_t,c)               (the teacher gets no gradient)
 * loss_sum[0] = sum_i loss_i, loss_sum[1] = the number of counted pixels.  The loss is formed in the log domain and both softmaxes
 * by the same instructions: teacher_lo == scores_lo gives loss_sum[0] == 0.0 and dscores_lo == 0.0 exactly; a class with
 * p_t == 0 adds exactly 0; finite scores of +-1e4 give finite results.  -inf / NaN scores in the C real channels are unsupported
 * (not checked).  Channels at and past C of either map are never read into a result.
 * dscores_lo (NULL: loss only), all ld channels overwritten, exactly 0 at and past C.  loss_sum[2] overwritten.  workspace: 16-byte
 * aligned, >= lc2is_head_upsample_ce_workspace_bytes(B, h, w, C, S, mode, dscores_lo != NULL), overwritten.  One forward + backward
 * launch and the fixed-order finish launch of lc2is_head_upsample_ce: NO read-modify-write atomics, LDS included, the same bytes
 * every run; captures into a graph.
 * replaces: T*T * F.kl_div(F.log_softmax(student_logits / T, 1), F.softmax(teacher_logits / T, 1), reduction='none').sum(1) on two
 *   materialised [B,K,H,W] logit maps (Hinton's KD per pixel: mmrazor's KLDivergence, structured KD's pixel-wise term; the soft
 *   consistency of mean teacher / FixMatch / UniMatch), times pixel_weight, plus autograd through the student's softmax. */
int lc2is_head_upsample_kd(const float* scores_lo, const float* teacher_lo, int ld, const int64_t* labels /*NULL ok*/,
                           const float* pixel_weight /*NULL ok*/, float* dscores_lo /*NULL: loss only*/, float* loss_sum,
                           int B, int h, int w, int C, int S, int mode, long ignore_index, float temperature, float grad_scale,
                           void* workspace, size_t workspace_bytes, lc2is_stream_t stream);

/* ---- self-training on the fused head: class map + confidence + pseudo-labels, and cross-entropy with a per-pixel weight ------
 * Both on the fused head of lc2is_head_upsample_ce: scores_lo fp32 [B,h,w,ld] channels-last, 16-byte aligned, C <= ld <= 192,
 * ld % 64 == 0 (else LC2IS_ERR_SHAPE); S in {4, 8, 16} and a known mode (else LC2IS_ERR_UNSUPPORTED).  Refusals in the order NULL,
 * SHAPE, UNSUPPORTED, WORKSPACE, from the arguments alone, before any launch.  The xS map is never materialised.  NO
 * read-modify-write atomics, LDS included: the same bytes every run; both capture into a graph.
 *
 * lc2is_head_upsample_conf: forward only.  Per output pixel the class of lc2is_head_upsample_argmax (the same bytes: ties to the
 * lowest class, the index clamped into [0, C)) and its softmax probability conf = 1 / sum_c exp(z_c - max), formed as the winner's
 * own exponential over the sum so that a pixel with one dominant class gives exactly 1.  A pixel whose sum is not a number (all
 * scores -inf, a NaN or a +inf score) gets conf = 1 / C: conf is always finite and in (0, 1].  Each output is optional (NULL = not
 * written):
 *   pred   uint8 [B,H,W]: the class map.
 *   conf   fp32  [B,H,W]: the confidence.
 *   pseudo int64 [B,H,W]: the class where conf >= thresh, else ignore_index.
 *   counts int32 [B][2]:  per image {pixels with conf >= thresh, pixels inside the image = H W}.  Needs a 16-byte aligned workspace
 *          >= lc2is_head_upsample_conf_workspace_bytes(...) (a pure host function; 0 for a call that would be refused): B * tiles * 2
 *          int32, summed per image in a fixed order by a second launch.
 * thresh must be in [0, 1] and not a NaN (else LC2IS_ERR_SHAPE); all four outputs NULL: LC2IS_ERR_NULL.  Every pixel of a given
 * output is written.
 * replaces: model(inputs)["outputs"].softmax(1).max(1) on the materialised [B,K,H,W] logits of the teacher's forward, the
 *   thresholding `where(conf >= t, pred, ignore_index)` and the per-image share of confident pixels (FixMatch, ST++, DAFormer).
 *
 * lc2is_head_upsample_ce_pw: lc2is_head_upsample_ce_opts with pixel_weight fp32 [B,H,W] (finite and >= 0: documented, not checked on
 * the device).  Per counted pixel i (label != ignore_index && 0 <= label < C), a1 = 1 - eps, ac = eps / C, W = sum_c w_c:
 *   loss_i  = pw_i [ a1 w_y (lse - z_y) + ac (W lse - sum_c w_c z_c) ],   count_i = w_y  (NOT multiplied by pw_i)
 *   dz_k    = grad_scale pw_i [ (a1 w_y + ac W) p_k - a1 w_y [k == y] - ac w_k ]
 * loss_sum[0] = sum_i loss_i, loss_sum[1] = sum_i w_y: the denominator of the mean stays that of lc2is_head_upsample_ce_opts, so
 * pixel_weight == 1 is that loss and a per-image weight scales the image's loss instead of cancelling (mmseg's
 * weight_reduce_loss).  class_weight: device fp32 [C] or NULL (ones); label_smoothing in [0, 1].  dscores_lo (NULL: loss only), all
 * ld channels overwritten, exactly 0 at and past C.  workspace: 16-byte aligned, >= lc2is_head_upsample_ce_workspace_bytes(B, h, w,
 * C, S, mode, dscores_lo != NULL).  One forward + backward launch and the fixed-order finish launch of lc2is_head_upsample_ce.
 * replaces: (F.cross_entropy(model(inputs)["outputs"], labels, weight, reduction='none', label_smoothing) * pixel_weight).sum() /
 *   sum_i w_y on the materialised logits (DAFormer's pseudo-label weight, confidence weighting, U-Net's boundary-weight maps), plus
 *   its autograd. */
size_t lc2is_head_upsample_conf_workspace_bytes(int B, int h, int w, int C, int S, int mode);
int lc2is_head_upsample_conf(const float* scores_lo, int ld, uint8_t* pred, float* conf, int64_t* pseudo, int32_t* counts, int B,
                             int h, int w, int C, int S, int mode, float thresh, long ignore_index, void* workspace,
                             size_t workspace_bytes, lc2is_stream_t stream);
int lc2is_head_upsample_ce_pw(const float* scores_lo, int ld, const int64_t* labels, const float* pixel_weight, float* dscores_lo,
                              float* loss_sum, int B, int h, int w, int C, int S, int mode, long ignore_index, float grad_scale,
                              const float* class_weight, float label_smoothing, void* workspace, size_t workspace_bytes,
                              lc2is_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LC2IS_HIP_H */
