"""The NT GEMM dispatch seen from the host (no GPU): which kernels lc2is_gemm_nt_bf16 launches over which rows.

Every NT kernel accumulates in the same K order, so all plans give bitwise the same output and a dispatch regression is a pure
slowdown that no output check can see.  ``ops.gemm_nt_plan`` returns the plan without launching; the table below pins it for the
shapes the step and the GPU tests run.  The expected records were RECORDED from the dispatch as it stood before the planner was
split out of the launcher (its launches intercepted, the same arguments), not derived by hand."""
import ctypes

import pytest

from lc2is_amd import ops


@pytest.fixture(scope="module", autouse=True)
def _library():
    from lc2is_amd import _lib
    if not _lib.lib_path().exists():
        import __graft_entry__ as ge
        ge.build()
    yield
    ops.set_cu_budget(0)


# (M, N, K, arguments of ops.gemm_nt_plan, CU budget, [(cfg, row0, rows, tail_rows, staged_epi), ...] or the error code)
PLANS = [
    # the eight GEMMs of a ViT-B/16 layer (tools/gemm_shapes.py) at B = 32 and B = 16 images of 1025 tokens
    (32800, 2304, 768, dict(), 0, [(16, 0, 32768, 32, 1)]),   # qkv
    (32800, 768, 768, dict(out_bf16=False, out_f32=True, resid=True), 0, [(16, 0, 32768, 32, 2)]),   # out_proj
    (32800, 3072, 768, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 0, [(15, 0, 32768, 32, 1)]),   # fc1
    (32800, 768, 3072, dict(out_bf16=False, out_f32=True, resid=True), 0, [(16, 0, 32768, 32, 2)]),   # fc2
    (32800, 3072, 768, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 0, [(15, 0, 32768, 0, 1), (17, 32768, 32, 0, 1)]),   # dfc2
    (32800, 768, 3072, dict(out_bf16=False, out_f32=True), 0, [(16, 0, 32768, 32, 2)]),   # dfc1
    (32800, 768, 768, dict(), 0, [(16, 0, 32768, 32, 1)]),   # dout_proj
    (32800, 768, 2304, dict(out_bf16=False, out_f32=True), 0, [(16, 0, 32768, 32, 2)]),   # dqkv
    (16416, 2304, 768, dict(), 0, [(15, 0, 16416, 0, 1)]),   # qkv
    (16416, 768, 768, dict(out_bf16=False, out_f32=True, resid=True), 0, [(6, 0, 16416, 0, 2)]),   # out_proj
    (16416, 3072, 768, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 0, [(15, 0, 16384, 32, 1)]),   # fc1
    (16416, 768, 3072, dict(out_bf16=False, out_f32=True, resid=True), 0, [(6, 0, 16416, 0, 2)]),   # fc2
    (16416, 3072, 768, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 0, [(15, 0, 16384, 0, 1), (17, 16384, 32, 0, 1)]),   # dfc2
    (16416, 768, 3072, dict(out_bf16=False, out_f32=True), 0, [(6, 0, 16416, 0, 2)]),   # dfc1
    (16416, 768, 768, dict(), 0, [(6, 0, 16416, 0, 1)]),   # dout_proj
    (16416, 768, 2304, dict(out_bf16=False, out_f32=True), 0, [(6, 0, 16416, 0, 2)]),   # dqkv
    # test_gemm_nt_auto_plan_picks_exact_round_and_matches: rows 2 and 7 above
    # test_gemm_nt_auto_plan_persistent_with_folded_tail
    (16416, 3072, 128, dict(), 0, [(15, 0, 16384, 32, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 0, [(15, 0, 16384, 32, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 0, [(15, 0, 16384, 0, 1), (17, 16384, 32, 0, 1)]),
    (16416, 3072, 768, dict(), 0, [(15, 0, 16384, 32, 1)]),
    (16416, 2304, 192, dict(), 0, [(15, 0, 16416, 0, 1)]),
    (16416, 2304, 192, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 0, [(15, 0, 16416, 0, 1)]),
    (16416, 2304, 192, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 0, [(15, 0, 16416, 0, 1)]),
    # test_gemm_nt_auto_plan_ragged_rows (forward with the saved derivative, backward through it)
    (16416, 3072, 128, dict(act=ops.ACT_QUICK_GELU_GRAD, resid=True, out_f32=True, aux_out=True), 0, [(4, 0, 16416, 0, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_MUL_AUX, aux_in=True), 0, [(4, 0, 16416, 0, 1)]),
    (16416, 768, 192, dict(act=ops.ACT_QUICK_GELU_GRAD, resid=True, out_f32=True, aux_out=True), 0, [(6, 0, 16416, 0, 1)]),
    (16416, 768, 192, dict(act=ops.ACT_MUL_AUX, aux_in=True), 0, [(6, 0, 16416, 0, 1)]),
    (16416, 2304, 128, dict(act=ops.ACT_QUICK_GELU_GRAD, resid=True, out_f32=True, aux_out=True), 0, [(4, 0, 16416, 0, 1)]),
    (16416, 2304, 128, dict(act=ops.ACT_MUL_AUX, aux_in=True), 0, [(4, 0, 16416, 0, 1)]),
    # test_cu_budget_changes_plans_not_results
    (32800, 768, 256, dict(out_bf16=False, out_f32=True, resid=True), 0, [(4, 0, 32800, 0, 2)]),
    (32800, 768, 256, dict(), 0, [(16, 0, 32768, 32, 1)]),
    (32800, 3072, 256, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 0, [(15, 0, 32768, 32, 1)]),
    # test_gemm_nt_auto_plan_separate_f32_tail: at K = 64 the extra launch costs more than the round it saves, from K = 256 on the
    # tail is its own launch (the only default plan whose tail launch carries resid and out_f32)
    (16416, 1024, 64, dict(out_bf16=False, out_f32=True, resid=True), 0, [(4, 0, 16416, 0, 2)]),
    (16416, 1024, 256, dict(out_bf16=False, out_f32=True, resid=True), 0, [(4, 0, 16384, 0, 2), (17, 16384, 32, 0, 2)]),
    # every operand and output at once, padded leading dimension
    (16416, 1024, 768, dict(act=ops.ACT_ADD_AUX, resid=True, aux_in=True, out_f32=True, aux_out=True, ld=1032), 0,
     [(4, 0, 16384, 0, 1), (17, 16384, 32, 0, 1)]),
    # the small families, the family border, the unstaged epilogue, no peel past 64 ragged rows, activations off the persistent list
    (515, 384, 192, dict(), 0, [(3, 0, 515, 0, 1)]),
    (4100, 2304, 768, dict(), 0, [(6, 0, 4100, 0, 1)]),
    (1025, 768, 768, dict(), 0, [(3, 0, 1025, 0, 1)]),
    (16208, 1024, 768, dict(), 0, [(4, 0, 16208, 0, 1)]),
    (32800, 3072, 768, dict(ld=3076), 0, [(4, 0, 32768, 0, 0), (17, 32768, 32, 0, 0)]),
    (32800, 768, 768, dict(out_bf16=False, out_f32=True, resid=True, ld=772), 0, [(16, 0, 32768, 32, 2)]),
    (32833, 3072, 768, dict(), 0, [(15, 0, 32833, 0, 1)]),
    (32800, 1024, 768, dict(act=ops.ACT_RELU), 0, [(15, 0, 32768, 32, 1)]),
    (32800, 1024, 768, dict(act=ops.ACT_GELU_ERF), 0, [(4, 0, 32768, 0, 1), (17, 32768, 32, 0, 1)]),
    # a forced tile_cfg is one record over all rows, or refused where that kernel does not take the problem
    (32800, 768, 768, dict(tile_cfg=4), 0, [(4, 0, 32800, 0, 1)]),
    (32800, 768, 768, dict(tile_cfg=16), 0, [(16, 0, 32800, 0, 1)]),
    (32800, 3072, 768, dict(tile_cfg=15), 0, [(15, 0, 32800, 0, 1)]),
    (33, 768, 768, dict(tile_cfg=17), 0, [(17, 0, 33, 0, 1)]),
    (300, 192, 128, dict(tile_cfg=2), 0, [(2, 0, 300, 0, 1)]),
    (32800, 1024, 768, dict(tile_cfg=16), 0, -3),
    (65, 768, 768, dict(tile_cfg=17), 0, -3),
    (32800, 3072, 768, dict(tile_cfg=15, out_f32=True), 0, -3),
    (1025, 768, 768, dict(tile_cfg=13), 0, -3),
    # the same shapes with 224 CUs to count on: no round is exact any more, nothing is peeled
    (32800, 2304, 768, dict(), 224, [(15, 0, 32800, 0, 1)]),
    (32800, 768, 768, dict(out_bf16=False, out_f32=True, resid=True), 224, [(4, 0, 32800, 0, 2)]),
    (32800, 3072, 768, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 224, [(15, 0, 32800, 0, 1)]),
    (32800, 768, 3072, dict(out_bf16=False, out_f32=True, resid=True), 224, [(4, 0, 32800, 0, 2)]),
    (32800, 3072, 768, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 224, [(15, 0, 32800, 0, 1)]),
    (32800, 768, 3072, dict(out_bf16=False, out_f32=True), 224, [(4, 0, 32800, 0, 2)]),
    (32800, 768, 768, dict(), 224, [(15, 0, 32800, 0, 1)]),
    (32800, 768, 2304, dict(out_bf16=False, out_f32=True), 224, [(4, 0, 32800, 0, 2)]),
    (16416, 2304, 768, dict(), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 768, 768, dict(out_bf16=False, out_f32=True, resid=True), 224, [(6, 0, 16416, 0, 2)]),
    (16416, 3072, 768, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 768, 3072, dict(out_bf16=False, out_f32=True, resid=True), 224, [(6, 0, 16416, 0, 2)]),
    (16416, 3072, 768, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 768, 3072, dict(out_bf16=False, out_f32=True), 224, [(6, 0, 16416, 0, 2)]),
    (16416, 768, 768, dict(), 224, [(6, 0, 16416, 0, 1)]),
    (16416, 768, 2304, dict(out_bf16=False, out_f32=True), 224, [(6, 0, 16416, 0, 2)]),
    (16416, 3072, 128, dict(), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 3072, 768, dict(), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 2304, 192, dict(), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 2304, 192, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 2304, 192, dict(act=ops.ACT_DQUICK_GELU, aux_in=True), 224, [(15, 0, 16416, 0, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_QUICK_GELU_GRAD, resid=True, out_f32=True, aux_out=True), 224, [(4, 0, 16416, 0, 1)]),
    (16416, 3072, 128, dict(act=ops.ACT_MUL_AUX, aux_in=True), 224, [(4, 0, 16416, 0, 1)]),
    (16416, 768, 192, dict(act=ops.ACT_QUICK_GELU_GRAD, resid=True, out_f32=True, aux_out=True), 224, [(6, 0, 16416, 0, 1)]),
    (16416, 768, 192, dict(act=ops.ACT_MUL_AUX, aux_in=True), 224, [(6, 0, 16416, 0, 1)]),
    (16416, 2304, 128, dict(act=ops.ACT_QUICK_GELU_GRAD, resid=True, out_f32=True, aux_out=True), 224, [(4, 0, 16416, 0, 1)]),
    (16416, 2304, 128, dict(act=ops.ACT_MUL_AUX, aux_in=True), 224, [(4, 0, 16416, 0, 1)]),
    (32800, 768, 256, dict(out_bf16=False, out_f32=True, resid=True), 224, [(4, 0, 32800, 0, 2)]),
    (32800, 768, 256, dict(), 224, [(15, 0, 32800, 0, 1)]),
    (32800, 3072, 256, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 224, [(15, 0, 32800, 0, 1)]),
    (16416, 1024, 64, dict(out_bf16=False, out_f32=True, resid=True), 224, [(4, 0, 16416, 0, 2)]),
    (16416, 1024, 256, dict(out_bf16=False, out_f32=True, resid=True), 224, [(4, 0, 16416, 0, 2)]),
    (16416, 1024, 768, dict(act=ops.ACT_ADD_AUX, resid=True, aux_in=True, out_f32=True, aux_out=True, ld=1032), 224,
     [(4, 0, 16416, 0, 1)]),
    # the other budgets test_cu_budget_changes_plans_not_results sets
    (32800, 768, 256, dict(out_bf16=False, out_f32=True, resid=True), 200, [(4, 0, 32800, 0, 2)]),
    (32800, 768, 256, dict(), 200, [(15, 0, 32800, 0, 1)]),
    (32800, 3072, 256, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 200, [(15, 0, 32800, 0, 1)]),
    (32800, 768, 256, dict(out_bf16=False, out_f32=True, resid=True), 240, [(4, 0, 32800, 0, 2)]),
    (32800, 768, 256, dict(), 240, [(15, 0, 32800, 0, 1)]),
    (32800, 3072, 256, dict(act=ops.ACT_QUICK_GELU, aux_out=True), 240, [(15, 0, 32800, 0, 1)]),
]


def _plan(M, N, K, kw, budget):
    ops.set_cu_budget(budget)
    try:
        return ops.gemm_nt_plan(M, N, K, **kw)
    finally:
        ops.set_cu_budget(0)


def test_default_plans_are_the_recorded_ones():
    wrong = []
    for M, N, K, kw, budget, want in PLANS:
        if isinstance(want, int):
            with pytest.raises(RuntimeError, match=f"rc={want}"):
                _plan(M, N, K, kw, budget)
            continue
        got = [r[:5] for r in _plan(M, N, K, kw, budget)]
        if got != want:
            wrong.append((M, N, K, kw, budget, want, got))
    assert not wrong, wrong


def test_records_tile_the_rows_once_and_move_every_operand():
    """The records of a plan cover [0, M) exactly once (tail_rows follow their launch's rows), and the pointers of each launch —
    as the executor's rows_from() makes them — lie row0 rows of their OWN leading dimension past the caller's: no operand or
    output of a tail launch stays at row 0, whichever of them the problem has."""
    two = 0
    for M, N, K, kw, budget, want in PLANS:
        if isinstance(want, int):
            continue
        ld = kw.get("ld", N)
        has = dict(resid=False, aux_in=False, out_bf16=True, out_f32=False, aux_out=False)
        has.update({k: v for k, v in kw.items() if k in has})
        row_bytes = (K * 2, has["resid"] * ld * 4, has["aux_in"] * ld * 2, has["out_bf16"] * ld * 2, has["out_f32"] * ld * 4,
                     has["aux_out"] * ld * 2)       # a, resid, aux_in, out_bf16, out_f32, aux_out
        at = 0
        recs = _plan(M, N, K, kw, budget)
        for cfg, row0, rows, tail_rows, staged, offsets in recs:
            assert row0 == at and rows > 0 and tail_rows >= 0, (M, N, K, kw, recs)
            assert offsets == tuple(row0 * b for b in row_bytes), (M, N, K, kw, recs)
            at = row0 + rows + tail_rows
        assert at == M, (M, N, K, kw, recs)
        two += len(recs) == 2
    assert two >= 5          # (the table holds separate tail launches to check)
    every = _plan(16416, 1024, 768, dict(act=ops.ACT_ADD_AUX, resid=True, aux_in=True, out_f32=True, aux_out=True, ld=1032), 0)
    assert every[1][:2] == (17, 16384) and all(off > 0 for off in every[1][5])


# ---- refusals: each entry point's checks in its order; a case breaks the named check AND a later one, the earlier code wins ----
_A = 1 << 40    # never dereferenced
NT_OK = dict(A=_A, lda=64, W=_A, ldw=64, bias=None, resid=None, ldr=0, aux_in=None, ldx=0, out_bf16=_A, ldo=64, out_f32=None, ldf=0,
             aux_out=None, ldy=0, M=8, N=64, K=64, act=0, tile_cfg=0)
NT_REFUSALS = [
    (dict(A=None, M=0), -2),                                   # operand NULL, before the shape
    (dict(out_bf16=None, K=63), -2),                           # no output
    (dict(M=0, act=3), -1),                                    # empty shape, before the missing aux_in
    (dict(K=96, act=3), -1), (dict(N=66, ldo=68, act=3), -1),  # K % 64, N % 4
    (dict(lda=32, act=3), -1), (dict(ldw=68, act=3), -1),      # operand rows shorter than K / off 16 bytes
    (dict(ldo=60, act=3), -1), (dict(out_f32=_A, ldf=66, act=11), -1), (dict(resid=_A, ldr=32, act=3), -1),
    (dict(act=3, M=4000000, K=768, lda=768, ldw=768), -2),     # the derivative needs aux_in: before the 2 GiB limit
    (dict(act=9), -2), (dict(act=6), -2), (dict(act=8), -2), (dict(act=4), -2),
    (dict(act=10, M=4000000, K=768, lda=768, ldw=768), -3), (dict(act=-1), -3),
    (dict(M=4000000, K=768, lda=768, ldw=768), -3),            # operand panel past 2 GiB
    (dict(tile_cfg=16), -3), (dict(tile_cfg=17, M=65), -3), (dict(tile_cfg=15, out_f32=_A, ldf=64), -3), (dict(tile_cfg=5), -3),
]
LN_OK = dict(A=_A, lda=64, W=_A, ldw=64, bias=None, resid=None, ldr=0, out_f32=_A, ldf=768, gamma=_A, beta=None, eps=1e-5, ln_out=_A,
             ldl=768, mean=None, rstd=None, xchg=_A, xchg_bytes=512 * 32, M=512, N=768, K=64)
LN_REFUSALS = [
    (dict(gamma=None, M=0), -2), (dict(ln_out=None, K=63), -2), (dict(A=None), -2),
    (dict(M=0, N=512), -1), (dict(K=96, N=512), -1), (dict(lda=32, N=512), -1), (dict(ldw=68, M=100), -1),
    (dict(ldl=772, N=384), -1), (dict(ldf=764, M=100), -1), (dict(resid=_A, ldr=766, M=100), -1),
    (dict(N=512, ldf=512, ldl=512, xchg=None), -3), (dict(M=255, xchg=None), -3),
    (dict(M=3000000, xchg=None), -3), (dict(M=3000000, K=768, lda=768, ldw=768, ldf=8, xchg=None), -1),
    (dict(xchg=None, M=612), -4), (dict(xchg_bytes=512 * 32 - 1), -4), (dict(xchg=_A + 4), -4),   # workspace before the ragged-row limit
    (dict(M=612, xchg_bytes=612 * 32), -3),
]
BATCHED_OK = dict(A=_A, lda=64, stride_a=64 * 8, W=_A, ldw=64, stride_w=64 * 64, out_bf16=None, ldo=0, stride_ob=0, out_f32=_A, ldf=64,
                  stride_of=64 * 8, M=8, N=64, K=64, batch=2)
BATCHED_REFUSALS = [
    (dict(W=None, batch=0), -2), (dict(out_f32=None, K=63), -2),
    (dict(batch=0, M=4000000), -1), (dict(batch=65536), -1), (dict(K=96), -1), (dict(N=66), -1), (dict(lda=32), -1),
    (dict(stride_a=4, M=4000000, K=768, lda=768, ldw=768), -1), (dict(stride_w=12), -1), (dict(ldf=60), -1), (dict(stride_of=2), -1),
    (dict(out_bf16=_A, ldo=64, stride_ob=6, M=4000000, K=768, lda=768, ldw=768), -1),
    (dict(M=4000000, K=768, lda=768, ldw=768), -3),
]


@pytest.mark.parametrize("entry,ok,refusals", [
    ("lc2is_gemm_nt_bf16", NT_OK, NT_REFUSALS), ("lc2is_gemm_nt_plan", NT_OK, NT_REFUSALS),
    ("lc2is_gemm_nt_ln_bf16", LN_OK, LN_REFUSALS), ("lc2is_gemm_nt_bf16_batched", BATCHED_OK, BATCHED_REFUSALS)])
def test_entry_points_refuse_in_order_before_any_gpu_call(entry, ok, refusals):
    f = ops._fn(entry)
    recs = (ops._GemmNtLaunch * 2)()
    last = (ctypes.addressof(recs), 2) if entry.endswith("_plan") else (None,)      # (records, cap) / the stream
    got = [(change, f(*{**ok, **change}.values(), *last)) for change, _ in refusals]
    assert got == [(change, rc) for change, rc in refusals]
    codes = {rc for _, rc in refusals}
    assert codes == ({-1, -2, -3, -4} if "_ln_" in entry else {-1, -2, -3})
    if entry.endswith("_plan"):
        assert f(*ok.values(), *last) == 1          # the unchanged arguments are a valid problem


def test_size_queries_return_size_t():
    """lc2is_gemm_nt_ln_xchg_bytes is a size_t query like the *_workspace_bytes ones: 32 bytes per row do not fit an int from
    M = 2^26 rows on."""
    f = ops._fn("lc2is_gemm_nt_ln_xchg_bytes")
    assert f.restype is ctypes.c_size_t
    assert f(200_000_000, 768) == 6_400_000_000 and f(512, 384) == 0
