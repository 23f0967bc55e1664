"""The C launchers of the dense hot path refuse a misaligned BASE pointer (the rule of include/lc2is_hip.h) with LC2IS_ERR_SHAPE,
next to their ``ld %`` checks and before any HIP call.

Every launcher is called with well-shaped arguments and fake pointers (``1 << 40``): one operand at a time is moved off its
alignment and the call must return -1.  That the arguments are otherwise well shaped is shown by the same call with aligned
pointers and ONE later refusal provoked (an unknown activation, p = 2, a missing workspace, an unsupported N): it returns that
later code, so every shape test before it passed.  ``lc2is_gemm_nt_plan`` reports the same refusals and succeeds when aligned.

Runs where there is NO GPU only: should a regression ever let a fake pointer through, it must not become a launch on a real device."""
import ctypes as C

import pytest
import torch

P = 1 << 40
SHAPE, UNSUPPORTED, WORKSPACE = -1, -3, -4

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: only where nothing can be launched")


def _offsets(align, elem):
    """Byte offsets (of +2, +4, +8: whole elements) that leave a pointer below ``align``."""
    return [o for o in (2, 4, 8) if o % elem == 0 and o % align]


def _sweep(fn, args, ptrs, later):
    """args: the aligned call; ptrs: {argument index: (alignment the rule asks, element bytes)}; later: the code the aligned call
    returns (a refusal that comes after every shape test).  Moves one pointer at a time."""
    assert fn(*args) == later, "the aligned call must pass every shape test"
    for i, (align, elem) in ptrs.items():
        offs = _offsets(align, elem)
        assert offs, (i, align, elem)
        for o in offs:
            bad = list(args)
            bad[i] = args[i] + o
            assert fn(*bad) == SHAPE, (i, o)
        for o in (2, 4, 8):
            if o % elem == 0 and o % align == 0:      # e.g. +8 on bf16 rows whose ld is only a multiple of 4: still within the rule
                ok = list(args)
                ok[i] = args[i] + o
                assert fn(*ok) == later, (i, o)


def test_gemm_nt_launcher_and_plan_query():
    from lc2is_amd import ops
    M, N, K = 300, 192, 128
    #       A  lda W  ldw bias resid ldr aux_in ldx out_bf16 ldo out_f32 ldf aux_out ldy
    base = [P, K, P, K, P, P, N, P, N, P, N, P, N, P, N, M, N, K]
    ptrs = {0: (16, 2), 2: (16, 2), 4: (16, 4), 5: (16, 4), 7: (16, 2), 9: (16, 2), 11: (16, 4), 13: (16, 2)}
    _sweep(ops._fn("lc2is_gemm_nt_bf16"), base + [99, 0, None], ptrs, UNSUPPORTED)                       # act = 99
    recs = (ops._GemmNtLaunch * 2)()
    plan = ops._fn("lc2is_gemm_nt_plan")
    _sweep(plan, base + [99, 0, recs, 2], ptrs, UNSUPPORTED)
    assert plan(*base, ops.ACT_MUL_AUX, 0, recs, 2) >= 1                                                  # aligned: the plan
    # bf16 rows whose ld is only a multiple of 4 (the unstaged epilogue): an 8-byte base is enough, 2 and 4 bytes are not
    ld4 = list(base)
    ld4[8] = ld4[10] = ld4[14] = N + 4
    _sweep(plan, ld4 + [99, 0, recs, 2], {7: (8, 2), 9: (8, 2), 13: (8, 2)}, UNSUPPORTED)
    assert plan(*(ld4[:9] + [P + 8] + ld4[10:]), ops.ACT_MUL_AUX, 0, recs, 2) >= 1


def test_gemm_nt_ln_and_batched_launchers():
    from lc2is_amd import ops
    M, N, K = 512, 512, 128           # N = 512: LC2IS_ERR_UNSUPPORTED after the shape tests
    #       A  lda W  ldw bias resid ldr out_f32 ldf gamma beta eps ln_out ldl mean rstd xchg bytes
    args = [P, K, P, K, P, P, N, P, N, P, P, 1e-5, P, N, P, P, P, 1 << 20, M, N, K, None]
    _sweep(ops._fn("lc2is_gemm_nt_ln_bf16"), args, {0: (16, 2), 2: (16, 2), 4: (16, 4), 5: (16, 4), 7: (16, 4), 9: (16, 4), 10: (16, 4),
                                                    12: (16, 2)}, UNSUPPORTED)
    # batched: an A panel past 2 GiB is LC2IS_ERR_UNSUPPORTED after the shape tests
    lda = 1 << 20
    #       A  lda stride_a  W  ldw stride_w out_bf16 ldo stride_ob out_f32 ldf stride_of M  N   K   batch
    args = [P, lda, 1024 * lda, P, 64, 64 * 64, P, 64, 1024 * 64, P, 64, 1024 * 64, 1024, 64, 64, 2, None]
    _sweep(ops._fn("lc2is_gemm_nt_bf16_batched"), args, {0: (16, 2), 3: (16, 2), 6: (16, 2), 9: (16, 4)}, UNSUPPORTED)
    args[7] = 68                      # ldo = 4 (mod 8)
    _sweep(ops._fn("lc2is_gemm_nt_bf16_batched"), args, {6: (8, 2)}, UNSUPPORTED)


def test_gemm_tn_colsum_launchers():
    from lc2is_amd import ops
    M, N, K = 1025, 768, 768          # several M-splits: needs a workspace -> LC2IS_ERR_WORKSPACE after the shape tests
    assert ops._fn("lc2is_gemm_tn_workspace_bytes")(M, N, K) > 0
    #       dY ldy X  ldx dW ldw db
    args = [P, N, P, K, P, K, P, M, N, K, 0, None, 0, None]
    _sweep(ops._fn("lc2is_gemm_tn_bf16"), args, {0: (16, 2), 2: (16, 2), 4: (16, 4)}, WORKSPACE)
    args = [P, N, P, 100, 64, 0, None, 0, None]
    _sweep(ops._fn("lc2is_colsum_bf16"), args, {0: (16, 2)}, WORKSPACE)
    # grouped: the plan query runs the launcher's own operand tests (0 = well formed), the launcher itself stops at its workspace
    summary, recs = ops._TnGroupPlan(), (ops._TnGroupRec * 2)()
    plan, launch = ops._fn("lc2is_gemm_tn_grouped_plan"), ops._fn("lc2is_gemm_tn_grouped")
    fields = {"dY": (16, 2), "X": (16, 2), "dW": (16, 4)}

    def problems(**moved):
        arr = (ops.TnProblem * 2)()
        for i in range(2):
            arr[i] = ops.TnProblem(P, P, P, P, N, K, K, M, N, K, 0)
        for f, o in moved.items():
            setattr(arr[1], f, P + o)
        return arr
    assert plan(problems(), 2, C.addressof(summary), recs, 2) == 0 and summary.workspace_bytes > 0
    assert launch(problems(), 2, None, 0, None) == WORKSPACE
    for f, (align, elem) in fields.items():
        for o in _offsets(align, elem):
            assert plan(problems(**{f: o}), 2, C.addressof(summary), recs, 2) == SHAPE, (f, o)
            assert launch(problems(**{f: o}), 2, None, 0, None) == SHAPE, (f, o)


def test_layernorm_launchers():
    from lc2is_amd import ops
    M, Cc = 100, 192
    bwd = ops._fn("lc2is_layernorm_bwd")
    for x_bf16, ld in ((0, Cc), (1, Cc), (1, Cc + 4)):
        xa = (16, 4) if not x_bf16 else (16 if ld % 8 == 0 else 8, 2)
        #       dy_bf16 lddy dy_f32 lddyf x ldx x_is_bf16 gamma mean rstd dres lddres dres_is_bf16 dx_f32 lddx dx_bf16 lddxb dgamma dbeta
        args = [P, ld, None, 0, P, ld, x_bf16, P, P, P, P, ld, x_bf16, P, Cc, P, ld, P, P, 0, M, Cc, None, 0, None]   # no workspace
        _sweep(bwd, args, {0: xa, 4: xa, 7: (16, 4), 10: xa, 13: (16, 4), 15: xa}, WORKSPACE)
    args = [None, 0, P, Cc, P, Cc, 0, P, P, P, None, 0, 0, P, Cc, None, 0, None, None, 0, M, Cc, None, 0, None]
    _sweep(bwd, args, {2: (16, 4)}, WORKSPACE)                                  # fp32 dy
    # forward: nothing is refused after the shape tests, so only the misaligned calls are made (C, ld and M are those of above)
    fwd = ops._fn("lc2is_layernorm_fwd")
    for x_bf16, ld in ((0, Cc), (1, Cc), (1, Cc + 4)):
        xa = (16, 4) if not x_bf16 else (16 if ld % 8 == 0 else 8, 2)
        #       x ldx x_is_bf16 gamma beta y_bf16 ldy y_f32 ldyf mean rstd
        args = [P, ld, x_bf16, P, P, P, ld, P, Cc, P, P, M, Cc, 1e-5, None]
        for i, (align, elem) in {0: xa, 3: (16, 4), 4: (16, 4), 5: (16 if ld % 8 == 0 else 8, 2), 7: (16, 4)}.items():
            for o in _offsets(align, elem):
                bad = list(args)
                bad[i] = P + o
                assert fwd(*bad) == SHAPE, (x_bf16, ld, i, o)


def test_attention_launchers():
    from lc2is_amd import ops
    B, H, Sq, Sk, D = 2, 2, 77, 40, 64
    Cc = H * D
    #      Q ldq K ldk V ldv O ldo lse2 kbias
    fwd = [P, Cc, P, Cc, P, Cc, P, Cc, P, P, B, H, Sq, Sk, D, 0.125, 0]
    ptrs = {0: (16, 2), 2: (16, 2), 4: (16, 2), 6: (16, 2)}
    _sweep(ops._fn("lc2is_attention_fwd_dropout"), fwd + [2.0, 1, None], ptrs, UNSUPPORTED)              # p = 2
    plain = ops._fn("lc2is_attention_fwd")
    for i in ptrs:
        bad = list(fwd) + [None]
        bad[i] = P + 8
        assert plain(*bad) == SHAPE, i
    ld4 = list(fwd)
    ld4[7] = Cc + 4                   # O rows on 8-byte boundaries only: the 16-byte stores have no narrower path
    assert ops._fn("lc2is_attention_fwd_dropout")(*ld4, 2.0, 1, None) == SHAPE and plain(*ld4, None) == SHAPE
    #      Q ldq K ldk V ldv O ldo dO lddo dQ lddq dK lddk dV lddv lse2 delta kbias
    bwd = [P, Cc, P, Cc, P, Cc, P, Cc, P, Cc, P, Cc, P, Cc, P, Cc, P, P, P, B, H, Sq, Sk, D, 0.125, 0]
    ptrs = {i: (16, 2) for i in range(0, 16, 2)}
    _sweep(ops._fn("lc2is_attention_bwd_dropout"), bwd + [2.0, 1, None], ptrs, UNSUPPORTED)
    plain = ops._fn("lc2is_attention_bwd")
    for i in ptrs:
        bad = list(bwd) + [None]
        bad[i] = P + 8
        assert plain(*bad) == SHAPE, i
    ld4 = list(bwd)
    ld4[13] = ld4[15] = Cc + 4        # dK / dV leave as 8-byte stores: ld % 4 with an 8-byte base is taken ...
    _sweep(ops._fn("lc2is_attention_bwd_dropout"), ld4 + [2.0, 1, None], {12: (8, 2), 14: (8, 2)}, UNSUPPORTED)
    ld4[11] = Cc + 4                  # ... dQ leaves as 16-byte stores: refused
    assert ops._fn("lc2is_attention_bwd_dropout")(*ld4, 2.0, 1, None) == SHAPE


def test_dropout_launchers():
    from lc2is_amd import ops
    M, Cc = 300, 64
    #       x ldx resid ldr y32 ldy y16 ldy16
    args = [P, Cc, P, Cc, P, Cc, P, Cc, M, Cc, 0, 2.0, 1, None]                # p = 2: LC2IS_ERR_UNSUPPORTED
    _sweep(ops._fn("lc2is_dropout_rows_f32"), args, {0: (16, 4), 2: (16, 4), 4: (16, 4), 6: (16, 2)}, UNSUPPORTED)
    args[7] = Cc + 4
    _sweep(ops._fn("lc2is_dropout_rows_f32"), args, {6: (8, 2)}, UNSUPPORTED)
    for ld, align in ((Cc, 16), (Cc + 4, 8)):
        _sweep(ops._fn("lc2is_dropout_rows_bf16"), [P, ld, P, ld, M, Cc, 2.0, 1, None], {0: (align, 2), 2: (align, 2)}, UNSUPPORTED)


def test_swin_launchers():
    from lc2is_amd import ops
    nwin, wpi, nwx, Hp, Wp, ws, shift, nH = 4, 4, 2, 14, 14, 7, 3, 3
    Cc = nH * 32
    assert ops._fn("lc2is_swin_attn_bwd_workspace_bytes")(nwin, ws, nH) > 0
    #       qkv ld o ld_o dout lddo lse bias dqkv lddq dbias acc
    args = [P, 3 * Cc, P, Cc, P, Cc, P, P, P, 3 * Cc, P, 0, nwin, wpi, nwx, Hp, Wp, ws, shift, nH, Cc, 0.17, None, 0, None]   # dbias, no workspace
    _sweep(ops._fn("lc2is_swin_attn_bwd"), args, {0: (16, 2), 2: (16, 2), 4: (16, 2), 8: (16, 2)}, WORKSPACE)
    # forward: nothing is refused after the shape tests; the geometry is the one the backward call above passed with
    fwd = ops._fn("lc2is_swin_attn_fwd")
    #       qkv ld out ldo lse bias
    args = [P, 3 * Cc, P, Cc, P, P, nwin, wpi, nwx, Hp, Wp, ws, shift, nH, Cc, 0.17, None]
    for i in (0, 2):
        for o in (2, 4, 8):
            bad = list(args)
            bad[i] = P + o
            assert fwd(*bad) == SHAPE, (i, o)
