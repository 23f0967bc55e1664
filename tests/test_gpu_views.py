"""The dense hot-path launchers on OFFSET VIEWS against fp64 of the same bf16 / fp32 values.

The modules hand these kernels column slices of packed buffers (``w_cinT[:, C:]``, ``kv[:, :C]``, ``dkv[:, C:]``, ``h16[:, :C]``):
every operand with its own leading dimension and a base that is not the start of an allocation.  The dense op-level tests never
do.  Here every operand of every case is a view of a wider, taller buffer filled with a sentinel (tests/view_util.py), and each
case asserts three things: (1) the bound of the op's dense test against fp64 (test_gpu_gemm_ln.py, test_gpu_attention.py,
test_gpu_dropout.py: quoted at each assertion, not re-tuned), (2) ``torch.equal`` with the same call on ``.contiguous()`` copies,
(3) every sentinel outside the output views untouched.  View bases follow the alignment rule of include/lc2is_hip.h: multiples of
8 elements for bf16 rows with ld % 8, of 4 elements for bf16 rows with only ld % 4 and for fp32.

The ld = 4 (mod 8) layouts: gemm_nt's bf16 output with ldo = N + 4 takes the unstaged epilogue and layernorm / dropout / the
attention backward's dK, dV move 8 bytes per access: they run here.  The attention forward's O and the backward's dQ leave as
16-byte buffer stores with no narrower path: those launchers refuse such an ld now (test_gpu_hot_refusals.py)."""
import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from view_util import Guard, VecGuard, bf, embed, out_view, rel, vec  # noqa: E402

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ---- gemm_nt --------------------------------------------------------------------------------------------------------------------
NT_SHAPES = [(70, 64, 64), (300, 192, 128), (515, 384, 192), (300, 384, 64), (300, 200, 128), (17, 200, 64)]
NT_CFGS = (0, 1, 2, 3, 4, 6, 15, 16, 17)
NT_FORMS = ("f32_resid", "f32_inplace", "bf16_ld8", "bf16_ld4", "quick_gelu_aux", "dquick_gelu", "mul_aux", "bf16_resid")
_nt_ran = {}      # form -> {cfg} that ran for some shape


def _nt_operands(dev, M, N, K, seed):
    g = _gen(seed)
    a = bf(torch.randn(M, K, generator=g)).to(dev)
    w = bf(torch.randn(N, K, generator=g) * 0.05).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    resid = torch.randn(M, N, generator=g).to(dev)
    aux = bf(torch.randn(M, N, generator=g)).to(dev)
    av = embed(a, top=3, left=8, right=16)              # a = bufA[3:3+M, 8:8+K], lda = K + 24
    wv = embed(w, top=0, left=64, right=K, bottom=0)    # w = bufW[:, 64:64+K], ldw = 2K + 64: the w_cinT[:, C:] form
    assert av.stride(0) == K + 24 and wv.stride(0) == 2 * K + 64 and wv.storage_offset() == 64
    return a, w, bias, resid, aux, av, wv, vec(bias)


def _quick_gelu_d(s):
    sg = torch.sigmoid(1.702 * s)
    return sg * (1 + 1.702 * s * (1 - sg))


def _run_nt_form(dev, form):
    from lc2is_amd import ops
    ran = set()
    for M, N, K in NT_SHAPES:
        a, w, bias, resid, aux, av, wv, bv = _nt_operands(dev, M, N, K, M * 7 + N + K)
        z = a.double() @ w.double().T
        for cfg in NT_CFGS:
            where = (form, M, N, K, cfg)
            ldo = N + 4 if form == "bf16_ld4" else N + 8          # one row and 4 (or 8) columns in from the buffer's edge
            ob, of, ao = out_view(M, N, torch.bfloat16, dev, left=ldo - N), out_view(M, N, torch.float32, dev, left=4, right=4), \
                out_view(M, N, torch.bfloat16, dev, left=8)
            guards = []
            if form in ("f32_resid", "f32_inplace"):
                if form == "f32_inplace":
                    of.view.copy_(resid)
                    rv = of.view
                else:
                    rv = embed(resid, left=4, right=8)
                dense = lambda: ops.gemm_nt(a, w, bias, resid=resid, out_bf16=None, out_f32=True, tile_cfg=cfg)          # noqa: E731
                views = lambda: ops.gemm_nt(av, wv, bv, resid=rv, out_bf16=None, out_f32=of.view, tile_cfg=cfg)         # noqa: E731
                plan_kw, guards = dict(resid=True, out_bf16=False, out_f32=True), [of]
                refs = [None, z + bias.double() + resid.double(), None]
            elif form in ("bf16_ld8", "bf16_ld4"):
                dense = lambda: ops.gemm_nt(a, w, bias, tile_cfg=cfg)                                                    # noqa: E731
                views = lambda: ops.gemm_nt(av, wv, bv, out_bf16=ob.view, tile_cfg=cfg)                                 # noqa: E731
                plan_kw, guards = dict(), [ob]
                refs = [z + bias.double(), None, None]
            elif form == "quick_gelu_aux":
                dense = lambda: ops.gemm_nt(a, w, bias, act=ops.ACT_QUICK_GELU, aux_out=True, tile_cfg=cfg)             # noqa: E731
                views = lambda: ops.gemm_nt(av, wv, bv, act=ops.ACT_QUICK_GELU, out_bf16=ob.view, aux_out=ao.view, tile_cfg=cfg)  # noqa: E731
                plan_kw, guards = dict(act=ops.ACT_QUICK_GELU, aux_out=True), [ob, ao]
                zz = z + bias.double()
                refs = [zz * torch.sigmoid(1.702 * zz), None, zz]
            elif form in ("dquick_gelu", "mul_aux"):
                act = ops.ACT_DQUICK_GELU if form == "dquick_gelu" else ops.ACT_MUL_AUX
                xv = embed(aux, left=8, right=16)
                dense = lambda: ops.gemm_nt(a, w, None, act=act, aux_in=aux, tile_cfg=cfg)                               # noqa: E731
                views = lambda: ops.gemm_nt(av, wv, None, act=act, aux_in=xv, out_bf16=ob.view, tile_cfg=cfg)           # noqa: E731
                plan_kw, guards = dict(act=act, aux_in=True), [ob]
                refs = [z * (_quick_gelu_d(aux.double()) if form == "dquick_gelu" else aux.double()), None, None]
            else:   # a bf16 residual view: the ACT_ADD_AUX epilogue
                xv = embed(aux, left=16, right=8)
                dense = lambda: ops.gemm_nt(a, w, bias, resid=aux, tile_cfg=cfg)                                         # noqa: E731
                views = lambda: ops.gemm_nt(av, wv, bv, resid=xv, out_bf16=ob.view, tile_cfg=cfg)                       # noqa: E731
                plan_kw, guards = dict(act=ops.ACT_ADD_AUX, aux_in=True), [ob]
                refs = [z + bias.double() + aux.double(), None, None]
            try:
                want = dense()
            except RuntimeError:
                assert cfg != 0, where          # the automatic plan takes everything
                continue                         # a forced kernel that does not take this problem (16: N % 384, 17: M > 64, ...)
            try:
                staged = [[r[4] for r in ops.gemm_nt_plan(M, N, K, tile_cfg=cfg, ld=ld, **plan_kw)] for ld in (N, ldo)]   # (staged_epi of each launch)
            except RuntimeError:
                assert form == "bf16_ld4" and cfg in (15, 16), where     # the kernels that have only the staged epilogue
                continue
            got = views()                        # what the plan query takes for these leading dimensions, the launcher must take
            ran.add(cfg)
            if form == "bf16_ld4":
                assert staged[0] != staged[1], where      # ldo % 8 != 0: the unstaged epilogue; only the fp64 bound holds across the two
            else:
                assert staged[0] == staged[1], where
            for i, (gt, wt, ref) in enumerate(zip(got, want, refs)):
                if ref is None:
                    assert gt is None, where
                    continue
                if gt.dtype == torch.float32:
                    e_rel, e_abs = rel(gt, ref), (gt.double() - ref).abs().max().item()
                    print(where, "fp32 rel", e_rel, "abs", e_abs)
                    assert e_rel < 2e-6 * (K ** 0.5) and e_abs < 1e-3, where      # test_gemm_nt_plain / _fp32_only_output
                else:
                    e_rel = rel(gt.float(), ref)
                    print(where, "bf16 out", i, "rel", e_rel)
                    assert e_rel < (5e-3 if form in ("dquick_gelu", "mul_aux") else 4e-3), where   # 4e-3 bf16 output, 5e-3 derivative epilogues
                if staged[0] == staged[1]:
                    assert torch.equal(gt, wt), where
            assert all(g_.untouched() for g_ in guards), where
            assert got[0] is None or got[0].data_ptr() == ob.view.data_ptr()
    _nt_ran[form] = ran
    return ran


@pytest.mark.parametrize("form", NT_FORMS)
def test_gemm_nt_views(dev, form):
    ran = _run_nt_form(dev, form)
    assert {0, 1, 2, 3, 4, 6} <= ran, ran


def test_gemm_nt_views_ran_every_forced_kernel(dev):
    """Each of tile_cfg 0, 1, 2, 3, 4, 6, 15, 16, 17 took at least one (form, shape) of test_gemm_nt_views."""
    for form in NT_FORMS:
        if form not in _nt_ran:
            _run_nt_form(dev, form)
    assert set().union(*_nt_ran.values()) == set(NT_CFGS), _nt_ran


# ---- gemm_nt_ln -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(512, 768, 128), (300, 768, 192), (1024, 384, 64)])
def test_gemm_nt_ln_views(dev, M, N, K):
    from lc2is_amd import ops
    g = _gen(M * 13 + K)
    a = bf(torch.randn(M, K, generator=g)).to(dev)
    w = bf(torch.randn(N, K, generator=g) * 0.05).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    resid = (torch.randn(M, N, generator=g) * 3.0 + 0.7).to(dev)
    resid[:, 5] += 40.0
    gamma = (torch.rand(N, generator=g) + 0.5).to(dev)
    beta = torch.randn(N, generator=g).to(dev)
    av, wv = embed(a, top=3, left=8, right=16), embed(w, top=0, left=64, right=K, bottom=0)
    xo, ho = out_view(M, N, torch.float32, dev, left=4, right=4), out_view(M, N, torch.bfloat16, dev, left=8, right=8)
    x_d, h_d, m_d, r_d = ops.gemm_nt_ln(a, w, bias, resid, gamma, beta, 1e-5)
    x, h, mean, rstd = ops.gemm_nt_ln(av, wv, vec(bias), embed(resid, left=4, right=8), vec(gamma), vec(beta), 1e-5,
                                      out_f32=xo.view, ln_out=ho.view)
    torch.cuda.synchronize()
    assert x.data_ptr() == xo.view.data_ptr() and h.data_ptr() == ho.view.data_ptr()
    assert torch.equal(x, x_d) and torch.equal(h, h_d) and torch.equal(mean, m_d) and torch.equal(rstd, r_d)
    assert xo.untouched() and ho.untouched()
    # the bounds of test_gemm_nt_ln_fused_matches_the_two_launches, against the two launches on dense operands
    _, x_ref, _ = ops.gemm_nt(a, w, bias, resid=resid, out_bf16=None, out_f32=True)
    h_ref, _, m_ref, r_ref = ops.layernorm_fwd(x_ref, gamma, beta, 1e-5)
    assert torch.equal(x, x_ref)
    assert (mean - m_ref).abs().max().item() <= 2e-6 * m_ref.abs().max().item() + 1e-6
    assert ((rstd - r_ref).abs() / r_ref).max().item() < 5e-6
    d = (h.float() - h_ref.float()).abs()
    assert (d <= h_ref.float().abs() * 2.0 ** -7 + 1e-6).all() and (d > 0).float().mean().item() < 2e-2
    xd = x.double()
    ln = (xd - xd.mean(1, keepdim=True)) / (xd.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt() * gamma.double() + beta.double()
    e = rel(h.float(), ln)
    print((M, N, K), "h vs fp64", e)
    assert e < 4e-3
    assert rel(x, a.double() @ w.double().T + bias.double() + resid.double()) < 2e-6 * (K ** 0.5)
    for buf in ops._xchg_cache.values():
        assert int(buf.view(torch.int64).ne(0).sum().item()) == 0      # the exchange buffer is all zero afterwards


# ---- gemm_tn, gemm_tn_grouped, colsum -------------------------------------------------------------------------------------------
# the smallest rows of test_gpu_gemm_ln.TN_ROWS that run {128x128, 256x256 LDS-DMA} x {one split, several splits}
TN_VIEW_ROWS = [(33, 8, 8), (2050, 152, 512), (300, 3072, 3072), (4100, 2304, 768)]


def test_gemm_tn_view_rows_cover_both_kernels_with_and_without_slabs():
    from lc2is_amd import ops
    from test_gpu_gemm_ln import TN_ROWS
    assert set(TN_VIEW_ROWS) <= set(TN_ROWS)
    plans = [ops.gemm_tn_plan(M, N, K) for M, N, K in TN_VIEW_ROWS]
    assert {p["big"] for p in plans} == {0, 1}
    assert {p["splits"] == 1 for p in plans} == {True, False}
    assert {(p["big"], p["splits"] > 1) for p in plans} == {(0, False), (0, True), (1, False), (1, True)}


def _tn_views(dev, M, N, K, g):
    dy = bf(torch.randn(M, N, generator=g)).to(dev)
    x = bf(torch.randn(M, K, generator=g)).to(dev)
    ybuf = torch.full((M, 2 * N + 16), 7.0, dtype=torch.bfloat16, device=dev)
    dyv = ybuf[:, N + 16:]                                  # the second half of an [M, 2N + 16] buffer (the dkv[:, C:] form)
    dyv.copy_(dy)
    xv = embed(x, top=0, left=8, right=8, bottom=0)         # x = wide[:, 8:8+K]
    assert dyv.stride(0) == 2 * N + 16 and xv.stride(0) == K + 16
    return dy, x, dyv, xv


@pytest.mark.parametrize("M,N,K", TN_VIEW_ROWS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_gemm_tn_views(dev, M, N, K, accumulate):
    from lc2is_amd import ops
    g = _gen(M + N + K)
    dy, x, dyv, xv = _tn_views(dev, M, N, K, g)
    w0, b0 = torch.randn(N, K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    wo = out_view(N, K, torch.float32, dev, left=4, right=0)          # ldw = K + 4
    bo = VecGuard(N, dev)
    wo.view.copy_(w0); bo.view.copy_(b0)
    dw_d, db_d = w0.clone(), b0.clone()
    ops.gemm_tn(dy, x, dw_d, accumulate=accumulate, db=db_d)
    out = ops.gemm_tn(dyv, xv, wo.view, accumulate=accumulate, db=bo.view)
    assert out.data_ptr() == wo.view.data_ptr() and wo.view.stride(0) == K + 4
    ref_w = dy.double().T @ x.double() + (w0.double() if accumulate else 0.0)
    ref_b = dy.double().sum(0) + (b0.double() if accumulate else 0.0)
    print((M, N, K, accumulate), "dw", rel(wo.view, ref_w), "db", rel(bo.view, ref_b))
    assert rel(wo.view, ref_w) < 1e-5 and rel(bo.view, ref_b) < 1e-5      # test_gemm_tn
    assert torch.equal(wo.view, dw_d) and torch.equal(bo.view, db_d)
    assert wo.untouched() and bo.untouched()


@pytest.mark.parametrize("shapes", [[(64, 64), (128, 136), (200, 8)], [(256, 256), (512, 256), (256, 512)]])
def test_gemm_tn_grouped_views(dev, shapes):
    """Three problems, each dy at its own column offset of ONE shared buffer (the dqkv thirds), x / dw / db views; the 128x128 body
    and the 256x256 LDS-DMA body; mixed accumulate."""
    from lc2is_amd import ops
    g = _gen(17 + shapes[0][0])
    M = 300
    summary, _ = ops.gemm_tn_grouped_plan(shapes, M=M)
    assert bool(summary["small"]) == (shapes[0][0] == 64)
    ncols = 8 + sum(n for n, _ in shapes) + 8
    ybuf = torch.full((M + 3, ncols), 7.0, dtype=torch.bfloat16, device=dev)
    col, probs, dense, refs, guards = 8, [], [], [], []
    for i, (N, K) in enumerate(shapes):
        dy, x = bf(torch.randn(M, N, generator=g)).to(dev), bf(torch.randn(M, K, generator=g)).to(dev)
        dyv = ybuf[2:2 + M, col:col + N]
        dyv.copy_(dy)
        col += N
        acc = i % 2 == 1
        w0, b0 = torch.randn(N, K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
        wo, bo = out_view(N, K, torch.float32, dev, left=4, right=0), VecGuard(N, dev)
        wo.view.copy_(w0); bo.view.copy_(b0)
        probs.append((dyv, embed(x, top=0, left=8, right=8, bottom=0), wo.view, bo.view if i != 2 else None, acc))
        dense.append((dy, x, w0.clone(), b0.clone() if i != 2 else None, acc))
        refs.append((dy.double().T @ x.double() + (w0.double() if acc else 0.0), dy.double().sum(0) + (b0.double() if acc else 0.0)))
        guards += [wo, bo]
    assert len({p[0].storage_offset() % ncols for p in probs}) == 3
    ops.gemm_tn_grouped(probs)
    ops.gemm_tn_grouped(dense)
    for p, d, (rw, rb) in zip(probs, dense, refs):
        assert rel(p[2], rw) < 1e-5                                       # test_gemm_tn_grouped
        assert torch.equal(p[2], d[2])
        if p[3] is not None:
            assert rel(p[3], rb) < 1e-5 and torch.equal(p[3], d[3])
    assert all(g_.untouched() for g_ in guards)       # (the third problem's db guard too: db = None writes nothing)


@pytest.mark.parametrize("M,N", [(300, 128), (1025, 768)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum_views(dev, M, N, accumulate):
    from lc2is_amd import ops
    g = _gen(M + N)
    dy, _, dyv, _ = _tn_views(dev, M, N, 8, g)
    b0 = torch.randn(N, generator=g).to(dev)
    bo = VecGuard(N, dev)
    bo.view.copy_(b0)
    db_d = ops.colsum(dy, b0.clone(), accumulate=accumulate)
    ops.colsum(dyv, bo.view, accumulate=accumulate)
    assert rel(bo.view, dy.double().sum(0) + (b0.double() if accumulate else 0.0)) < 1e-5      # test_colsum
    assert torch.equal(bo.view, db_d) and bo.untouched()


# ---- layernorm ------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(37, 64), (100, 192), (300, 768), (9, 2048)]


LN_PAD = dict(left=4, right=8)      # ld = C + 12: for bf16 rows that is 4 (mod 8), the 8-byte layout these kernels admit


@pytest.mark.parametrize("M,C", LN_SHAPES)
@pytest.mark.parametrize("x_bf16", [False, True])
def test_layernorm_fwd_views(dev, M, C, x_bf16):
    from lc2is_amd import ops
    g = _gen(C + M)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dev)
    x = bf(x) if x_bf16 else x
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    xv = embed(x, top=3, **LN_PAD)
    yb, yf = out_view(M, C, torch.bfloat16, dev, left=4, right=8), out_view(M, C, torch.float32, dev, left=4, right=4)
    assert xv.stride(0) == C + 12 and yb.view.stride(0) % 8 == 4
    want = ops.layernorm_fwd(x, gamma, beta, 1e-5, out_bf16=True, out_f32=True)
    got = ops.layernorm_fwd(xv, vec(gamma), vec(beta), 1e-5, out_bf16=yb.view, out_f32=yf.view)
    assert got[0].data_ptr() == yb.view.data_ptr() and got[1].data_ptr() == yf.view.data_ptr()
    ref = torch.nn.functional.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    e_abs, e_rel = (got[1].double() - ref).abs().max().item(), rel(got[0].float(), ref)
    print((M, C, x_bf16), "y abs", e_abs, "bf16 rel", e_rel)
    assert e_abs < 2e-5 and e_rel < 4e-3                    # test_layernorm_fwd_bwd
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert yb.untouched() and yf.untouched()
    # no beta, bf16 output only (the decoder norms of torch 2.10's bias=False)
    yb2 = out_view(M, C, torch.bfloat16, dev, left=8, right=8)
    got2 = ops.layernorm_fwd(xv, vec(gamma), None, 1e-5, out_bf16=yb2.view)
    assert torch.equal(got2[0], ops.layernorm_fwd(x, gamma, None, 1e-5)[0]) and yb2.untouched()
    assert rel(got2[0].float(), ref - beta.double()) < 4e-3


@pytest.mark.parametrize("M,C", LN_SHAPES)
@pytest.mark.parametrize("x_bf16", [False, True])
@pytest.mark.parametrize("kernel", ["generic", "lean"])
def test_layernorm_bwd_views(dev, M, C, x_bf16, kernel):
    """generic: fp32 dy / dres, fp32 + bf16 dx.  lean: bf16 dy / dres, bf16 dx only (want_f32=False).  dgamma / dbeta go to vector views."""
    from lc2is_amd import ops
    g = _gen(C * 3 + M)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dev)
    x = bf(x) if x_bf16 else x
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
    dy, dres = torch.randn(M, C, generator=g).to(dev), torch.randn(M, C, generator=g).to(dev)
    lean = kernel == "lean"
    if lean:
        dy, dres = bf(dy), bf(dres)
    _, _, mean, rstd = ops.layernorm_fwd(x, gamma, None, 1e-5)
    xv, dyv, drv = embed(x, top=3, **LN_PAD), embed(dy, left=4, right=8), embed(dres, top=2, left=4, right=16 if not lean else 8)
    dg, db = VecGuard(C, dev), VecGuard(C, dev)
    # mean / rstd as slices of one longer statistics vector (4-byte reads: any element offset)
    stats = torch.cat([torch.full((3,), 7.0, device=dev), mean, torch.full((5,), 7.0, device=dev), rstd])
    mv, rv = stats[3:3 + M], stats[3 + M + 5:]
    want = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, want_f32=not lean)
    got = ops.layernorm_bwd(dyv, xv, vec(gamma), mv, rv, dres=drv, dgamma=dg.view, dbeta=db.view, want_f32=not lean)
    xd, gd = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    bd = torch.zeros(C, dtype=torch.float64, device=dev, requires_grad=True)
    torch.nn.functional.layer_norm(xd, (C,), gd, bd, 1e-5).backward(dy.double())
    ref_dx = xd.grad + dres.double()
    figs = dict(dxb=rel(got[1].float(), ref_dx), dg=rel(got[2], gd.grad), db=rel(got[3], bd.grad))
    if not lean:
        figs["dxf"] = rel(got[0], ref_dx)
    print((M, C, x_bf16, kernel), figs)
    assert figs["dxb"] < 4e-3 and figs["dg"] < 1e-5 and figs["db"] < 1e-5        # test_layernorm_fwd_bwd / _bwd_lean_kernel
    assert lean and got[0] is None or figs["dxf"] < 1e-5
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, want))
    assert got[2].data_ptr() == dg.view.data_ptr() and dg.untouched() and db.untouched()


# ---- attention ------------------------------------------------------------------------------------------------------------------
def _ref_attention(q, k, v, B, H, Sq, Sk, D, scale, causal, kbias, mult=None):
    q4, k4, v4 = (t.reshape(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    s = q4 @ k4.transpose(-1, -2) * scale
    if kbias is not None:
        s = s + kbias.double()[:, None, None, :]
    if causal:
        s = s + torch.full((Sq, Sk), float("-inf"), dtype=torch.float64, device=q.device).triu(1)
    p = torch.softmax(s, dim=-1)
    if mult is not None:
        p = p * mult
    return (p @ v4).transpose(1, 2).reshape(B * Sq, H * D), torch.logsumexp(s, dim=-1)


ATT_CASES = [
    # B, H, Sq, Sk, D, layout, causal, mask, p
    (2, 2, 65, 65, 64, "packed", False, False, 0.0),       # self-attention: qkv a [B*S, 3C + 8] buffer, all three 8 columns in
    (2, 2, 77, 40, 96, "cross", False, True, 0.0),         # own q buffer, kv[:, :C] / kv[:, C:] of a padded kv, key-padding bias
    (2, 2, 77, 77, 64, "plain", True, True, 0.0),          # causal with mask
    (1, 2, 129, 200, 128, "plain", False, False, 0.0),
    (2, 2, 33, 130, 128, "cross", False, True, 0.2),       # through the dropout entries, with the exported mask
]


@pytest.mark.parametrize("B,H,Sq,Sk,D,layout,causal,mask,p", ATT_CASES)
def test_attention_views(dev, B, H, Sq, Sk, D, layout, causal, mask, p):
    from lc2is_amd import ops
    g = _gen(B * 1000 + Sq + D)
    C = H * D
    q = bf(torch.randn(B * Sq, C, generator=g)).to(dev)
    k = bf(torch.randn(B * Sk, C, generator=g)).to(dev)
    v = bf(torch.randn(B * Sk, C, generator=g)).to(dev)
    do = bf(torch.randn(B * Sq, C, generator=g) * (0.5 if p else 1.0)).to(dev)
    kbias = None
    if mask:
        valid = torch.randint(1, Sk + 1, (B,), generator=g)
        kbias = torch.zeros(B, Sk)
        for i in range(B):
            kbias[i, valid[i]:] = float("-inf")
        kbias = kbias.to(dev)
    if layout == "packed":
        buf = torch.full((B * Sq + 3, 3 * C + 8), 7.0, dtype=torch.bfloat16, device=dev)
        qv, kv_, vv = (buf[1:1 + B * Sq, 8 + i * C:8 + (i + 1) * C] for i in range(3))
        qv.copy_(q); kv_.copy_(k); vv.copy_(v)
    else:
        qv = embed(q, top=2, left=8, right=16)
        if layout == "cross":
            kv = embed(torch.cat([k, v], 1), left=8, right=8)
            kv_, vv = kv[:, :C], kv[:, C:]
        else:
            kv_, vv = embed(k, left=16, right=8), embed(v, top=3, left=8, right=24)
    dov = embed(do, left=8, right=8)
    seed, scale = 0x1234567890ABCDEF + Sq, 1.0 / math.sqrt(D)
    kw = dict(causal=causal, kbias=kbias, dropout_p=p, seed=seed)
    og = out_view(B * Sq, C, torch.bfloat16, dev, left=8, right=0)            # ldo = C + 8 (C + 4 is refused: 16-byte stores)
    o_d, lse_d = ops.attention_fwd(q, k, v, B, H, Sq, Sk, D, scale, **kw)
    o, lse = ops.attention_fwd(qv, kv_, vv, B, H, Sq, Sk, D, scale, out=og.view, **kw)
    assert o.data_ptr() == og.view.data_ptr() and og.view.stride(0) == C + 8
    mult = None
    if p:
        keep = 1.0 - round(p * 65536) / 65536.0
        mult = (ops.dropout_mask(B * H * Sq, Sk, p, seed, dev).double() / keep).reshape(B, H, Sq, Sk)
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    ro, rlse = _ref_attention(qd, kd, vd, B, H, Sq, Sk, D, scale, causal, kbias, mult)
    e_abs, e_rel = (o.double() - ro.detach()).abs().max().item(), rel(o, ro.detach())
    e_lse = (lse.double() * math.log(2.0) - rlse.detach()).abs().max().item()
    print((B, H, Sq, Sk, D, layout, p), "o abs", e_abs, "rel", e_rel, "lse", e_lse)
    assert e_abs < 2e-2 and e_rel < 6e-3 and e_lse < 2e-3              # test_attention_fwd
    assert torch.equal(o, o_d) and torch.equal(lse, lse_d) and og.untouched()
    # backward: o from the view above (ld % 8), dq a view with ld = C + 8, dk / dv views with ld = C + 4 (8-byte stores)
    ro.backward(do.double())
    want = ops.attention_bwd(q, k, v, o_d, do, lse_d, B, H, Sq, Sk, D, scale, **kw)
    gq = out_view(B * Sq, C, torch.bfloat16, dev, left=8, right=0)
    gk, gv = out_view(B * Sk, C, torch.bfloat16, dev, left=4, right=0), out_view(B * Sk, C, torch.bfloat16, dev, left=4, right=8, top=2)
    assert gk.view.stride(0) == C + 4 and gv.view.stride(0) % 8 == 4
    got = ops.attention_bwd(qv, kv_, vv, o, dov, lse, B, H, Sq, Sk, D, scale, dq=gq.view, dk=gk.view, dv=gv.view, **kw)
    # ... and the decoders' form: dk = dkv[:, :C], dv = dkv[:, C:] of one padded buffer
    gkv = out_view(B * Sk, 2 * C, torch.bfloat16, dev, left=8, right=8)
    gq2 = out_view(B * Sq, C, torch.bfloat16, dev, left=16, right=8)
    got2 = ops.attention_bwd(qv, kv_, vv, o, dov, lse, B, H, Sq, Sk, D, scale, dq=gq2.view, dk=gkv.view[:, :C], dv=gkv.view[:, C:], **kw)
    for name, a, a2, w_, ref in zip(("dq", "dk", "dv"), got, got2, want, (qd.grad, kd.grad, vd.grad)):
        e = rel(a, ref)
        print("   ", name, e)
        assert e < 1.5e-2, name                                              # test_attention_bwd
        assert torch.equal(a, w_) and torch.equal(a2, w_), name
    assert all(g_.untouched() for g_ in (gq, gk, gv, gkv, gq2))


# ---- dropout_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_per_sample", [0, 100])
def test_dropout_rows_f32_views(dev, rows_per_sample):
    from lc2is_amd import ops
    M, C, p, seed = 300, 64, 0.25, 99
    g = _gen(0)
    x, r = torch.randn(M, C, generator=g).to(dev), torch.randn(M, C, generator=g).to(dev)
    y32, y16 = out_view(M, C, torch.float32, dev, left=4, right=4), out_view(M, C, torch.bfloat16, dev, left=4, right=8)
    assert y16.view.stride(0) % 8 == 4
    want = ops.dropout_rows_f32(x, p, seed, resid=r, out_f32=True, out_bf16=True, rows_per_sample=rows_per_sample)
    got = ops.dropout_rows_f32(embed(x, top=3, left=4, right=8), p, seed, resid=embed(r, left=8, right=4), out_f32=y32.view,
                               out_bf16=y16.view, rows_per_sample=rows_per_sample)
    if rows_per_sample:
        mk = ops.dropout_mask(M // rows_per_sample, 1, p, seed, dev).float().repeat_interleave(rows_per_sample, 0)
    else:
        mk = ops.dropout_mask(M, C, p, seed, dev).float()
    assert torch.allclose(got[0], r + x * mk / 0.75, rtol=1e-6, atol=1e-6) and torch.equal(got[1], got[0].bfloat16())   # test_dropout_kernels_...
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].data_ptr() == y32.view.data_ptr() and y32.untouched() and y16.untouched()


def test_dropout_rows_bf16_views(dev):
    from lc2is_amd import ops
    M, C, p, seed = 300, 64, 0.25, 99
    xb = bf(torch.randn(M, C, generator=_gen(0))).to(dev)
    mk = ops.dropout_mask(M, C, p, seed, dev).float()
    want = (xb.float() * mk / 0.75).bfloat16()
    y = out_view(M, C, torch.bfloat16, dev, left=4, right=8)
    xv = embed(xb, top=3, left=4, right=0)                  # ld = C + 4
    got = ops.dropout_rows_bf16(xv, p, seed, out=y.view)
    assert torch.equal(got, want) and torch.equal(xv, xb) and y.untouched()
    inplace = Guard(M, C, torch.bfloat16, dev, top=1, left=8, right=4)
    inplace.view.copy_(xb)
    assert ops.dropout_rows_bf16(inplace.view, p, seed).data_ptr() == inplace.view.data_ptr()
    assert torch.equal(inplace.view, want) and inplace.untouched()
