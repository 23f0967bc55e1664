"""The dense hot-path wrappers of lc2is_amd/ops.py refuse a bad operand BEFORE any launch, naming it.

These kernels index every tensor by the call's integers alone: a tensor that is one row short is read or written out of bounds, a
base below the alignment of include/lc2is_hip.h misaligns every 8- / 16-byte access.  For every tensor argument of every wrapper:
one row short and one row long, a wrong column count, a wrong dtype, a ``.cpu()`` tensor, a non-contiguous vector and a misaligned
base (``buf[:, 1:1+K]``) raise ``RuntimeError("lc2is_amd.<op>: <name> ...")``.  Everything runs under ``no_launch`` (``ops._fn``
raises AssertionError), so a refusal that comes late fails the test and nothing can be launched with a bad operand.  The last test
makes the modules' own view-shaped calls through the real entry points: they are not refused."""
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from view_util import SENT  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def no_launch(monkeypatch):
    """Any attempt to reach a kernel entry point fails the test: the refusal has to come first."""
    from lc2is_amd import ops

    def boom(name):
        raise AssertionError(f"{name} was about to be launched")
    monkeypatch.setattr(ops, "_fn", boom)
    return ops


def _full(dev, dtype, *shape):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def _variants(t, vector):
    """(what, bad tensor) for one well-formed operand ``t``: rows with an ld (2-D / 3-D), or a vector the kernel takes no ld for."""
    other = F32 if t.dtype == BF else BF
    yield "one row short", t[:-1]
    yield "one row long", torch.cat([t, t[:1]])
    if t.dim() >= 2:
        yield "wrong column count", t[..., :-4]
    yield "wrong dtype", t.to(other)
    yield "on the CPU", t.cpu()
    if vector:
        yield "not contiguous", torch.stack([t, t], -1)[..., 0]
    else:
        wide = torch.full(t.shape[:-1] + (t.shape[-1] + 8,), SENT, dtype=t.dtype, device=t.device)
        yield "misaligned base", wide[..., 1:1 + t.shape[-1]]               # buf[:, 1:1+K]: 2 (bf16) or 4 (fp32) bytes off
        yield "inner stride 2", torch.stack([t, t], -1)[..., 0]


def _sweep(op, call, good, kinds, outputs=(), defines=()):
    """call(**operands) with one operand at a time replaced by each bad variant.  kinds: name -> "rows" | "vec" | "vec16" (a vector
    with a float4 reader: also refused one element in).  ``defines``: the operands whose shape DEFINES the call's sizes (M, N, K): a changed
    row or column count of one of them is refused under the name of whichever operand no longer fits."""
    for name, kind in kinds.items():
        bad = list(_variants(good[name], kind != "rows"))
        if kind == "vec16":
            n = good[name].numel()
            bad.append(("base one element in", torch.full((n + 4,), SENT, device=good[name].device)[1:1 + n]))
        for what, t in bad:
            who = r"\w+" if name in defines and ("row" in what or "column" in what) else re.escape(name)
            with pytest.raises(RuntimeError, match=rf"lc2is_amd\.{op}: {who}\b"):
                call(**{**good, name: t})
    for name in outputs:
        assert bool((good[name] == SENT).all()), f"{op}: {name} was written"


def test_gemm_nt_refuses(dev, no_launch):
    ops = no_launch
    M, N, K = 70, 64, 64
    good = dict(a=_full(dev, BF, M, K), w=_full(dev, BF, N, K), bias=_full(dev, F32, N), resid=_full(dev, F32, M, N),
                aux_in=_full(dev, BF, M, N), out_bf16=_full(dev, BF, M, N), out_f32=_full(dev, F32, M, N), aux_out=_full(dev, BF, M, N))

    def call(a, w, bias, resid, aux_in, out_bf16, out_f32, aux_out):
        ops.gemm_nt(a, w, bias, act=ops.ACT_MUL_AUX, resid=resid, aux_in=aux_in, out_bf16=out_bf16, out_f32=out_f32, aux_out=aux_out)
    _sweep("gemm_nt", call, good, dict(a="rows", w="rows", bias="vec16", resid="rows", aux_in="rows", out_bf16="rows", out_f32="rows",
                                       aux_out="rows"), outputs=("out_bf16", "out_f32", "aux_out"), defines=("a", "w"))
    # a bf16 residual is checked as the residual it is
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.gemm_nt: resid\b"):
        ops.gemm_nt(good["a"], good["w"], good["bias"], resid=good["aux_in"][:-1])
    # bf16 rows with ld = 4 (mod 8): an 8-byte base is taken (nothing is refused before the launch), a 4-byte base is not
    wide = _full(dev, BF, M + 1, N + 4)
    with pytest.raises(AssertionError, match="about to be launched"):
        ops.gemm_nt(good["a"], good["w"], out_bf16=wide[1:, 4:])
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.gemm_nt: out_bf16\b"):
        ops.gemm_nt(good["a"], good["w"], out_bf16=wide[1:, 2:2 + N])
    assert bool((wide == SENT).all())


def test_gemm_nt_ln_refuses(dev, no_launch):
    ops = no_launch
    M, N, K = 256, 384, 64
    good = dict(a=_full(dev, BF, M, K), w=_full(dev, BF, N, K), bias=_full(dev, F32, N), resid=_full(dev, F32, M, N),
                gamma=_full(dev, F32, N), beta=_full(dev, F32, N), out_f32=_full(dev, F32, M, N), ln_out=_full(dev, BF, M, N))

    def call(a, w, bias, resid, gamma, beta, out_f32, ln_out):
        ops.gemm_nt_ln(a, w, bias, resid, gamma, beta, out_f32=out_f32, ln_out=ln_out)
    _sweep("gemm_nt_ln", call, good, dict(a="rows", w="rows", bias="vec16", resid="rows", gamma="vec16", beta="vec16", out_f32="rows",
                                          ln_out="rows"), outputs=("out_f32", "ln_out"), defines=("a", "w"))


def test_gemm_nt_batched_refuses(dev, no_launch):
    ops = no_launch
    Bn, M, N, K = 2, 16, 8, 64
    good = dict(a=_full(dev, BF, Bn, M, K), w=_full(dev, BF, Bn, N, K), out_bf16=_full(dev, BF, Bn, M, N), out_f32=_full(dev, F32, Bn, M, N))

    def call(a, w, out_bf16, out_f32):
        ops.gemm_nt_batched(a, w, out_bf16=out_bf16, out_f32=out_f32)
    _sweep("gemm_nt_batched", call, good, dict(a="rows", w="rows", out_bf16="rows", out_f32="rows"), outputs=("out_bf16", "out_f32"),
           defines=("a", "w"))


def test_gemm_tn_and_colsum_refuse(dev, no_launch):
    ops = no_launch
    M, N, K = 33, 16, 8
    good = dict(dy=_full(dev, BF, M, N), x=_full(dev, BF, M, K), dw=_full(dev, F32, N, K), db=_full(dev, F32, N))

    def call(dy, x, dw, db):
        ops.gemm_tn(dy, x, dw, accumulate=True, db=db)
    _sweep("gemm_tn", call, good, dict(dy="rows", x="rows", dw="rows", db="vec"), outputs=("dw", "db"), defines=("dy", "x"))

    def grouped(dy, x, dw, db):
        ok = (good["dy"], good["x"], good["dw"], good["db"], False)
        ops.gemm_tn_grouped([ok, (dy, x, dw, db, True)])
    _sweep("gemm_tn_grouped", grouped, good, dict(dy="rows", x="rows", dw="rows", db="vec"), outputs=("dw", "db"), defines=("dy", "x"))
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.gemm_tn_grouped: dw\b.*problem 1"):
        grouped(good["dy"], good["x"], good["dw"][:-1], good["db"])

    def colsum(dy, db):
        ops.colsum(dy, db, accumulate=True)
    # (dy alone defines M: another row count of it is another valid call; another column count no longer fits db)
    for what, t in _variants(good["dy"], False):
        if "row" not in what:
            with pytest.raises(RuntimeError, match=r"lc2is_amd\.colsum: (dy|db)\b"):
                colsum(t, good["db"])
    _sweep("colsum", colsum, dict(dy=good["dy"], db=good["db"]), dict(db="vec"), outputs=("db",))


def test_layernorm_refuses(dev, no_launch):
    ops = no_launch
    M, Cc = 9, 64
    for xdt in (F32, BF):
        good = dict(x=_full(dev, xdt, M, Cc), gamma=_full(dev, F32, Cc), beta=_full(dev, F32, Cc), out_bf16=_full(dev, BF, M, Cc),
                    out_f32=_full(dev, F32, M, Cc))

        def fwd(x, gamma, beta, out_bf16, out_f32):
            ops.layernorm_fwd(x, gamma, beta, out_bf16=out_bf16, out_f32=out_f32)
        # x may be bf16 or fp32, so "the other dtype" is a valid call: it gets a dtype the kernel has no path for instead
        for what, t in list(_variants(good["x"], False)) + [("int32", good["x"].to(torch.int32))]:
            if what != "wrong dtype":
                with pytest.raises(RuntimeError, match=r"lc2is_amd\.layernorm_fwd: \w+"):
                    fwd(**{**good, "x": t})
        _sweep("layernorm_fwd", fwd, good, dict(gamma="vec16", beta="vec16", out_bf16="rows", out_f32="rows"), outputs=("out_bf16", "out_f32"))
    good = dict(dy=_full(dev, BF, M, Cc), x=_full(dev, BF, M, Cc), gamma=_full(dev, F32, Cc), mean=_full(dev, F32, M), rstd=_full(dev, F32, M),
                dres=_full(dev, BF, M, Cc), dgamma=_full(dev, F32, Cc), dbeta=_full(dev, F32, Cc))

    def bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta):
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, dgamma=dgamma, dbeta=dbeta, accumulate=True)
    # dy / x / dres may each be bf16 or fp32, so the other dtype is a valid call: they get a dtype the kernel has no path for
    for name in ("dy", "x", "dres"):
        for what, t in list(_variants(good[name], False)) + [("int32", good[name].to(torch.int32))]:
            if what == "wrong dtype":
                continue
            with pytest.raises(RuntimeError, match=r"lc2is_amd\.layernorm_bwd: \w+"):
                bwd(**{**good, name: t})
    _sweep("layernorm_bwd", bwd, good, dict(gamma="vec16", mean="vec", rstd="vec", dgamma="vec", dbeta="vec"), outputs=("dgamma", "dbeta"))


def test_attention_refuses(dev, no_launch):
    ops = no_launch
    B, H, Sq, Sk, D = 2, 2, 5, 3, 64
    Cc = H * D
    good = dict(q=_full(dev, BF, B * Sq, Cc), k=_full(dev, BF, B * Sk, Cc), v=_full(dev, BF, B * Sk, Cc), kbias=_full(dev, F32, B, Sk),
                out=_full(dev, BF, B * Sq, Cc))

    def fwd(q, k, v, kbias, out):
        ops.attention_fwd(q, k, v, B, H, Sq, Sk, D, 0.125, kbias=kbias, out=out)
    _sweep("attention_fwd", fwd, good, dict(q="rows", k="rows", v="rows", kbias="vec", out="rows"), outputs=("out",))
    # O rows on 8-byte boundaries only (ldo = C + 4): the kernel stores whole 16-byte chunks and has no narrower path
    pad4 = _full(dev, BF, B * Sq + 1, Cc + 4)
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.attention_fwd: out\b.*multiple of 8"):
        fwd(**{**good, "out": pad4[1:, 4:]})
    assert bool((pad4 == SENT).all())
    good = dict(q=good["q"], k=good["k"], v=good["v"], o=_full(dev, BF, B * Sq, Cc), do=_full(dev, BF, B * Sq, Cc),
                lse2=_full(dev, F32, B, H, Sq), kbias=good["kbias"], dq=_full(dev, BF, B * Sq, Cc), dk=_full(dev, BF, B * Sk, Cc),
                dv=_full(dev, BF, B * Sk, Cc))

    def bwd(q, k, v, o, do, lse2, kbias, dq, dk, dv):
        ops.attention_bwd(q, k, v, o, do, lse2, B, H, Sq, Sk, D, 0.125, kbias=kbias, dq=dq, dk=dk, dv=dv)
    _sweep("attention_bwd", bwd, good, dict(q="rows", k="rows", v="rows", o="rows", do="rows", lse2="vec", kbias="vec", dq="rows", dk="rows",
                                            dv="rows"), outputs=("dq", "dk", "dv"))
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.attention_bwd: lse2\b"):
        bwd(**{**good, "lse2": _full(dev, F32, B, Sq, H).transpose(1, 2)})          # [B,H,Sq] by shape, not contiguous
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.attention_bwd: dq\b.*multiple of 8"):
        bwd(**{**good, "dq": pad4[1:, 4:]})
    pad4k = _full(dev, BF, B * Sk + 1, Cc + 4)
    with pytest.raises(AssertionError, match="about to be launched"):                 # dk / dv with ld = C + 4 on an 8-byte base are taken
        bwd(**{**good, "dk": pad4k[1:, 4:]})
    with pytest.raises(RuntimeError, match=r"lc2is_amd\.attention_bwd: dv\b"):        # ... on a 4-byte base they are not
        bwd(**{**good, "dv": pad4k[1:, 2:2 + Cc]})
    assert bool((pad4 == SENT).all()) and bool((pad4k == SENT).all())


def test_dropout_rows_refuse(dev, no_launch):
    ops = no_launch
    M, Cc = 6, 8
    good = dict(x=_full(dev, F32, M, Cc), resid=_full(dev, F32, M, Cc), out_f32=_full(dev, F32, M, Cc), out_bf16=_full(dev, BF, M, Cc))

    def f32(x, resid, out_f32, out_bf16):
        ops.dropout_rows_f32(x, 0.25, 3, resid=resid, out_f32=out_f32, out_bf16=out_bf16)
    _sweep("dropout_rows_f32", f32, good, dict(x="rows", resid="rows", out_f32="rows", out_bf16="rows"), outputs=("out_f32", "out_bf16"),
           defines=("x",))
    good = dict(x=_full(dev, BF, M, Cc), out=_full(dev, BF, M, Cc))

    def b16(x, out):
        ops.dropout_rows_bf16(x, 0.25, 3, out=out)
    _sweep("dropout_rows_bf16", b16, good, dict(x="rows", out="rows"), outputs=("out",), defines=("x",))


def test_swin_attn_refuses(dev, no_launch):
    ops = no_launch
    nwin, wpi, nwx, Hp, Wp, ws, shift, nH = 4, 4, 2, 4, 4, 2, 1, 2
    S, Cc = ws * ws, nH * 32
    geom = (nwin, wpi, nwx, Hp, Wp, ws, shift, nH, 0.17)
    good = dict(qkv=_full(dev, BF, nwin * S, 3 * Cc), bias=_full(dev, F32, nH, S, S), out=_full(dev, BF, nwin * S, Cc))

    def fwd(qkv, bias, out):
        ops.swin_attn_fwd(qkv, bias, *geom, out=out)
    _sweep("swin_attn_fwd", fwd, good, dict(qkv="rows", bias="vec", out="rows"), outputs=("out",), defines=("qkv",))
    good = dict(qkv=good["qkv"], o=_full(dev, BF, nwin * S, Cc), do=_full(dev, BF, nwin * S, Cc), lse=_full(dev, F32, nwin, nH, S),
                bias=good["bias"], dbias=_full(dev, F32, nH, S, S), dqkv=_full(dev, BF, nwin * S, 3 * Cc))

    def bwd(qkv, o, do, lse, bias, dbias, dqkv):
        ops.swin_attn_bwd(qkv, o, do, lse, bias, *geom, dbias=dbias, accumulate_dbias=True, dqkv=dqkv)
    _sweep("swin_attn_bwd", bwd, good, dict(qkv="rows", o="rows", do="rows", lse="vec", bias="vec", dbias="vec", dqkv="rows"),
           outputs=("dbias", "dqkv"), defines=("qkv",))


def test_ce_nchw_refuses(dev, no_launch):
    """ops.ce_nchw_fwd / ce_nchw_bwd index labels, lse and grad_px by B, H, W of the logits alone: a tensor that is short is read
    out of bounds.  Each bad operand is refused before any launch (the well-formed call reaches the launcher)."""
    ops = no_launch
    B, C, H, W = 1, 3, 4, 5
    z = torch.zeros(B, C, H, W, device=dev)
    lab = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    lse = torch.zeros(B, H, W, device=dev)
    short = torch.zeros(B, H, W - 1, device=dev)
    strided = torch.zeros(B, H, 2 * W, device=dev)[..., :W]          # the right shape, rows 2 W apart
    fwd_bad = dict(labels_short=(z, lab[..., :W - 1].contiguous()), labels_int32=(z, lab.int()),
                   logits_not_contiguous=(torch.zeros(B, C, H, 2 * W, device=dev)[..., :W], lab))
    for what, (logits, labels) in fwd_bad.items():
        with pytest.raises(RuntimeError, match=r"lc2is_amd"):
            ops.ce_nchw_fwd(logits, labels)
    bwd_bad = dict(labels_short=dict(labels=lab[..., :W - 1].contiguous()), lse_short=dict(lse=short),
                   lse_not_contiguous=dict(lse=strided), grad_px_short=dict(grad_px=short))
    for what, swap in bwd_bad.items():
        a = {**dict(labels=lab, lse=lse, grad_px=None), **swap}
        with pytest.raises(RuntimeError, match=r"lc2is_amd"):
            ops.ce_nchw_bwd(z, a["labels"], a["lse"], None, 1.0, grad_px=a["grad_px"])
    with pytest.raises(AssertionError, match="about to be launched"):
        ops.ce_nchw_fwd(z, lab)
    with pytest.raises(AssertionError, match="about to be launched"):
        ops.ce_nchw_bwd(z, lab, lse, None, 1.0, grad_px=lse)


def test_module_shaped_calls_are_not_refused(dev):
    """What nn/hier.py, nn/ftn.py, nn/decoder.py and nn/swin.py pass — column slices of packed buffers, outputs inside padded ones —
    goes through the real entry points."""
    from lc2is_amd import ops
    g = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)        # noqa: E731
    C, M, Mk, B, H = 128, 70, 40, 2, 2
    D = C // H
    # ops.gemm_nt(dkv2, s["w_cinT"][:, C:], None, resid=dmem32, out_f32=dmem32): W a column slice with ldw = 3C > K and a base offset
    w_cinT = rnd(C, 3 * C).bfloat16()
    dkv2, dmem32 = rnd(M, 2 * C).bfloat16(), rnd(M, C)
    want = dmem32.double() + dkv2.double() @ w_cinT[:, C:].double().T
    ops.gemm_nt(dkv2, w_cinT[:, C:], None, resid=dmem32, out_bf16=None, out_f32=dmem32)
    assert ((dmem32.double() - want).norm() / want.norm()).item() < 2e-6 * (2 * C) ** 0.5
    # ops.gemm_tn(dkv[:, C:], mem16, ...)
    dkv, mem16 = rnd(Mk * B, 2 * C).bfloat16(), rnd(Mk * B, C).bfloat16()
    dw = ops.gemm_tn(dkv[:, C:], mem16, db=torch.empty(C, device=dev))
    assert ((dw.double() - dkv[:, C:].double().T @ mem16.double()).norm() / dw.double().norm()).item() < 1e-5
    # attention_fwd(q, kv[:, :C], kv[:, C:]) with Sq != Sk, attention_bwd(..., dk=dkv[:, :C], dv=dkv[:, C:])
    Sq, Sk = M // B, Mk
    q, kv, do = rnd(M, C).bfloat16(), rnd(Mk * B, 2 * C).bfloat16(), rnd(M, C).bfloat16()
    o, lse = ops.attention_fwd(q, kv[:, :C], kv[:, C:], B, H, Sq, Sk, D, D ** -0.5)
    dq, dk, dv = ops.attention_bwd(q, kv[:, :C], kv[:, C:], o, do, lse, B, H, Sq, Sk, D, D ** -0.5, dk=dkv[:, :C], dv=dkv[:, C:])
    assert dk.data_ptr() == dkv.data_ptr() and dv.data_ptr() == dkv[:, C:].data_ptr()
    # Swin: out_bf16 = h16[:, :C] and out = o16p[:, :C] inside padded buffers
    h16 = torch.zeros(M, C + 64, dtype=torch.bfloat16, device=dev)
    ops.layernorm_fwd(dmem32, torch.ones(C, device=dev), torch.zeros(C, device=dev), out_bf16=h16[:, :C])
    nwin, ws, nH = 4, 2, 4
    qkv = rnd(nwin * ws * ws, 3 * C).bfloat16()
    o16p = torch.zeros(nwin * ws * ws, C + 64, dtype=torch.bfloat16, device=dev)
    ops.swin_attn_fwd(qkv, rnd(nH, ws * ws, ws * ws), nwin, 4, 2, 4, 4, ws, 1, nH, 32 ** -0.5, out=o16p[:, :C])
    torch.cuda.synchronize()
    assert bool((h16[:, C:] == 0).all()) and bool((o16p[:, C:] == 0).all()) and bool(h16[:, :C].float().abs().sum() > 0)
