"""The row-streaming glue kernels (csrc/misc.hip, csrc/spatial.hip) against the fp64 references of tests/glue_ref.py at the shapes
and with the options the modules use: rectangular grids, running gradients, strided views, bf16 sources, repeated ids, rows the
eps clamp holds, and one case per op whose item count needs a second grid-stride round.  Copies, conversions and sums in a
documented order are compared bitwise; every bf16 twin is compared bitwise with ``.bfloat16()`` of the fp32 output of the same
call; every buffer written in part carries a sentinel around the part.  The refusal tests at the end launch nothing."""
import pytest
import torch

import glue_ref as G

pytestmark = pytest.mark.gpu

SENT = -12288.0   # exact in bf16 and far from N(0,1) data


def _randn(dev, seed, *shape, dtype=torch.float32):
    """N(0,1) on the device: from a CPU generator for the small cases, drawn on the device where a copy would dominate."""
    n = 1
    for s in shape:
        n *= s
    if n > (1 << 20):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.randn(*shape, generator=g, device=dev).to(dtype)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(dev)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _col_slice(dev, seed, rows, C, off, extra, dtype=torch.float32):
    """A [rows, C] view of a wider tensor (ld = C + off + extra, starting at column off)."""
    wide = _randn(dev, seed, rows, C + off + extra, dtype=dtype)
    return wide[:, off:off + C]


# ------------------------------------------------------------------------------------------------------------------------------
# bilinear_up_fwd / bilinear_up_bwd          (nn/ftn.py calls them with h != w: the height stays, the width grows 4x a repeat)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.BILINEAR_CASES + [G.BILINEAR_BIG])
def test_bilinear_up_fwd(dev, case):
    from lc2is_amd import ops
    B, h, w, C, S = case
    x = _randn(dev, 100 + h + w, B * h * w, C)
    of, ob = ops.bilinear_up_fwd(x, B, h, w, S, want_bf16=True)
    ref = G.bilinear_up(x, B, h, w, S)
    assert of.shape == ref.shape and of.dtype == torch.float32
    err = (of.double() - ref).abs().max().item()
    print(f"bilinear fwd {case}: max abs err {err:.3e}")
    assert err < 1e-5
    assert torch.equal(ob, of.bfloat16())
    none, ob2 = ops.bilinear_up_fwd(x, B, h, w, S, want_f32=False, want_bf16=True)
    assert none is None and torch.equal(ob2, ob)
    if S == 1:
        assert torch.equal(of, x)


@pytest.mark.parametrize("case", G.BILINEAR_CASES + [G.BILINEAR_BIG])
def test_bilinear_up_bwd(dev, case):
    from lc2is_amd import ops
    B, h, w, C, S = case
    dout = _randn(dev, 200 + h + w, B * h * S * w * S, C)
    din, d16 = ops.bilinear_up_bwd(dout, B, h, w, S, want_bf16=True)
    ref = G.bilinear_up_adjoint(dout, B, h, w, S)
    assert din.shape == ref.shape
    r = _rel(din, ref)
    print(f"bilinear bwd {case}: rel err {r:.3e}")
    assert r < 1e-5
    assert torch.equal(d16, din.bfloat16())
    old = _randn(dev, 300 + h + w, B * h * w, C)
    run = old.clone()
    din2, d16b = ops.bilinear_up_bwd(dout, B, h, w, S, din=run, accumulate=True, want_bf16=True)
    assert din2 is run
    assert _rel(din2, old.double() + ref) < 1e-5
    assert torch.equal(d16b, din2.bfloat16())
    if S == 1:
        assert torch.equal(din, dout)


# ------------------------------------------------------------------------------------------------------------------------------
# sr_gather
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,h,w,C", G.SR_CASES)
def test_sr_gather_and_scatter_are_the_reference_permutation(dev, B, h, w, C):
    from lc2is_amd import ops
    x = _randn(dev, 400 + h + w, B * h * w, C, dtype=torch.bfloat16)
    gth = ops.sr_gather(x, B, h, w)
    assert torch.equal(gth, G.sr_gather(x, B, h, w))
    g = _randn(dev, 401 + h + w, B * h * w // 4, 4 * C, dtype=torch.bfloat16)
    sc = ops.sr_gather(g, B, h, w, scatter=True)
    assert torch.equal(sc, G.sr_scatter(g, B, h, w))
    assert torch.equal(ops.sr_gather(gth, B, h, w, scatter=True), x)


# ------------------------------------------------------------------------------------------------------------------------------
# l2norm_fwd / l2norm_bwd
# ------------------------------------------------------------------------------------------------------------------------------
def _check_l2norm(dev, x, eps, seed):
    from lc2is_amd import ops
    M, C = x.shape
    xf = x.to(dev)
    yf, yb, inv = ops.l2norm_fwd(xf, eps)
    xd = xf.double().requires_grad_(True)
    ref = G.l2norm(xd, eps)
    err = (yf.double() - ref.detach()).abs()
    assert err.max().item() < 1e-6
    # relative to each row's own magnitude: a row the clamp scales down (norm < eps) is not allowed a unit row's absolute error
    assert (err.amax(1) <= 1e-6 * ref.detach().abs().amax(1)).all()
    assert torch.equal(yb, yf.bfloat16())
    want_inv = 1.0 / xd.detach().norm(dim=1).clamp_min(eps)
    assert ((inv.double() - want_inv).abs() <= 1e-6 * want_inv).all()
    none, yb2, inv2 = ops.l2norm_fwd(xf, eps, want_f32=False)
    assert none is None and torch.equal(yb2, yb) and torch.equal(inv2, inv)
    yf3, none, inv3 = ops.l2norm_fwd(xf, eps, want_bf16=False)
    assert none is None and torch.equal(yf3, yf) and torch.equal(inv3, inv)
    dy = _randn(dev, seed, M, C)
    ref.backward(dy.double())
    dx = ops.l2norm_bwd(dy, xf, inv, eps)
    num = (dx.double() - xd.grad).norm(dim=1)
    den = xd.grad.norm(dim=1)
    assert torch.isfinite(dx).all() and (den > 0).all()
    assert (num <= 1e-5 * den).all(), (num / den).max().item()   # every row: the zero row and the clamped rows give dy / eps


@pytest.mark.parametrize("eps", [1e-12, 1e-6])
@pytest.mark.parametrize("C", G.L2NORM_C)
@pytest.mark.parametrize("M", G.L2NORM_M)
def test_l2norm_planted_rows(dev, M, C, eps):
    kinds = G.l2norm_kinds(eps)
    for k0 in range(0, len(kinds), M):   # M = 1 holds one planted row a launch; every kind is run at every (M, C)
        x, _ = G.l2norm_input(M, C, eps, kinds[k0:k0 + M], 500 + M + C + k0)
        _check_l2norm(dev, x, eps, 600 + M + C + k0)


# ------------------------------------------------------------------------------------------------------------------------------
# add_n
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 8), (4,), (G.SP_GRID_ITEMS * 4 + 4 * 1000,)])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_add_n(dev, n, shape):
    from lc2is_amd import ops
    ts = [_randn(dev, 700 + i, *shape) for i in range(n)]
    of, ob = ops.add_n(ts, want_bf16=True)
    assert of.shape == tuple(shape) and torch.equal(of, G.add_n(ts, torch.float32))
    assert torch.equal(ob, of.bfloat16())
    none, ob2 = ops.add_n(ts, want_f32=False, want_bf16=True)
    assert none is None and torch.equal(ob2, ob)


def test_add_n_refuses_one_and_five_addends(dev):
    from lc2is_amd import ops
    ts = [_randn(dev, 710 + i, 8) for i in range(5)]
    with pytest.raises(RuntimeError, match="2 to 4"):
        ops.add_n(ts[:1])
    with pytest.raises(RuntimeError, match="2 to 4"):
        ops.add_n(ts)


# ------------------------------------------------------------------------------------------------------------------------------
# cast_bf16 / transpose_bf16                  (nn/swin.py and nn/hier.py cast into buf[:, :C])
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(7, 20), (2050, 2052)])   # 2050 * 513 float4 items: more than 4096 x 256
def test_cast_bf16_strided_source_and_destination(dev, M, C):
    from lc2is_amd import ops
    assert M * (C // 4) > G.EW_GRID_ITEMS or M < 64
    src = _col_slice(dev, 800 + M, M, C, 4, 8)
    buf = torch.full((M, C + 12), SENT, dtype=torch.bfloat16, device=dev)
    out = ops.cast_bf16(src, buf[:, :C])
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :C], src.bfloat16()) and (buf[:, C:] == SENT).all()
    assert torch.equal(ops.cast_bf16(src), src.bfloat16())


def _special_f32():
    pats = [0x00000000, 0x80000000,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,    # exact midpoints above an even / an odd bf16 mantissa: ties to even
            0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,    # one fp32 ulp to either side of them
            0x7F7FFFFF, 0xFF7FFFFF,                            # the largest finite fp32 rounds to infinity
            0x7F7F7FFF, 0x7F7F8000,                            # the last value that stays finite, the first that does not
            0x7F800000, 0xFF800000,
            0x00000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,   # fp32 denormals (and their midpoints)
            0x00800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF]               # smallest normal; quiet and signalling NaNs
    v = torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int32).view(torch.float32)
    # pack_bf16x2 converts pairs: each value once in the low lane and once in the high lane of a pair
    filler = torch.full_like(v, 1.5)
    return torch.stack([v, filler, filler, v], 1).reshape(-1)


def test_cast_bf16_special_values(dev):
    from lc2is_amd import ops
    row = _special_f32()
    n = row.numel()
    assert n % 4 == 0
    x = torch.randn(3, n, generator=torch.Generator().manual_seed(810))
    x[1] = row
    want = x.bfloat16()                       # the CPU conversion: round to nearest even on the bits, denormals kept
    nan = torch.isnan(x)
    assert nan.sum().item() == 8 and torch.isnan(want[nan]).all() and torch.isinf(want[1]).sum().item() == 10
    wide = torch.zeros(3, n + 8)
    wide[:, 4:4 + n] = x
    buf = torch.full((3, n + 4), SENT, dtype=torch.bfloat16, device=dev)
    ops.cast_bf16(wide.to(dev)[:, 4:4 + n], buf[:, :n])
    got = buf[:, :n].cpu()
    assert torch.isnan(got[nan]).all()
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    assert (buf[:, n:] == SENT).all()
    # the same values through a bf16 twin of another kernel (the pair conversion is shared by every bf16 epilogue)
    a = x.to(dev)
    _, ob = ops.add_n([a, torch.zeros_like(a)], want_bf16=True)   # x + 0 keeps every value but -0, which becomes +0
    keep = ~nan & ~((x == 0) & torch.signbit(x))
    assert torch.equal(_bits(ob.cpu())[keep], _bits(want)[keep]) and torch.isnan(ob.cpu()[nan]).all()


@pytest.mark.parametrize("R,C", [(1, 1), (65, 63), (64, 129)])
def test_transpose_bf16_strided(dev, R, C):
    from lc2is_amd import ops
    src = _col_slice(dev, 820 + R, R, C, 1, 2, dtype=torch.bfloat16)
    buf = torch.full((C, R + 5), SENT, dtype=torch.bfloat16, device=dev)
    ops.transpose_bf16(src, buf[:, :R])
    assert torch.equal(buf[:, :R], src.T) and (buf[:, R:] == SENT).all()
    assert torch.equal(ops.transpose_bf16(src), src.T.contiguous())


# ------------------------------------------------------------------------------------------------------------------------------
# ShadowTable
# ------------------------------------------------------------------------------------------------------------------------------
def _shadow_entry(dev, seed, N, K, kind):
    """-> (entry, checks): kind in 'both' (bf16 + transposed twin, N % 4 == 0), 'wide' (dst with ld > K), 'vec16' / 'vec32' (1-D
    source to bf16 / fp32), 'mat32' (2-D fp32 copy)."""
    if kind in ("vec16", "vec32"):
        src = _randn(dev, seed, K)
        dst = torch.full((K + 4,), SENT, dtype=torch.bfloat16 if kind == "vec16" else torch.float32, device=dev)
        return (src, dst[:K], None), [(dst[:K], src.to(dst.dtype)), (dst[K:], None)]
    src = _randn(dev, seed, N, K)
    if kind == "mat32":
        dst = torch.full((N, K + 4), SENT, device=dev)
        return (src, dst[:, :K], None), [(dst[:, :K], src), (dst[:, K:], None)]
    if kind == "wide":
        dst = torch.full((N + 1, K + 8), SENT, dtype=torch.bfloat16, device=dev)
        return (src, dst[:N, :K], None), [(dst[:N, :K], src.bfloat16()), (dst[:N, K:], None), (dst[N:], None)]
    dst = torch.full((N, K), SENT, dtype=torch.bfloat16, device=dev)
    dstT = torch.full((K + 1, N + 4), SENT, dtype=torch.bfloat16, device=dev)
    return (src, dst, dstT[:K, :N]), [(dst, src.bfloat16()), (dstT[:K, :N], src.bfloat16().T), (dstT[:K, N:], None), (dstT[K:], None)]


def _run_shadow(dev, specs):
    from lc2is_amd import ops
    built = [_shadow_entry(dev, 900 + i, N, K, kind) for i, (N, K, kind) in enumerate(specs)]
    tab = ops.ShadowTable([e for e, _ in built], dev)
    tab.refresh()
    for i, (_, checks) in enumerate(built):
        for got, want in checks:
            if want is None:
                assert (got == SENT).all(), (i, specs[i])
            else:
                assert torch.equal(got, want), (i, specs[i])
    return tab


@pytest.mark.parametrize("spec", [(20, 36, "both"), (1, 4, "wide"), (0, 68, "vec16"), (0, 4, "vec32"), (5, 8, "mat32")])
def test_shadow_table_of_one_entry(dev, spec):
    tab = _run_shadow(dev, [spec])
    assert tab.n == 1


def test_shadow_table_of_forty_mixed_entries(dev):
    """Tile counts 1, 2, 3, 4, 6, 8 ... in no order: the search for the entry that owns a block has to land on every one; N and K
    are not multiples of 64 (K % 4 == 0, and N % 4 == 0 where there is a transposed twin)."""
    shapes = [(4, 4), (68, 60), (132, 200), (12, 68), (64, 64), (100, 36), (8, 260), (196, 4)]
    kinds = ["both", "wide", "vec16", "both", "vec32", "mat32", "both", "wide", "vec16", "both"]
    specs = [(*shapes[i % len(shapes)], kinds[i % len(kinds)]) for i in range(40)]
    odd = [(7, 12, "wide"), (3, 132, "mat32"), (65, 68, "wide")]   # N % 4 != 0 where no twin is asked for
    specs[5], specs[17], specs[29] = odd
    assert len(specs) == 40 and {k for _, _, k in specs} == {"both", "wide", "vec16", "vec32", "mat32"}
    tab = _run_shadow(dev, specs)
    assert tab.n == 40 and tab.total_tiles > 40


# ------------------------------------------------------------------------------------------------------------------------------
# patchify
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,ps,kpad", G.PATCHIFY_CASES)
def test_patchify(dev, B, H, ps, kpad):
    from lc2is_amd import ops
    pix = _randn(dev, 1000 + H, B, 3, H, H)
    cols = ops.patchify(pix, ps, kpad)
    ref = G.patchify(pix, ps, kpad).bfloat16()
    k = 3 * ps * ps
    assert cols.shape == ref.shape and torch.equal(cols, ref)
    assert cols.shape[1] == k or (cols[:, k:] == 0).all()


def test_patchify_refuses_a_rectangular_image(dev):
    from lc2is_amd import ops
    with pytest.raises(RuntimeError):
        ops.patchify(_randn(dev, 1010, 1, 3, 16, 24), 8)


# ------------------------------------------------------------------------------------------------------------------------------
# vit_embed_fwd / vit_embed_bwd               (nn/clip.py passes accumulate=True once the gradients are running)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,C", G.VIT_CASES)
def test_vit_embed(dev, B, P, C):
    from lc2is_amd import ops
    patch = _col_slice(dev, 1100 + P, B * P, C, 4, 4)
    cls, pos = _randn(dev, 1101 + P, C), _randn(dev, 1102 + P, P + 1, C)
    x = ops.vit_embed_fwd(patch, cls, pos, B, P)
    assert torch.equal(x, G.vit_embed_fwd(patch, cls, pos, B, P, torch.float32))
    dx = _randn(dev, 1103 + P, B * (P + 1), C)
    _, _, want_patch = G.vit_embed_bwd(dx, B, P)
    # fresh gradients into buffers that hold junk, with two rows of dpos the op must not touch
    dpos = torch.full((P + 3, C), SENT, device=dev)
    dcls = torch.full((C,), SENT, device=dev)
    dpatch = ops.vit_embed_bwd(dx, dpos, dcls, B, P)
    fp, fc = G.vit_embed_bwd_sequential(dx, B, P)
    assert torch.equal(dpos[:P + 1], fp) and torch.equal(dcls, fc) and (dpos[P + 1:] == SENT).all()
    assert torch.equal(dpatch, want_patch.bfloat16())
    e64p, e64c, _ = G.vit_embed_bwd(dx, B, P)
    assert (dpos[:P + 1].double() - e64p).abs().max().item() < 1e-5 and (dcls.double() - e64c).abs().max().item() < 1e-5
    # running gradients: both non-zero, each old + fresh, and d cls without the old d pos[0]
    dpos0, dcls0 = _randn(dev, 1104 + P, P + 3, C), _randn(dev, 1105 + P, C)
    dpos, dcls = dpos0.clone(), dcls0.clone()
    dpatch2 = ops.vit_embed_bwd(dx, dpos, dcls, B, P, accumulate=True)
    ap, ac = G.vit_embed_bwd_sequential(dx, B, P, dpos0, dcls0)
    assert torch.equal(dpos[:P + 1], ap) and torch.equal(dpos[P + 1:], dpos0[P + 1:])
    assert torch.equal(dcls, ac)
    assert not torch.equal(dcls, ac + dpos0[0]) and (dcls - (fc + dcls0)).abs().max().item() == 0
    assert torch.equal(dpatch2, dpatch)


# ------------------------------------------------------------------------------------------------------------------------------
# text_embed_fwd / text_embed_bwd             (nn/clip.py always passes accumulate=True; prompts repeat ids)
# ------------------------------------------------------------------------------------------------------------------------------
def _text_setup(dev, B, L, V, C, ids):
    tok, pos = _randn(dev, 1200 + C, V, C), _randn(dev, 1201 + C, G.TEXT_POS_ROWS, C)
    dx = _col_slice(dev, 1202 + C, B * L, C, 1, 3)   # ldx = C + 4
    return tok, pos, dx


def _dtok_in_sentinels(dev, dtok0):
    V, C = dtok0.shape
    big = torch.full((V + 2, C), SENT, device=dev)
    big[1:V + 1] = dtok0
    return big, big[1:V + 1]


@pytest.mark.parametrize("B,L,V,C", G.TEXT_CASES)
def test_text_embed(dev, B, L, V, C):
    from lc2is_amd import ops
    ids_c = G.text_ids(B, L, V, 11)
    ids = ids_c.to(dev)
    tok, pos, dx = _text_setup(dev, B, L, V, C, ids)
    x = ops.text_embed_fwd(ids, tok, pos)
    assert torch.equal(x, G.text_embed_fwd(ids, tok, pos, torch.float32))
    dx_c = dx.cpu()
    dtok0, dpos0 = _randn(dev, 1203 + C, V, C), _randn(dev, 1204 + C, G.TEXT_POS_ROWS, C)
    # from a running gradient, accumulate=True as the module calls it
    big, dtok = _dtok_in_sentinels(dev, dtok0)
    dpos = dpos0.clone()
    ops.text_embed_bwd(ids, dx, dtok, dpos, accumulate=True)
    seq = G.text_embed_dtok_sequential(ids_c, dx_c, dtok0.cpu())
    assert torch.equal(dtok.cpu(), seq)
    assert (big[0] == SENT).all() and (big[V + 1] == SENT).all()
    used = torch.zeros(V, dtype=torch.bool)
    used[ids_c.reshape(-1)] = True
    assert torch.equal(_bits(dtok.cpu()[~used]), _bits(dtok0.cpu()[~used]))
    assert torch.equal(dpos.cpu(), G.text_embed_dpos_sequential(dx_c, B, L, dpos0.cpu()))
    assert torch.equal(dpos[L:], dpos0[L:])
    first = dtok.clone()
    # two calls in a row add twice
    ops.text_embed_bwd(ids, dx, dtok, dpos, accumulate=True)
    assert torch.equal(dtok.cpu(), G.text_embed_dtok_sequential(ids_c, dx_c, first.cpu()))
    fresh64, _ = G.text_embed_bwd(ids_c, dx_c, V)
    # two runs give the same bits
    big2, dtok2 = _dtok_in_sentinels(dev, dtok0)
    dposb = dpos0.clone()
    ops.text_embed_bwd(ids, dx, dtok2, dposb, accumulate=True)
    assert torch.equal(dtok2, first) and (big2[0] == SENT).all() and (big2[V + 1] == SENT).all()
    # accumulate=False overwrites rows [0, L) of dpos and no other; dtok still adds
    dposc = dpos0.clone()
    ops.text_embed_bwd(ids, dx, dtok2, dposc, accumulate=False)
    assert torch.equal(dposc.cpu()[:L], G.text_embed_dpos_sequential(dx_c, B, L)) and torch.equal(dposc[L:], dpos0[L:])
    # The bound of a sequential fp32 sum against the exact one, R * 2^-23 * sum_rows |dx| elementwise, has no term for the
    # running gradient: the last add rounds by 2^-24 |dtok0 + sum|, which the bound covers when |dtok0| <= R * sum_rows |dx|.
    # So the running gradient of this check is half the exact fresh one (an earlier step of the same prompts).
    half = (0.5 * fresh64).float()
    _, dtok3 = _dtok_in_sentinels(dev, half.to(dev))
    ops.text_embed_bwd(ids, dx, dtok3, dpos0.clone(), accumulate=True)
    diff = (dtok3.cpu().double() - (half.double() + fresh64)).abs()
    bound = G.dtok_bound(ids_c, dx_c, V)
    print(f"text dtok {(B, L, V, C)}: max err {diff.max().item():.3e}, max bound {bound.max().item():.3e}")
    assert (diff <= bound).all()
    assert torch.equal(dtok3.cpu(), G.text_embed_dtok_sequential(ids_c, dx_c, half))


@pytest.mark.parametrize("B,L,V,C", G.TEXT_CASES)
@pytest.mark.parametrize("bad", [-1, "V", 2 ** 40])
def test_text_embed_ids_out_of_range_use_one_clamped_row(dev, B, L, V, C, bad):
    from lc2is_amd import ops
    bad = V if bad == "V" else bad
    ids_c = G.text_ids(B, L, V, 11)
    R = B * L
    ids_c.view(-1)[R // 2] = bad
    if R >= 3:
        ids_c.view(-1)[R - 1] = bad
    row = 0 if bad < 0 else V - 1
    assert (G.clamp_ids(ids_c, V).view(-1)[R // 2] == row)
    ids = ids_c.to(dev)
    tok, pos, dx = _text_setup(dev, B, L, V, C, ids)
    x = ops.text_embed_fwd(ids, tok, pos)
    assert torch.equal(x, G.text_embed_fwd(ids, tok, pos, torch.float32))
    assert torch.equal(x[R // 2], tok[row] + pos[(R // 2) % L])
    dtok0 = _randn(dev, 1210 + C, V, C)
    big, dtok = _dtok_in_sentinels(dev, dtok0)
    dpos = torch.zeros(G.TEXT_POS_ROWS, C, device=dev)
    ops.text_embed_bwd(ids, dx, dtok, dpos, accumulate=True)
    assert (big[0] == SENT).all() and (big[V + 1] == SENT).all()
    assert torch.equal(dtok.cpu(), G.text_embed_dtok_sequential(ids_c, dx.cpu(), dtok0.cpu()))   # the reference clamps the same way


# ------------------------------------------------------------------------------------------------------------------------------
# rows_copy                                   (nn/clip.py: drop and re-insert the CLS row, fp32 or bf16 stream, one destination)
# ------------------------------------------------------------------------------------------------------------------------------
def _rows_copy_check(dev, src, S_src, src_off, S_dst, dst_off, B, n, mode):
    from lc2is_amd import ops
    C = src.shape[1]
    d32 = torch.full((B * S_dst, C), SENT, device=dev) if mode in ("f32", "both") else None
    d16 = torch.full((B * S_dst, C), SENT, dtype=torch.bfloat16, device=dev) if mode in ("bf16", "both") else None
    ops.rows_copy(src, S_src, src_off, S_dst, dst_off, B, n, dst_f32=d32, dst_bf16=d16)
    for d in (d32, d16):
        if d is not None:
            want = G.rows_copy(src, S_src, src_off, torch.full_like(d, SENT), S_dst, dst_off, B, n)
            assert torch.equal(d, want)
            rest = torch.ones(S_dst, dtype=torch.bool, device=dev)
            rest[dst_off:dst_off + n] = False
            assert (d.view(B, S_dst, C)[:, rest] == SENT).all()
    return d32, d16


@pytest.mark.parametrize("mode", ["f32", "bf16", "both"])
@pytest.mark.parametrize("sdt", [torch.float32, torch.bfloat16])
def test_rows_copy_offsets_and_destinations(dev, sdt, mode):
    S_src, src_off, S_dst, dst_off, n = 19, 2, 23, 5, 11
    B, C = 3, 8
    src = _randn(dev, 1300, B * S_src, C, dtype=sdt)
    _rows_copy_check(dev, src, S_src, src_off, S_dst, dst_off, B, n, mode)


@pytest.mark.parametrize("sdt", [torch.float32, torch.bfloat16])
def test_rows_copy_cls_drop_and_reinsert_at_tower_size(dev, sdt):
    B, n, C = 8, 1024, 768
    assert B * n * C // 4 > G.EW_GRID_ITEMS
    x = _randn(dev, 1310, B * (n + 1), C, dtype=sdt)
    out, _ = _rows_copy_check(dev, x, n + 1, 1, n, 0, B, n, "f32")          # the module's output leaves the stream without CLS
    assert torch.equal(out.view(B, n, C), x.view(B, n + 1, C)[:, 1:].float())
    _, g16 = _rows_copy_check(dev, out, n, 0, n + 1, 1, B, n, "bf16")       # its gradient goes back in below a CLS row
    assert torch.equal(g16.view(B, n + 1, C)[:, 1:], out.view(B, n, C).bfloat16())
    g32, _ = _rows_copy_check(dev, out, n, 0, n + 1, 1, B, n, "f32")
    assert torch.equal(g32.view(B, n + 1, C)[:, 1:], out.view(B, n, C))


@pytest.mark.parametrize("sdt", [torch.float32, torch.bfloat16])
def test_rows_copy_refuses_a_window_past_either_end(dev, sdt):
    from lc2is_amd import ops
    B, C = 2, 8
    src = _randn(dev, 1320, B * 19, C, dtype=sdt)
    dst = torch.full((B * 23, C), SENT, device=dev)
    with pytest.raises(RuntimeError):
        ops.rows_copy(src, 19, 9, 23, 0, B, 11, dst_f32=dst)    # src_off + n = 20 > 19
    with pytest.raises(RuntimeError):
        ops.rows_copy(src, 19, 0, 23, 13, B, 11, dst_f32=dst)   # dst_off + n = 24 > 23
    with pytest.raises(RuntimeError):
        ops.rows_copy(src, 18, 0, 23, 0, B, 11, dst_f32=dst)    # src does not have B * S_src rows
    assert (dst == SENT).all()


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: a tensor that does not have the rows or columns the integer arguments imply is refused before any launch
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    """Any attempt to reach a kernel entry point fails the test: the refusal has to come first."""
    from lc2is_amd import ops

    def boom(name):
        raise AssertionError(f"{name} was about to be launched")
    monkeypatch.setattr(ops, "_fn", boom)
    return ops


def _refused(name, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=name):
        fn(*args, **kw)


def test_spatial_wrappers_refuse_mismatched_rows(dev, no_launch):
    ops = no_launch
    B, h, w, C, S = 2, 4, 6, 8, 2
    x = _randn(dev, 1400, B * h * w, C)
    _refused("x", ops.bilinear_up_fwd, x, B, h, w + 1, S)
    _refused("x", ops.bilinear_up_fwd, x, B + 1, h, w, S)
    _refused("x", ops.bilinear_up_fwd, x.cpu(), B, h, w, S)
    dout = _randn(dev, 1401, B * h * S * w * S, C)
    _refused("dout", ops.bilinear_up_bwd, dout, B, h, w, S + 1)
    _refused("dout", ops.bilinear_up_bwd, dout, B, w + 2, h, S)
    din = torch.full((B * h * w - 1, C), SENT, device=dev)
    _refused("din", ops.bilinear_up_bwd, dout, B, h, w, S, din=din, accumulate=True)
    _refused("din", ops.bilinear_up_bwd, dout, B, h, w, S, din=torch.full((B * h * w, C + 4), SENT, device=dev))
    assert (din == SENT).all()
    x16 = x.bfloat16()
    _refused("x", ops.sr_gather, x16, B, h, w + 2)
    _refused("x", ops.sr_gather, x16, B, h, w, scatter=True)                    # scatter takes B*h*w/4 rows
    g16 = _randn(dev, 1402, B * h * w // 4, 4 * C, dtype=torch.bfloat16)
    _refused("x", ops.sr_gather, g16, B, h, w)                                  # gather takes B*h*w rows
    _refused("x", ops.sr_gather, g16, B, h + 2, w, scatter=True)
    with pytest.raises(RuntimeError, match="even"):
        ops.sr_gather(x16[:B * 3 * w], B, 3, w)
    dst = torch.full((B * h * w, C), SENT, device=dev)
    _refused("src", ops.sr_scatter_add, g16[:-1], dst, B, h, w)
    _refused("dst", ops.sr_scatter_add, g16, dst, B, h, w + 2)
    assert (dst == SENT).all()
    M = 5
    xf, dy = _randn(dev, 1403, M, C), _randn(dev, 1404, M, C)
    _refused("inv", ops.l2norm_bwd, dy, xf, torch.ones(M - 1, device=dev))
    _refused("inv", ops.l2norm_bwd, dy, xf, torch.ones(M + 3, device=dev))
    _refused("inv", ops.l2norm_bwd, dy, xf, torch.ones(M, device=dev, dtype=torch.float64))
    _refused("inv", ops.l2norm_bwd, dy, xf, torch.ones(M))
    _refused("inv", ops.l2norm_bwd, dy, xf, torch.ones(M, 2, device=dev)[:, 0])
    _refused("dy", ops.l2norm_bwd, dy[:M - 1], xf, torch.ones(M, device=dev))


def test_vit_embed_wrappers_refuse_mismatched_tensors(dev, no_launch):
    ops = no_launch
    B, P, C = 2, 5, 8
    patch, cls, pos = _randn(dev, 1410, B * P, C), _randn(dev, 1411, C), _randn(dev, 1412, P + 1, C)
    _refused("patch", ops.vit_embed_fwd, patch, cls, pos, B, P + 1)
    _refused("patch", ops.vit_embed_fwd, patch[:-1], cls, pos, B, P)
    _refused("pos", ops.vit_embed_fwd, patch, cls, pos[:P], B, P)                                     # fewer than P + 1 rows
    _refused("pos", ops.vit_embed_fwd, patch, cls, _randn(dev, 1413, P + 1, C + 4)[:, :C], B, P)      # leading dimension != C
    _refused("pos", ops.vit_embed_fwd, patch, cls, _randn(dev, 1413, P + 1, C + 4), B, P)
    _refused("pos", ops.vit_embed_fwd, patch, cls, pos.double(), B, P)
    _refused("pos", ops.vit_embed_fwd, patch, cls, pos.cpu(), B, P)
    _refused("cls", ops.vit_embed_fwd, patch, cls[:C - 4], pos, B, P)
    _refused("cls", ops.vit_embed_fwd, patch, cls.bfloat16(), pos, B, P)
    _refused("cls", ops.vit_embed_fwd, patch, cls.cpu(), pos, B, P)
    _refused("cls", ops.vit_embed_fwd, patch, _randn(dev, 1414, C, 2)[:, 0], pos, B, P)
    dx = _randn(dev, 1415, B * (P + 1), C)
    dpos, dcls = torch.full((P + 1, C), SENT, device=dev), torch.full((C,), SENT, device=dev)
    _refused("dx", ops.vit_embed_bwd, dx, dpos, dcls, B, P + 1)
    _refused("dx", ops.vit_embed_bwd, dx[:B * P], dpos, dcls, B, P)
    _refused("dpos", ops.vit_embed_bwd, dx, dpos[:P], dcls, B, P, accumulate=True)
    _refused("dpos", ops.vit_embed_bwd, dx, torch.full((P + 1, C + 4), SENT, device=dev)[:, :C], dcls, B, P)
    _refused("dpos", ops.vit_embed_bwd, dx, dpos.double(), dcls, B, P)
    _refused("dpos", ops.vit_embed_bwd, dx, dpos.cpu(), dcls, B, P)
    _refused("dcls", ops.vit_embed_bwd, dx, dpos, dcls[:C - 4], B, P)
    _refused("dcls", ops.vit_embed_bwd, dx, dpos, dcls.double(), B, P)
    _refused("dcls", ops.vit_embed_bwd, dx, dpos, dcls.cpu(), B, P)
    assert (dpos == SENT).all() and (dcls == SENT).all()


def test_text_embed_wrappers_refuse_mismatched_tensors(dev, no_launch):
    ops = no_launch
    B, L, V, C = 2, 7, 9, 8
    ids = G.text_ids(B, L, V, 3).to(dev)
    tok, pos = _randn(dev, 1420, V, C), _randn(dev, 1421, G.TEXT_POS_ROWS, C)
    _refused("pos", ops.text_embed_fwd, ids, tok, pos[:L - 1])                                        # fewer than L rows
    _refused("pos", ops.text_embed_fwd, ids, tok, _randn(dev, 1422, L, C + 4)[:, :C])                 # leading dimension != C
    _refused("pos", ops.text_embed_fwd, ids, tok, _randn(dev, 1422, L, C + 4))
    _refused("pos", ops.text_embed_fwd, ids, tok, pos.double())
    _refused("pos", ops.text_embed_fwd, ids, tok, pos.cpu())
    _refused("tok", ops.text_embed_fwd, ids, _randn(dev, 1423, V, C + 4)[:, :C], pos)
    _refused("tok", ops.text_embed_fwd, ids, tok.bfloat16(), pos)
    _refused("tok", ops.text_embed_fwd, ids, tok.cpu(), pos)
    wide_ids = torch.zeros(B, L + 3, dtype=torch.int64, device=dev)
    _refused("input_ids", ops.text_embed_fwd, wide_ids[:, :L], tok, pos)
    dx = _randn(dev, 1424, B * L, C)
    dtok, dpos = torch.full((V, C), SENT, device=dev), torch.full((G.TEXT_POS_ROWS, C), SENT, device=dev)
    _refused("input_ids", ops.text_embed_bwd, wide_ids[:, :L], dx, dtok, dpos, accumulate=True)
    _refused("input_ids", ops.text_embed_bwd, wide_ids.t()[:L].t(), dx, dtok, dpos)
    _refused("input_ids", ops.text_embed_bwd, ids.int(), dx, dtok, dpos)
    _refused("dx", ops.text_embed_bwd, ids, dx[:-1], dtok, dpos, accumulate=True)
    _refused("dx", ops.text_embed_bwd, ids[:1], dx, dtok, dpos)
    _refused("dx", ops.text_embed_bwd, ids, dx.cpu(), dtok, dpos)
    _refused("dtok", ops.text_embed_bwd, ids, dx, dtok.double(), dpos)
    _refused("dtok", ops.text_embed_bwd, ids, dx, dtok.bfloat16(), dpos)
    _refused("dtok", ops.text_embed_bwd, ids, dx, dtok.cpu(), dpos)
    _refused("dtok", ops.text_embed_bwd, ids, dx, torch.full((V, C + 4), SENT, device=dev)[:, :C], dpos)
    _refused("dtok", ops.text_embed_bwd, ids, dx, torch.full((V, C + 4), SENT, device=dev), dpos)
    _refused("dtok", ops.text_embed_bwd, ids, dx, dtok.reshape(-1), dpos)
    _refused("dpos", ops.text_embed_bwd, ids, dx, dtok, dpos[:L - 1], accumulate=True)
    _refused("dpos", ops.text_embed_bwd, ids, dx, dtok, dpos.double())
    _refused("dpos", ops.text_embed_bwd, ids, dx, dtok, dpos.cpu())
    _refused("dpos", ops.text_embed_bwd, ids, dx, dtok, torch.full((L, C + 4), SENT, device=dev)[:, :C])
    _refused("dpos", ops.text_embed_bwd, ids, dx, dtok, dpos[:, :C - 4])
    assert (dtok == SENT).all() and (dpos == SENT).all()


def test_the_calls_the_modules_make_are_not_refused(dev):
    """The shapes of the call sites, through the real entry points: a rectangular FTN grid, running ViT and text gradients with a
    77-row position table, a cast into buf[:, :C]."""
    from lc2is_amd import ops
    B, h = 2, 4
    x = _randn(dev, 1430, B * h * 16, 8)
    of, ob = ops.bilinear_up_fwd(x, B, h, 16, 2, want_bf16=True)
    g, _ = ops.bilinear_up_bwd(of, B, h, 16, 2)
    assert g.shape == x.shape and ob.shape == of.shape
    ids = G.text_ids(3, 9, 12, 4).to(dev)
    tok, pos = _randn(dev, 1431, 12, 8), _randn(dev, 1432, G.TEXT_POS_ROWS, 8)
    xe = ops.text_embed_fwd(ids, tok, pos)
    gt, gp = torch.zeros_like(tok), torch.zeros_like(pos)
    ops.text_embed_bwd(ids, xe, gt, gp, accumulate=True)
    assert gp[9:].abs().sum().item() == 0 and gp[:9].abs().sum().item() > 0
