"""Geometric views on the MI355X (lc2is_geo_params, lc2is_geo_apply, data.GeometricAugment) against tests/geo_ref.py: switches,
translations, label cells, weights and every copy bit for bit (the map is held as integers); the matrix within one Q16 unit; warped
pixels within a bound derived from the fp32 roundings of the three lerps.

The paths of geo_apply_kernel and where each is hit: the copy stream (rows with flags 0 and bad rows; S = 8 is the smallest side the
library takes: one block whose lanes past S * S / 4 = 16 quads leave) and the mapped tile (every other row; S = 8: one 32 x 32 tile
of which 8 x 8 is inside; S = 68 and 132: several tiles per axis with a ragged last one), each for pixel blocks and for label-cell
blocks (L = 2 .. 132: less than one block of 256 cells up to 69 blocks).  Both sides of the copy / mapped switch run in the launches
of test_apply_matches_the_restatement that hold row 5, next to two mapped rows.  A mapped tile takes its taps from the STAGED source
box when the box holds at most 4096 words per channel and DIRECTLY from global memory otherwise (geo_ref.tile_box restates the rule):
up to S = 64 the whole image is 4096 words, so every mapped row at S = 8, 12 and 20 is staged; S = 68 is the smallest side at which
the direct form can occur, and row 24 of the hand-written rows makes it occur there (tile (0, 0): a 68 x 68 box); at S = 132 rows 9
and 18 (scale 0.25) and row 24 take it on their inner tiles while their outer tiles and every other row are staged.  Asserted from
the restatement in test_apply_matches_the_restatement."""
import functools

import numpy as np
import pytest
import torch

import geo_ref as GR

pytestmark = pytest.mark.gpu

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
SEED = 1234
ONE = GR.ONE


def pixel_tol(A):
    """Absolute.  Every tap the kernel uses is the restatement's by construction (integer indices, exact fractions), so the difference
    is fp32 rounding alone: a lerp a + f (b - a) is three roundings (difference, product, sum) of magnitudes <= 2 A, three lerps make
    an output, nested twice, so about 12 roundings of 2^-24 * A reach it; times the margin of 4 that test_gpu_strong.py takes:
    48 * 2^-24 * A, A = max |input|, |fill| (2.9e-6 A).  A wrong convention (align_corners=True) or a tap shifted by one pixel is off
    by more than 1e-2 on the noise input (asserted below from the reference alone)."""
    return 48.0 * 2.0 ** -24 * A


def _geo(**kw):
    from lc2is_amd.data import GeometricAugment
    kw.setdefault("seed", SEED)
    return GeometricAugment(image_mean=MEAN, image_std=STD, **kw)


def _t(a, dev, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np_bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. params ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _keys():
    rng = np.random.default_rng(5)
    return np.concatenate([np.arange(2048), rng.integers(0, 2 ** 62, 2046), [2 ** 62, 2 ** 62 - 1]]).astype(np.int64)


@pytest.mark.parametrize("epoch", [0, 1, 77, 2 ** 31 - 1])
def test_params_match_the_restatement(dev, epoch):
    """4096 keys (small ones and keys up to 2^62) at the LIMITS of the config (180 degrees, scale 0.25 .. 4, shear 45 degrees, half the
    side: the library accepts them and |m| passes 4 * 65536).  Flags, tx, ty and words 12 .. 15 equal; theta, phi, fx, fy equal too
    (one rounding, restated exactly); m within 1 Q16 unit: about 8 fp32 roundings (sinf, cosf, tanf, the quotient, two products, a
    sum) of magnitudes <= 8 * 65536 = 2^19 are under 8 * 2^-24 * 2^19 = 0.25 unit, then the rounding to an integer; the recorded fp32
    fields within 1e-5 * max(1, |x|)."""
    from lc2is_amd import ops
    geo = _geo(prob=0.5, rotate_deg=180.0, scale_range=(0.25, 4.0), shear_deg=45.0, translate=0.5, flip_prob=0.5)
    keys = _keys()
    got = ops.geo_params(_t(keys, dev), _t([epoch], dev, torch.int32), geo.config).cpu().numpy()
    ref = GR.draw_params(GR.config_dict(geo.config), keys, epoch)
    assert got.shape == (4096, GR.P_WORDS) and (got[:, 12:] == 0).all()
    assert np.array_equal(got[:, GR.FLAGS], ref["flags"])
    assert np.array_equal(got[:, GR.T0], ref["tx"]) and np.array_equal(got[:, GR.T0 + 1], ref["ty"])
    dm = np.abs(got[:, GR.M0:GR.M0 + 4].astype(np.int64) - ref["m"])
    f = got.view(np.float32).astype(np.float64)
    worst = {name: (np.abs(f[:, GR.REC0 + j] - ref[name].astype(np.float64)) / np.maximum(1.0, np.abs(ref[name].astype(np.float64)))).max()
             for j, name in enumerate(GR.REC_NAMES)}
    exact = {name: np.array_equal(got[:, GR.REC0 + j], ref[name].view(np.int32)) for j, name in enumerate(GR.REC_NAMES)}
    print(f"geo_params epoch {epoch}: rows whose m differs from the float64 rounding: {100.0 * (dm.max(axis=1) > 0).mean():.2f} % "
          f"(max {dm.max()} unit); recorded fields: scaled errors {worst}, bit-equal {exact}; max |m| {np.abs(got[:, 1:5]).max()}")
    assert dm.max() <= 1
    assert all(v <= 1e-5 for v in worst.values()), worst
    assert all(exact[name] for name in ("theta", "phi", "fx", "fy")), exact
    # the draw is not trivial: every switch combination, entries past 4.0 (scale 0.25 with a shear) and shifts near half the side
    assert set(ref["flags"].tolist()) == {0, 1, 2, 3} and np.abs(ref["m"]).max() > 4 * ONE and np.abs(ref["tx"]).max() > 0.49 * ONE
    assert 0.45 < ref["warp"].mean() < 0.55 and 0.45 < ref["flip"].mean() < 0.55


# ---- 2. apply on hand-written rows ----------------------------------------------------------------------------------------------
EXACT = {"identity": (GR.WARP, (ONE, 0, 0, ONE), (0, 0)), "flip": (GR.FLIP, (-ONE, 0, 0, ONE), (0, 0)),
         "quarter turn": (GR.WARP, (0, -ONE, ONE, 0), (0, 0)), "shift": (GR.WARP, (ONE, 0, 0, ONE), (16384, 0)),
         "flipped quarter turn": (GR.WARP | GR.FLIP, (0, -ONE, -ONE, 0), (0, 0)), "copy": (0, (0, -ONE, ONE, 0), (777, -777))}


def _exact_want(name, a, outside):
    """The torch slicing / flip / rot90 that an exact row is; a: [..., n, n] tensor; outside: a tensor broadcastable to a."""
    if name in ("identity", "copy"):
        return a
    if name == "flip":
        return a.flip(-1)
    if name == "quarter turn":
        return torch.rot90(a, 1, (-2, -1))
    if name == "flipped quarter turn":                                          # the flip acts on the OUTPUT's x: M = R * diag(-1, 1)
        return torch.rot90(a, 1, (-2, -1)).flip(-1)
    n = a.shape[-1]
    q = (n + 2) // 4                                                            # floor(x + n / 4 + 1 / 2) - x: n / 4 where n % 4 == 0
    return torch.cat([a[..., q:], outside.expand(*a.shape[:-1], q).to(a.dtype)], dim=-1)


@functools.lru_cache(maxsize=None)
def _hand_rows():
    """27 rows: the six exact ones; rotations of 10, 45 and 170 degrees, scale 0.25 and 4, shear 45 degrees, translations of +-0.5, and
    a mixed one - each plain and flipped; row 24 with |m| at the limit 8 * 65536 and |t| at the limit 65536 (still mapped: a zoom-out
    by 8 shifted so that output tile (0, 0) looks at the whole image), row 25 with |t| at the limit alone; FLIP with a matrix that is no
    flip (the bits are not told apart: the map is applied)."""
    rows = [GR.make_row(f, m, t) for f, m, t in EXACT.values()]
    for flip in (False, True):
        rows += [GR.affine_row(10.0, flip=flip), GR.affine_row(45.0, flip=flip), GR.affine_row(170.0, flip=flip), GR.affine_row(0.0, 0.25, flip=flip),
                 GR.affine_row(0.0, 4.0, flip=flip), GR.affine_row(0.0, 1.0, 45.0, flip=flip), GR.affine_row(0.0, 1.0, 0.0, 0.5, -0.5, flip=flip),
                 GR.affine_row(0.0, 1.0, 0.0, -0.5, 0.5, flip=flip), GR.affine_row(-33.0, 0.8, 12.0, 0.07, -0.11, flip=flip)]
    rows += [GR.make_row(GR.WARP, (GR.MAX_M, 0, 0, GR.MAX_M), (GR.MAX_T, GR.MAX_T)), GR.make_row(GR.WARP, (ONE, 0, 0, ONE), (-GR.MAX_T, GR.MAX_T)),
             GR.make_row(GR.FLIP, (30000, 50000, -50000, 30000), (1000, 2000))]
    assert len(rows) == 27 and all(GR.row_is_mapped(r) for r in rows[:5] + rows[6:]) and not GR.row_is_mapped(rows[5])
    return np.stack(rows)


def _plant(x):
    """NaN, +-inf and NaNs with payloads, in corners and in the interior: next to taps that exact rows select."""
    x = x.copy()
    S = x.shape[-1]
    x[0, 0, 0, 0], x[0, 1, 5, 7], x[0, 2, S - 1, S - 1], x[1, 0, 0, S - 1] = np.nan, np.inf, -np.inf, np.nan
    x.view(np.int32)[0, 0, 1, 1] = 0x7FC12345
    x.view(np.int32)[2, 1, 2, 2] = -4194303                                    # 0xFFC00001: a negative NaN with a payload
    return x


@functools.lru_cache(maxsize=None)
def _inputs(S, L):
    """B = 3: noise pixels, labels 0 .. 149 with some ignore cells, weights in (0, 1); and the same with non-finite values planted."""
    rng = np.random.default_rng(1000 * S + L)
    px = rng.standard_normal((3, 3, S, S)).astype(np.float32)
    lab = rng.integers(0, 150, (3, L, L)).astype(np.int64)
    lab[rng.random((3, L, L)) < 0.1] = -100
    pw = rng.random((3, L, L)).astype(np.float32)
    pw_planted = pw.copy()
    pw_planted[0, 0, 0], pw_planted[1, L - 1, L - 1] = np.nan, np.inf
    pw_planted.view(np.int32)[2, 1, 1] = 0x7FC54321
    return px, lab, pw, _plant(px), pw_planted


def _check_launch(ops, cfg, dev, px, lab, pw, pick, names=None, worst=None):
    """One launch of three rows against the restatement: labels and weights equal (weights as bits), copies bit for bit, warped
    pixels within pixel_tol; with `names` the exact rows are also held to the torch op they are, bit for bit."""
    fill, ign = [float(v) for v in cfg.fill], int(cfg.ignore_index)
    d = lambda a, dt=None: None if a is None else torch.from_numpy(a).to(dev)
    dpx, dlab, dpw = d(px), d(lab), d(pw)
    gpx, glab, gpw = ops.geo_apply((dpx, dlab, dpw), torch.from_numpy(pick.copy()).to(dev), cfg)
    rpx, rlab, rpw = GR.apply_ref(px, lab, pw, pick, fill, ign)
    assert (glab is None) == (lab is None) and (gpw is None) == (pw is None)
    if lab is not None:
        assert np.array_equal(glab.cpu().numpy(), rlab)
    if pw is not None:
        assert np.array_equal(_np_bits(gpw.cpu().numpy()), _np_bits(rpw))
    got = gpx.cpu().numpy()
    A = max(float(np.nanmax(np.abs(np.where(np.isfinite(px), px, 0.0)))), max(abs(v) for v in fill))
    for b in range(3):
        if not GR.row_is_mapped(pick[b]):
            assert np.array_equal(_np_bits(got[b]), _np_bits(px[b]))
            continue
        if names is not None:
            want = _exact_want(names[b], dpx[b], torch.tensor(fill, device=dev).view(3, 1, 1))
            assert _same_bits(gpx[b], want), names[b]
            if lab is not None:
                assert torch.equal(glab[b], _exact_want(names[b], dlab[b], torch.tensor(ign, device=dev)))
            if pw is not None:
                assert _same_bits(gpw[b], _exact_want(names[b], dpw[b], torch.tensor(0.0, device=dev)))
            assert np.array_equal(_np_bits(got[b]), _np_bits(rpx[b].astype(np.float32))), names[b]
            continue
        err = np.abs(got[b].astype(np.float64) - rpx[b]).max()
        if worst is not None:
            worst.append(err / A)
        assert err <= pixel_tol(A), (pick[b, :7], err, pixel_tol(A))


@pytest.mark.parametrize("S,L", [(8, 8), (8, 2), (12, 6), (20, 20), (20, 5), (68, 68), (68, 17), (132, 132), (132, 33)])
def test_apply_matches_the_restatement(dev, S, L):
    """Hand-written rows, three different ones per launch (B = 3), labels and weights of L = S, L = S / 4 and one r = S / L = 2 that is
    no multiple of 4.  Row 5 (flags 0 with a quarter turn in its words: the copy) sits next to mapped rows in the first launch and in
    launch j = 5: both sides of the block-uniform switch in one grid, from S = 8 on.  S = 8 and 68 run with a non-zero fill and ignore_index = 255."""
    from lc2is_amd import ops
    special = S in (8, 68)
    cfg = _geo(fill=(255.0, 0.0, 100.0), ignore_index=255).config if special else _geo().config
    assert (max(abs(float(v)) for v in cfg.fill) > 1.0) == special
    px, lab, pw, px_planted, pw_planted = _inputs(S, L)
    rows, names = _hand_rows(), list(EXACT)
    # the exact rows on the planted input: bit-equal to the torch ops, whatever lies next to a selected tap
    for pick in ([0, 1, 5], [2, 3, 4]):
        _check_launch(ops, cfg, dev, px_planted, lab, pw_planted, rows[pick], names=[names[i] for i in pick])
    worst = []
    for j in range(9):
        _check_launch(ops, cfg, dev, px, lab, pw, rows[[j, j + 9, j + 18]], worst=worst)
    print(f"geo_apply S={S} L={L}: max |kernel - fp64| / A over {len(worst)} warped rows = {max(worst):.2e} (bound {pixel_tol(1.0):.2e})")
    if (S, L) == (20, 5):                                                       # a map that is not given is neither read nor made
        for lab_, pw_ in ((None, pw), (lab, None), (None, None)):
            _check_launch(ops, cfg, dev, px, lab_, pw_, rows[[7, 5, 14]])
    # what the bound tells apart, from the reference alone: align_corners=True, and a tap shifted by one pixel
    import torch.nn.functional as F
    row = rows[14]                                                              # (a map WITH a translation: without one the two conventions agree)
    ref = GR.warp_pixels(px[0], row, (0.0,) * 3)
    theta = torch.from_numpy(GR.theta_of(row))[None]
    wrong = F.grid_sample(torch.from_numpy(px[0].astype(np.float64))[None], F.affine_grid(theta, (1, 3, S, S), align_corners=True),
                          "bilinear", "zeros", align_corners=True)[0].numpy()
    assert np.abs(wrong - ref).max() > 1e-2 and np.abs(GR.warp_pixels(np.roll(px[0], 1, axis=-1), row, (0.0,) * 3) - ref).max() > 1e-2
    # which form the tiles take (see the module docstring): nothing direct up to S = 64; row 24 at S = 68; rows 9, 18, 24 at S = 132
    direct = {i: GR.direct_tiles(rows[i], S) for i in range(27) if i != 5}
    if S <= 64:
        assert not any(direct.values())
    else:
        assert direct[24] and not direct[7] and not direct[14] and (direct[24] == [(0, 0)] if S == 68 else (direct[9] and direct[18]))
        assert all(len(v) < ((S + 31) // 32) ** 2 for v in direct.values())       # and every row has staged tiles too
    # out-of-frame cells exist in this set and carry ignore_index / weight 0 (zoomed out: scale 0.25)
    ys, xs, inside = GR.cell_index(rows[9], L)
    assert (~inside).any() and (inside.any() or L == 2)                          # (two cells a side, zoomed out by 4: all four look outside)


# ---- 3. bad rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 68])
def test_bad_rows_render_the_copy_bits_included(dev, S):
    from lc2is_amd import ops
    cfg = _geo().config
    L = S // 4
    _, lab, _, px, pw = _inputs(S, L)
    dpx, dlab, dpw = (torch.from_numpy(a[:1].copy()).to(dev) for a in (px, lab, pw))
    turn = (0, -ONE, ONE, 0)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    bad = [GR.make_row(GR.WARP, (GR.MAX_M + 1, 0, 0, ONE)), GR.make_row(GR.WARP, (ONE, 0, -GR.MAX_M - 1, ONE)),
           GR.make_row(GR.WARP, turn, (GR.MAX_T + 1, 0)), GR.make_row(GR.WARP, turn, (0, -GR.MAX_T - 1)),
           GR.make_row(4 | GR.WARP, turn), GR.make_row((1 << 30) | GR.FLIP, turn), GR.make_row(4, turn), GR.make_row(0, turn, (5, 5)),
           np.full(GR.P_WORDS, -1, np.int32), np.full(GR.P_WORDS, lo, np.int32), np.full(GR.P_WORDS, hi, np.int32)]
    for word in range(7):                                                       # INT32_MIN / INT32_MAX in every word the kernel reads
        for v in (lo, hi):
            row = GR.make_row(GR.WARP, turn)
            row[word] = v
            bad.append(row)
    for row in bad:
        assert not GR.row_is_mapped(row)
        out = ops.geo_apply((dpx, dlab, dpw), torch.from_numpy(row[None].copy()).to(dev), cfg)
        assert _same_bits(out[0], dpx) and torch.equal(out[1], dlab) and _same_bits(out[2], dpw), row[:7]
    # and the neighbours inside the limits are mapped: the quarter turn moves the sample
    out = ops.geo_apply((dpx, dlab, dpw), torch.from_numpy(GR.make_row(GR.WARP, turn)[None].copy()).to(dev), cfg)
    assert _same_bits(out[0], torch.rot90(dpx, 1, (-2, -1))) and torch.equal(out[1], torch.rot90(dlab, 1, (-2, -1)))


# ---- 4. reproducibility, batch independence, views --------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes_and_a_sample_does_not_depend_on_its_batch(dev):
    from lc2is_amd import ops
    S, L = 68, 17
    geo = _geo(prob=0.7, flip_prob=0.5, translate=0.2)
    rows = _hand_rows()
    rng = np.random.default_rng(9)
    px = torch.from_numpy(rng.standard_normal((5, 3, S, S)).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rng.integers(0, 150, (5, L, L))).to(dev)
    pw = torch.from_numpy(rng.random((5, L, L)).astype(np.float32)).to(dev)
    for pick in ([5, 1, 7, 14, 23], [4, 20, 26, 9, 0]):                         # row 2: 45 degrees; the FLIP row with a rotation in it
        table = torch.from_numpy(rows[pick]).to(dev)
        a = ops.geo_apply((px, lab, pw), table, geo.config)
        b = ops.geo_apply((px, lab, pw), table, geo.config)
        assert all(_same_bits(u, v) for u, v in zip(a, b))
        one = ops.geo_apply((px[2:3], lab[2:3], pw[2:3]), table[2:3].contiguous(), geo.config)      # B = 1 against row 2 of B = 5
        assert all(_same_bits(u[0], v[2]) for u, v in zip(one, a))
    keys = [7, 8, 9, 10, 11]
    full = geo((px, lab, pw), keys, 2)
    alone = geo((px[2:3], lab[2:3], pw[2:3]), keys[2:3], 2)
    assert all(_same_bits(u[0], v[2]) for u, v in zip(alone, full))


def test_out_and_views(dev):
    """Preallocated outputs are written and returned; every overlapping out is refused; a batch slice (contiguous, offset) is HANDLED;
    a strided, permuted or misaligned view is REFUSED (RuntimeError), never copied silently."""
    S, L = 20, 5
    geo = _geo(translate=0.1, flip_prob=0.5)
    rng = np.random.default_rng(4)
    big = torch.from_numpy(rng.standard_normal((9, 3, S, S)).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rng.integers(0, 150, (9, L, L))).to(dev)
    pw = torch.from_numpy(rng.random((9, L, L)).astype(np.float32)).to(dev)
    keys = list(range(9))
    want = geo((big, lab, pw), keys, 1)
    assert not _same_bits(want[0], big)
    out = (torch.empty_like(big), torch.empty_like(lab), torch.empty_like(pw))
    got = geo((big, lab, pw), keys, 1, out=out)
    assert all(g is o for g, o in zip(got, out)) and all(_same_bits(g, w) for g, w in zip(got, want))
    view, lab_v, pw_v = geo.view({"pixel_values": big, "input_ids": keys}, lab, pw, keys, 1)
    assert view["input_ids"] is keys and _same_bits(view["pixel_values"], want[0]) and torch.equal(lab_v, want[1])
    only_px = geo((big, None, None), keys, 1)
    assert only_px[1] is None and only_px[2] is None and _same_bits(only_px[0], want[0])
    part = geo((big[3:7], lab[3:7], pw[3:7]), keys[3:7], 1)                     # an offset view of the batch
    assert all(_same_bits(p, w[3:7]) for p, w in zip(part, want))
    # overlapping outputs: in place, half, the last 16 (8, 4) bytes - pixels, labels, weights; adjacent is fine
    for which, src, unit in ((0, big, 4), (1, lab, 2), (2, pw, 1)):
        n = src.numel()
        buf = torch.zeros(2 * n, dtype=src.dtype, device=dev)
        x_in = buf[:n].view_as(src).copy_(src)
        batch = [big, lab, pw]
        batch[which] = x_in
        for bad_out in (x_in, buf[n // 2:n // 2 + n].view_as(src), buf[n - unit:2 * n - unit].view_as(src)):
            outs = [None, None, None]
            outs[which] = bad_out
            with pytest.raises(RuntimeError, match="overlap"):
                geo(tuple(batch), keys, 1, out=tuple(outs))
        outs = [None, None, None]
        outs[which] = buf[n:].view_as(src)
        got = geo(tuple(batch), keys, 1, out=tuple(outs))
        assert got[which] is outs[which] and all(_same_bits(g, w) for g, w in zip(got, want))
    wide = torch.zeros(2, 3, S, S + 4, device=dev)
    flat = torch.zeros(2 * 3 * S * S + 1, device=dev)
    for bad in (wide[..., :S], torch.zeros(2, S, S, 3, device=dev).permute(0, 3, 1, 2), big[::2][:2], flat[1:].view(2, 3, S, S)):
        with pytest.raises(RuntimeError):
            geo((bad, None, None), keys[:2], 1)
    with pytest.raises(RuntimeError):
        geo((big[:2], torch.zeros(2, L, L + 1, dtype=torch.int64, device=dev)[..., :L], None), keys[:2], 1)
    with pytest.raises(RuntimeError):
        geo((big[:2], None, torch.zeros(2, L, L, 2, device=dev)[..., 0]), keys[:2], 1)
    with pytest.raises(RuntimeError):
        geo((big, lab, pw), keys, 1, out=(torch.empty(9, 3, S, S + 4, device=dev)[..., :S], None, None))


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
def _check_class_against_the_table(geo, batch_np, keys, epoch, got):
    px, lab, pw = batch_np
    rows = geo.last_params.cpu().numpy()
    want = GR.draw_params(GR.config_dict(geo.config), keys, epoch)
    assert np.array_equal(rows[:, GR.FLAGS], want["flags"]) and np.array_equal(rows[:, GR.T0], want["tx"])
    assert np.abs(rows[:, GR.M0:GR.M0 + 4].astype(np.int64) - want["m"]).max() <= 1
    rpx, rlab, rpw = GR.apply_ref(px, lab, pw, rows, [float(v) for v in geo.config.fill], int(geo.config.ignore_index))
    assert np.array_equal(got[1].cpu().numpy(), rlab) and np.array_equal(_np_bits(got[2].cpu().numpy()), _np_bits(rpw))
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - rpx).reshape(len(keys), -1).max(axis=1)
    A = max(float(np.abs(px).max()), max(abs(float(v)) for v in geo.config.fill))
    assert (err <= pixel_tol(A)).all(), (epoch, err, pixel_tol(A))
    return rows


def test_the_pair_replays_from_a_graph(dev):
    """Capture both launches; write a new value into the device epoch tensor; the replay equals the restatement for the new epoch and
    the eager call's bits; the tables differ between epochs."""
    S, L = 20, 5
    kw = dict(prob=0.7, rotate_deg=40.0, shear_deg=10.0, translate=0.2, flip_prob=0.4)
    geo = _geo(**kw)
    rng = np.random.default_rng(6)
    batch_np = (rng.standard_normal((6, 3, S, S)).astype(np.float32), rng.integers(0, 150, (6, L, L)).astype(np.int64),
                rng.random((6, L, L)).astype(np.float32))
    batch = tuple(torch.from_numpy(a).to(dev) for a in batch_np)
    keys_np = [21, 22, 23, 24, 25, 26]
    keys = _t(keys_np, dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = tuple(torch.empty_like(t) for t in batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        geo(batch, keys, epoch, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        geo(batch, keys, epoch, out=out)
    seen = []
    for e in (0, 3, 77):
        epoch.fill_(e)
        graph.replay()
        rows = _check_class_against_the_table(geo, batch_np, keys_np, e, out)
        eager = _geo(**kw)(batch, keys, epoch)
        assert all(_same_bits(a, b) for a, b in zip(out, eager))
        seen.append(rows[:, :7].tolist())
    assert seen[0] != seen[1] and seen[1] != seen[2] and seen[0] != seen[2]


# ---- 6. the class ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 68])
def test_the_class_matches_the_restatement_given_its_device_table(dev, S):
    """The launch pair through GeometricAugment, B = 6; the table is read back (here, not by the class)."""
    L = S // 4
    geo = _geo(prob=0.6, rotate_deg=60.0, scale_range=(0.5, 2.0), shear_deg=20.0, translate=0.25, flip_prob=0.5, fill=(0.0, 128.0, 255.0),
               ignore_index=255)
    rng = np.random.default_rng(S)
    batch_np = (rng.standard_normal((6, 3, S, S)).astype(np.float32), rng.integers(0, 150, (6, L, L)).astype(np.int64),
                rng.random((6, L, L)).astype(np.float32))
    keys = [3, 2 ** 50 + 1, 9, 10, 11, 12]
    got = geo(tuple(torch.from_numpy(a).to(dev) for a in batch_np), keys, 3)
    rows = _check_class_against_the_table(geo, batch_np, keys, 3, got)
    assert set(rows[:, GR.FLAGS].tolist()) == {0, 1, 2, 3}, rows[:, GR.FLAGS]           # copy, warp, flip and both in one batch


# ---- 7. the recipe --------------------------------------------------------------------------------------------------------------
def test_geometric_views_feed_the_train_step(dev):
    """Weak view -> the teacher's pseudo-labels -> strong view -> geo.view with the pseudo-labels -> PseudoLabeler.combine -> one
    TrainStep.step of the tiny BaseModelWithText: a finite loss, and the cells the warp brought in from outside carry ignore_index and
    weight 0."""
    import lc2is_amd.nn as N
    from lc2is_amd.data import DeviceImagePool, StrongAugment, TrainAugment
    from lc2is_amd.selftrain import PseudoLabeler
    from lc2is_amd.step import TrainStep
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64).to(dev).train()
    ids = torch.randint(1, 500, (2, 8), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, -1] = 510, 511
    text = {"input_ids": ids.to(dev), "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    rng = np.random.default_rng(3)
    pool = DeviceImagePool.from_arrays([rng.integers(0, 256, (80, 96, 3), dtype=np.uint8) for _ in range(2)],
                                       [rng.integers(0, 2, (80, 96), dtype=np.uint8) for _ in range(2)], device=dev)
    keys, epoch = [0, 1], 4
    batch_u = TrainAugment(crop_size=64, label_size=16, base_size=64, photometric=False, image_mean=MEAN, image_std=STD, seed=SEED)(pool, keys, epoch)
    text_u = {k: v.clone() for k, v in text.items()}                            # the unlabelled images' own prompts: combine concatenates them
    weak = {**text_u, "pixel_values": batch_u["pixel_values"]}
    labels_u, pw_u, _ = PseudoLabeler(m, threshold=0.5, weight="confidence")(weak)
    assert labels_u.shape == (2, 16, 16) and bool((labels_u >= 0).any()) and pw_u.shape == (2, 16, 16)
    strong_view = StrongAugment(image_mean=MEAN, image_std=STD, seed=SEED).view(weak, keys, epoch)
    geo = _geo(rotate_deg=30.0, translate=0.25)
    view, labels_g, pw_g = geo.view(strong_view, labels_u, pw_u, keys, epoch)
    assert set(view) == set(weak) and view["input_ids"] is text_u["input_ids"] and view["pixel_values"].shape == (2, 3, 64, 64)
    assert (geo.last_params[:, GR.FLAGS] == GR.WARP).all() and not _same_bits(view["pixel_values"], strong_view["pixel_values"])
    rows = geo.last_params.cpu().numpy()
    outside = np.stack([~GR.cell_index(rows[b], 16)[2] for b in range(2)])
    assert outside.any() and not outside.all()
    lab_np, pw_np = labels_g.cpu().numpy(), pw_g.cpu().numpy()
    assert (lab_np[outside] == -100).all() and (pw_np[outside] == 0.0).all() and (lab_np[~outside] >= 0).any()
    _, ref_lab, ref_pw = GR.apply_ref(view["pixel_values"].cpu().numpy(), labels_u.cpu().numpy(), pw_u.cpu().numpy(), rows, [0.0] * 3, -100)
    assert np.array_equal(lab_np, ref_lab) and np.array_equal(_np_bits(pw_np), _np_bits(ref_pw))
    inputs = {**text, "pixel_values": torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)}
    halves = (torch.arange(16) >= 8).to(torch.int64)
    labels = torch.stack([halves[None].expand(16, 16), halves[:, None].expand(16, 16)]).contiguous().to(dev)
    both, labels_b, pw_b = PseudoLabeler.combine(labelled=(inputs, labels), pseudo=(view, labels_g, pw_g))
    assert both["pixel_values"].shape == (4, 3, 64, 64) and labels_b.shape == (4, 16, 16)
    loss = float(TrainStep(m, optimizer="sgd", lr=1e-3).step(both, labels_b, pw_b))
    print("loss of one step fed by a geometric view with its pseudo-labels:", loss)
    assert np.isfinite(loss)
