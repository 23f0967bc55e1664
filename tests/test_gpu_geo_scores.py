"""A teacher's score map under a geometric view on the MI355X (lc2is_geo_scores, ops.geo_scores, GeometricAugment.warp_scores /
view_distill) against tests/geo_scores_ref.py: copies, exact rows (every fraction 0), weights and the in-frame mask bit for bit (the
map is held as integers); blended scores within test_gpu_geo.py's pixel_tol - the arithmetic is the same three nested lerps on exact
fractions.

The paths of geo_scores_kernel and where each is hit: the copy stream (row 5, flags 0, and row 6, out of range) and the mapped patch
(every other row), each for score blocks and for weight-cell blocks, next to each other in one grid at every shape.  A score block owns
a 4 x 4 patch of cells and 16 * ld / 4 items for 256 lanes: ld = 4 leaves 240 lanes idle, ld = 192 gives three items a lane, ld = 256
four (the copy loop's whole unroll); g = 5 and 7 have ragged last patches (and copy blocks past the end of the sample), g = 8 and 32
whole ones; L = 5 is less than one weight block, L = 128 is 64 of them."""
import functools

import numpy as np
import pytest
import torch

import geo_ref as GR
import geo_scores_ref as SR
from test_gpu_geo import MEAN, STD, pixel_tol

pytestmark = pytest.mark.gpu

SEED = 1234
ONE = GR.ONE
SHAPES = [(27, 8, 192, 32), (5, 5, 4, 5), (3, 7, 256, 112), (2, 32, 192, 128)]


def _geo(**kw):
    from lc2is_amd.data import GeometricAugment
    kw.setdefault("seed", SEED)
    return GeometricAugment(image_mean=MEAN, image_std=STD, **kw)


def _d(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _np_bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def _hand_rows():
    """27 rows: identity, flip, the three turns, the copy (flags 0 with a turn in its words) and an out-of-range row; whole-cell shifts
    at g = 8 (1 / 8 and - 2 / 8 of the side; at g = 32 whole cells too, at g = 5 and 7 blends); then 10 degrees, 45 degrees at 0.8,
    shear, shifts of +- 0.5, scale 0.25 and 4 and a mixed map, each plain and flipped."""
    rows = [GR.make_row(GR.WARP), GR.make_row(GR.FLIP, (-ONE, 0, 0, ONE)), GR.make_row(GR.WARP, (0, -ONE, ONE, 0)),
            GR.make_row(GR.WARP, (-ONE, 0, 0, -ONE)), GR.make_row(GR.WARP, (0, ONE, -ONE, 0)), GR.make_row(0, (0, -ONE, ONE, 0), (777, -777)),
            GR.make_row(GR.WARP, (GR.MAX_M + 1, 0, 0, ONE)), GR.make_row(GR.WARP, t=(8192, 0)), GR.make_row(GR.WARP | GR.FLIP, (-ONE, 0, 0, ONE), (0, -16384)),
            GR.make_row(GR.WARP, t=(-8192, 24576)), GR.make_row(GR.WARP | GR.FLIP, (0, -ONE, -ONE, 0))]
    for flip in (False, True):
        rows += [GR.affine_row(10.0, flip=flip), GR.affine_row(45.0, 0.8, flip=flip), GR.affine_row(0.0, 1.0, 30.0, flip=flip),
                 GR.affine_row(0.0, 1.0, 0.0, 0.5, -0.5, flip=flip), GR.affine_row(0.0, 1.0, 0.0, -0.5, 0.5, flip=flip),
                 GR.affine_row(0.0, 0.25, flip=flip), GR.affine_row(0.0, 4.0, flip=flip), GR.affine_row(-33.0, 0.8, 12.0, 0.07, -0.11, flip=flip)]
    assert len(rows) == 27 and [GR.row_is_mapped(r) for r in rows] == [i not in (5, 6) for i in range(27)]
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _inputs(B, g, ld, L):
    """Noise scores fp32 [B*g*g, ld] and weights in (0, 1) fp32 [B, L, L]; and the same with non-finite values planted: NaN, +-inf and
    a NaN with a payload in every sample's scores, next to taps that exact rows select."""
    rng = np.random.default_rng(1000 * g + ld + L)
    sc = rng.standard_normal((B * g * g, ld)).astype(np.float32)
    tw = rng.random((B, L, L)).astype(np.float32)
    planted, tw_planted = sc.copy(), tw.copy()
    v = planted.reshape(B, g, g, ld)
    v[:, 0, 0, 0], v[:, 1, 2, ld - 1], v[:, g - 1, g - 1, 1], v[:, 2, 1, 3] = np.nan, np.inf, -np.inf, np.nan
    v.view(np.int32)[:, 1, 1, 2] = 0x7FC12345
    v.view(np.int32)[:, g - 2, 3, 0] = -4194303                                # 0xFFC00001: a negative NaN with a payload
    tw_planted[0, 0, 0], tw_planted[-1, L - 1, L - 1] = np.nan, np.inf
    tw_planted.view(np.int32)[B // 2, 1, 1] = 0x7FC54321
    return sc, tw, planted, tw_planted


def _check_launch(ops, dev, sc, tw, rows, g, L, mask, finite, worst):
    """One launch against the restatement.  Weights (or the mask) by bits; copy rows and exact rows by bits against the input's own
    elements; blended rows within pixel_tol when the input is finite (on the planted input they are not looked at)."""
    B = len(rows)
    got_sc, got_tw = ops.geo_scores(_d(sc, dev), _d(rows, dev), B, g, teacher_weight=None if mask else _d(tw, dev), label_size=L if mask else None)
    ref_sc, ref_tw = SR.scores_ref(sc, None if mask else tw, rows, B, g, L)
    assert np.array_equal(_np_bits(got_tw.cpu().numpy()), _np_bits(ref_tw))
    if mask:
        assert set(np.unique(ref_tw).tolist()) <= {0.0, 1.0}
    got = got_sc.cpu().numpy().reshape(B, g, g, -1)
    x, ref = sc.reshape(B, g, g, -1), ref_sc.reshape(B, g, g, -1)
    A = float(np.abs(np.where(np.isfinite(sc), sc, 0.0)).max())
    for b in range(B):
        if not GR.row_is_mapped(rows[b]):
            assert np.array_equal(_np_bits(got[b]), _np_bits(x[b])), rows[b, :7]
        elif SR.is_exact(rows[b], g):
            assert np.array_equal(_np_bits(got[b]), _np_bits(SR.select_scores(x[b], rows[b]))), rows[b, :7]
        elif finite:
            err = np.abs(got[b].astype(np.float64) - ref[b]).max()
            worst.append(err / A)
            assert err <= pixel_tol(A), (rows[b, :7], err, pixel_tol(A))
    return got_sc, got_tw


@pytest.mark.parametrize("B,g,ld,L", SHAPES)
def test_scores_match_the_restatement(dev, B, g, ld, L):
    """The 27 hand-written rows, B per launch (the last launch wraps round), on the noise input with the weights and on the planted
    input with the mask."""
    from lc2is_amd import ops
    rows = _hand_rows()
    sc, tw, planted, tw_planted = _inputs(B, g, ld, L)
    worst, exact = [], 0
    for j in range(0, 27, B):
        pick = rows[[(j + i) % 27 for i in range(B)]]
        exact += sum(GR.row_is_mapped(r) and SR.is_exact(r, g) for r in pick)
        _check_launch(ops, dev, sc, tw, pick, g, L, False, True, worst)
        _check_launch(ops, dev, planted, tw_planted, pick, g, L, False, False, worst)
        _check_launch(ops, dev, planted, None, pick, g, L, True, False, worst)
    print(f"geo_scores B={B} g={g} ld={ld} L={L}: max |kernel - fp64| / A over {len(worst)} blended rows = {max(worst):.2e} "
          f"(bound {pixel_tol(1.0):.2e}); {exact} exact rows by bits")
    assert len(worst) >= 10 and exact >= (9 if g in (8, 32) else 6)
    # the exact rows are the torch ops they are, on the planted input, by bits
    x = _d(planted, dev).view(B, g, g, ld)[:1]
    want = {0: x, 1: x.flip(2), 2: torch.rot90(x, 1, (1, 2)), 3: torch.rot90(x, 2, (1, 2)), 4: torch.rot90(x, 3, (1, 2)), 5: x, 6: x,
            10: torch.rot90(x, 1, (1, 2)).flip(2)}
    if g == 8:
        want[7] = torch.cat([x[:, :, 1:], x[:, :, -1:]], dim=2)
        want[8] = torch.cat([x[:, :1], x[:, :1], x[:, :-2]], dim=1).flip(2)
    for i, w in want.items():
        got, _ = ops.geo_scores(x.reshape(g * g, ld), _d(rows[i:i + 1], dev), 1, g)
        assert _same_bits(got.view(1, g, g, ld), w), i
    # no weight map asked for: none made; out-of-frame cells exist in this set and are 0 in the mask, the border in the scores
    assert ops.geo_scores(x.reshape(g * g, ld), _d(rows[:1], dev), 1, g)[1] is None
    zoom = next(r for r in rows if GR.row_is_mapped(r) and not SR.split(r, g)[4].all())
    assert not GR.cell_index(zoom, L)[2].all()


def test_bad_rows_render_the_copy_bits_included(dev):
    from lc2is_amd import ops
    B, g, ld, L = 1, 7, 20, 14
    _, _, sc, tw = _inputs(B, g, ld, L)
    dsc, dtw = _d(sc, dev), _d(tw, dev)
    turn = (0, -ONE, ONE, 0)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    bad = [GR.make_row(GR.WARP, (ONE, 0, -GR.MAX_M - 1, ONE)), GR.make_row(GR.WARP, turn, (GR.MAX_T + 1, 0)), GR.make_row(GR.WARP, turn, (0, -GR.MAX_T - 1)),
           GR.make_row(4 | GR.WARP, turn), GR.make_row((1 << 30) | GR.FLIP, turn), GR.make_row(4, turn), np.full(GR.P_WORDS, -1, np.int32),
           np.full(GR.P_WORDS, lo, np.int32), np.full(GR.P_WORDS, hi, np.int32)]
    for word in range(7):                                                       # INT32_MIN / INT32_MAX in every word the kernel reads
        for v in (lo, hi):
            row = GR.make_row(GR.WARP, turn)
            row[word] = v
            bad.append(row)
    for row in bad:
        assert not GR.row_is_mapped(row)
        table = _d(row[None].copy(), dev)
        out = ops.geo_scores(dsc, table, B, g, teacher_weight=dtw)
        assert _same_bits(out[0], dsc) and _same_bits(out[1], dtw), row[:7]
        assert bool((ops.geo_scores(dsc, table, B, g, label_size=L)[1] == 1.0).all())
    # the rows at the limits are mapped, and whatever they hold every tap stays inside the sample: against the restatement
    edge = np.stack([GR.make_row(GR.WARP, (GR.MAX_M, 0, 0, GR.MAX_M), (GR.MAX_T, GR.MAX_T)), GR.make_row(GR.WARP, (GR.MAX_M, -GR.MAX_M, -GR.MAX_M, GR.MAX_M), (-GR.MAX_T, 3)),
                     GR.make_row(GR.WARP, (0, 0, 0, 0), (7, -7)), GR.make_row(GR.FLIP, (30000, 50000, -50000, 30000), (1000, 2000))])
    clean = _inputs(4, g, ld, L)
    _check_launch(ops, dev, clean[0], clean[1], edge, g, L, False, True, [])


def test_agreement_with_geo_apply(dev):
    """g = S = 8, L = 8: three columns of the scores as the three channels of ops.geo_apply with fill 0.  Where the four taps are in
    frame (geo_scores_ref.split) the two kernels blend the same taps: within pixel_tol; the weight map equals geo_apply's
    pixel_weight output by bits."""
    from lc2is_amd import ops
    rows = _hand_rows()
    B, g, ld, L = 27, 8, 192, 8
    sc, tw, _, _ = _inputs(B, g, ld, L)
    cols = [5, 150, 191]
    px = np.ascontiguousarray(sc.reshape(B, g, g, ld)[..., cols].transpose(0, 3, 1, 2))
    cfg = _geo().config
    assert [float(v) for v in cfg.fill] == [0.0, 0.0, 0.0]
    table = _d(rows, dev)
    apx, _, apw = ops.geo_apply((_d(px, dev), None, _d(tw, dev)), table, cfg)
    gsc, gtw = ops.geo_scores(_d(sc, dev), table, B, g, teacher_weight=_d(tw, dev))
    assert _same_bits(gtw, apw)
    mine = gsc.view(B, g, g, ld)[..., cols].permute(0, 3, 1, 2)
    A = float(np.abs(sc).max())
    seen = partial = 0
    for b in range(B):
        in_frame = torch.from_numpy(SR.split(rows[b], g)[4] if GR.row_is_mapped(rows[b]) else np.ones((g, g), bool)).to(dev)
        seen += int(in_frame.sum())
        partial += int(0 < int(in_frame.sum()) < g * g)
        d = (mine[b].double() - apx[b].double()).abs()[:, in_frame]
        assert d.numel() == 0 or float(d.max()) <= pixel_tol(A), (b, float(d.max()))
    assert seen > 8 * g * g and partial >= 8                                   # rows with cells on both sides of the frame


def test_batch_independence_out_and_untouched_weights(dev):
    """A sample's output has the same bits alone, in a batch and at another position; out= buffers are written and returned, an
    overlapping one is refused; views that are not contiguous or aligned are refused, not copied; with want_tw off the library
    leaves the weight buffers alone, whatever L and the weight pointers are."""
    from lc2is_amd import ops
    rows = _hand_rows()
    B, g, ld, L = 5, 7, 24, 21
    sc, tw, _, _ = _inputs(B, g, ld, L)
    dsc, dtw = _d(sc, dev), _d(tw, dev)
    pick = [12, 5, 16, 1, 25]
    table = _d(rows[pick], dev)
    full = ops.geo_scores(dsc, table, B, g, teacher_weight=dtw)
    again = ops.geo_scores(dsc, table, B, g, teacher_weight=dtw)
    assert all(_same_bits(a, b) for a, b in zip(full, again)) and not _same_bits(full[0], dsc)
    n = g * g
    for b in range(B):
        alone = ops.geo_scores(dsc[b * n:(b + 1) * n], table[b:b + 1].contiguous(), 1, g, teacher_weight=dtw[b:b + 1])      # offset views
        assert _same_bits(alone[0], full[0][b * n:(b + 1) * n]) and _same_bits(alone[1], full[1][b:b + 1]), b
    perm = [3, 4, 0, 1, 2]
    moved = ops.geo_scores(dsc.view(B, n, ld)[perm].reshape(B * n, ld).contiguous(), table[perm].contiguous(), B, g, teacher_weight=dtw[perm].contiguous())
    assert _same_bits(moved[0].view(B, n, ld), full[0].view(B, n, ld)[perm]) and _same_bits(moved[1], full[1][perm])
    # out=
    out = (torch.empty_like(dsc), torch.empty_like(dtw))
    got = ops.geo_scores(dsc, table, B, g, teacher_weight=dtw, out=out)
    assert got[0] is out[0] and got[1] is out[1] and all(_same_bits(a, b) for a, b in zip(got, full))
    mask = torch.full((B, L, L), 7.0, device=dev)
    got = ops.geo_scores(dsc, table, B, g, label_size=L, out=(None, mask))
    assert got[1] is mask and _same_bits(got[0], full[0]) and _same_bits(mask, ops.geo_scores(dsc, table, B, g, label_size=L)[1])
    assert bool(((mask == 0.0) | (mask == 1.0)).all()) and bool((mask == 0.0).any())
    for which, src in ((0, dsc), (1, dtw)):
        m = src.numel()
        unit = 4 if which == 0 else 1
        buf = torch.zeros(2 * m, device=dev)
        x_in = buf[:m].view_as(src).copy_(src)
        ops_in = [dsc, dtw]
        ops_in[which] = x_in
        for bad_out in (x_in, buf[m // 2 // 4 * 4:m // 2 // 4 * 4 + m].view_as(src), buf[m - unit:2 * m - unit].view_as(src)):
            outs = [None, None]
            outs[which] = bad_out
            with pytest.raises(RuntimeError, match="overlap"):
                ops.geo_scores(ops_in[0], table, B, g, teacher_weight=ops_in[1], out=tuple(outs))
        outs = [None, None]
        outs[which] = buf[m:].view_as(src)                                      # adjacent is fine
        got = ops.geo_scores(ops_in[0], table, B, g, teacher_weight=ops_in[1], out=tuple(outs))
        assert got[which] is outs[which] and all(_same_bits(a, b) for a, b in zip(got, full))
    wide = torch.zeros(B * n, ld + 4, device=dev)
    flat = torch.zeros(B * n * ld + 1, device=dev)
    for bad in (wide[:, :ld], torch.zeros(ld, B * n, device=dev).t(), flat[1:].view(B * n, ld), dsc[::2]):
        with pytest.raises(RuntimeError):
            ops.geo_scores(bad, table, B, g)
    for bad_tw in (torch.zeros(B, L, L + 1, device=dev)[..., :L], torch.zeros(B, L, L, 2, device=dev)[..., 0]):
        with pytest.raises(RuntimeError):
            ops.geo_scores(dsc, table, B, g, teacher_weight=bad_tw)
    for kw in (dict(label_size=20), dict(label_size=0), dict(out=(None, mask))):
        with pytest.raises(ValueError):
            ops.geo_scores(dsc, table, B, g, **kw)
    with pytest.raises(ValueError):
        ops.geo_scores(dsc, table, 0, g)
    for bad_B, bad_table in ((B + 1, table), (B, table[:4].contiguous())):
        with pytest.raises(RuntimeError):
            ops.geo_scores(dsc, bad_table, bad_B, g)
    # want_tw == 0 at the library: the weight buffers keep their bytes; L and the weight pointers are not looked at
    f = ops._fn("lc2is_geo_scores")
    keep_in, keep_out, o = dtw.clone(), torch.full((B, L, L), 7.0, device=dev), torch.empty_like(dsc)
    stream = torch.cuda.current_stream().cuda_stream
    for L_arg, tw_ptr, out_ptr in ((L, keep_in.data_ptr(), keep_out.data_ptr()), (0, keep_in.data_ptr() + 1, keep_out.data_ptr() + 2), (5, None, None),
                                   (L, keep_out.data_ptr(), keep_out.data_ptr())):
        o.zero_()
        assert f(dsc.data_ptr(), tw_ptr, table.data_ptr(), B, g, ld, L_arg, 0, o.data_ptr(), out_ptr, stream) == 0
        assert _same_bits(o, full[0]) and bool((keep_out == 7.0).all()) and _same_bits(keep_in, dtw)


@pytest.mark.parametrize("epoch", [0, 3])
def test_drawn_tables_through_warp_scores(dev, epoch):
    """GeometricAugment over 64 keys, then warp_scores with the table it left on the device: against the restatement of the table
    read back (here, not by the class); with a weight map, with the mask, and with params= given."""
    B, g, ld, L, S = 64, 8, 32, 16, 16
    geo = _geo(prob=0.6, rotate_deg=60.0, scale_range=(0.5, 2.0), shear_deg=20.0, translate=0.25, flip_prob=0.5)
    sc, tw, _, _ = _inputs(B, g, ld, L)
    rng = np.random.default_rng(epoch)
    px = torch.from_numpy(rng.standard_normal((B, 3, S, S)).astype(np.float32)).to(dev)
    keys = list(range(100, 100 + B))
    with pytest.raises(RuntimeError, match="table"):
        geo.warp_scores(_d(sc, dev))
    geo((px, None, None), keys, epoch)
    rows = geo.last_params.cpu().numpy()
    want = GR.draw_params(GR.config_dict(geo.config), keys, epoch)
    assert np.array_equal(rows[:, GR.FLAGS], want["flags"]) and set(rows[:, GR.FLAGS].tolist()) == {0, 1, 2, 3}
    got_sc, got_tw = geo.warp_scores(_d(sc, dev), _d(tw, dev))
    ref_sc, ref_tw = SR.scores_ref(sc, tw, rows, B, g, L)
    A = float(np.abs(sc).max())
    err = np.abs(got_sc.cpu().numpy().astype(np.float64) - ref_sc).reshape(B, -1).max(axis=1)
    print(f"warp_scores epoch {epoch}: max |kernel - fp64| / A over {B} drawn rows = {err.max() / A:.2e} (bound {pixel_tol(1.0):.2e})")
    assert (err <= pixel_tol(A)).all() and np.array_equal(_np_bits(got_tw.cpu().numpy()), _np_bits(ref_tw))
    copies = rows[:, GR.FLAGS] == 0
    assert np.array_equal(_np_bits(got_sc.cpu().numpy().reshape(B, -1)[copies]), _np_bits(sc.reshape(B, -1)[copies]))
    only, none = geo.warp_scores(_d(sc, dev))
    assert none is None and _same_bits(only, got_sc)
    again, mask = geo.warp_scores(_d(sc, dev), label_size=L, params=geo.last_params.clone())
    assert _same_bits(again, got_sc) and np.array_equal(_np_bits(mask.cpu().numpy()), _np_bits(SR.scores_ref(sc, None, rows, B, g, L)[1]))
    out = (torch.empty_like(got_sc), torch.empty_like(got_tw))
    res = geo.warp_scores(_d(sc, dev), _d(tw, dev), out=out)
    assert res[0] is out[0] and res[1] is out[1] and _same_bits(out[0], got_sc) and _same_bits(out[1], got_tw)
    with pytest.raises(ValueError):
        geo.warp_scores(_d(sc, dev)[:B * g * g - 1])


def test_the_three_launches_replay_from_a_graph(dev):
    """Capture geo_params + geo_apply + geo_scores; write a new value into the device epoch tensor; the replay equals the eager
    view_distill of a fresh augmenter by bits, and the epochs differ from each other."""
    from lc2is_amd import ops
    B, g, ld, L, S = 6, 5, 20, 10, 20
    kw = dict(prob=0.7, rotate_deg=40.0, shear_deg=10.0, translate=0.2, flip_prob=0.4)
    geo = _geo(**kw)
    cfg = geo.config
    sc, tw, _, _ = _inputs(B, g, ld, L)
    rng = np.random.default_rng(6)
    px = torch.from_numpy(rng.standard_normal((B, 3, S, S)).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rng.integers(0, 150, (B, L, L)).astype(np.int64)).to(dev)
    dsc, dtw = _d(sc, dev), _d(tw, dev)
    keys = torch.arange(21, 21 + B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    table = torch.empty(B, ops.GEO_PARAM_WORDS, dtype=torch.int32, device=dev)
    out = (torch.empty_like(px), torch.empty_like(lab), torch.empty_like(dtw))
    out_s = (torch.empty_like(dsc), torch.empty_like(dtw))

    def three():
        ops.geo_params(keys, epoch, cfg, out=table)
        ops.geo_apply((px, lab, dtw), table, cfg, out=out)
        ops.geo_scores(dsc, table, B, g, teacher_weight=dtw, out=out_s)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        three()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        three()
    seen = []
    for e in (0, 3, 77):
        epoch.fill_(e)
        graph.replay()
        view, lab_e, pw_e, sc_e, tw_e = _geo(**kw).view_distill({"pixel_values": px}, lab, dsc, keys, epoch, pixel_weight=dtw, teacher_weight=dtw)
        assert _same_bits(out[0], view["pixel_values"]) and torch.equal(out[1], lab_e) and _same_bits(out[2], pw_e)
        assert _same_bits(out_s[0], sc_e) and _same_bits(out_s[1], tw_e) and _same_bits(tw_e, pw_e)
        rows = table.cpu().numpy()
        ref_sc, ref_tw = SR.scores_ref(sc, tw, rows, B, g, L)
        assert np.abs(out_s[0].cpu().numpy().astype(np.float64) - ref_sc).max() <= pixel_tol(float(np.abs(sc).max()))
        assert np.array_equal(_np_bits(out_s[1].cpu().numpy()), _np_bits(ref_tw))
        seen.append((rows[:, :7].tolist(), out_s[0].clone()))
    assert seen[0][0] != seen[1][0] and seen[1][0] != seen[2][0] and seen[0][0] != seen[2][0]
    assert not _same_bits(seen[0][1], seen[1][1]) and not _same_bits(seen[1][1], seen[2][1]) and not _same_bits(seen[0][1], seen[2][1])


def _tiny(dev):
    import lc2is_amd.nn as N
    torch.manual_seed(7)
    return N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256), text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511),
                               nhead=2, dim_feedforward=128, out_dim=64).to(dev).train()


def test_view_distill_feeds_the_soft_teacher_step(dev):
    """The soft recipe under a geometric view on the tiny model of test_gpu_geo.py's self-training test: the teacher's head_scores of
    the weak view under ema_weights() -> view_distill -> TrainStep(distill=...).step_distill.  With a flip-only augmenter the five
    outputs are the torch flips by bits and the step's loss is, bit for bit, that of a step_distill on the by-hand flipped tensors
    from the same state; with a rotation and a shift the loss is finite and the mask is the restatement's."""
    from lc2is_amd.step import TrainStep
    m_a, m_b = _tiny(dev), _tiny(dev)
    ids = torch.randint(1, 500, (2, 8), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, -1] = 510, 511
    text = {"input_ids": ids.to(dev), "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    gen = torch.Generator().manual_seed(3)
    weak = {**text, "pixel_values": torch.randn(2, 3, 64, 64, generator=gen).to(dev)}
    halves = (torch.arange(16) >= 8).to(torch.int64)
    labels = torch.stack([halves[None].expand(16, 16), halves[:, None].expand(16, 16)]).contiguous().to(dev)
    pw = torch.rand(2, 16, 16, generator=gen).to(dev)
    mk = lambda m: TrainStep(m, optimizer="sgd", lr=1e-3, ema_decay=0.99, distill=(1.0, 1.0, "all"))   # noqa: E731
    s_a, s_b = mk(m_a), mk(m_b)
    for s, m in ((s_a, m_a), (s_b, m_b)):
        s.step_distill(weak, labels, m.head_scores(weak))                       # one step: the EMA is no longer the student
    assert torch.equal(s_a.arena.flat, s_b.arena.flat)
    with s_a.ema_weights():
        scores_t = m_a.head_scores(weak)                                        # fp32 [B*g*g, class_pad(K)]: the teacher saw the weak view
    g, ld = 4, scores_t.shape[1]
    assert scores_t.shape[0] == 2 * g * g and scores_t.dtype == torch.float32
    keys, epoch = [0, 1], 4
    flip = _geo(prob=0.0, flip_prob=1.0)
    view, lab_f, pw_f, sc_f, tw_f = flip.view_distill(weak, labels, scores_t, keys, epoch, pixel_weight=pw)
    assert set(view) == set(weak) and view["input_ids"] is weak["input_ids"] and (flip.last_params[:, GR.FLAGS] == GR.FLIP).all()
    hand = (weak["pixel_values"].flip(-1).contiguous(), labels.flip(-1).contiguous(), pw.flip(-1).contiguous(),
            scores_t.view(2, g, g, ld).flip(2).reshape(2 * g * g, ld).contiguous(), torch.ones(2, 16, 16, device=dev))
    assert _same_bits(view["pixel_values"], hand[0]) and torch.equal(lab_f, hand[1]) and _same_bits(pw_f, hand[2])
    assert _same_bits(sc_f, hand[3]) and _same_bits(tw_f, hand[4]) and not _same_bits(sc_f, scores_t)
    loss_a = s_a.step_distill(view, lab_f, sc_f, teacher_weight=tw_f)
    loss_b = s_b.step_distill({**weak, "pixel_values": hand[0]}, hand[1], hand[3], teacher_weight=hand[4])
    print("loss of the flipped soft step:", float(loss_a), float(loss_b))
    assert bool(torch.isfinite(loss_a)) and torch.equal(loss_a, loss_b) and torch.equal(s_a.arena.flat, s_b.arena.flat)
    # a rotation and a shift: cells come in from outside, the mask takes them out of the KL, the loss is finite
    geo = _geo(rotate_deg=30.0, translate=0.25)
    with s_a.ema_weights():
        scores_t = m_a.head_scores(weak)
    view, lab_g, pw_g, sc_g, tw_g = geo.view_distill(weak, labels, scores_t, keys, epoch)
    assert pw_g is None and tw_g.shape == (2, 16, 16) and sc_g.shape == scores_t.shape
    rows = geo.last_params.cpu().numpy()
    assert (rows[:, GR.FLAGS] == GR.WARP).all()
    ref_sc, ref_tw = SR.scores_ref(scores_t.cpu().numpy(), None, rows, 2, g, 16)
    assert np.array_equal(_np_bits(tw_g.cpu().numpy()), _np_bits(ref_tw)) and 0.0 < float(tw_g.mean()) < 1.0
    assert bool(((lab_g == -100) == (tw_g == 0.0)).all())                       # one map: the cells without a label are the cells without a KL
    A = float(scores_t.abs().max())
    assert np.abs(sc_g.cpu().numpy().astype(np.float64) - ref_sc).max() <= pixel_tol(A)
    loss = s_a.step_distill(view, lab_g, sc_g, teacher_weight=tw_g)
    print("loss of one soft step under a geometric view:", float(loss))
    assert bool(torch.isfinite(loss))
