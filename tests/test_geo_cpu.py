"""Geometric views (random affine warp, labels follow), the part that needs no GPU: the bindings and the library's refusals (host
code, before any launch), the argument checks of GeometricAugment and the ops wrappers, and the properties of the numpy restatement
tests/geo_ref.py that tests/test_gpu_geo.py holds the kernels to - above all that its integer rule IS grid_sample / affine_grid."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R
import geo_ref as GR
import mix_ref as MR
import strong_ref as SR

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("lc2is_geo_params", "lc2is_geo_apply")
SIDES = (8, 12, 20, 68, 132)


def test_bindings_and_header_declare_the_entry_points():
    from lc2is_amd import _lib, ops
    header = (ROOT / "include" / "lc2is_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and hasattr(lib, name)
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(ops._ARGTYPES[name]) == len(m.group(1).split(","))
        assert ops._fn(name).argtypes == ops._ARGTYPES[name]
        comment = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "replaces:" in comment, name
    for c_name, value in (("LC2IS_GEO_PARAM_WORDS", ops.GEO_PARAM_WORDS), ("LC2IS_GEO_FLAGS", ops.GEO_FLAGS), ("LC2IS_GEO_M", ops.GEO_M),
                          ("LC2IS_GEO_T", ops.GEO_T), ("LC2IS_GEO_REC", ops.GEO_REC), ("LC2IS_GEO_WARP", ops.GEO_WARP),
                          ("LC2IS_GEO_FLIP", ops.GEO_FLIP), ("LC2IS_GEO_ONE", ops.GEO_ONE), ("LC2IS_GEO_MAX_M", ops.GEO_MAX_M),
                          ("LC2IS_GEO_MAX_T", ops.GEO_MAX_T), ("LC2IS_GEO_MIN_SIDE", ops.GEO_MIN_SIDE)):
        assert re.search(rf"#define {c_name} {value}\b", header), c_name
    assert f"#define LC2IS_GEO_STREAM 0x{ops.GEO_STREAM:08X}u" in header and int(GR.STREAM) == ops.GEO_STREAM == 0x47454F31
    assert (GR.P_WORDS, GR.FLAGS, GR.M0, GR.T0, GR.REC0, GR.WARP, GR.FLIP, GR.ONE, GR.MAX_M, GR.MAX_T) == \
        (ops.GEO_PARAM_WORDS, ops.GEO_FLAGS, ops.GEO_M, ops.GEO_T, ops.GEO_REC, ops.GEO_WARP, ops.GEO_FLIP, ops.GEO_ONE, ops.GEO_MAX_M,
         ops.GEO_MAX_T)
    assert ops.GEO_MAX_M == 8 * 65536 and ops.GEO_PARAM_WORDS == 16
    # the struct: 4 uint32, 5 floats, 3 floats, one int64 on an 8-byte boundary, no padding
    c = ops.GeoConfig
    assert ctypes.sizeof(c) == 56 and c.warp_thr.offset == 8 and c.rotate.offset == 16 and c.translate.offset == 32
    assert (c.fill.offset, c.ignore_index.offset) == (36, 48)
    fields = re.search(r"typedef struct \{([^}]*)\} lc2is_geo_config;", code).group(1)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in c._fields_]
    tool = (ROOT / "tools" / "check_kernel_resources.py").read_text()
    assert '"geo_params_kernel"' in tool and '"geo_apply_kernel"' in tool


def _cfg(**kw):
    from lc2is_amd.data import GeometricAugment
    return GeometricAugment(**kw).config


def test_the_library_refuses_null_then_shape_before_any_launch():
    """Pointers are only tested, never followed: every call below returns from the checks."""
    from lc2is_amd import ops
    f, g = ops._fn("lc2is_geo_params"), ops._fn("lc2is_geo_apply")
    p = 0x1000
    good = _cfg()

    def bad_cfgs():
        for name, value in (("rotate", 3.2), ("rotate", -0.1), ("rotate", float("nan")), ("scale_lo", 0.2), ("scale_hi", 4.5),
                            ("scale_lo", 2.0), ("scale_hi", float("nan")), ("shear", 0.8), ("shear", -0.1), ("translate", 0.51),
                            ("translate", -0.01), ("warp_thr", (1 << 24) + 1), ("flip_thr", 1 << 25)):
            cfg = _cfg()
            setattr(cfg, name, value)
            yield name, value, cfg

    def par(cfg=good, keys=p, B=3, epoch=p, params=p):
        return f(keys, B, epoch, ctypes.addressof(cfg) if cfg is not None else None, params, None)

    worse = next(bad_cfgs())[2]
    for missing in ("keys", "epoch", "params"):
        assert par(cfg=worse, B=0, **{missing: None}) == -2, missing               # NULL first, whatever else is wrong
    assert par(cfg=None, B=0) == -2
    for kw in (dict(B=0), dict(B=-1), dict(keys=p + 4), dict(epoch=p + 2), dict(params=p + 1)):
        assert par(**kw) == -1, kw
    for name, value, cfg in bad_cfgs():
        assert par(cfg=cfg) == -1, (name, value)
    # the limits themselves are inside: 180 degrees, 45 degrees, the whole scale range, half the side
    edge = _cfg(rotate_deg=180.0, shear_deg=45.0, scale_range=(0.25, 4.0), translate=0.5)
    assert edge.rotate == np.float32(np.pi) and edge.shear == np.float32(np.pi / 4)
    ops._geo_config(edge, "geo_params")                                            # (the host check; the library's twin runs on the GPU tests)

    big = 0x40000000

    def app(px=big, lab=3 * big, pw=5 * big, params=p, cfg=good, B=3, S=16, L=4, out_px=2 * big, out_lab=4 * big, out_pw=6 * big):
        return g(px, lab, pw, params, ctypes.addressof(cfg) if cfg is not None else None, B, S, L, out_px, out_lab, out_pw, None)

    for missing in ("px", "params", "out_px", "out_lab", "out_pw"):
        assert app(S=7, B=0, **{missing: None}) == -2, missing
    assert app(cfg=None, S=7) == -2
    for kw in (dict(B=0), dict(B=65536), dict(S=4), dict(S=0), dict(S=14), dict(S=18), dict(S=4100), dict(L=0), dict(L=3), dict(L=32),
               dict(px=big + 8), dict(out_px=2 * big + 4), dict(lab=3 * big + 4), dict(out_lab=4 * big + 4), dict(pw=5 * big + 2),
               dict(out_pw=6 * big + 1), dict(params=p + 2)):
        assert app(**kw) == -1, kw
    for name, value, cfg in bad_cfgs():
        assert app(cfg=cfg) == -1, (name, value)
    # an output overlapping its input: in place, the input's last bytes, the output's last bytes - pixels, labels, weights
    npx, nlab, npw = 3 * 3 * 16 * 16 * 4, 3 * 4 * 4 * 8, 3 * 4 * 4 * 4
    assert app(out_px=big) == -1 and app(out_px=big + npx - 16) == -1 and app(out_px=big - npx + 16) == -1
    assert app(out_lab=3 * big) == -1 and app(out_lab=3 * big + nlab - 8) == -1 and app(out_lab=3 * big - nlab + 8) == -1
    assert app(out_pw=5 * big) == -1 and app(out_pw=5 * big + npw - 4) == -1 and app(out_pw=5 * big - npw + 4) == -1
    # a map that is not given has no output to miss or to overlap: NULL inputs with NULL outputs pass the NULL check (S = 7: SHAPE)
    assert app(lab=None, out_lab=None, S=7) == -1 and app(pw=None, out_pw=None, S=7) == -1
    assert app(lab=None, pw=None, out_lab=None, out_pw=None, S=7) == -1


def test_geometricaugment_refuses_bad_settings():
    from lc2is_amd.data import GeometricAugment
    for kw in (dict(prob=1.5), dict(flip_prob=-0.1), dict(rotate_deg=181.0), dict(rotate_deg=-1.0), dict(shear_deg=46.0),
               dict(scale_range=(0.2, 1.0)), dict(scale_range=(1.0, 4.5)), dict(scale_range=(1.5, 0.5)), dict(translate=0.6),
               dict(translate=-0.1), dict(rotate_deg=float("nan")), dict(fill=(0, 0, 256)), dict(fill=(-1, 0, 0)),
               dict(image_std=(0.2, 0.0, 0.2)), dict(image_mean=(0.5, 0.5)), dict(ignore_index=2 ** 63)):
        with pytest.raises(ValueError):
            GeometricAugment(**kw)
    for kw in (dict(prob="0.8"), dict(flip_prob=None), dict(prob=True), dict(scale_range=1.0), dict(scale_range=(0.5,)),
               dict(rotate_deg="20"), dict(fill=128), dict(fill=(1, 2)), dict(fill=("a", 0, 0)), dict(ignore_index=1.0),
               dict(ignore_index=None), dict(seed=1.5), dict(seed=None)):
        with pytest.raises(TypeError):
            GeometricAugment(**kw)
    g = GeometricAugment(prob=0.5, rotate_deg=180.0, scale_range=(0.25, 4.0), shear_deg=45.0, translate=0.5, flip_prob=1.0,
                         fill=(255, 0, 127.5), ignore_index=255, image_mean=(0.5, 0.25, 0.5), image_std=(0.5, 0.25, 0.25), seed=2 ** 40 + 5)
    c = g.config
    assert (c.warp_thr, c.flip_thr) == (1 << 23, 1 << 24) and (c.seed_lo, c.seed_hi) == (5, 256) and c.ignore_index == 255
    assert abs(c.rotate - np.pi) < 1e-6 and abs(c.shear - np.pi / 4) < 1e-6 and (c.scale_lo, c.scale_hi, c.translate) == (0.25, 4.0, 0.5)
    assert [float(v) for v in c.fill] == [1.0, -1.0, 0.0] and g.last_params is None
    d = GeometricAugment().config
    assert (d.warp_thr, d.flip_thr) == (1 << 24, 0) and abs(d.rotate - np.radians(20.0)) < 1e-7 and d.ignore_index == -100
    assert [float(v) for v in d.fill] == [0.0, 0.0, 0.0] and d.shear == 0.0 and d.translate == 0.0      # the mean colour: exactly 0.0
    assert (d.scale_lo, d.scale_hi) == (np.float32(0.8), 1.25)


def test_geometricaugment_and_the_wrappers_check_arguments_before_device_work():
    from lc2is_amd import ops
    from lc2is_amd.data import GeometricAugment
    geo = GeometricAugment()
    keys = torch.arange(2)
    x, lab, pw = torch.zeros(2, 3, 16, 16), torch.zeros(2, 4, 4, dtype=torch.int64), torch.zeros(2, 4, 4)
    for bad in ((x.double(), lab, pw), (x.half(), None, None), (x.numpy(), lab, pw), (None, lab, pw), (x, lab.int(), pw), (x, lab, pw.double()),
                (x, lab.numpy(), pw), x, (x, lab)):
        with pytest.raises(TypeError):
            geo(bad, keys, 0)
    for bad in ((torch.zeros(2, 3, 4, 4), None, None), (torch.zeros(2, 3, 14, 14), None, None), (torch.zeros(2, 1, 16, 16), lab, pw),
                (torch.zeros(2, 3, 16, 20), lab, pw), (torch.zeros(3, 16, 16), lab, pw), (torch.zeros(0, 3, 16, 16), None, None),
                (x, torch.zeros(2, 3, 3, dtype=torch.int64), None), (x, torch.zeros(3, 4, 4, dtype=torch.int64), None),
                (x, lab, torch.zeros(2, 8, 8)), (x, torch.zeros(2, 4, 8, dtype=torch.int64), None), (x, None, torch.zeros(2, 4))):
        with pytest.raises(ValueError):
            geo(bad, keys, 0)
    # host tensors of the right types: there is no CPU path
    for batch in ((x, lab, pw), (x, None, None), (x, lab, None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            geo(batch, keys, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geo.view({"pixel_values": x, "input_ids": None}, lab, pw, keys, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.geo_params(keys, torch.zeros(1, dtype=torch.int32), geo.config)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.geo_apply((x, lab, pw), torch.zeros(2, ops.GEO_PARAM_WORDS, dtype=torch.int32), geo.config)
    with pytest.raises(TypeError):
        ops.geo_apply(x, torch.zeros(2, ops.GEO_PARAM_WORDS, dtype=torch.int32), geo.config)
    for name, value in (("rotate", 3.2), ("scale_lo", 0.1), ("shear", 1.0), ("translate", 0.75), ("warp_thr", 1 << 25)):
        cfg = GeometricAugment().config
        setattr(cfg, name, value)
        with pytest.raises(ValueError):
            ops._geo_config(cfg, "geo_params")
    assert geo.last_params is None


def test_the_selftraining_recipe_warps_the_labels_with_the_view():
    from lc2is_amd import selftrain
    doc = selftrain.__doc__
    scope = doc[doc.index("Out of scope here"):]
    assert "geometric" not in scope.lower()
    recipe = doc[:doc.index("Out of scope here")]
    assert "GeometricAugment" in recipe and "geo.view(strong_view, labels_u, pw_u, keys, epoch)" in recipe
    assert recipe.index("labeler(weak") < recipe.index("strong.view(weak") < recipe.index("geo.view(strong_view")


# ---- the draws ------------------------------------------------------------------------------------------------------------------
def test_the_draws_over_4096_keys():
    """Every switch combination occurs; the values lie in their ranges with means near the middle (a uniform mean over n draws has sd
    (hi - lo) / sqrt(12 n); the bound is five of them); the matrix is (1/s) R H; no draw is shared with the other streams."""
    from lc2is_amd.data import GeometricAugment
    g = GeometricAugment(prob=0.5, rotate_deg=30.0, scale_range=(0.5, 2.0), shear_deg=15.0, translate=0.125, flip_prob=0.5, seed=1234)
    cfg = GR.config_dict(g.config)
    keys = np.arange(4096)
    p = GR.draw_params(cfg, keys, 3)
    assert set(p["flags"].tolist()) == {0, 1, 2, 3}
    for name, prob in (("warp", 0.5), ("flip", 0.5)):
        assert abs(p[name].mean() - prob) <= 5.0 * np.sqrt(0.25 / 4096), (name, p[name].mean())
    for name, lo, hi in (("theta", -cfg["rotate"], cfg["rotate"]), ("s", cfg["scale_lo"], cfg["scale_hi"]), ("phi", -cfg["shear"], cfg["shear"]),
                         ("fx", -cfg["translate"], cfg["translate"]), ("fy", -cfg["translate"], cfg["translate"])):
        v = p[name].astype(np.float64)
        assert v.min() >= lo and v.max() <= hi and v.dtype == np.float64 and p[name].dtype == np.float32
        assert abs(v.mean() - 0.5 * (lo + hi)) <= 5.0 * (hi - lo) / np.sqrt(12 * 4096), (name, v.mean())
        assert v.max() - v.min() > 0.99 * (hi - lo)
    # no warp: the identity (or the flip) and no shift, exactly; warp: det = 1 / s^2 up to the flip's sign, within the integer rounding
    off = p["warp"] == 0
    assert (p["m"][off][:, 1:3] == 0).all() and (p["m"][off][:, 3] == 65536).all() and (np.abs(p["m"][off][:, 0]) == 65536).all()
    assert (p["tx"][off] == 0).all() and (p["ty"][off] == 0).all() and (p["tx"][~off] != 0).any()
    assert ((p["m"][:, 0] < 0) == (p["flip"] == 1))[off].all()
    m = p["m"].astype(np.float64) / 65536
    det = m[:, 0] * m[:, 3] - m[:, 1] * m[:, 2]
    sign = np.where(p["flip"] == 1, -1.0, 1.0)
    on = ~off
    assert np.abs(det[on] * sign[on] * p["s"][on].astype(np.float64) ** 2 - 1.0).max() < 1e-3
    assert np.abs(p["m"]).max() <= GR.MAX_M and np.abs(p["tx"]).max() <= 0.125 * 65536
    rows = GR.param_rows(p)
    assert rows.shape == (4096, GR.P_WORDS) and not rows[:, 12:].any() and all(GR.row_is_mapped(r) == (r[0] != 0) for r in rows[:64])
    # the epoch, the key and the seed change the draw
    base = GR.param_rows(GR.draw_params(cfg, [11], 4))
    assert not np.array_equal(base, GR.param_rows(GR.draw_params(cfg, [11], 5)))
    assert not np.array_equal(base, GR.param_rows(GR.draw_params(cfg, [12], 4)))
    assert np.array_equal(base, GR.param_rows(GR.draw_params(cfg, [11], 4)))
    # one seed, four streams: the sample hashes differ for every key, and so does every draw vector (k = 0 .. 6)
    assert int(GR.STREAM) not in (0, int(MR.STREAM), int(SR.STREAM))
    hashes = [R.sample_hash(1234, 3, keys), MR.mix_hash(1234, 3, keys), SR.strong_hash(1234, 3, keys), GR.geo_hash(1234, 3, keys)]
    assert (hashes[3] == hashes[0] ^ GR.STREAM).all()
    draws = [np.stack([R.u24(h, k) for k in range(7)], axis=1) for h in hashes]
    for other in range(3):
        assert (hashes[3] != hashes[other]).all()
        assert not (draws[3] == draws[other]).all(axis=1).any()
        assert (draws[3] == draws[other]).mean() < 1e-3                             # 28672 pairs of 24-bit numbers: chance is 6e-8 each


# ---- the integer rule is grid_sample ------------------------------------------------------------------------------------------
def _random_rows(rng, n):
    return [GR.affine_row(rng.uniform(-180, 180), np.exp(rng.uniform(np.log(0.25), np.log(4.0))), rng.uniform(-45, 45),
                          rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), bool(rng.integers(2))) for _ in range(n)]


def _grid(row, n):
    theta = torch.from_numpy(GR.theta_of(row))[None]
    return F.affine_grid(theta, (1, 1, n, n), align_corners=False)


@pytest.mark.parametrize("S", SIDES)
def test_the_restated_pixels_are_bilinear_grid_sample(S):
    """40 random maps per size over the whole range of the config (rotation +-180 degrees, scale 0.25 .. 4, shear +-45 degrees,
    translation +-0.5, flip): the integer rule against float64 affine_grid + grid_sample(bilinear, zeros) within 1e-10."""
    rng = np.random.default_rng(100 + S)
    x = rng.standard_normal((3, S, S))
    worst = 0.0
    for row in _random_rows(rng, 40):
        assert GR.row_is_mapped(row)
        want = F.grid_sample(torch.from_numpy(x)[None], _grid(row, S), "bilinear", "zeros", align_corners=False)[0].numpy()
        worst = max(worst, np.abs(GR.warp_pixels(x, row, (0.0, 0.0, 0.0)) - want).max())
    print(f"geo_ref S={S}: max |integer rule - fp64 grid_sample| over 40 maps = {worst:.2e}")
    assert worst <= 1e-10


def test_the_restated_cells_are_nearest_grid_sample_outside_a_band_at_cell_edges():
    """Labels against grid_sample(mode="nearest") on the cell grid, 40 maps per size.  Where the source position lies within 2^-10 cell
    of a cell edge the float64 grid and the integers may round to different cells; those cells are left out, and they are at most 1 %
    of all (expected: 2 axes * 2 * 2^-10 = 0.39 %).  Everywhere else: no mismatch."""
    rng = np.random.default_rng(7)
    cells = band_cells = 0
    for L in SIDES:
        lab = rng.integers(0, 150, (L, L))
        for row in _random_rows(rng, 40):
            U, V = GR.source_uv(row, L)
            pos = np.stack([(U + L * 65536) / 131072.0, (V + L * 65536) / 131072.0])       # exact in float64: the cell is floor(pos)
            frac = pos - np.floor(pos)
            band = ((frac < 2.0 ** -10) | (frac > 1.0 - 2.0 ** -10)).any(axis=0)
            want = F.grid_sample(torch.from_numpy(lab + 1.0)[None, None], _grid(row, L), "nearest", "zeros", align_corners=False)[0, 0].numpy()
            want = np.where(want == 0.0, -100, want.astype(np.int64) - 1)
            got = GR.warp_cells(lab, row, -100)
            assert np.array_equal(got[~band], want[~band])
            cells, band_cells = cells + L * L, band_cells + int(band.sum())
    print(f"geo_ref nearest: {cells} cells, {band_cells} ({100.0 * band_cells / cells:.2f} %) inside the 2^-10 band")
    assert cells == 40 * sum(L * L for L in SIDES) and band_cells <= 0.01 * cells


@pytest.mark.parametrize("S", SIDES)
def test_the_exact_cases(S):
    """Identity, flip, the quarter turn and a shift by S / 4: the restatement moves values and blends nothing, whatever lies next to
    a selected tap."""
    rng = np.random.default_rng(S)
    x = rng.standard_normal((3, S, S)).astype(np.float32)
    x[0, 1, 1], x[1, 0, S - 1], x[2, S - 1, 0] = np.nan, np.inf, -np.inf
    lab = rng.integers(0, 150, (S, S))
    fill = (0.5, -1.0, 2.0)
    one = GR.ONE
    cases = (("identity", GR.make_row(GR.WARP), lambda a, f: a),
             ("flip", GR.make_row(GR.FLIP, (-one, 0, 0, one)), lambda a, f: a[..., ::-1]),
             ("quarter turn", GR.make_row(GR.WARP, (0, -one, one, 0)), lambda a, f: np.rot90(a, 1, (-2, -1))),
             ("half turn", GR.make_row(GR.WARP, (-one, 0, 0, -one)), lambda a, f: np.rot90(a, 2, (-2, -1))))
    for name, row, want in cases:
        got = GR.warp_pixels(x, row, fill)
        assert np.array_equal(got.astype(np.float32).view(np.int32), np.ascontiguousarray(want(x, fill)).view(np.int32)), name
        assert np.array_equal(GR.warp_cells(lab, row, -100), want(lab, -100)), name
    # tx = 16384: out[y, x] = in[y, x + S / 4], fill past the right edge (every side here is a multiple of 4)
    q = S // 4
    got = GR.warp_pixels(x, GR.make_row(GR.WARP, t=(16384, 0)), fill)
    want = np.concatenate([x[..., q:], np.broadcast_to(np.array(fill, np.float32)[:, None, None], (3, S, q))], axis=-1)
    assert np.array_equal(got.astype(np.float32).view(np.int32), want.view(np.int32))
    got = GR.warp_cells(lab, GR.make_row(GR.WARP, t=(16384, 0)), -100)
    assert np.array_equal(got, np.concatenate([lab[:, q:], np.full((S, q), -100)], axis=1))
    # and the copy: flags 0, or a row out of range
    for row in (GR.make_row(0, (0, -one, one, 0)), GR.make_row(4 | GR.WARP, (0, -one, one, 0)), GR.make_row(GR.WARP, (GR.MAX_M + 1, 0, 0, one)),
                GR.make_row(GR.WARP, t=(0, -GR.MAX_T - 1)), np.full(GR.P_WORDS, -1, np.int32)):
        assert not GR.row_is_mapped(row)
        px, lb, pw = GR.apply_ref(x[None], lab[None], None, row[None], fill, -100)
        assert np.array_equal(px.astype(np.float32).view(np.int32), x[None].view(np.int32)) and np.array_equal(lb[0], lab) and pw is None


def test_what_the_pixel_bound_tells_apart():
    """On the noise input a wrong convention is far from the restatement: align_corners=True and a tap shifted by one pixel both
    differ by more than 1e-2."""
    rng = np.random.default_rng(3)
    for S in (8, 20, 68):
        x = rng.standard_normal((3, S, S))
        row = GR.affine_row(10.0, 1.1, 5.0, 0.03, -0.02)
        ref = GR.warp_pixels(x, row, (0.0,) * 3)
        theta = torch.from_numpy(GR.theta_of(row))[None]
        wrong = F.grid_sample(torch.from_numpy(x)[None], F.affine_grid(theta, (1, 3, S, S), align_corners=True), "bilinear", "zeros",
                              align_corners=True)[0].numpy()
        assert np.abs(wrong - ref).max() > 1e-2
        assert np.abs(GR.warp_pixels(np.roll(x, 1, axis=-1), row, (0.0,) * 3) - ref).max() > 1e-2


def test_the_staged_box_holds_every_tap_of_its_tile():
    """The rule geo_apply_kernel stages by (geo_ref.tile_box: the corners' near taps, + 1, clipped, whole quads): for random maps and
    for maps at the limits, every in-image tap of every pixel of a tile lies inside the tile's box, the box lies inside the image,
    and up to S = 64 every box fits the budget."""
    rng = np.random.default_rng(11)
    rows = _random_rows(rng, 12) + [GR.make_row(GR.WARP, (GR.MAX_M, 0, 0, GR.MAX_M), (GR.MAX_T, GR.MAX_T)), GR.make_row(GR.FLIP, (-GR.ONE, 0, 0, GR.ONE)),
                                    GR.make_row(GR.WARP, (GR.MAX_M, -GR.MAX_M, -GR.MAX_M, GR.MAX_M), (-GR.MAX_T, 3)), GR.make_row(GR.WARP, (0, 0, 0, 0), (7, -7))]
    for S in (8, 20, 64, 68, 132):
        for row in rows:
            U, V = GR.source_uv(row, S)
            x0, y0 = (U + (S - 1) * GR.ONE) >> 17, (V + (S - 1) * GR.ONE) >> 17
            n = (S + GR.TILE - 1) // GR.TILE
            for ty in range(n):
                for tx in range(n):
                    w, h, bx, by = GR.tile_box(row, S, ty, tx)
                    assert w % 4 == 0 and bx % 4 == 0 and 0 <= bx and bx + w <= S and 0 <= by and by + h <= S
                    assert S > 64 or w * h <= GR.BOX_WORDS
                    sl = (slice(ty * GR.TILE, (ty + 1) * GR.TILE), slice(tx * GR.TILE, (tx + 1) * GR.TILE))
                    for dy in (0, 1):
                        for dx in (0, 1):
                            yy, xx = y0[sl] + dy, x0[sl] + dx
                            inside = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
                            assert ((yy[inside] >= by) & (yy[inside] < by + h) & (xx[inside] >= bx) & (xx[inside] < bx + w)).all()
        assert bool(GR.direct_tiles(rows[12], S)) == (S > 64)                      # the zoom-out by 8: direct from the first side that allows it
