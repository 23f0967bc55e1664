"""A teacher's score map under a geometric view (lc2is_geo_scores, ops.geo_scores, GeometricAugment.warp_scores / view_distill), the
part that needs no GPU: the binding and the library's refusals (host code, before any launch), the argument checks of the wrappers,
and the properties of the numpy restatement tests/geo_scores_ref.py that tests/test_gpu_geo_scores.py holds the kernel to - above all
that its integer rule IS grid_sample with border padding."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import geo_ref as GR
import geo_scores_ref as SR

ROOT = Path(__file__).resolve().parent.parent
NAME = "lc2is_geo_scores"
ONE = GR.ONE


def test_the_header_declares_the_entry_point_and_ops_binds_it():
    from lc2is_amd import _lib, ops
    header = (ROOT / "include" / "lc2is_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert NAME in _lib.header_symbols() and hasattr(lib, NAME)
    m = re.search(rf"\bint\s+{NAME}\s*\(([^)]*)\)\s*;", code)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["in_scores", "in_tw", "params", "B", "g", "ld", "L", "want_tw", "out_scores", "out_tw",
                                                         "stream"]
    assert len(ops._ARGTYPES[NAME]) == len(args) == 11 and ops._fn(NAME).argtypes == ops._ARGTYPES[NAME]
    comment = header[:header.index(f"int {NAME}(")].rsplit("/*", 1)[1]
    for word in ("replaces:", "geo_scores_kernel", "border", "LC2IS_ERR_NULL", "LC2IS_ERR_SHAPE", "want_tw"):
        assert word in comment, word
    assert (ops.GEO_SCORES_MAX_G, ops.GEO_SCORES_MAX_LD) == (512, 1024) and callable(ops.geo_scores)
    tool = (ROOT / "tools" / "check_kernel_resources.py").read_text()
    assert '"geo_scores_kernel"' in tool
    src = (ROOT / "lc2is_amd" / "csrc" / "geo.hip").read_text()
    kernel = src[src.index("void geo_scores_kernel("):src.index("bool geo_overlap(")]
    assert "geo_map(" in kernel and "geo_narrow(" in kernel and "__shared__" not in kernel and "atomic" not in kernel


def test_the_library_refuses_null_then_shape_before_any_launch():
    """Pointers are only tested, never followed: every call below returns from the checks."""
    from lc2is_amd import ops
    f = ops._fn(NAME)
    p, big = 0x1000, 0x40000000

    def call(sc=big, tw=3 * big, params=p, B=3, g=4, ld=16, L=8, want=1, out_sc=2 * big, out_tw=4 * big):
        return f(sc, tw, params, B, g, ld, L, want, out_sc, out_tw, None)

    for missing in ("sc", "params", "out_sc", "out_tw"):                           # NULL first, whatever else is wrong
        assert call(B=0, g=0, ld=5, **{missing: None}) == -2, missing
    assert call(tw=None, B=0) == -1 and call(tw=None, out_tw=None, B=0) == -2         # in_tw may be NULL; out_tw may not, when wanted
    assert call(want=0, tw=None, out_tw=None, B=0) == -1                              # not wanted: no output to miss
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(g=0), dict(g=-3), dict(g=513), dict(ld=0), dict(ld=3), dict(ld=18), dict(ld=1028),
               dict(ld=-4), dict(L=0), dict(L=-8), dict(L=6), dict(L=4100), dict(L=2), dict(sc=big + 8), dict(sc=big + 4),
               dict(out_sc=2 * big + 4), dict(tw=3 * big + 2), dict(out_tw=4 * big + 1), dict(params=p + 2)):
        assert call(**kw) == -1, kw
    # (that want_tw == 0 leaves L and the weight pointers alone can only be seen with a launch: tests/test_gpu_geo_scores.py)
    nsc, ntw = 3 * 4 * 4 * 16 * 4, 3 * 8 * 8 * 4
    # an output overlapping its input: in place, the input's last bytes, the output's last bytes - scores, weights
    assert call(out_sc=big) == -1 and call(out_sc=big + nsc - 16) == -1 and call(out_sc=big - nsc + 16) == -1
    assert call(out_tw=3 * big) == -1 and call(out_tw=3 * big + ntw - 4) == -1 and call(out_tw=3 * big - ntw + 4) == -1
    assert call(want=0, out_sc=big) == -1


# ---- the integer rule is grid_sample with border padding ---------------------------------------------------------------------
def _rows():
    """Rotations, scale 0.25 and 4, shear, shift 0.5, flip - and their mixtures."""
    rows = [GR.affine_row(10.0), GR.affine_row(45.0, 0.8), GR.affine_row(90.0), GR.affine_row(170.0), GR.affine_row(-33.0, 1.3, 12.0, 0.07, -0.11),
            GR.affine_row(0.0, 0.25), GR.affine_row(0.0, 4.0), GR.affine_row(0.0, 1.0, 45.0), GR.affine_row(0.0, 1.0, -20.0, flip=True),
            GR.affine_row(0.0, 1.0, 0.0, 0.5, -0.5), GR.affine_row(0.0, 1.0, 0.0, -0.5, 0.5, flip=True), GR.affine_row(25.0, 0.25, 5.0, 0.5, 0.5),
            GR.affine_row(-60.0, 4.0, -45.0, -0.5, 0.25, flip=True), GR.make_row(GR.FLIP, (-ONE, 0, 0, ONE)), GR.affine_row(0.0, 0.25, flip=True)]
    rng = np.random.default_rng(17)
    rows += [GR.affine_row(rng.uniform(-180, 180), np.exp(rng.uniform(np.log(0.25), np.log(4.0))), rng.uniform(-45, 45), rng.uniform(-0.5, 0.5),
                           rng.uniform(-0.5, 0.5), bool(rng.integers(2))) for _ in range(25)]
    assert all(GR.row_is_mapped(r) for r in rows)
    return rows


def _grid_sample(x, row, mode="bilinear", padding="border"):
    """x float64 [g, g, ld] -> F.grid_sample of the recorded matrix on the [1, ld, g, g] view, back in [g, g, ld]."""
    g = x.shape[0]
    theta = torch.from_numpy(GR.theta_of(row))[None]
    grid = F.affine_grid(theta, (1, 1, g, g), align_corners=False)
    out = F.grid_sample(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None], grid, mode, padding, align_corners=False)
    return out[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("g", [5, 8, 32])
def test_the_restated_scores_are_bilinear_grid_sample_with_border_padding(g):
    rng = np.random.default_rng(200 + g)
    x = rng.standard_normal((g, g, 12))
    worst = 0.0
    for row in _rows():
        worst = max(worst, np.abs(SR.warp_scores(x, row) - _grid_sample(x, row)).max())
    print(f"geo_scores_ref g={g}: max |integer rule - fp64 grid_sample(border)| over {len(_rows())} maps = {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("L,g", [(5, 5), (8, 8), (32, 8), (112, 7), (128, 32)])
def test_the_restated_weights_are_the_cell_rule_with_zero_outside(L, g):
    rng = np.random.default_rng(L)
    tw = rng.random((3, L, L)).astype(np.float32)
    rows = _rows()
    outside = 0
    for j in range(0, len(rows) - 2, 3):
        pick = np.stack(rows[j:j + 3])
        sc = rng.standard_normal((3 * g * g, 4)).astype(np.float32)
        _, got = SR.scores_ref(sc, tw, pick, 3, g, L)
        _, mask = SR.scores_ref(sc, None, pick, 3, g, L)
        for b in range(3):
            assert np.array_equal(got[b].view(np.int32), GR.warp_cells(tw[b], pick[b], 0.0).view(np.int32))
            inside = GR.cell_index(pick[b], L)[2]
            assert np.array_equal(mask[b], inside.astype(np.float32)) and mask.dtype == np.float32
            outside += int((~inside).sum())
    assert outside > 0
    # a copy row: the weights themselves, or ones; no weight map asked for: none made
    copy = np.stack([GR.make_row(0, (0, -ONE, ONE, 0)), GR.make_row(4 | GR.WARP), GR.make_row(GR.WARP, t=(GR.MAX_T + 1, 0))])
    sc = rng.standard_normal((3 * g * g, 4)).astype(np.float32)
    out, got = SR.scores_ref(sc, tw, copy, 3, g, L)
    assert np.array_equal(got, tw) and np.array_equal(out, sc.astype(np.float64))
    assert (SR.scores_ref(sc, None, copy, 3, g, L)[1] == 1.0).all() and SR.scores_ref(sc, None, copy, 3, g)[1] is None


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@pytest.mark.parametrize("g", [5, 8, 32])
def test_the_exact_cases(g):
    """Copy, flip, quarter and half turn (and at g = 8 a whole-cell shift): the restatement moves values and blends nothing, whatever
    lies next to a selected tap."""
    rng = np.random.default_rng(g)
    x = rng.standard_normal((g, g, 8)).astype(np.float32)
    x[1, 1, 0], x[0, g - 1, 3], x[g - 1, 0, 5] = np.nan, np.inf, -np.inf
    x.view(np.int32)[2, 3, 1] = 0x7FC12345
    cases = (("identity", GR.make_row(GR.WARP), lambda a: a), ("flip", GR.make_row(GR.FLIP, (-ONE, 0, 0, ONE)), lambda a: a[:, ::-1]),
             ("quarter turn", GR.make_row(GR.WARP, (0, -ONE, ONE, 0)), lambda a: np.rot90(a, 1, (0, 1))),
             ("half turn", GR.make_row(GR.WARP, (-ONE, 0, 0, -ONE)), lambda a: np.rot90(a, 2, (0, 1))),
             ("three quarter turns", GR.make_row(GR.WARP, (0, ONE, -ONE, 0)), lambda a: np.rot90(a, 3, (0, 1))))
    for name, row, want in cases:
        assert SR.is_exact(row, g), name
        assert np.array_equal(_bits(SR.warp_scores(x, row)), _bits(want(x))), name
        assert np.array_equal(_bits(SR.select_scores(x, row)), _bits(want(x))), name
    for row in (GR.make_row(0, (0, -ONE, ONE, 0)), GR.make_row(4 | GR.WARP, (0, -ONE, ONE, 0)), GR.make_row(GR.WARP, (GR.MAX_M + 1, 0, 0, ONE)),
                GR.make_row(GR.WARP, t=(0, -GR.MAX_T - 1)), np.full(GR.P_WORDS, -1, np.int32)):
        assert not GR.row_is_mapped(row)
        out, _ = SR.scores_ref(x.reshape(g * g, 8), None, row[None], 1, g)
        assert np.array_equal(_bits(out), _bits(x.reshape(g * g, 8)))
    assert not SR.is_exact(GR.affine_row(10.0), g)
    if g == 8:
        # tx = 1 / 8 of the side: out[y, x] = in[y, x + 1], the border cell repeated past the right edge; ty = -2 / 8: two cells down
        got = SR.warp_scores(x, GR.make_row(GR.WARP, t=(8192, 0)))
        assert SR.is_exact(GR.make_row(GR.WARP, t=(8192, 0)), g)
        assert np.array_equal(_bits(got), _bits(np.concatenate([x[:, 1:], x[:, -1:]], axis=1)))
        got = SR.warp_scores(x, GR.make_row(GR.WARP, t=(0, -16384)))
        assert np.array_equal(_bits(got), _bits(np.concatenate([x[:1], x[:1], x[:-2]], axis=0)))


def test_what_the_bound_tells_apart():
    """On noise a zeros-padding reference and a tap shifted by one cell are both far from the restatement (more than 1e-2): the bound
    the GPU tests hold the kernel to (2.9e-6 of the largest input) separates right from wrong."""
    rng = np.random.default_rng(3)
    for g in (5, 8, 32):
        x = rng.standard_normal((g, g, 12))
        for row in (GR.affine_row(0.0, 0.25), GR.affine_row(10.0, 1.0, 0.0, 0.5, -0.5), GR.affine_row(45.0, 0.8)):
            ref = SR.warp_scores(x, row)
            zeros = np.abs(_grid_sample(x, row, padding="zeros") - ref).max()
            shifted = np.abs(SR.warp_scores(np.roll(x, 1, axis=1), row) - ref).max()
            print(f"geo_scores_ref g={g}: zeros padding differs by {zeros:.2f}, a tap shifted by one cell by {shifted:.2f}")
            assert zeros > 1e-2 and shifted > 1e-2
        # and in the frame of a gentle map the two paddings agree: the difference above is the border's alone
        row = GR.affine_row(10.0)
        in_frame = SR.split(row, g)[4]
        d = np.abs(_grid_sample(x, row, padding="zeros") - SR.warp_scores(x, row)).max(axis=-1)
        assert in_frame.any() and d[in_frame].max() <= 1e-13


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_bad_arguments_before_device_work():
    from lc2is_amd import ops
    from lc2is_amd.data import GeometricAugment
    geo = GeometricAugment()
    B, g, ld, L = 2, 4, 16, 8
    sc, tw = torch.zeros(B * g * g, ld), torch.zeros(B, L, L)
    table = torch.zeros(B, ops.GEO_PARAM_WORDS, dtype=torch.int32)
    # ops.geo_scores: types first, then the device
    for kw in (dict(B=2.0), dict(B=True), dict(g="4"), dict(g=None), dict(label_size=8.0), dict(out=sc), dict(out=(sc,)), dict(out=(sc, tw, tw)),
               dict(scores=sc.numpy()), dict(scores=None), dict(teacher_weight=tw.numpy()), dict(out=(sc.numpy(), None))):
        a = dict(scores=sc, params=table, B=B, g=g, teacher_weight=None, label_size=None, out=None)
        a.update(kw)
        with pytest.raises(TypeError):
            ops.geo_scores(a["scores"], a["params"], a["B"], a["g"], teacher_weight=a["teacher_weight"], label_size=a["label_size"], out=a["out"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.geo_scores(sc, table, B, g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.geo_scores(sc, table, B, g, teacher_weight=tw)
    # warp_scores: no table yet; then types, then shapes, then the device
    with pytest.raises(RuntimeError, match="table"):
        geo.warp_scores(sc)
    for kw in (dict(scores=sc.double()), dict(scores=sc.numpy()), dict(scores=None), dict(teacher_weight=tw.double()), dict(teacher_weight=tw.int()),
               dict(label_size=8.0), dict(label_size=True), dict(params=table.long()), dict(params=table.numpy())):
        a = dict(scores=sc, teacher_weight=None, label_size=None, params=table)
        a.update(kw)
        with pytest.raises(TypeError):
            geo.warp_scores(a["scores"], a["teacher_weight"], a["label_size"], params=a["params"])
    for kw in (dict(scores=torch.zeros(B * g * g + 1, ld)), dict(scores=torch.zeros(B * 15, ld)), dict(scores=torch.zeros(B, g * g, ld)),
               dict(scores=torch.zeros(1, ld)), dict(scores=torch.zeros(B * g * g, 18)), dict(scores=torch.zeros(B * g * g, 2)),
               dict(scores=torch.zeros(B * g * g, 1028)), dict(scores=torch.zeros(B * 513 * 513, 0)), dict(teacher_weight=torch.zeros(B, L, L + 1)),
               dict(teacher_weight=torch.zeros(B + 1, L, L)), dict(teacher_weight=torch.zeros(B, 6, 6)), dict(teacher_weight=torch.zeros(B, L)),
               dict(label_size=6), dict(label_size=0), dict(label_size=-8), dict(label_size=4100), dict(teacher_weight=tw, label_size=16),
               dict(params=torch.zeros(B, 8, dtype=torch.int32)), dict(params=torch.zeros(ops.GEO_PARAM_WORDS, dtype=torch.int32)),
               dict(params=torch.zeros(0, ops.GEO_PARAM_WORDS, dtype=torch.int32))):
        a = dict(scores=sc, teacher_weight=None, label_size=None, params=table)
        a.update(kw)
        with pytest.raises(ValueError):
            geo.warp_scores(a["scores"], a["teacher_weight"], a["label_size"], params=a["params"])
    for kw in (dict(), dict(teacher_weight=tw), dict(label_size=L)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            geo.warp_scores(sc, params=table, **kw)
    # view_distill: the same checks, before the view is made
    px, lab, keys = torch.zeros(B, 3, 16, 16), torch.zeros(B, L, L, dtype=torch.int64), torch.arange(B)
    inputs = {"pixel_values": px, "input_ids": None}
    with pytest.raises(TypeError):
        geo.view_distill(inputs, lab, sc.double(), keys, 0)
    with pytest.raises(TypeError):
        geo.view_distill(inputs, lab, sc, keys, 0, teacher_weight=tw.double())
    with pytest.raises(TypeError):
        geo.view_distill({"pixel_values": None}, lab, sc, keys, 0)
    for bad in (torch.zeros(B * 15, ld), torch.zeros(B * g * g, 18), torch.zeros(B * 9, ld)):     # (g = 3 does not divide L = 8)
        with pytest.raises(ValueError):
            geo.view_distill(inputs, lab, bad, keys, 0)
    with pytest.raises(ValueError):
        geo.view_distill(inputs, None, sc, keys, 0)                                # nothing gives the size of the mask
    with pytest.raises(ValueError):
        geo.view_distill(inputs, lab, sc, keys, 0, teacher_weight=torch.zeros(B, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        geo.view_distill(inputs, lab, sc, keys, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geo.view_distill(inputs, None, sc, keys, 0, pixel_weight=tw, teacher_weight=tw)
    assert geo.last_params is None


def test_the_soft_recipe_warps_the_teacher_scores_with_the_view():
    from lc2is_amd import selftrain
    from lc2is_amd.data import GeometricAugment
    doc = selftrain.__doc__
    recipe, scope = doc[:doc.index("Out of scope here")], doc[doc.index("Out of scope here"):]
    assert "geo.view_distill(" in recipe and "step.step_distill(" in recipe and "teacher_weight=" in recipe
    assert recipe.index("head_scores(weak") < recipe.index("geo.view_distill(")
    assert "inverse map" in scope
    assert "border" in GeometricAugment.warp_scores.__doc__ and "mask" in GeometricAugment.view_distill.__doc__
    readme, integration = (ROOT / "README.md").read_text(), (ROOT / "INTEGRATION.md").read_text()
    assert "geo_scores" in readme and "view_distill" in readme and "lc2is_geo_scores" in integration
