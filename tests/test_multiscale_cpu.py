"""CPU checks of multi-scale evaluation: the scale -> size, plan and canvas logic against hand-written values, the 16-canvas
limit, the C ABI of lc2is_resize_argmax_multiscale (declared, bound, exported, refusing bad arguments before any launch), the
Python layer's refusals before it allocates, and the reference alone: its unsure shares under the cap for both cases and modes, and
one canvas giving slide_ref.fp64_reference."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multiscale_ref as M  # noqa: E402
import slide_ref as R  # noqa: E402

from lc2is_amd import _lib, ops, slide  # noqa: E402


def test_scale_size_rounds_to_the_cell_grid():
    assert [slide.scale_size(512, s, 4) for s in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)] == [256, 384, 512, 640, 768, 896]
    assert [slide.scale_size(64, s, 4) for s in (0.5, 1.0, 1.5)] == [32, 64, 96]
    assert slide.scale_size(64, 0.53, 4) == 32 and slide.scale_size(64, 0.54, 4) == 36      # 33.92 -> 32, 34.56 -> 36
    assert slide.scale_size(64, 0.01, 4) == 4                                                # never below one cell


def test_plan_multiscale_matches_hand_written_plans():
    # crop 64, cells of 4 (grid 16), stride 40 = 10 cells
    got = slide.plan_multiscale(40, 70, (0.5, 1.0, 1.5), 64, 64, 40, 4)
    assert got[0] == ((32, 56), (8, 14), [(0, 0)])                       # below the crop: one window that overhangs the canvas
    assert got[1] == ((64, 112), (16, 28), [(0, 0), (0, 10), (0, 12)])   # SlidingWindowInference's plan
    assert got[2] == ((96, 168), (24, 42), [(oy, ox) for oy in (0, 8) for ox in (0, 10, 20, 26)])
    got = slide.plan_multiscale(50, 50, (0.5, 1.0, 1.5), 64, 64, 40, 4)
    assert got == [((32, 32), (8, 8), [(0, 0)]), ((64, 64), (16, 16), [(0, 0)]),
                   ((96, 96), (24, 24), [(0, 0), (0, 8), (8, 0), (8, 8)])]
    # short in y only: 20 x 90 at scale 0.5 -> 32 x 144: the x axis is windowed, every window overhangs in y
    assert slide.plan_multiscale(20, 90, (0.5,), 64, 64, 40, 4) == [((32, 144), (8, 36), [(0, 0), (0, 10), (0, 20)])]
    # the real recipe on a 512 x 683 image: 256 x 341 -> 340 pixels = 85 cells, one window; 1.75 -> 896 x 1195 -> 1196
    real = slide.plan_multiscale(512, 683, (0.5, 1.75), 512, 512, 340, 4)
    assert real[0] == ((256, 340), (64, 85), [(0, 0)])
    assert real[1][:2] == ((896, 1196), (224, 299)) and len(real[1][2]) == 3 * 4
    # edges are rounded to the nearest cell, as eval_size does: 30 x 47 at 32 -> int(32 * 47 / 30) = 50 -> 52
    assert slide.plan_multiscale(30, 47, (0.5,), 64, 64, 40, 4)[0][:2] == ((32, 52), (8, 13))


def test_multiscale_canvases_orders_views_and_splits_flips():
    plan = slide.plan_multiscale(40, 70, (0.5, 1.0), 64, 64, 40, 4)
    cl, n = slide.multiscale_canvases(plan, 5, True, "prob")
    assert n == 8 and cl == [((8, 14), [(5, 0, 0, False)]), ((8, 14), [(6, 0, 0, True)]),
                             ((16, 28), [(7, 0, 0, False), (8, 0, 10, False), (9, 0, 12, False)]),
                             ((16, 28), [(10, 0, 0, True), (11, 0, 10, True), (12, 0, 12, True)])]
    cl, n = slide.multiscale_canvases(plan, 0, True, "logit")
    assert n == 8 and cl == [((8, 14), [(0, 0, 0, False), (1, 0, 0, True)]),
                             ((16, 28), [(2, 0, 0, False), (3, 0, 10, False), (4, 0, 12, False),
                                         (5, 0, 0, True), (6, 0, 10, True), (7, 0, 12, True)])]
    for average in ("prob", "logit"):
        cl, n = slide.multiscale_canvases(plan, 0, False, average)
        assert n == 4 and cl == [((8, 14), [(0, 0, 0, False)]), ((16, 28), [(1, 0, 0, False), (2, 0, 10, False), (3, 0, 12, False)])]


class _Grid:
    out_size = 128

    def to(self, device):
        return self


def test_inference_refuses_more_than_sixteen_canvases_and_bad_arguments_before_touching_the_device():
    nine = tuple(0.5 + 0.125 * i for i in range(9))
    with pytest.raises(ValueError, match="18 canvases"):
        slide.MultiScaleInference(_Grid(), {}, scales=nine, flip=True, average="prob")
    with pytest.raises(ValueError, match="17 canvases"):
        slide.MultiScaleInference(_Grid(), {}, scales=tuple(0.5 + 0.1 * i for i in range(17)), flip=True, average="logit")
    for kw in (dict(average="mean"), dict(scales=()), dict(scales=(1.0, 0.0)), dict(scales=(-1.0,)), dict(stride=341), dict(size=510)):
        with pytest.raises(ValueError):
            slide.MultiScaleInference(_Grid(), {}, **kw)
    assert issubclass(slide.MultiScaleInference, slide.SlidingWindowInference)
    # 9 scales as logits (9 canvases) and 8 with flip as probabilities (16) pass the limit: the next refusal is the device's
    for kw in (dict(scales=nine, average="logit"), dict(scales=nine[:8], average="prob")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            slide.MultiScaleInference(_Grid(), {}, device="cpu", **kw)


def test_header_declares_ops_binds_and_library_exports_the_entry_point():
    s = "lc2is_resize_argmax_multiscale"
    assert s in _lib.header_symbols() and s in ops._ARGTYPES
    assert hasattr(_lib.load(), s)
    header = (Path(__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    assert "#define LC2IS_MS_MAX_CANVAS 16" in header and ops.MS_MAX_CANVAS == 16
    assert "#define LC2IS_MS_LOGIT 0" in header and "#define LC2IS_MS_PROB 1" in header
    assert ops._MS_MODES == {"logit": 0, "prob": 1}


def test_c_entry_point_refuses_before_launching():
    """Error codes come back from argument checks alone: the pointers (never dereferenced) need not be device memory."""
    f = ops._fn("lc2is_resize_argmax_multiscale")
    P = 0x10000   # 16-byte aligned stand-in
    ok = dict(views=P, ld=152, V=4, h=128, w=128, K=151, desc=P, N=1, canv=P, n_canv=12, win=P, n_win=4, n_tiles=1376,
              total_px=683 * 512, gt=P, gt_bytes=1, ignore=0, mode=1, pred=P, counts=P, ws=P, ws_bytes=1376 * 3 * 151 * 4)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["views"], a["ld"], a["V"], a["h"], a["w"], a["K"], a["desc"], a["N"], a["canv"], a["n_canv"], a["win"], a["n_win"],
                 a["n_tiles"], a["total_px"], a["gt"], a["gt_bytes"], a["ignore"], a["mode"], a["pred"], a["counts"], a["ws"],
                 a["ws_bytes"], None)

    assert call(mode=2) == -1 and call(mode=-1) == -1     # LC2IS_ERR_SHAPE: a mode outside {0, 1}
    assert call(K=193, ld=196) == -3                      # LC2IS_ERR_UNSUPPORTED: K > 192
    assert call(gt_bytes=2) == -3
    assert call(views=None) == -2 and call(desc=None) == -2 and call(canv=None) == -2 and call(win=None) == -2
    assert call(pred=None, counts=None) == -2
    assert call(gt=None) == -2 and call(ws=None) == -2    # counts need gt and the workspace
    assert call(ld=150) == -1 and call(ld=154) == -1 and call(views=P + 4) == -1 and call(win=P + 4) == -1
    assert call(n_tiles=0) == -1 and call(V=0) == -1 and call(N=0) == -1 and call(n_win=0) == -1 and call(n_canv=0) == -1
    assert call(ignore=-2) == -1
    assert call(ws_bytes=1376 * 3 * 151 * 4 - 1) == -4    # LC2IS_ERR_WORKSPACE


def test_python_layer_refuses_bad_calls_before_allocating():
    x = torch.zeros(2, 37, 8, 8)                          # CPU views
    f = ops.resize_argmax_multiscale
    one = [[((8, 14), [(0, 0, 0, False), (1, 0, 6, True)])]]
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(x, one, [(20, 30)])
    with pytest.raises(RuntimeError, match="no CPU path"):                 # a canvas smaller than a view is allowed here
        f(x, [[((5, 7), [(0, 0, 0, False)]), ((8, 14), one[0][0][1])]], [(20, 30)], mode="logit")
    with pytest.raises(ValueError, match="mode"):
        f(x, one, [(20, 30)], mode="mean")
    with pytest.raises(ValueError, match="covered by no window"):
        f(x, [[((8, 15), one[0][0][1])]], [(20, 30)])                      # column 14 uncovered
    with pytest.raises(ValueError, match="covered by no window"):
        f(x, [[((9, 7), [(0, 0, 0, False)])]], [(20, 30)])                 # overhangs along x, row 8 uncovered
    with pytest.raises(ValueError, match="0 canvases"):
        f(x, [[]], [(20, 30)])
    with pytest.raises(ValueError, match="17 canvases"):
        f(x, [one[0] * 17], [(20, 30)])
    with pytest.raises(ValueError, match="65 windows"):
        f(x, [[((8, 8), [(0, 0, 0, False)] * 65)]], [(20, 30)])
    with pytest.raises(ValueError, match="0 windows"):
        f(x, [[((8, 8), [])]], [(20, 30)])
    for view in (2, -1):
        with pytest.raises(ValueError, match="view index"):
            f(x, [[((8, 8), [(view, 0, 0, False)])]], [(20, 30)])
    for oy, ox in ((0, 14), (8, 0), (-1, 0), (0, -1)):
        with pytest.raises(ValueError, match="origin"):
            f(x, [[((8, 14), [(0, 0, 0, False), (1, 0, 6, False), (1, oy, ox, False)])]], [(20, 30)])
    with pytest.raises(ValueError):
        f(x, one * 2, [(20, 30)])                                          # two images, one size
    with pytest.raises(ValueError):
        f(x, one, [(20, 0)])
    with pytest.raises(ValueError, match="ignore_index"):
        f(x, one, [(20, 30)], ignore_index=-1)
    with pytest.raises(RuntimeError, match="192"):
        f(torch.zeros(1, 193, 8, 8), [[((8, 8), [(0, 0, 0, False)])]], [(16, 16)])
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        f(x, one, None, gt=[torch.zeros(20, 30, dtype=torch.int16)])
    with pytest.raises(ValueError, match="smaller than a view"):           # ... and stays refused by the one-canvas op
        ops.resize_argmax_windows(x, [[(0, 0, 0, False)]], [(5, 7)], [(20, 30)])


def test_canvas_mean_with_overhanging_windows_on_a_hand_case():
    P = M.POISON
    views = torch.tensor([[[[1., 2., 3.]]], [[[20., 10., P]]], [[[5., P, P]]]])      # three 1 x 3 views, K = 1
    # canvas 1 x 4: view 0 at 0, view 1 mirrored at 2 (two cells on the canvas: 10, 20), view 2 at 3 (one cell)
    wl = [(0, 0, 0, False), (1, 0, 2, True), (2, 0, 3, False)]
    assert M.canvas_mean(views, wl, 1, 4).tolist() == [[[1.0, 2.0, (3.0 + 10.0) / 2, (20.0 + 5.0) / 2]]]
    # windows inside the canvas: slide_ref's restatement
    v, w = R.make_case(37, 8, 8, 14, 4, True)
    assert torch.equal(M.canvas_mean(v, w, 8, 14), R.canvas_mean(v, w, 8, 14))


def test_cases_overhang_and_poison_where_the_kernel_paths_need_it():
    views, canvases, amax = M.make_case("small")
    assert [c for c, _ in canvases] == [(8, 12), (12, 18), (5, 7), (14, 6)] and amax < 10
    assert [len(w) for _, w in canvases] == [2, 2 * 2 * 4, 1, 2 * 3]
    assert canvases[2][1] == ((18, 0, 0, False),) and (views[18][:, 5:, :] == M.POISON).all() and (views[18][:, :, 7:] == M.POISON).all()
    assert all(ox == 0 for _, _, ox, _ in canvases[3][1]) and [m for *_, m in canvases[3][1]] == [False, True] * 3
    assert (views[19:, :, :, 6:] == M.POISON).all() and not (views[:18] == M.POISON).any()
    views, canvases, _ = M.make_case("real_k")
    assert [len(w) for _, w in canvases] == [2, 4, 2 * 3, 1] and (views[-1][:, 20:, :] == M.POISON).all()


@pytest.mark.parametrize("name", list(M.CASES))
@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_reference_alone_unsure_share_is_under_the_cap_and_fp32_torch_agrees_outside_the_margin(name, mode):
    """A condition on the inputs, asked of the fp64 reference alone (the GPU test asserts the same figures), and what the GPU test
    asks of the kernel, asked of torch's own fp32 arithmetic: no disagreement with fp64 outside the near-tie margin."""
    for size in M.CASES[name][3]:
        ref, sure, unsure = M.fp64_reference(name, size, mode)
        got = M.fp32_argmax(*M.make_case(name)[:2], size, mode)
        bad = int(((got != ref) & sure).sum())
        print(f"case {name} mode {mode} size {size}: unsure share {unsure:.2e}, fp32 torch disagrees outside the margin on {bad} pixels")
        assert ref.shape == size and unsure <= R.UNSURE_CAP
        assert bad == 0


@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_one_canvas_reference_is_slide_refs(mode):
    """One canvas: the argmax of a softmax is the argmax of the logits, so both modes give slide_ref.fp64_reference's argmax, and
    the logit margin is slide_ref's."""
    args = (37, 8, 8, 14, 4, True)
    views, windows = R.make_case(*args)
    amax = views.abs().max().item()
    for size in ((50, 90), (5, 9), (33, 17), (1, 1)):
        want, want_sure, _ = R.fp64_reference(args, size)
        ref, sure, _ = M.ref_argmax(views, [((8, 14), windows)], size, mode, amax)
        assert torch.equal(ref, want)
        if mode == "logit":
            assert torch.equal(sure, want_sure)
