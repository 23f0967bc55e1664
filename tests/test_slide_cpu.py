"""CPU checks of sliding-window evaluation: the window plan and evaluation size against hand-written values, the C ABI of
lc2is_resize_argmax_windows (declared, bound, exported, refusing bad arguments before any launch), the Python layer's refusals
before it allocates, metrics.dataset_iou against a hand count, and the reference-alone condition of the GPU test's fp64 cases."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import slide_ref as R  # noqa: E402

from lc2is_amd import _lib, evalloop, metrics, ops, slide  # noqa: E402


def test_plan_windows_matches_hand_written_grids():
    assert slide.plan_windows(14, 8, 4) == [0, 4, 6]
    assert slide.plan_windows(8, 8, 4) == [0]
    assert slide.plan_windows(172, 128, 85) == [0, 44]       # 683 -> 684 pixels = 171 cells of 4; 172: a 688-pixel edge
    assert slide.plan_windows(171, 128, 85) == [0, 43]
    assert slide.plan_windows(5, 8, 4) == [0]                # shorter than the window: one window at 0 (the caller pads or refuses)
    assert slide.plan_windows(12, 8, 4) == [0, 4]
    assert slide.plan_windows(13, 8, 4) == [0, 4, 5]
    with pytest.raises(ValueError):
        slide.plan_windows(8, 8, 0)


@pytest.mark.parametrize("win,stride", [(8, 4), (8, 8), (8, 3), (128, 85), (5, 7)])
def test_plan_windows_covers_every_cell(win, stride):
    for n in range(win, win + 5 * stride + 3):
        o = slide.plan_windows(n, win, stride)
        assert o == sorted(set(o)) and o[0] == 0 and o[-1] == n - win
        covered = set()
        for a in o:
            assert 0 <= a <= n - win
            covered.update(range(a, a + win))
        if stride <= win:
            assert covered == set(range(n)), (n, win, stride)
        assert all(b - a <= stride for a, b in zip(o, o[1:]))


def test_eval_size():
    assert slide.eval_size(512, 683, 512, 4) == (512, 684)   # 683 -> 684: the nearest multiple of 4
    assert slide.eval_size(683, 512, 512, 4) == (684, 512)
    assert slide.eval_size(512, 512, 512, 4) == (512, 512)
    assert slide.eval_size(300, 400, 512, 4) == (512, 684)   # int(512 * 400 / 300) = 682 -> 684
    assert slide.eval_size(512, 681, 512, 4) == (512, 680)   # 681 -> 680: rounds down too
    assert slide.eval_size(40, 70, 64, 4) == (64, 112)
    assert slide.eval_size(100, 100, 32, 4, crop=64) == (64, 64)          # never below the crop
    for H, W in ((480, 640), (1, 9), (2048, 1536), (333, 777)):
        nh, nw = slide.eval_size(H, W, 512, 4)
        assert nh % 4 == 0 and nw % 4 == 0 and min(nh, nw) == 512
    with pytest.raises(ValueError):
        slide.eval_size(512, 683, 510, 4)                    # a size off the cell grid


class _Grid:
    out_size = 128

    def to(self, device):
        return self


def test_inference_refuses_a_stride_or_size_off_the_cell_grid_before_touching_the_device():
    for kw in (dict(stride=341), dict(size=510), dict(crop=500), dict(stride=0), dict(window_batch=0)):
        with pytest.raises(ValueError):
            slide.SlidingWindowInference(_Grid(), {}, **kw)
    with pytest.raises(ValueError):
        slide.SlidingWindowInference(_Grid(), {}, grid=96)   # 512 % 96 != 0


def test_header_declares_ops_binds_and_library_exports_the_entry_point():
    s = "lc2is_resize_argmax_windows"
    assert s in _lib.header_symbols() and s in ops._ARGTYPES
    assert hasattr(_lib.load(), s)
    header = (Path(__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    assert "#define LC2IS_SLIDE_MAX_WIN 64" in header and ops.SLIDE_MAX_WIN == 64


def test_c_entry_point_refuses_before_launching():
    """Error codes come back from argument checks alone: the pointers (never dereferenced) need not be device memory."""
    f = ops._fn("lc2is_resize_argmax_windows")
    P = 0x10000   # 16-byte aligned stand-in
    ok = dict(views=P, ld=152, V=4, h=128, w=128, K=151, desc=P, N=1, win=P, n_win=4, n_tiles=1376, total_px=683 * 512, gt=P,
              gt_bytes=1, ignore=0, pred=P, counts=P, ws=P, ws_bytes=1376 * 3 * 151 * 4)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["views"], a["ld"], a["V"], a["h"], a["w"], a["K"], a["desc"], a["N"], a["win"], a["n_win"], a["n_tiles"],
                 a["total_px"], a["gt"], a["gt_bytes"], a["ignore"], a["pred"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert call(K=193, ld=196) == -3                      # LC2IS_ERR_UNSUPPORTED: K > 192
    assert call(gt_bytes=2) == -3
    assert call(views=None) == -2 and call(desc=None) == -2 and call(win=None) == -2 and call(pred=None, counts=None) == -2
    assert call(gt=None) == -2 and call(ws=None) == -2    # counts need gt and the workspace
    assert call(ld=150) == -1 and call(ld=154) == -1 and call(views=P + 4) == -1 and call(win=P + 4) == -1
    assert call(n_tiles=0) == -1 and call(V=0) == -1 and call(N=0) == -1 and call(n_win=0) == -1 and call(ignore=-2) == -1
    assert call(ws_bytes=1376 * 3 * 151 * 4 - 1) == -4    # LC2IS_ERR_WORKSPACE
    assert ops._fn("lc2is_resize_argmax_workspace_bytes")(1376, 151) == 1376 * 3 * 151 * 4   # the workspace is resize_argmax's


def test_python_layer_refuses_bad_calls_before_allocating():
    x = torch.zeros(2, 37, 8, 8)                          # CPU views
    one = [[(0, 0, 0, False), (1, 0, 6, True)]]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_argmax_windows(x, one, [(8, 14)], [(20, 30)])
    with pytest.raises(ValueError, match="covered by no window"):
        ops.resize_argmax_windows(x, one, [(8, 15)], [(20, 30)])          # column 14 uncovered
    with pytest.raises(ValueError, match="covered by no window"):
        ops.resize_argmax_windows(x, [[(0, 0, 0, False)]], [(9, 8)], [(20, 30)])
    with pytest.raises(ValueError, match="65 windows"):
        ops.resize_argmax_windows(x, [[(0, 0, 0, False)] * 65], [(8, 8)], [(20, 30)])
    with pytest.raises(ValueError, match="0 windows"):
        ops.resize_argmax_windows(x, [[]], [(8, 8)], [(20, 30)])
    with pytest.raises(ValueError, match="view index"):
        ops.resize_argmax_windows(x, [[(2, 0, 0, False)]], [(8, 8)], [(20, 30)])
    with pytest.raises(ValueError, match="view index"):
        ops.resize_argmax_windows(x, [[(-1, 0, 0, False)]], [(8, 8)], [(20, 30)])
    for oy, ox in ((0, 7), (1, 0), (-1, 0), (0, -1)):
        with pytest.raises(ValueError, match="origin"):
            ops.resize_argmax_windows(x, [[(0, 0, 0, False), (1, oy, ox, False)]], [(8, 14)], [(20, 30)])
    with pytest.raises(ValueError, match="smaller than a view"):
        ops.resize_argmax_windows(x, [[(0, 0, 0, False)]], [(7, 8)], [(20, 30)])
    with pytest.raises(ValueError):
        ops.resize_argmax_windows(x, one, [(8, 14), (8, 14)], [(20, 30)])  # one window list, two canvases
    with pytest.raises(ValueError):
        ops.resize_argmax_windows(x, one, [(8, 14)], [(20, 0)])
    with pytest.raises(ValueError, match="ignore_index"):
        ops.resize_argmax_windows(x, one, [(8, 14)], [(20, 30)], ignore_index=-1)
    with pytest.raises(RuntimeError, match="192"):
        ops.resize_argmax_windows(torch.zeros(1, 193, 8, 8), [[(0, 0, 0, False)]], [(8, 8)], [(16, 16)])
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        ops.resize_argmax_windows(x, one, [(8, 14)], None, gt=[torch.zeros(20, 30, dtype=torch.int16)])


def test_dataset_iou_against_a_hand_count():
    # classes: 0 = ignore_index, 1..3 seen, 4 never predicted nor labelled (empty union)
    inter = torch.tensor([0, 30, 10, 0, 0])
    pred = torch.tensor([5, 40, 25, 10, 0])      # class 0 predicted on 5 counted pixels: must not enter any mean
    lab = torch.tensor([0, 50, 20, 10, 0])
    d = metrics.dataset_iou(torch.stack([inter, pred, lab]), ignore_index=0)
    iou = [30 / 60, 10 / 35, 0 / 20]
    assert d["mIoU"].dtype == torch.float64 and d["mIoU"].item() == pytest.approx(sum(iou) / 3, abs=1e-15)
    assert d["mAcc"].item() == pytest.approx((30 / 50 + 10 / 20 + 0 / 10) / 3, abs=1e-15)
    assert d["aAcc"].item() == pytest.approx(40 / 80, abs=1e-15)
    assert d["IoU"].shape == (5,) and torch.isnan(d["IoU"][0]) and torch.isnan(d["IoU"][4])
    assert d["IoU"][1:4].tolist() == pytest.approx(iou, abs=1e-15)
    # without an ignored class, class 0 counts: union 5, IoU 0
    d2 = metrics.dataset_iou(torch.stack([inter, pred, lab]), ignore_index=None)
    assert d2["mIoU"].item() == pytest.approx(sum(iou) / 4, abs=1e-15) and d2["IoU"][0].item() == 0.0
    with pytest.raises(ValueError):
        metrics.dataset_iou(torch.zeros(2, 3, 5, dtype=torch.int64))
    assert hasattr(evalloop, "SlideEvaluator")


def test_canvas_mean_restatement_on_a_hand_case():
    views = torch.tensor([[[[1., 2., 3.]]], [[[10., 20., 30.]]]])        # two 1 x 3 views, K = 1
    got = R.canvas_mean(views, [(0, 0, 0, False), (1, 0, 1, True)], 1, 4)
    assert got.tolist() == [[[1.0, (2.0 + 30.0) / 2, (3.0 + 20.0) / 2, 10.0]]]
    assert R.cover_counts([(0, 0, 0, False), (1, 0, 1, True)], 1, 3, 1, 4).tolist() == [[1, 2, 2, 1]]


@pytest.mark.parametrize("args,sizes", R.FP64_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_reference_alone_fp32_restatement_agrees_with_fp64_outside_the_margin(args, sizes):
    """What the GPU test asks of the kernel, asked of torch itself: an fp32 canvas mean followed by torch's fp32 bicubic disagrees
    with the fp64 reference on no pixel outside the near-tie margin, and the share of pixels inside the margin is under the cap."""
    views, windows = R.make_case(*args)
    K, h, Hc, Wc = args[:4]
    cnt = R.cover_counts(windows, h, h, Hc, Wc)
    assert int(cnt.min()) >= 1
    c32 = R.canvas_mean(views, windows, Hc, Wc, torch.float32)
    for size in sizes:
        ref, sure, unsure = R.fp64_reference(args, size)
        got = R.fp32_argmax(c32, size)
        bad = int(((got != ref) & sure).sum())
        print(f"case {args} size {size}: unsure share {unsure:.2e}, fp32 torch disagrees outside the margin on {bad} pixels")
        assert unsure <= R.UNSURE_CAP
        assert bad == 0


def test_cases_have_the_cover_counts_the_kernel_paths_need():
    _, w1 = R.make_case(37, 8, 8, 14, 4, True)
    assert len(w1) == 6 and sorted(R.cover_counts(w1, 8, 8, 8, 14).unique().tolist()) == [2, 4, 6]
    _, w2 = R.make_case(37, 8, 12, 14, 4, False)
    assert len(w2) == 6 and sorted(R.cover_counts(w2, 8, 8, 12, 14).unique().tolist()) == [1, 2, 3, 4, 6]
