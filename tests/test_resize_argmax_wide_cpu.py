"""CPU-side checks of the resize + argmax entries past 192 classes (lc2is_resize_argmax_wide, _windows_wide, _multiscale_wide):
the C ABI is declared and bound, the workspace query is a pure host function with the stated formula, every C entry point returns
its codes from argument checks alone, the Python wrappers and the layers above them refuse bad calls before they allocate, and
the fp64 references of the GPU tests stay under the near-tie cap on their own."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resize_wide_ref as W  # noqa: E402
import slide_ref as R  # noqa: E402

from lc2is_amd import _lib, metrics, ops  # noqa: E402

SYMS = ("lc2is_resize_argmax_wide_workspace_bytes", "lc2is_resize_argmax_wide", "lc2is_resize_argmax_windows_wide",
        "lc2is_resize_argmax_multiscale_wide")
P = 0x10000   # 16-byte aligned stand-in pointer, never dereferenced
TILES, PX = 1376, 683 * 512
WS847 = TILES * 3 * 847 * 4


def test_header_declares_ops_binds_and_library_exports_the_four_symbols():
    syms = _lib.header_symbols()
    for s in SYMS:
        assert s in syms and s in ops._ARGTYPES
        assert hasattr(_lib.load(), s)
    header = (Path(__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    assert "#define LC2IS_RESIZE_WIDE_KMAX 1024" in header and ops.RESIZE_WIDE_KMAX == 1024 and ops.RESIZE_KMAX == 192
    for narrow, wide in zip(("lc2is_resize_argmax", "lc2is_resize_argmax_windows", "lc2is_resize_argmax_multiscale"), SYMS[1:]):
        assert ops._ARGTYPES[wide] == ops._ARGTYPES[narrow]           # the narrow argument list, pred a pointer either way


def test_workspace_query_is_a_pure_host_function():
    ws = ops._fn("lc2is_resize_argmax_wide_workspace_bytes")
    assert ws(5, 847) == 5 * 3 * 847 * 4
    assert ws(1, 1024) == 1 * 3 * 1024 * 4 and ws(3, 151) == 3 * 3 * 151 * 4
    assert ws(10, 1025) == 0 and ws(0, 847) == 0 and ws(10, 0) == 0
    # the sizes the header states: 12 KB per tile at K = 1024, 14 MB and 125 MB per image at K = 847
    assert ws(1, 1024) == 12 * 1024
    assert round(ws(TILES, 847) / 1e6) == 14 and round(ws(12288, 847) / 1e6) == 125
    assert ops._fn("lc2is_resize_argmax_workspace_bytes")(10, 193) == 0   # the narrow query keeps its limit


def test_resize_argmax_wide_refuses_before_launching():
    f = ops._fn("lc2is_resize_argmax_wide")
    ok = dict(scores=P, ld=848, N=1, h=128, w=128, K=847, desc=P, n_tiles=TILES, total_px=PX, gt=P, gt_bytes=1, pred=P, counts=P,
              ws=P, ws_bytes=WS847)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["scores"], a["ld"], a["N"], a["h"], a["w"], a["K"], a["desc"], a["n_tiles"], a["total_px"], a["gt"],
                 a["gt_bytes"], a["pred"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert call(K=1025, ld=1028) == -3                    # LC2IS_ERR_UNSUPPORTED: K > 1024
    assert call(gt_bytes=2) == -3
    assert call(scores=None) == -2 and call(desc=None) == -2 and call(pred=None, counts=None) == -2
    assert call(gt=None) == -2 and call(ws=None) == -2    # counts need gt and the workspace
    assert call(ld=846) == -1 and call(ld=850) == -1 and call(scores=P + 4) == -1 and call(n_tiles=0) == -1
    assert call(ws_bytes=WS847 - 1) == -4                 # LC2IS_ERR_WORKSPACE
    assert call(scores=None, K=1025) == -2 and call(ld=846, K=1025) == -1 and call(K=1025, ld=1028, ws_bytes=0) == -3   # the order


def test_resize_argmax_windows_wide_refuses_before_launching():
    f = ops._fn("lc2is_resize_argmax_windows_wide")
    ok = dict(views=P, ld=848, V=4, h=128, w=128, K=847, desc=P, N=1, win=P, n_win=4, n_tiles=TILES, total_px=PX, gt=P,
              gt_bytes=1, ignore=0, pred=P, counts=P, ws=P, ws_bytes=WS847)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["views"], a["ld"], a["V"], a["h"], a["w"], a["K"], a["desc"], a["N"], a["win"], a["n_win"], a["n_tiles"],
                 a["total_px"], a["gt"], a["gt_bytes"], a["ignore"], a["pred"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert call(K=1025, ld=1028) == -3
    assert call(gt_bytes=2) == -3
    assert call(views=None) == -2 and call(desc=None) == -2 and call(win=None) == -2 and call(pred=None, counts=None) == -2
    assert call(gt=None) == -2 and call(ws=None) == -2
    assert call(ld=846) == -1 and call(ld=850) == -1 and call(views=P + 4) == -1 and call(win=P + 4) == -1
    assert call(n_tiles=0) == -1 and call(V=0) == -1 and call(N=0) == -1 and call(n_win=0) == -1 and call(ignore=-2) == -1
    assert call(ws_bytes=WS847 - 1) == -4


def test_resize_argmax_multiscale_wide_refuses_before_launching():
    f = ops._fn("lc2is_resize_argmax_multiscale_wide")
    ok = dict(views=P, ld=848, V=4, h=128, w=128, K=847, desc=P, N=1, canv=P, n_canv=12, win=P, n_win=4, n_tiles=TILES,
              total_px=PX, gt=P, gt_bytes=1, ignore=0, mode=1, pred=P, counts=P, ws=P, ws_bytes=WS847)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["views"], a["ld"], a["V"], a["h"], a["w"], a["K"], a["desc"], a["N"], a["canv"], a["n_canv"], a["win"], a["n_win"],
                 a["n_tiles"], a["total_px"], a["gt"], a["gt_bytes"], a["ignore"], a["mode"], a["pred"], a["counts"], a["ws"],
                 a["ws_bytes"], None)

    assert call(mode=2) == -1 and call(mode=-1) == -1     # LC2IS_ERR_SHAPE: a mode outside {0, 1}
    assert call(K=1025, ld=1028) == -3
    assert call(gt_bytes=2) == -3
    assert call(views=None) == -2 and call(desc=None) == -2 and call(canv=None) == -2 and call(win=None) == -2
    assert call(pred=None, counts=None) == -2
    assert call(gt=None) == -2 and call(ws=None) == -2
    assert call(ld=846) == -1 and call(ld=850) == -1 and call(views=P + 4) == -1 and call(win=P + 4) == -1
    assert call(n_tiles=0) == -1 and call(V=0) == -1 and call(N=0) == -1 and call(n_win=0) == -1 and call(n_canv=0) == -1
    assert call(ignore=-2) == -1
    assert call(ws_bytes=WS847 - 1) == -4
    assert call(mode=0, ws_bytes=WS847 - 1) == -4 and call(mode=0, K=1025, ld=1028) == -3


def _gt(H, W, dtype=torch.int64):
    return torch.zeros(H, W, dtype=dtype)


def test_resize_argmax_wide_wrapper_refuses_bad_calls_before_allocating():
    x = torch.zeros(2, 847, 8, 8)                         # CPU scores
    f = ops.resize_argmax_wide
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(x, [(5, 7), (9, 3)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(torch.zeros(1, 37, 8, 8), [(5, 7)])             # any 1 <= K <= 1024 is taken
    with pytest.raises(RuntimeError, match="1024"):
        f(torch.zeros(1, 1025, 8, 8), [(16, 16)])
    with pytest.raises(RuntimeError, match="NCHW"):
        f(torch.zeros(847, 8, 8), [(16, 16)])
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        f(x, None, gt=[_gt(5, 7, torch.int16), _gt(9, 3)])
    with pytest.raises(ValueError, match="shapes"):
        f(x, [(5, 7), (3, 9)], gt=[_gt(5, 7), _gt(9, 3)])
    with pytest.raises(ValueError):
        f(x, [(5, 7)], gt=[_gt(5, 7)])                    # one gt map for two images
    with pytest.raises(ValueError):
        f(x, [(5, 7), (0, 3)])
    with pytest.raises(ValueError, match="nothing to compute"):
        f(x, [(5, 7), (9, 3)], want_pred=False)


def test_resize_argmax_windows_wide_wrapper_refuses_bad_calls_before_allocating():
    x = torch.zeros(2, 257, 8, 8)
    f = ops.resize_argmax_windows_wide
    one = [[(0, 0, 0, False), (1, 0, 6, True)]]
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(x, one, [(8, 14)], [(20, 30)])
    with pytest.raises(RuntimeError, match="1024"):
        f(torch.zeros(1, 1025, 8, 8), [[(0, 0, 0, False)]], [(8, 8)], [(16, 16)])
    with pytest.raises(ValueError, match="covered by no window"):
        f(x, one, [(8, 15)], [(20, 30)])
    with pytest.raises(ValueError, match="covered by no window"):
        f(x, [[(0, 0, 0, False)]], [(9, 8)], [(20, 30)])
    with pytest.raises(ValueError, match="65 windows"):
        f(x, [[(0, 0, 0, False)] * 65], [(8, 8)], [(20, 30)])
    with pytest.raises(ValueError, match="0 windows"):
        f(x, [[]], [(8, 8)], [(20, 30)])
    for view in (2, -1):
        with pytest.raises(ValueError, match="view index"):
            f(x, [[(view, 0, 0, False)]], [(8, 8)], [(20, 30)])
    for oy, ox in ((0, 7), (1, 0), (-1, 0), (0, -1)):
        with pytest.raises(ValueError, match="origin"):
            f(x, [[(0, 0, 0, False), (1, oy, ox, False)]], [(8, 14)], [(20, 30)])
    with pytest.raises(ValueError, match="smaller than a view"):
        f(x, [[(0, 0, 0, False)]], [(7, 8)], [(20, 30)])
    with pytest.raises(ValueError):
        f(x, one, [(8, 14), (8, 14)], [(20, 30)])
    with pytest.raises(ValueError):
        f(x, one, [(8, 14)], [(20, 0)])
    with pytest.raises(ValueError, match="ignore_index"):
        f(x, one, [(8, 14)], [(20, 30)], ignore_index=-1)
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        f(x, one, [(8, 14)], None, gt=[torch.zeros(20, 30, dtype=torch.int16)])
    with pytest.raises(ValueError, match="shapes"):
        f(x, one, [(8, 14)], [(20, 30)], gt=[_gt(30, 20)])


def test_resize_argmax_multiscale_wide_wrapper_refuses_bad_calls_before_allocating():
    x = torch.zeros(2, 257, 8, 8)
    f = ops.resize_argmax_multiscale_wide
    one = [[((8, 14), [(0, 0, 0, False), (1, 0, 6, True)])]]
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(x, one, [(20, 30)])
    with pytest.raises(RuntimeError, match="no CPU path"):                 # a canvas smaller than a view is allowed here
        f(x, [[((5, 7), [(0, 0, 0, False)]), ((8, 14), one[0][0][1])]], [(20, 30)], mode="logit")
    with pytest.raises(RuntimeError, match="1024"):
        f(torch.zeros(1, 1025, 8, 8), [[((8, 8), [(0, 0, 0, False)])]], [(16, 16)])
    with pytest.raises(ValueError, match="mode"):
        f(x, one, [(20, 30)], mode="mean")
    with pytest.raises(ValueError, match="covered by no window"):
        f(x, [[((8, 15), one[0][0][1])]], [(20, 30)])
    with pytest.raises(ValueError, match="covered by no window"):
        f(x, [[((9, 7), [(0, 0, 0, False)])]], [(20, 30)])
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
        f(x, one * 2, [(20, 30)])
    with pytest.raises(ValueError):
        f(x, one, [(20, 0)])
    with pytest.raises(ValueError, match="ignore_index"):
        f(x, one, [(20, 30)], ignore_index=-1)
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        f(x, one, None, gt=[torch.zeros(20, 30, dtype=torch.int16)])


def test_the_layers_dispatch_on_the_class_count():
    """Past 192 classes the metrics reach the wide wrapper (its last check: no CPU path) instead of the narrow limit."""
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.original_size_predictions(torch.zeros(1, 300, 8, 8), [(16, 16)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.compute_gt_mIOU(torch.zeros(1, 847, 8, 8), [_gt(5, 7)], [(5, 7)])
    with pytest.raises(RuntimeError, match="1024"):
        metrics.original_size_predictions(torch.zeros(1, 1025, 8, 8), [(16, 16)])
    with pytest.raises(RuntimeError, match="no CPU path"):                 # at 192 and below: the narrow wrapper, as before
        metrics.original_size_predictions(torch.zeros(1, 192, 8, 8), [(16, 16)])


def test_dataset_iou_and_the_per_image_rule_at_847_classes():
    """metrics.dataset_iou and metrics._per_image_iou on K = 847 counts against a plain restatement in Python floats."""
    g = torch.Generator().manual_seed(0)
    K = 847
    lab = torch.randint(0, 50, (2, K), generator=g) * (torch.rand(2, K, generator=g) < 0.3)
    pred = torch.randint(0, 50, (2, K), generator=g) * (torch.rand(2, K, generator=g) < 0.3)
    inter = torch.minimum(lab, pred) // 2
    counts = torch.stack([inter, pred, lab], 1).int()                      # [2, 3, K]
    got = metrics._per_image_iou(counts, 0)
    for i in range(2):
        ious = [inter[i, c].item() / (pred[i, c] + lab[i, c] - inter[i, c]).item() for c in range(1, K) if lab[i, c] > 0]
        assert got[i].item() == pytest.approx(sum(ious) / len(ious), abs=1e-12)
    tot = counts.sum(0, dtype=torch.int64)
    d = metrics.dataset_iou(tot, 0)
    seen = [c for c in range(1, K) if (tot[1, c] + tot[2, c] - tot[0, c]) > 0]
    want = sum(tot[0, c].item() / (tot[1, c] + tot[2, c] - tot[0, c]).item() for c in seen) / len(seen)
    assert d["IoU"].shape == (K,) and d["mIoU"].item() == pytest.approx(want, abs=1e-12)
    assert d["aAcc"].item() == pytest.approx(tot[0, 1:].sum().item() / tot[2, 1:].sum().item(), abs=1e-12)


# ---- the fp64 references of the GPU tests stay under the near-tie cap on their own --------------------------------------------
@pytest.mark.parametrize("K", W.KS)
def test_grid_reference_alone_is_under_the_cap(K):
    x = W.grid_logits(K)
    assert x.shape == (1, K, 10, 12)
    for size in W.SIZES:
        ref, sure, unsure = W.grid_reference(K, size)
        print(f"grid K {K} size {size}: unsure share {unsure:.2e}")
        assert ref.shape == size and unsure <= R.UNSURE_CAP, (K, size, unsure)
    if K == 257:                                          # the planted class wins on part of the image, and only there
        share = (W.grid_reference(K, (50, 90))[0] == 256).float().mean().item()
        assert 0.2 < share < 0.7
    if K >= 847:                                          # most pixels fall on classes that need the ninth bit by themselves
        assert (W.grid_reference(K, (50, 90))[0] >= 256).float().mean().item() > 0.5


@pytest.mark.parametrize("K", W.KS)
def test_slide_reference_alone_is_under_the_cap(K):
    views, windows = W.slide_case(K)
    assert views.shape == (6, K, 8, 8) and len(windows) == 6
    for size in W.SLIDE_SIZES:
        _, _, unsure = W.slide_reference(K, size)
        print(f"slide K {K} size {size}: unsure share {unsure:.2e}")
        assert unsure <= R.UNSURE_CAP, (K, size, unsure)


@pytest.mark.parametrize("mode", ["prob", "logit"])
@pytest.mark.parametrize("K", W.KS)
def test_multiscale_reference_alone_is_under_the_cap(K, mode):
    views, canvases, amax = W.ms_case(K)
    assert [c for c, _ in canvases] == [(8, 12), (12, 18), (5, 7), (14, 6)] and views.shape[1] == K and amax < 10
    assert (views[18][:, 5:, :] == W.M.POISON).all() and (views[19:, :, :, 6:] == W.M.POISON).all()
    for size in W.MS_SIZES:
        _, _, unsure = W.ms_reference(K, size, mode)
        print(f"multiscale K {K} mode {mode} size {size}: unsure share {unsure:.2e}")
        assert unsure <= R.UNSURE_CAP, (K, mode, size, unsure)
