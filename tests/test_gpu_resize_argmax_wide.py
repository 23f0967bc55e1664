"""The resize + argmax kernels past 192 classes on the GPU (ops.resize_argmax_wide, _windows_wide, _multiscale_wide and the
layers that dispatch to them): torch's fp64 bicubic references of the narrow tests at K = 193 / 257 / 847 / 1024 outside the
near-tie margin, a host recount of the counts under both counting rules and three gt dtypes, the lowest-index tie rule past class
255, the narrow kernels' pred values and count bytes at K = 151 and 192, batch independence and repeatability, and metrics /
SlidingWindowInference / MultiScaleInference / SlideEvaluator on a stub model that returns 257 classes.
Shapes are the smallest at which the tile end can go wrong: 8- to 12-cell grids, outputs of several tiles with partial edge
tiles, the downscale band path and a single pixel."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multiscale_ref as M  # noqa: E402
import resize_wide_ref as W  # noqa: E402
import slide_ref as R  # noqa: E402

from lc2is_amd import evalloop, metrics, ops, slide  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(p, ref, sure, unsure, size, what):
    got = p.cpu().long()
    assert p.dtype == torch.int16 and got.shape == size, what
    bad = int(((got != ref) & sure).sum())
    print(f"{what} size {size}: unsure share {unsure:.2e}, {bad} pixels differ outside the margin, {int((got != ref).sum())} in all")
    assert bad == 0, f"{what}: {bad} pixels differ from fp64 torch outside the near-tie margin at {size}"
    assert unsure <= R.UNSURE_CAP


# ---- against fp64 torch bicubic -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", W.KS)
def test_grid_matches_torch_bicubic_argmax_in_fp64(dev, K):
    x = W.grid_logits(K)
    sizes = list(W.SIZES)
    preds, _ = ops.resize_argmax_wide(x.expand(len(sizes), -1, -1, -1).to(dev), sizes)
    for p, size in zip(preds, sizes):
        _check(p, *W.grid_reference(K, size), size, f"grid K {K}")
    if K == 257:
        assert bool((preds[0] == 256).any())              # the planted class: the ninth bit of pred is stored


@pytest.mark.parametrize("K", W.KS)
def test_windows_match_torch_bicubic_argmax_of_the_fp64_canvas_mean(dev, K):
    views, windows = W.slide_case(K)
    sizes = list(W.SLIDE_SIZES)
    Hc, Wc = W.SLIDE_ARGS[1], W.SLIDE_ARGS[2]
    n = len(sizes)
    preds, _ = ops.resize_argmax_windows_wide(views.to(dev), [list(windows)] * n, [(Hc, Wc)] * n, sizes)
    for p, size in zip(preds, sizes):
        _check(p, *W.slide_reference(K, size), size, f"windows K {K}")


@pytest.mark.parametrize("mode", ["prob", "logit"])
@pytest.mark.parametrize("K", W.KS)
def test_multiscale_matches_fp64_torch_outside_the_near_tie_margin(dev, K, mode):
    """Four canvases, two of them smaller than a view or overhung, mirrored views, poisoned overhangs."""
    views, canvases, _ = W.ms_case(K)
    sizes = list(W.MS_SIZES)
    preds, _ = ops.resize_argmax_multiscale_wide(views.to(dev), [list(canvases)] * len(sizes), sizes, mode=mode)
    for p, size in zip(preds, sizes):
        _check(p, *W.ms_reference(K, size, mode), size, f"multiscale K {K} mode {mode}")


# ---- counts ------------------------------------------------------------------------------------------------------------------
def _gt_maps(sizes, seed, k):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, s, generator=g) for s in sizes]


def _three_calls(K, dev):
    """name -> call(gt, want_pred, ignore_index) for the three wide kernels (both multiscale modes) over two images."""
    sizes = [(50, 90), (33, 17)]
    x = W.grid_logits(K).expand(2, -1, -1, -1).to(dev)
    sv, sw = W.slide_case(K)
    sv = sv.to(dev)
    mv, mc, _ = W.ms_case(K)
    mv = mv.to(dev)
    Hc, Wc = W.SLIDE_ARGS[1], W.SLIDE_ARGS[2]
    calls = {"grid": lambda gt, wp, ign: ops.resize_argmax_wide(x, sizes, gt=gt, want_pred=wp),
             "windows": lambda gt, wp, ign: ops.resize_argmax_windows_wide(sv, [list(sw)] * 2, [(Hc, Wc)] * 2, sizes, gt=gt,
                                                                           want_pred=wp, ignore_index=ign)}
    for mode in ("prob", "logit"):
        calls["multiscale " + mode] = lambda gt, wp, ign, mode=mode: ops.resize_argmax_multiscale_wide(
            mv, [list(mc)] * 2, sizes, gt=gt, want_pred=wp, ignore_index=ign, mode=mode)
    return sizes, calls


@pytest.mark.parametrize("K", W.KS)
def test_counts_match_a_host_recount_under_both_rules_and_three_gt_dtypes(dev, K):
    sizes, calls = _three_calls(K, dev)
    gt = _gt_maps(sizes, 4, K)                            # drawn over [0, K): bins past 255 are labelled
    gt[0][:3, :] = -1; gt[0][3:6, :] = K; gt[0][6:9, :] = 1 << 20; gt[0][9:14, :] = 0; gt[0][14:17, :] = 300 % K
    gt[1][0, :10] = -1; gt[1][:, :3] = 5
    gt32 = [g.int().to(dev) for g in gt]
    g8 = _gt_maps(sizes, 5, 256)                          # uint8 holds values up to 255 only
    g8[0][:4, :] = 255; g8[0][4:8, :] = 0; g8[1][:, :3] = 5
    gt8 = [g.to(torch.uint8).to(dev) for g in g8]
    for name, call in calls.items():
        preds, c_all = call(gt, True, None)
        assert c_all.dtype == torch.int32 and c_all.shape == (2, 3, K), name
        assert all(p.dtype == torch.int16 for p in preds), name
        for i, (p, g) in enumerate(zip(preds, gt)):
            assert int(p.min()) >= 0 and int(p.max()) < K, name
            assert torch.equal(c_all[i].cpu(), W.recount(p, g, K)), (name, i)
            assert int(c_all[i, 1].sum()) == sizes[i][0] * sizes[i][1]            # ignore_index=None: every pixel is predicted
        assert int(c_all[0, 2].sum()) == (50 - 9) * 90                            # the planted -1 / K / 2^20 rows are unlabelled
        _, c32 = call(gt32, False, None)
        assert torch.equal(c32, c_all), name
        _, c8 = call(gt8, False, None)
        for i, (p, g) in enumerate(zip(preds, g8)):
            assert torch.equal(c8[i].cpu(), W.recount(p, g, K)), (name, i, "uint8")
        if name == "grid":
            continue                                      # lc2is_resize_argmax's rule only
        for ign in (0, 5):
            _, c_ign = call(gt, False, ign)
            _, c_ign32 = call(gt32, False, ign)
            _, c_ign8 = call(gt8, False, ign)
            assert torch.equal(c_ign, c_ign32), (name, ign)
            for i, p in enumerate(preds):
                assert torch.equal(c_ign[i].cpu(), W.recount(p, gt[i], K, ign)), (name, ign, i)
                assert torch.equal(c_ign8[i].cpu(), W.recount(p, g8[i], K, ign)), (name, ign, i, "uint8")
                counted = int(((gt[i] >= 0) & (gt[i] < K) & (gt[i] != ign)).sum())
                assert int(c_ign[i, 1].sum()) == counted and int(c_ign[i, 2].sum()) == counted


# ---- the tie rule past class 255 ---------------------------------------------------------------------------------------------
def test_lowest_index_wins_ties_past_class_255(dev):
    K = 847
    x = torch.randn(2, K, 10, 12, generator=torch.Generator().manual_seed(1))
    x[:, 300] += 5.0
    x[:, 700] = x[:, 300]                                # bitwise copy: every interpolated value ties with channel 300
    xd = x.to(dev)
    y = x.clone()
    y[0, 260, :4] = 50.0; y[0, 511, :4] = 50.0; y[0, 840, :4] = 50.0     # planted three-way ties: 260 wins
    ident, _ = ops.resize_argmax_wide(y.to(dev), [(10, 12), (10, 12)])
    want = y.argmax(1)
    for i in range(2):
        assert ident[i].dtype == torch.int16 and torch.equal(ident[i].cpu().long(), want[i])
    assert bool((ident[0][:4] == 260).all()) and not bool((torch.stack(ident) == 700).any())
    wl = [(0, 0, 0, False)]
    resized = [ops.resize_argmax_wide(xd, [(50, 90), (5, 9)])[0],
               ops.resize_argmax_windows_wide(xd[:1], [wl] * 2, [(10, 12)] * 2, [(50, 90), (5, 9)])[0],
               ops.resize_argmax_multiscale_wide(xd[:1], [[((10, 12), wl)] * 2] * 2, [(50, 90), (5, 9)], mode="logit")[0],
               ops.resize_argmax_multiscale_wide(xd[:1], [[((10, 12), wl)] * 2] * 2, [(50, 90), (5, 9)], mode="prob")[0]]
    for preds in resized:
        flat = torch.cat([p.reshape(-1) for p in preds])
        assert not bool((flat == 700).any())
        assert (preds[0] == 300).float().mean().item() > 0.5


# ---- wide equals narrow ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [151, 192])
def test_wide_returns_the_narrow_kernels_pred_and_count_bytes(dev, K):
    """The grid kernel on four sizes in one call, the "small" slide case, and the "small" multiscale case in both modes, each as
    a multi-image call with gt, under both counting rules."""
    sizes = [(50, 90), (5, 9), (33, 17), (1, 1)]
    gt = [g.to(dev) for g in _gt_maps(sizes, 2, K)]
    gt[0][:5, :] = 0
    x = torch.randn(4, K, 8, 8, generator=torch.Generator().manual_seed(1)).to(dev)
    views, windows = R.make_case(K, *W.SLIDE_ARGS)
    views = views.to(dev)
    Hc, Wc = W.SLIDE_ARGS[1], W.SLIDE_ARGS[2]
    g = torch.Generator().manual_seed(0)
    mv, mc, v0 = [], [], 0
    for hc, wc, stride, flip in W.MS_SPECS:
        v, wl, _ = M.make_canvas(K, W.MS_H, hc, wc, stride, flip, g, v0)
        mv.append(v); mc.append(((hc, wc), wl)); v0 += len(v)
    mv = torch.cat(mv).to(dev)
    pairs = [("grid", lambda f, ign: f(x, sizes, gt=gt), ops.resize_argmax, ops.resize_argmax_wide, (None,))]
    pairs.append(("windows", lambda f, ign: f(views, [list(windows)] * 4, [(Hc, Wc)] * 4, sizes, gt=gt, ignore_index=ign),
                  ops.resize_argmax_windows, ops.resize_argmax_windows_wide, (None, 0)))
    for mode in ("prob", "logit"):
        pairs.append(("multiscale " + mode, lambda f, ign, mode=mode: f(mv, [mc] * 4, sizes, gt=gt, ignore_index=ign, mode=mode),
                      ops.resize_argmax_multiscale, ops.resize_argmax_multiscale_wide, (None, 0)))
    for name, call, narrow, wide, igns in pairs:
        for ign in igns:
            pn, cn = call(narrow, ign)
            pw, cw = call(wide, ign)
            assert cw.dtype == torch.int32 and torch.equal(cw, cn), (name, ign)
            for a, b in zip(pw, pn):
                assert a.dtype == torch.int16 and b.dtype == torch.uint8 and torch.equal(a.long(), b.long()), (name, ign)


# ---- batches -----------------------------------------------------------------------------------------------------------------
def test_a_batch_of_two_sizes_equals_the_single_image_calls_bitwise_and_repeats(dev):
    K = 847
    sizes, calls = _three_calls(K, dev)
    gt = [g.to(dev) for g in _gt_maps(sizes, 9, K)]
    x = W.grid_logits(K).to(dev)
    sv, sw = W.slide_case(K)
    mv, mc, _ = W.ms_case(K)
    Hc, Wc = W.SLIDE_ARGS[1], W.SLIDE_ARGS[2]
    single = {"grid": lambda i: ops.resize_argmax_wide(x, [sizes[i]], gt=[gt[i]]),
              "windows": lambda i: ops.resize_argmax_windows_wide(sv.to(dev), [list(sw)], [(Hc, Wc)], [sizes[i]], gt=[gt[i]]),
              "multiscale prob": lambda i: ops.resize_argmax_multiscale_wide(mv.to(dev), [list(mc)], [sizes[i]], gt=[gt[i]], mode="prob"),
              "multiscale logit": lambda i: ops.resize_argmax_multiscale_wide(mv.to(dev), [list(mc)], [sizes[i]], gt=[gt[i]],
                                                                              mode="logit")}
    for name, call in calls.items():
        preds, counts = call(gt, True, None)
        preds2, counts2 = call(gt, True, None)
        assert torch.equal(counts, counts2) and all(torch.equal(a, b) for a, b in zip(preds, preds2)), name
        for i in range(2):
            p1, c1 = single[name](i)
            assert torch.equal(p1[0], preds[i]) and torch.equal(c1[0], counts[i]), (name, i)


# ---- the layers above --------------------------------------------------------------------------------------------------------
def _ref_gt_miou(x, gt_list, sizes, ignore_index=0):
    """compute_gt_mIOU restated in fp64 (tests/test_gpu_resize_argmax.py's ref_gt_miou)."""
    out = []
    for i, (g, size) in enumerate(zip(gt_list, sizes)):
        pred, _ = R.ref_argmax(x[i], tuple(size))
        c = W.recount(pred, g, x.shape[1]).double()
        iou = c[0] / (c[1] + c[2] - c[0]).clamp_min(1)
        classes = g.unique()
        classes = classes[classes != ignore_index].long()
        out.append(iou[classes].mean().item() if classes.numel() else float("nan"))
    return torch.tensor(out, dtype=torch.float64)


def test_gt_miou_and_original_size_predictions_at_257_classes(dev):
    K = 257
    sizes = [(50, 90), (37, 53), (16, 20)]
    x = torch.randn(3, K, 10, 12, generator=torch.Generator().manual_seed(6))
    x[:, 3] += 2.5; x[:, 256] += 2.5; x[:, 200] += 2.0   # a few dominant classes, one of them past 255
    gt = [torch.tensor([0, 3, 200, 256])[g] for g in _gt_maps(sizes, 7, 4)]
    gt[2].zero_()                                        # nothing but ignore_index: NaN on both sides
    got = metrics.per_image_gt_mIOU(x.to(dev), gt, sizes).cpu()
    want = _ref_gt_miou(x, gt, sizes)
    assert got.dtype == torch.float64 and got.shape == (3,)
    assert math.isnan(got[2]) and math.isnan(want[2])
    assert (got[:2] - want[:2]).abs().max().item() <= 1e-3
    d = metrics.compute_gt_mIOU(x[:2].to(dev), gt[:2], torch.tensor(sizes[:2]))
    assert list(d) == ["mIOU_gt"] and abs(d["mIOU_gt"] - want[:2].mean().item()) <= 1e-3
    preds = metrics.original_size_predictions(x.to(dev), sizes)
    direct, _ = ops.resize_argmax_wide(x.to(dev), sizes)
    assert all(p.dtype == torch.int16 and p.is_cuda and torch.equal(p, q) for p, q in zip(preds, direct))
    assert bool((preds[0] == 256).any())
    narrow = metrics.original_size_predictions(x[:, :192].to(dev), sizes)       # 192 classes and below: uint8, as before
    assert all(p.dtype == torch.uint8 for p in narrow)


class _Stub(torch.nn.Module):
    """A model of 257 classes on an 8 x 8 score grid for 32 x 32 windows: a fixed random projection of the 4 x 4 cell means.
    The last class follows the red channel alone with a large weight, so it wins wherever a cell is redder than the mean."""
    out_size = 8

    def __init__(self, K=257):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        w = torch.randn(K, 3, generator=g)
        w[K - 1] = torch.tensor([30.0, 0.0, 0.0])
        self.register_buffer("w", w)
        self.register_buffer("b", torch.randn(K, generator=g) * 0.1)

    def forward(self, inputs):
        cells = torch.nn.functional.avg_pool2d(inputs["pixel_values"], 4)
        return {"outputs": torch.einsum("kc,nchw->nkhw", self.w, cells) + self.b[None, :, None, None]}


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (20, 35, 3), dtype=np.uint8), rng.integers(0, 256, (25, 25, 3), dtype=np.uint8)]


def _gts(K):
    g = torch.Generator().manual_seed(6)
    gts = [torch.randint(0, K, (20, 35), generator=g), torch.randint(0, K, (25, 25), generator=g)]
    gts[0][:3] = 0; gts[1][:, :4] = -1; gts[1][:5, 10:] = 0
    return gts


@pytest.mark.parametrize("kind", ["slide", "multiscale prob", "multiscale logit"])
def test_inference_classes_and_slide_evaluator_at_257_classes(dev, kind):
    K = 257
    m = _Stub(K).to(dev)
    images, gts = _images(), _gts(K)
    kw = dict(size=32, crop=32, stride=20, flip=True, window_batch=3, device=dev)
    if kind == "slide":
        inf = slide.SlidingWindowInference(m, {}, **kw)
        views, windows, canvases, sizes = inf.views(images)
        op = lambda **k: ops.resize_argmax_windows_wide(views, windows, canvases, sizes, **k)
    else:
        inf = slide.MultiScaleInference(m, {}, scales=(0.5, 1.0, 1.5), average=kind.split()[1], **kw)
        views, canvases, sizes = inf.views(images)
        op = lambda **k: ops.resize_argmax_multiscale_wide(views, canvases, sizes, mode=inf.average, **k)
    assert (inf.grid, inf.cell) == (8, 4) and views.shape[1:] == (K, 8, 8)
    preds = inf.predict(images)
    assert [tuple(p.shape) for p in preds] == [(20, 35), (25, 25)] and all(p.dtype == torch.int16 and p.is_cuda for p in preds)
    by_hand, _ = op()
    assert all(torch.equal(a, b) for a, b in zip(preds, by_hand))
    assert max(int(p.max()) for p in preds) > 255         # the stub's scores do reach the classes past 255
    _, c_mm = op(gt=gts, want_pred=False, ignore_index=0)
    _, c_ref = op(gt=gts, want_pred=False)
    for i, (p, g) in enumerate(zip(preds, gts)):
        assert torch.equal(c_mm[i].cpu(), W.recount(p, g, K, 0)) and torch.equal(c_ref[i].cpu(), W.recount(p, g, K))
    assert torch.equal(inf.counts(images, gts), c_mm)
    both = inf.counts_both(images, gts, 0)
    assert torch.equal(both[0], c_mm) and torch.equal(both[1], c_ref)
    got = evalloop.SlideEvaluator(inf, [(images, gts), ([images[1]], [gts[1]])]).evaluate()
    assert set(got) == {"eval_mIoU", "eval_mAcc", "eval_aAcc", "eval_mIOU_gt"}
    assert all(math.isfinite(v) for v in got.values())
    mm = torch.cat([c_mm, c_mm[1:]]).cpu()
    ref = torch.cat([c_ref, c_ref[1:]]).cpu()
    want = metrics.dataset_iou(mm.sum(0, dtype=torch.int64), 0)
    for k in ("mIoU", "mAcc", "aAcc"):
        assert got["eval_" + k] == pytest.approx(want[k].item(), abs=1e-12), k
    assert got["eval_mIOU_gt"] == pytest.approx(metrics._per_image_iou(ref, 0).mean().item(), abs=1e-12)
