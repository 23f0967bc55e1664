"""Sliding-window evaluation on the GPU: lc2is_resize_argmax_windows / ops.resize_argmax_windows against ops.resize_argmax
(bitwise, where the canvas is one view), the fp32 canvas mean in the kernel's summation order (bitwise at the canvas size), torch's
fp64 bicubic + argmax of the fp64 canvas mean (outside the near-tie margin), a host recount of the counts under both counting
rules, hand-built bad descriptors, and SlidingWindowInference / SlideEvaluator end to end on a tiny BaseModelWithText."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import slide_ref as R  # noqa: E402

from lc2is_amd import evalloop, metrics, ops, slide  # noqa: E402
from lc2is_amd.data.preprocess import ClipImagePreprocessor  # noqa: E402

pytestmark = pytest.mark.gpu

K = 37
G = Path(__file__).resolve().parent / "golden"


def _gt_maps(sizes, seed, k=K):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, s, generator=g) for s in sizes]


def recount(pred, gt, k, ignore_index=None):
    """{intersection, predicted, labelled} [3, k] on the host.  ignore_index None: every pixel is predicted, labelled where
    0 <= gt < k; an int: only pixels with 0 <= gt < k and gt != ignore_index count, in all three rows."""
    p, g = pred.reshape(-1).long().cpu(), gt.reshape(-1).long().cpu()
    lab = (g >= 0) & (g < k)
    if ignore_index is not None:
        lab &= g != ignore_index
    predicted = p if ignore_index is None else p[lab]
    return torch.stack([torch.bincount(p[lab & (p == g)], minlength=k), torch.bincount(predicted, minlength=k),
                        torch.bincount(g[lab], minlength=k)]).int()


def test_one_view_canvas_is_resize_argmax_bitwise(dev):
    """K = 37: two channel chunks, the second partial, ld = 40; (5, 9) takes the downscale band path."""
    sizes = [(50, 90), (5, 9), (33, 17), (1, 1)]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, K, 8, 8, generator=g).to(dev)
    gt = [t.to(dev) for t in _gt_maps(sizes, 2)]
    want_p, want_c = ops.resize_argmax(x.expand(4, -1, -1, -1), sizes, gt=gt)
    arms = {"one window": (x, [(0, 0, 0, False)]),
            "listed twice: (x + x) / 2 is exact": (x, [(0, 0, 0, False), (0, 0, 0, False)]),
            "stored mirrored and flagged": (x.flip(-1).contiguous(), [(0, 0, 0, True)])}
    for name, (views, wl) in arms.items():
        p, c = ops.resize_argmax_windows(views, [wl] * 4, [(8, 8)] * 4, sizes, gt=gt)
        assert c.dtype == torch.int32 and torch.equal(c, want_c), name
        for a, b, s in zip(p, want_p, sizes):
            assert a.dtype == torch.uint8 and a.shape == s and torch.equal(a, b), (name, s)


def test_canvas_size_output_is_the_argmax_of_the_fp32_canvas_mean_in_list_order(dev):
    """Output size = canvas size: the bicubic weights are exactly (0, 1, 0, 0), so the kernel's mean itself is compared, cover
    counts 2, 4 and 6, mirrored views included."""
    views, windows = R.make_case(K, 8, 8, 14, 4, True)
    assert len(windows) == 6
    want = R.canvas_mean(views, windows, 8, 14, torch.float32).argmax(0)
    p, _ = ops.resize_argmax_windows(views.to(dev), [list(windows)], [(8, 14)], [(8, 14)])
    assert torch.equal(p[0].cpu().long(), want)


@pytest.mark.parametrize("args,sizes", R.FP64_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_matches_torch_bicubic_argmax_of_the_fp64_canvas_mean(dev, args, sizes):
    views, windows = R.make_case(*args)
    Hc, Wc = args[2], args[3]
    n = len(sizes)
    preds, _ = ops.resize_argmax_windows(views.to(dev), [list(windows)] * n, [(Hc, Wc)] * n, sizes)
    for p, size in zip(preds, sizes):
        ref, sure, unsure = R.fp64_reference(args, size)
        got = p.cpu().long()
        assert got.shape == size
        bad = int(((got != ref) & sure).sum())
        print(f"case {args} size {size}: unsure share {unsure:.2e}, {bad} pixels differ outside the margin")
        assert bad == 0, f"{bad} pixels differ from fp64 torch outside the near-tie margin at {size}"
        assert unsure <= R.UNSURE_CAP


def test_the_mean_is_an_ieee_division_not_a_reciprocal_multiply(dev):
    """Cover count 3, K = 2, output size = canvas size: channel 1 is the next float above channel 0 and the other two views are 0,
    so the sums are exact and the argmax is 1 exactly where fl(b / 3) > fl(a / 3), else 0 (the tie goes to the lower index).  A
    product with fl(1 / 3) rounds differently on many of the 1024 cells (asserted here on the host), so this pins the division."""
    g = torch.Generator().manual_seed(9)
    a = (torch.rand(32, 32, generator=g) + 1.0) * 3.0
    b = torch.nextafter(a, torch.full_like(a, 100.0))
    views = torch.zeros(3, 2, 32, 32)
    views[0, 0], views[0, 1] = a, b
    three = torch.tensor(3.0)
    want = ((b / three) > (a / three)).long()
    recip = 1.0 / three
    assert int((((b * recip) > (a * recip)).long() != want).sum()) > 20
    p, _ = ops.resize_argmax_windows(views.to(dev), [[(0, 0, 0, False), (1, 0, 0, False), (2, 0, 0, False)]], [(32, 32)], [(32, 32)])
    assert torch.equal(p[0].cpu().long(), want)


def _three_images():
    """Three images with different canvases and window counts over one view tensor."""
    v1, w1 = R.make_case(K, 8, 8, 14, 4, True)
    v2, w2 = R.make_case(K, 8, 12, 14, 4, False)
    v3 = torch.randn(1, K, 8, 8, generator=torch.Generator().manual_seed(3))
    views = torch.cat([v1, v2, v3])
    windows = [list(w1), [(v + len(v1), oy, ox, m) for v, oy, ox, m in w2], [(len(v1) + len(v2), 0, 0, False)]]
    return views, windows, [(8, 14), (12, 14), (8, 8)], [(50, 90), (33, 17), (100, 131)]


def test_counts_match_a_host_recount_under_both_rules_and_batches_are_independent(dev):
    views, windows, canvases, sizes = _three_images()
    views = views.to(dev)
    gt = _gt_maps(sizes, 4)
    gt[0][:3, :] = -1; gt[0][3:6, :] = K; gt[0][6:9, :] = 255; gt[0][9:14, :] = 0; gt[1][0, :10] = -1; gt[2][:, :7] = 5
    gt8 = [torch.where(g < 0, torch.full_like(g, 255), g).to(torch.uint8).to(dev) for g in gt]
    preds, c_all = ops.resize_argmax_windows(views, windows, canvases, sizes, gt=gt)
    for ign in (0, 5):
        _, c_ign = ops.resize_argmax_windows(views, windows, canvases, sizes, gt=gt, want_pred=False, ignore_index=ign)
        _, c_ign8 = ops.resize_argmax_windows(views, windows, canvases, sizes, gt=gt8, want_pred=False, ignore_index=ign)
        assert torch.equal(c_ign, c_ign8)
        for i, (p, g) in enumerate(zip(preds, gt)):
            assert torch.equal(c_ign[i].cpu(), recount(p, g, K, ign))
            counted = int(((g >= 0) & (g < K) & (g != ign)).sum())
            assert int(c_ign[i, 1].sum()) == counted and int(c_ign[i, 2].sum()) == counted and int(c_ign[i, :, ign].sum()) == \
                int(c_ign[i, 1, ign])                                   # the ignored class is neither labelled nor intersected
    for i, (p, g) in enumerate(zip(preds, gt)):
        assert torch.equal(c_all[i].cpu(), recount(p, g, K))
        assert int(c_all[i, 1].sum()) == sizes[i][0] * sizes[i][1]      # ignore_index=None: every pixel is predicted
    preds2, c2 = ops.resize_argmax_windows(views, windows, canvases, sizes, gt=gt)
    assert torch.equal(c_all, c2) and all(torch.equal(a, b) for a, b in zip(preds, preds2))
    for i in range(3):
        p1, c1 = ops.resize_argmax_windows(views, [windows[i]], [canvases[i]], [sizes[i]], gt=[gt[i]])
        assert torch.equal(p1[0], preds[i]) and torch.equal(c1[0], c_all[i])


def _raw(dev, views, desc_rows, win_rows, total_px, n_tiles):
    """lc2is_resize_argmax_windows on hand-built descriptors: pred prefilled with 255 (no class), no counts."""
    V, k, h, w = views.shape
    ld = (k + 3) // 4 * 4
    lo = torch.zeros(V, h, w, ld, dtype=torch.float32, device=dev)
    lo[..., :k] = views.to(dev).permute(0, 2, 3, 1)
    desc = torch.tensor(desc_rows, dtype=torch.int64).to(dev)
    win = torch.tensor(win_rows, dtype=torch.int32).to(dev)
    pred = torch.full((total_px,), 255, dtype=torch.uint8, device=dev)
    rc = ops._fn("lc2is_resize_argmax_windows")(lo.data_ptr(), ld, V, h, w, k, desc.data_ptr(), len(desc_rows), win.data_ptr(),
                                                len(win_rows), n_tiles, total_px, None, 0, -1, pred.data_ptr(), None, None, 0,
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return pred.cpu()


def test_bad_descriptors_are_skipped_not_followed(dev):
    """The kernel range-checks what the wrapper would have refused: windows with a bad view index or origin are skipped (the
    result is that of the list without them, order kept), and an image with too many windows, a window range outside the list or
    a canvas smaller than a view is left unwritten.  Nothing here faults: every bad value is only compared."""
    views, windows = R.make_case(K, 8, 8, 14, 4, True)
    V, H, W = len(views), 20, 30
    tiles = 2 * 2
    want, _ = ops.resize_argmax_windows(views.to(dev), [list(windows)], [(8, 14)], [(H, W)])
    want = want[0].cpu().reshape(-1)
    good = [[v, oy, ox, int(m)] for v, oy, ox, m in windows]
    bad = [[V, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 7, 1], [1, -1, 0, 0], [1, 0, -1, 0], [2 ** 31 - 1, 0, 0, 0]]
    mixed = [bad[0], good[0], bad[1], bad[2], good[1], good[2], bad[3], good[3], bad[4], good[4], bad[5], good[5], bad[6]]
    got = _raw(dev, views, [[H, W, 0, 0, 8, 14, 0, len(mixed)]], mixed, H * W, tiles)
    assert torch.equal(got, want)
    # four images: 65 windows; a window range past the list; a canvas lower than a view; and a good one, which is still computed
    many = good + [good[0]] * 59
    assert len(many) == 65
    rows = many + good
    desc = [[H, W, 0, 0, 8, 14, 0, 65], [H, W, H * W, tiles, 8, 14, 65, len(good) + 1], [H, W, 2 * H * W, 2 * tiles, 7, 14, 65, 6],
            [H, W, 3 * H * W, 3 * tiles, 8, 14, 65, 6]]
    got = _raw(dev, views, desc, rows, 4 * H * W, 4 * tiles).view(4, -1)
    assert (got[:3] == 255).all()
    assert torch.equal(got[3], want)


# ---- end to end on the tiny model of the module tests ----------------------------------------------------------------------
def _tiny(dev):
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(G / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).eval(), fx


def _text(fx, n):
    return {k: fx[k][:1].expand(n, -1).contiguous() for k in ("input_ids", "attention_mask")}


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (40, 70, 3), dtype=np.uint8), rng.integers(0, 256, (50, 50, 3), dtype=np.uint8)]


# pixel columns of the windows, written by hand: 40 x 70 -> 64 x 112 pixels (cells of 4: 16 x 28), stride 40 -> 0, 40, 48;
# 50 x 50 -> 64 x 64, one window
HAND = {(40, 70): ((64, 112), (16, 28), [0, 40, 48]), (50, 50): ((64, 64), (16, 16), [0])}


def _by_hand(m, fx, dev, images, flip, batch):
    """What SlidingWindowInference must produce, built without it: the CPU oracle's Pillow resize of the uint8 image, windows
    sliced at the hand-written pixel columns, normalised through the oracle's table, mirrored with a numpy slice, and the model run
    directly in batches of ``batch`` (the last one padded with its last window).  Returns (outputs, windows, canvases, sizes)."""
    from oracle import preprocess_cpu as P
    from lc2is_amd.data.preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    lut = P.normalize_lut(OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)
    px, windows, canvases, sizes = [], [], [], []
    for im in images:
        (nh, nw), canvas, cols = HAND[im.shape[:2]]
        r = P.resize_bicubic_u8(im, nh, nw)
        cut = [np.stack([lut[ch][r[0:64, c:c + 64, ch]] for ch in range(3)]) for c in cols]
        wl = [(len(px) + j, 0, c // 4, False) for j, c in enumerate(cols)]
        px += cut
        if flip:
            wl += [(len(px) + j, 0, c // 4, True) for j, c in enumerate(cols)]
            px += [w[:, :, ::-1].copy() for w in cut]
        windows.append(wl); canvases.append(canvas); sizes.append(tuple(im.shape[:2]))
    V = len(px)
    px += [px[-1]] * (-V % batch)
    x = torch.from_numpy(np.stack(px)).to(dev)
    with torch.no_grad():
        out = torch.cat([m({"pixel_values": x[b:b + batch], **_text_dev(fx, batch, dev)})["outputs"] for b in range(0, len(px), batch)])
    return out[:V], windows, canvases, sizes


def _text_dev(fx, n, dev):
    return {k: v.to(dev) for k, v in _text(fx, n).items()}


def test_sliding_window_inference_end_to_end(dev):
    m, fx = _tiny(dev)
    kc = fx["logits"].shape[1]
    images = _images()
    inf = slide.SlidingWindowInference(m, _text(fx, 3), size=64, crop=64, stride=40, flip=True, window_batch=3, device=dev)
    assert (inf.grid, inf.cell) == (16, 4)
    out, windows, canvases, sizes = _by_hand(m, fx, dev, images, flip=True, batch=3)
    assert windows == [[(0, 0, 0, False), (1, 0, 10, False), (2, 0, 12, False), (3, 0, 0, True), (4, 0, 10, True), (5, 0, 12, True)],
                       [(6, 0, 0, False), (7, 0, 0, True)]]
    views, w2, c2, s2 = inf.views(images)
    assert (w2, c2, s2) == (windows, canvases, sizes)
    assert views.shape == (8, kc, 16, 16)                            # 8 views in batches of 3: the padding is dropped
    assert torch.equal(views, out)                                   # the windows' pixels, their order and the mirrored copies
    assert not torch.equal(out[0], out[3]) and not torch.equal(out[1], out[2])
    preds = inf.predict(images)
    assert [tuple(p.shape) for p in preds] == sizes and all(p.dtype == torch.uint8 and p.is_cuda for p in preds)
    by_hand, _ = ops.resize_argmax_windows(out, windows, canvases, sizes)
    assert all(torch.equal(a, b) for a, b in zip(preds, by_hand))

    # the square image without flip is one window at (0, 0): the single forward of the centre-crop path, bitwise
    one = slide.SlidingWindowInference(m, _text(fx, 1), size=64, crop=64, stride=40, flip=False, window_batch=1, device=dev)
    with torch.no_grad():
        out = m({"pixel_values": ClipImagePreprocessor(size=64, crop_size=64, device=dev)([images[1]]), **_text_dev(fx, 1, dev)})["outputs"]
    want = metrics.original_size_predictions(out, [(50, 50)])[0]
    assert torch.equal(one.predict([images[1]])[0], want)


def _gts(kc):
    g = torch.Generator().manual_seed(6)
    gts = [torch.randint(0, kc, (40, 70), generator=g).to(torch.uint8), torch.randint(0, kc, (50, 50), generator=g).to(torch.uint8)]
    gts[0][:5] = 0; gts[1][:, :4] = 255; gts[1][:9, 10:] = 0
    return gts


def test_slide_evaluator_reports_dataset_and_per_image_scores(dev):
    """Against predictions made from hand-built window forwards: the dataset scores from a recount under mmseg's rule, and
    eval_mIOU_gt from a recount under the reference's rule (every pixel predicted; class 0 only leaves the mean)."""
    m, fx = _tiny(dev)
    kc = fx["logits"].shape[1]
    images, gts = _images(), _gts(kc)
    inf = slide.SlidingWindowInference(m, _text(fx, 2), size=64, crop=64, stride=40, flip=False, window_batch=2, device=dev)
    loader = [(images, gts), ([images[1]], [gts[1]])]
    got = evalloop.SlideEvaluator(inf, loader).evaluate()
    assert set(got) == {"eval_mIoU", "eval_mAcc", "eval_aAcc", "eval_mIOU_gt"}
    mm, ref = [], []
    for ims, gs in loader:
        out, windows, canvases, sizes = _by_hand(m, fx, dev, ims, flip=False, batch=2)
        preds, _ = ops.resize_argmax_windows(out, windows, canvases, sizes)
        mm += [recount(p, gt, kc, 0) for p, gt in zip(preds, gs)]
        ref += [recount(p, gt, kc) for p, gt in zip(preds, gs)]
    mm, ref = torch.stack(mm), torch.stack(ref)
    assert not torch.equal(mm, ref)                                  # the two rules differ on this gt (class 0 and 255 present)
    want = metrics.dataset_iou(mm.sum(0, dtype=torch.int64), 0)
    for k in ("mIoU", "mAcc", "aAcc"):
        assert got["eval_" + k] == pytest.approx(want[k].item(), abs=1e-12), k
    assert got["eval_mIOU_gt"] == pytest.approx(metrics._per_image_iou(ref, 0).mean().item(), abs=1e-12)
    assert got["eval_mIOU_gt"] != pytest.approx(metrics._per_image_iou(mm, 0).mean().item(), abs=1e-9)
    assert torch.equal(inf.counts(images, gts).cpu(), mm[:2])
    c_mm, c_ref = inf.counts_both(images, gts, 0)
    assert torch.equal(c_mm.cpu(), mm[:2]) and torch.equal(c_ref.cpu(), ref[:2])


def test_eval_miou_gt_of_a_one_window_image_is_the_centre_crop_evaluators(dev):
    """A square image is one window at (0, 0): eval_mIOU_gt must be metrics.per_image_gt_mIOU of the same single forward."""
    m, fx = _tiny(dev)
    kc = fx["logits"].shape[1]
    image, gt = _images()[1], _gts(kc)[1]
    one = slide.SlidingWindowInference(m, _text(fx, 1), size=64, crop=64, stride=40, flip=False, window_batch=1, device=dev)
    got = evalloop.SlideEvaluator(one, [([image], [gt])]).evaluate()
    with torch.no_grad():
        out = m({"pixel_values": ClipImagePreprocessor(size=64, crop_size=64, device=dev)([image]), **_text_dev(fx, 1, dev)})["outputs"]
    assert got["eval_mIOU_gt"] == metrics.per_image_gt_mIOU(out, [gt], [(50, 50)]).mean().item()
