"""Multi-scale + flip evaluation on the GPU: lc2is_resize_argmax_multiscale / ops.resize_argmax_multiscale against
ops.resize_argmax_windows (bitwise, one canvas summed as logits), torch's fp64 bicubic + softmax-sum / sum + argmax (outside the
near-tie margin, with windows that overhang their canvas and poisoned overhangs), the two modes where they must differ, a fixed
summation order and batch independence, a host recount of the counts under both rules, hand-built bad descriptors, and
MultiScaleInference / SlideEvaluator end to end on a tiny BaseModelWithText."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multiscale_ref as M  # noqa: E402
import slide_ref as R  # noqa: E402

from lc2is_amd import evalloop, metrics, ops, slide  # noqa: E402

pytestmark = pytest.mark.gpu

K = 37
G = Path(__file__).resolve().parent / "golden"


def _gt_maps(sizes, seed, k=K):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, s, generator=g) for s in sizes]


def recount(pred, gt, k, ignore_index=None):
    """{intersection, predicted, labelled} [3, k] on the host (tests/test_gpu_slide.py's).  ignore_index None: every pixel is
    predicted, labelled where 0 <= gt < k; an int: only pixels with 0 <= gt < k and gt != ignore_index count, in all three rows."""
    p, g = pred.reshape(-1).long().cpu(), gt.reshape(-1).long().cpu()
    lab = (g >= 0) & (g < k)
    if ignore_index is not None:
        lab &= g != ignore_index
    predicted = p if ignore_index is None else p[lab]
    return torch.stack([torch.bincount(p[lab & (p == g)], minlength=k), torch.bincount(predicted, minlength=k),
                        torch.bincount(g[lab], minlength=k)]).int()


def test_one_canvas_summed_as_logits_is_resize_argmax_windows_bitwise(dev):
    """The inputs of test_gpu_slide.py's one-view test (K = 37: two channel chunks, the second partial; (5, 9) takes the downscale
    band path) and its six-window canvas with cover counts 2, 4 and 6: predictions and counts under both counting rules."""
    sizes = [(50, 90), (5, 9), (33, 17), (1, 1)]
    x = torch.randn(1, K, 8, 8, generator=torch.Generator().manual_seed(1))
    gt = [t.to(dev) for t in _gt_maps(sizes, 2)]
    v6, w6 = R.make_case(K, 8, 8, 14, 4, True)
    arms = {"one window": (x, [(0, 0, 0, False)], (8, 8)),
            "listed twice": (x, [(0, 0, 0, False), (0, 0, 0, False)], (8, 8)),
            "stored mirrored and flagged": (x.flip(-1).contiguous(), [(0, 0, 0, True)], (8, 8)),
            "six windows, mirrored ones included": (v6, list(w6), (8, 14))}
    for name, (views, wl, canvas) in arms.items():
        views = views.to(dev)
        for ign in (None, 0):
            want_p, want_c = ops.resize_argmax_windows(views, [wl] * 4, [canvas] * 4, sizes, gt=gt, ignore_index=ign)
            p, c = ops.resize_argmax_multiscale(views, [[(canvas, wl)]] * 4, sizes, gt=gt, ignore_index=ign, mode="logit")
            assert c.dtype == torch.int32 and torch.equal(c, want_c), (name, ign)
            for a, b, s in zip(p, want_p, sizes):
                assert a.dtype == torch.uint8 and a.shape == s and torch.equal(a, b), (name, ign, s)


def test_the_three_kernels_agree_bitwise_where_the_bands_split_on_both_axes(dev):
    """One 24 x 24 view, K = 37.  At (9, 11) the one partial tile spans all 24 source rows and columns, so the row band halves
    9 -> 5 -> 3 and the column band 11 -> 6 -> 3 before a footprint fits 10: the band loops of the shared walk run several times
    on both axes, which no 8 x 8 grid reaches.  (50, 7) is upscaled along y and downscaled along x, (24, 24) is the identity,
    (40, 70) has more than one tile per axis.  resize_argmax == resize_argmax_windows == resize_argmax_multiscale(logit),
    predictions and counts."""
    sizes = [(9, 11), (50, 7), (24, 24), (40, 70)]
    x = torch.randn(1, K, 24, 24, generator=torch.Generator().manual_seed(11)).to(dev)
    gt = [t.to(dev) for t in _gt_maps(sizes, 12)]
    wl = [(0, 0, 0, False)]
    p0, c0 = ops.resize_argmax(x.expand(4, -1, -1, -1), sizes, gt)
    p1, c1 = ops.resize_argmax_windows(x, [wl] * 4, [(24, 24)] * 4, sizes, gt)
    p2, c2 = ops.resize_argmax_multiscale(x, [[((24, 24), wl)]] * 4, sizes, gt, mode="logit")
    assert c0.dtype == torch.int32 and torch.equal(c0, c1) and torch.equal(c1, c2)
    for a, b, c, s in zip(p0, p1, p2, sizes):
        assert a.dtype == torch.uint8 and a.shape == s and torch.equal(a, b) and torch.equal(b, c), s


@pytest.mark.parametrize("mode", ["prob", "logit"])
@pytest.mark.parametrize("name", list(M.CASES))
def test_matches_fp64_torch_outside_the_near_tie_margin(dev, name, mode):
    """Four canvases per image, two of them smaller than a view or overhung, views poisoned outside their on-canvas part."""
    views, canvases, _ = M.make_case(name)
    sizes = list(M.CASES[name][3])
    preds, _ = ops.resize_argmax_multiscale(views.to(dev), [list(canvases)] * len(sizes), sizes, mode=mode)
    for p, size in zip(preds, sizes):
        ref, sure, unsure = M.fp64_reference(name, size, mode)
        got = p.cpu().long()
        assert got.shape == size
        bad = int(((got != ref) & sure).sum())
        print(f"case {name} mode {mode} size {size}: unsure share {unsure:.2e}, {bad} pixels differ outside the margin, "
              f"{int((got != ref).sum())} in all")
        assert bad == 0, f"{bad} pixels differ from fp64 torch outside the near-tie margin at {size}"
        assert unsure <= R.UNSURE_CAP


def test_the_modes_differ_where_they_must(dev):
    """K = 2, four constant canvases: canvas 0 holds (10, 0), canvases 1 to 3 hold (0, 2).  As logits the sum is (10, 6): class 0.
    As probabilities it is about (1.36, 2.64): class 1.  A constant canvas resizes to itself (the bicubic weights sum to 1 up to
    rounding, far from either tie), so this holds at every pixel of every size."""
    views = torch.zeros(4, 2, 8, 8)
    views[0, 0] = 10.0
    views[1:, 1] = 2.0
    canvases = [((8, 8), [(a, 0, 0, False)]) for a in range(4)]
    sizes = [(40, 56), (5, 9), (17, 33), (1, 1)]
    for mode, cls in (("logit", 0), ("prob", 1)):
        preds, _ = ops.resize_argmax_multiscale(views.to(dev), [canvases] * len(sizes), sizes, mode=mode)
        for p, s in zip(preds, sizes):
            assert p.shape == s and bool((p == cls).all()), (mode, s)


def test_one_canvas_as_probabilities_is_one_canvas_as_logits_on_every_sure_pixel(dev):
    """The argmax of a softmax is the argmax of its logits; only a near tie may round apart."""
    args = (K, 8, 8, 14, 4, True)
    views, windows = R.make_case(*args)
    sizes = [(50, 90), (5, 9), (33, 17), (1, 1)]
    cl = [[((8, 14), list(windows))]] * len(sizes)
    pl, _ = ops.resize_argmax_multiscale(views.to(dev), cl, sizes, mode="logit")
    pp, _ = ops.resize_argmax_multiscale(views.to(dev), cl, sizes, mode="prob")
    for a, b, size in zip(pl, pp, sizes):
        _, sure, _ = M.ref_argmax(views, [((8, 14), windows)], size, "prob", views.abs().max().item())
        assert int(((a != b).cpu() & sure).sum()) == 0, size


def _three_images():
    """Three images with different sizes and canvas counts (4, 2, 1) over one view tensor."""
    v1, c1, _ = M.make_case("small")
    v2, w2 = R.make_case(K, 8, 12, 14, 4, False)
    v3, w3 = R.make_case(K, 8, 8, 14, 4, True)
    n1, n2 = len(v1), len(v1) + len(v2)
    views = torch.cat([v1, v2, v3])
    second = [((12, 14), [(v + n1, oy, ox, m) for v, oy, ox, m in w2]), ((8, 14), [(v + n2, oy, ox, m) for v, oy, ox, m in w3])]
    third = [((8, 14), [(v + n2, oy, ox, m) for v, oy, ox, m in w3])]
    return views, [[(c, list(w)) for c, w in c1], second, third], [(50, 90), (33, 17), (100, 131)]


@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_counts_match_a_host_recount_and_the_result_is_reproducible_and_batch_independent(dev, mode):
    views, canvases, sizes = _three_images()
    views = views.to(dev)
    gt = _gt_maps(sizes, 4)
    gt[0][:3, :] = -1; gt[0][3:6, :] = K; gt[0][6:9, :] = 255; gt[0][9:14, :] = 0; gt[1][0, :10] = -1; gt[2][:, :7] = 5
    preds, c_all = ops.resize_argmax_multiscale(views, canvases, sizes, gt=gt, mode=mode)
    for ign in (0, 5):
        _, c_ign = ops.resize_argmax_multiscale(views, canvases, sizes, gt=gt, want_pred=False, ignore_index=ign, mode=mode)
        for i, (p, g) in enumerate(zip(preds, gt)):
            assert torch.equal(c_ign[i].cpu(), recount(p, g, K, ign)), (ign, i)
    for i, (p, g) in enumerate(zip(preds, gt)):
        assert torch.equal(c_all[i].cpu(), recount(p, g, K)), i
        assert int(c_all[i, 1].sum()) == sizes[i][0] * sizes[i][1]      # ignore_index=None: every pixel is predicted
    # the same call again: the same bytes
    preds2, c2 = ops.resize_argmax_multiscale(views, canvases, sizes, gt=gt, mode=mode)
    assert torch.equal(c_all, c2) and all(torch.equal(a, b) for a, b in zip(preds, preds2))
    # each image alone: what it gave inside the batch
    for i in range(3):
        p1, c1 = ops.resize_argmax_multiscale(views, [canvases[i]], [sizes[i]], gt=[gt[i]], mode=mode)
        assert torch.equal(p1[0], preds[i]) and torch.equal(c1[0], c_all[i]), i


def _raw(dev, views, desc_rows, canv_rows, win_rows, total_px, n_tiles, mode):
    """lc2is_resize_argmax_multiscale on hand-built descriptors: pred prefilled with 255 (no class), no counts."""
    V, k, h, w = views.shape
    ld = (k + 3) // 4 * 4
    lo = torch.zeros(V, h, w, ld, dtype=torch.float32, device=dev)
    lo[..., :k] = views.to(dev).permute(0, 2, 3, 1)
    desc = torch.tensor(desc_rows, dtype=torch.int64).to(dev)
    canv = torch.tensor(canv_rows, dtype=torch.int64).to(dev)
    win = torch.tensor(win_rows, dtype=torch.int32).to(dev)
    pred = torch.full((total_px,), 255, dtype=torch.uint8, device=dev)
    rc = ops._fn("lc2is_resize_argmax_multiscale")(lo.data_ptr(), ld, V, h, w, k, desc.data_ptr(), len(desc_rows), canv.data_ptr(),
                                                   len(canv_rows), win.data_ptr(), len(win_rows), n_tiles, total_px, None, 0, -1,
                                                   ops._MS_MODES[mode], pred.data_ptr(), None, None, 0,
                                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return pred.cpu()


@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_bad_descriptors_are_skipped_not_followed(dev, mode):
    """The kernel range-checks what the wrapper would have refused.  Unusable windows (view out of range, origin at or beyond the
    canvas edge) are skipped: the result is that of the list without them.  An image whose canvas range runs past the table, with
    17 canvases, or with a canvas left without a usable window is left unwritten, and a good image of the same launch is right.
    Nothing here faults: every bad value is only compared, and every index that is followed stays inside the buffers."""
    views, canvases, _ = M.make_case("small")
    V, H, W = len(views), 20, 30
    tiles, npx = 2 * 2, H * W
    want, _ = ops.resize_argmax_multiscale(views.to(dev), [[(c, list(w)) for c, w in canvases]], [(H, W)], mode=mode)
    want = want[0].cpu().reshape(-1)
    # the window table: the good canvases' windows with unusable ones mixed in, then one-window lists for the bad canvases
    win, canv = [], []
    for (Hc, Wc), wl in canvases:
        first = len(win)
        unusable = [[0, Hc, 0, 0], [0, 0, Wc, 1], [-1, 0, 0, 0], [0, -1, 0, 0], [2 ** 31 - 1, 0, 0, 0], [0, 0, -1, 0]]
        win.append([V, 0, 0, 0])                                   # view index out of range
        for j, (v, oy, ox, m) in enumerate(wl):                    # two unusable windows after every good one
            win += [[v, oy, ox, int(m)], unusable[2 * j % 6], unusable[(2 * j + 1) % 6]]
        canv.append([Hc, Wc, first, len(win) - first])
    assert max(c[3] for c in canv) <= 64
    got = _raw(dev, views, [[H, W, 0, 0, 0, 4]], canv, win, npx, tiles, mode)
    assert torch.equal(got, want)
    # five images in one launch; the table holds the 4 good canvas rows, 17 copies of a good row, and two rows whose only window is
    # unusable (origin at Hc; view index V)
    w_oy, w_view = len(win), len(win) + 1
    win += [[0, 8, 0, 0], [V, 0, 0, 0]]
    canv += [canv[0]] * 17 + [[8, 12, w_oy, 1], [8, 12, w_view, 1]]
    n_canv = len(canv)
    assert n_canv == 4 + 17 + 2
    desc = [[H, W, 0 * npx, 0 * tiles, n_canv - 1, 2],             # the canvas range runs past the table
            [H, W, 1 * npx, 1 * tiles, 4, 17],                     # 17 canvases, all rows good and inside the table
            [H, W, 2 * npx, 2 * tiles, 0, 4],                      # good
            [H, W, 3 * npx, 3 * tiles, 20, 2],                     # a good canvas, then one whose window starts at Hc
            [H, W, 4 * npx, 4 * tiles, 22, 1]]                     # a canvas whose only window names view V
    got = _raw(dev, views, desc, canv, win, 5 * npx, 5 * tiles, mode).view(5, -1)
    assert (got[[0, 1, 3, 4]] == 255).all()
    assert torch.equal(got[2], want)


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


def _text_dev(fx, n, dev):
    return {k: v.to(dev) for k, v in _text(fx, n).items()}


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (40, 70, 3), dtype=np.uint8), rng.integers(0, 256, (50, 50, 3), dtype=np.uint8)]


SCALES = (0.5, 1.0, 1.5)
# written by hand for crop 64, cells of 4, stride 40: per scale (resized size in pixels, canvas in cells, window rows, window columns
# in pixels).  40 x 70 at 0.5: 32 x 56, one padded window, an 8 x 14 canvas; at 1.5: 96 x 168 = 24 x 42 cells, rows 0 and 8 cells,
# columns 0, 10, 20 and 26 cells
HAND = {(40, 70): [((32, 56), (8, 14), [0], [0]), ((64, 112), (16, 28), [0], [0, 40, 48]), ((96, 168), (24, 42), [0, 32], [0, 40, 80, 104])],
        (50, 50): [((32, 32), (8, 8), [0], [0]), ((64, 64), (16, 16), [0], [0]), ((96, 96), (24, 24), [0, 32], [0, 32])]}


def _pixels_by_hand(images, flip, average, scales=SCALES):
    """What MultiScaleInference must feed the model and pass to the op, built without it: the CPU oracle's Pillow resize, windows
    sliced at the hand-written pixel origins and normalised through the oracle's table, 0.0 beyond the image, the image part
    mirrored with a numpy slice.  Returns (pixel windows, canvases, sizes)."""
    from oracle import preprocess_cpu as P
    from lc2is_amd.data.preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    lut = P.normalize_lut(OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)
    px, canvases, sizes = [], [], []
    for im in images:
        cl = []
        for s, ((nh, nw), canvas, rows, cols) in zip(SCALES, HAND[im.shape[:2]]):
            if s not in scales:
                continue
            r = P.resize_bicubic_u8(im, nh, nw)
            plain, mirrored, origins = [], [], [(t, c) for t in rows for c in cols]
            for t, c in origins:
                part = r[t:t + 64, c:c + 64]
                ih, iw = part.shape[:2]
                w = np.zeros((3, 64, 64), dtype=np.float32)
                w[:, :ih, :iw] = np.stack([lut[ch][part[:, :, ch]] for ch in range(3)])
                wm = np.zeros_like(w)
                wm[:, :ih, :iw] = w[:, :ih, :iw][:, :, ::-1]
                plain.append(w); mirrored.append(wm)
            wl = [(len(px) + j, t // 4, c // 4, False) for j, (t, c) in enumerate(origins)]
            px += plain
            wlm = [(len(px) + j, t // 4, c // 4, True) for j, (t, c) in enumerate(origins)] if flip else []
            px += mirrored if flip else []
            cl += [(canvas, wl), (canvas, wlm)] if flip and average == "prob" else [(canvas, wl + wlm)]
        canvases.append(cl); sizes.append(tuple(im.shape[:2]))
    return px, canvases, sizes


def _forwards_by_hand(m, fx, dev, px, batch):
    V = len(px)
    x = torch.from_numpy(np.stack(px + [px[-1]] * (-V % batch))).to(dev)
    with torch.no_grad():
        out = torch.cat([m({"pixel_values": x[b:b + batch], **_text_dev(fx, batch, dev)})["outputs"] for b in range(0, len(x), batch)])
    return out[:V]


class _Recorder(torch.nn.Module):
    """The model, keeping a copy of every batch of pixels it is given."""

    def __init__(self, m):
        super().__init__()
        self.m, self.out_size, self.seen = m, m.out_size, []

    def forward(self, inputs):
        self.seen.append(inputs["pixel_values"].clone())
        return self.m(inputs)


@pytest.mark.parametrize("average", ["prob", "logit"])
def test_multi_scale_inference_end_to_end(dev, average):
    m, fx = _tiny(dev)
    kc = fx["logits"].shape[1]
    images = _images()
    rec = _Recorder(m)
    inf = slide.MultiScaleInference(rec, _text(fx, 5), scales=SCALES, size=64, crop=64, stride=40, flip=True, average=average,
                                    window_batch=5, device=dev)
    assert (inf.grid, inf.cell) == (16, 4)
    # the plans match the hand-written ones
    for im in images:
        assert inf.plan(*im.shape[:2]) == [(size, canvas, [(t // 4, c // 4) for t in rows for c in cols])
                                           for size, canvas, rows, cols in HAND[im.shape[:2]]]
    px, canvases, sizes = _pixels_by_hand(images, True, average)
    assert len(px) == 2 * ((1 + 3 + 8) + (1 + 1 + 4))
    assert [len(cl) for cl in canvases] == ([6, 6] if average == "prob" else [3, 3])
    views, c2, s2 = inf.views(images)
    assert (c2, s2) == (canvases, sizes)
    # every window's pixels: the oracle-resized image, 0.0 in the padding, mirrored windows padded on the same side; 36 windows in
    # batches of 5, the last one filled with its last window
    seen = torch.cat(rec.seen).cpu()
    assert [len(b) for b in rec.seen] == [5] * 8
    assert torch.equal(seen[:36], torch.from_numpy(np.stack(px))) and bool((seen[36:] == seen[35]).all())
    padded, padded_m = seen[0], seen[1]                              # 40 x 70 at scale 0.5: a 32 x 56 image in a 64 x 64 window
    assert bool((padded[:, 32:, :] == 0).all()) and bool((padded[:, :, 56:] == 0).all()) and bool((padded[:, :32, :56] != 0).any())
    assert torch.equal(padded_m[:, :, :56], padded[:, :, :56].flip(-1)) and bool((padded_m[:, :, 56:] == 0).all())
    out = _forwards_by_hand(m, fx, dev, px, 5)
    assert views.shape == (36, kc, 16, 16) and torch.equal(views, out)
    preds = inf.predict(images)
    assert [tuple(p.shape) for p in preds] == sizes and all(p.dtype == torch.uint8 and p.is_cuda for p in preds)
    by_hand, _ = ops.resize_argmax_multiscale(out, canvases, sizes, mode=average)
    assert all(torch.equal(a, b) for a, b in zip(preds, by_hand))


@pytest.mark.parametrize("flip", [True, False])
def test_one_scale_summed_as_logits_is_sliding_window_inference_bitwise(dev, flip):
    m, fx = _tiny(dev)
    kc = fx["logits"].shape[1]
    images = _images()
    gts = _gts(kc)
    kw = dict(size=64, crop=64, stride=40, flip=flip, window_batch=3, device=dev)
    one = slide.SlidingWindowInference(m, _text(fx, 3), **kw)
    ms = slide.MultiScaleInference(m, _text(fx, 3), scales=(1.0,), average="logit", **kw)
    assert all(torch.equal(a, b) for a, b in zip(ms.predict(images), one.predict(images)))
    assert torch.equal(ms.counts(images, gts), one.counts(images, gts))
    assert all(torch.equal(a, b) for a, b in zip(ms.counts_both(images, gts, 0), one.counts_both(images, gts, 0)))


def _gts(kc):
    g = torch.Generator().manual_seed(6)
    gts = [torch.randint(0, kc, (40, 70), generator=g).to(torch.uint8), torch.randint(0, kc, (50, 50), generator=g).to(torch.uint8)]
    gts[0][:5] = 0; gts[1][:, :4] = 255; gts[1][:9, 10:] = 0
    return gts


def test_slide_evaluator_takes_multi_scale_inference_unchanged(dev):
    """SlideEvaluator over MultiScaleInference: the dataset scores from a recount of predictions made from hand-built forwards
    under mmseg's rule, eval_mIOU_gt from a recount under the reference's rule."""
    m, fx = _tiny(dev)
    kc = fx["logits"].shape[1]
    images, gts = _images(), _gts(kc)
    inf = slide.MultiScaleInference(m, _text(fx, 4), scales=(0.5, 1.5), size=64, crop=64, stride=40, flip=True, average="prob",
                                    window_batch=4, device=dev)
    loader = [(images, gts), ([images[1]], [gts[1]])]
    got = evalloop.SlideEvaluator(inf, loader).evaluate()
    assert set(got) == {"eval_mIoU", "eval_mAcc", "eval_aAcc", "eval_mIOU_gt"}
    mm, ref = [], []
    for ims, gs in loader:
        px, canvases, sizes = _pixels_by_hand(ims, True, "prob", scales=(0.5, 1.5))
        preds, _ = ops.resize_argmax_multiscale(_forwards_by_hand(m, fx, dev, px, 4), canvases, sizes, mode="prob")
        mm += [recount(p, gt, kc, 0) for p, gt in zip(preds, gs)]
        ref += [recount(p, gt, kc) for p, gt in zip(preds, gs)]
    mm, ref = torch.stack(mm), torch.stack(ref)
    assert not torch.equal(mm, ref)                                  # the two rules differ on this gt (class 0 and 255 present)
    want = metrics.dataset_iou(mm.sum(0, dtype=torch.int64), 0)
    for k in ("mIoU", "mAcc", "aAcc"):
        assert got["eval_" + k] == pytest.approx(want[k].item(), abs=1e-12), k
    assert got["eval_mIOU_gt"] == pytest.approx(metrics._per_image_iou(ref, 0).mean().item(), abs=1e-12)
    c_mm, c_ref = inf.counts_both(images, gts, 0)
    assert torch.equal(c_mm.cpu(), mm[:2]) and torch.equal(c_ref.cpu(), ref[:2])
