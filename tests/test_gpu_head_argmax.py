"""The head's class map and accuracy / IoU counts on the HIP path (ops.head_upsample_argmax and what is built on it) against the
fp64 torch reference of tests/head_argmax_ref.py.

Gates: pred equals the fp64 argmax on every pixel whose fp64 top-2 gap exceeds 5e-5 * max|score| (the margin of
tests/test_gpu_resize_argmax.py; fp32 against fp64 differs by about 6e-7 on these inputs), at most 1 % of a case's pixels excluded;
counts are EXACTLY the bincount of the kernel's own pred against the labels; everything else is bitwise."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_argmax_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = R.IGN


def _mode(ops, mode):
    return ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR


@pytest.mark.parametrize("B,h,w,S,mode,C", R.CASES)
def test_pred_vs_fp64_and_counts_of_own_pred(dev, B, h, w, S, mode, C):
    from lc2is_amd import ops
    lo, labels = R.case_inputs(B, h, w, S, mode, C)
    arg, sure, _ = R.case_ref(B, h, w, S, mode, C)
    lod, lab = lo.to(dev), labels.to(dev)
    pred, counts = ops.head_upsample_argmax(lod, lab, B, h, w, C, S, _mode(ops, mode))
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (B, h * S, w * S)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, 3, C)
    p = pred.cpu().long()
    excluded = 1.0 - sure.double().mean().item()
    bad = int((p != arg)[sure].sum())
    print("head argmax figures", (B, h, w, S, mode, C), "excluded", excluded, "differ", bad, "differ inside margin", int((p != arg).sum()) - bad)
    assert excluded <= R.MAX_EXCLUDED
    assert int(p.max()) < C and bad == 0
    assert torch.equal(counts.cpu().long(), R.counts(p, labels, C, IGN))
    # class 0 ignored: its pixels leave all three rows; the class map does not depend on the labels
    pred0, counts0 = ops.head_upsample_argmax(lod, lab, B, h, w, C, S, _mode(ops, mode), ignore_index=0)
    assert torch.equal(pred0, pred)
    assert torch.equal(counts0.cpu().long(), R.counts(p, labels, C, 0)) and int(counts0[:, 2, 0].sum()) == 0
    # pred only (no labels, no workspace) and counts only
    pred1, none = ops.head_upsample_argmax(lod, None, B, h, w, C, S, _mode(ops, mode), want_counts=False)
    assert none is None and torch.equal(pred1, pred)
    none, counts1 = ops.head_upsample_argmax(lod, lab, B, h, w, C, S, _mode(ops, mode), want_pred=False)
    assert none is None and torch.equal(counts1, counts)
    # two runs give the same bytes
    pred2, counts2 = ops.head_upsample_argmax(lod, lab, B, h, w, C, S, _mode(ops, mode))
    assert torch.equal(pred2, pred) and torch.equal(counts2, counts)


@pytest.mark.parametrize("B,h,w,S,mode", R.SHAPES)
@pytest.mark.parametrize("C", [129, 192])
def test_exact_ties_go_to_the_lowest_class(dev, B, h, w, S, mode, C):
    from lc2is_amd import ops
    lo, labels = R.case_inputs(B, h, w, S, mode, C)
    lo = lo.clone()
    lo[:, 100] = lo[:, 3]
    lo[:, [3, 100]] += 10
    pred, counts = ops.head_upsample_argmax(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode))
    assert bool((pred == 3).all())
    assert int(counts[:, 1, 3].sum()) == int(R.counted(labels, C, IGN).sum()) and int(counts[:, 1].sum()) == int(counts[:, 1, 3].sum())


def test_all_minus_inf_is_class_zero_and_nan_stays_inside(dev):
    from lc2is_amd import ops
    B, h, w, S, mode, C = R.CASES[4]
    lo, labels = R.case_inputs(B, h, w, S, mode, C)
    ninf = torch.full_like(lo, float("-inf"))
    pred, counts = ops.head_upsample_argmax(ninf.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode))
    assert not pred.any() and torch.equal(counts.cpu().long(), R.counts(pred.cpu(), labels, C, IGN))
    nan = lo.clone()
    nan[::3, :C] = float("nan")
    pred, counts = ops.head_upsample_argmax(nan.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode))
    assert int(pred.max()) < C and torch.equal(counts.cpu().long(), R.counts(pred.cpu(), labels, C, IGN))


@pytest.mark.parametrize("B,h,w,S,mode,C", [R.CASES[4], R.CASES[6], R.CASES[15], R.CASES[23]])
def test_every_pixel_written_and_nothing_else(dev, B, h, w, S, mode, C):
    """pred pre-filled with 255 inside a guarded buffer: no 255 is left (C <= 192) and the guard bytes keep theirs."""
    from lc2is_amd import _lib, ops
    lo, labels = R.case_inputs(B, h, w, S, mode, C)
    lod = lo.to(dev)
    n, G = labels.numel(), 4096
    buf = torch.full((n + 2 * G,), 255, dtype=torch.uint8, device=dev)
    pred = buf[G:G + n]
    _lib.check(ops._fn("lc2is_head_upsample_argmax")(lod.data_ptr(), lod.shape[1], None, pred.data_ptr(), None, B, h, w, C, S,
                                                     _mode(ops, mode), IGN, None, 0, torch.cuda.current_stream().cuda_stream), "argmax")
    want, _ = ops.head_upsample_argmax(lod, None, B, h, w, C, S, _mode(ops, mode), want_counts=False)
    assert not (pred == 255).any() and torch.equal(pred.view(want.shape), want)
    assert bool((buf[:G] == 255).all()) and bool((buf[G + n:] == 255).all())


@pytest.mark.parametrize("B,h,w,S,mode,C", [R.CASES[4], R.CASES[14 + 5]])
def test_batch_independence(dev, B, h, w, S, mode, C):
    from lc2is_amd import ops
    assert B == 2
    lo, labels = R.case_inputs(B, h, w, S, mode, C)
    lod, lab = lo.to(dev), labels.to(dev)
    pred, counts = ops.head_upsample_argmax(lod, lab, B, h, w, C, S, _mode(ops, mode))
    for b in range(B):
        p1, c1 = ops.head_upsample_argmax(lod[b * h * w:(b + 1) * h * w].contiguous(), lab[b:b + 1].contiguous(), 1, h, w, C, S,
                                          _mode(ops, mode))
        assert torch.equal(p1[0], pred[b]) and torch.equal(c1[0], counts[b])


def test_many_tiles_sum_in_the_finish_launch(dev):
    """B = 3, 16 x 16 cells, S = 4: 25 tiles per image, more than the finish launch's four strided parts."""
    from lc2is_amd import ops
    B, h, S, C = 3, 16, 4, 151
    g = torch.Generator().manual_seed(0)
    lo = torch.full((B * h * h, 192), R.PAD_SCORE)
    lo[:, :C] = torch.randn(B * h * h, C, generator=g)
    labels = torch.randint(-2, C + 3, (B, h * S, h * S), generator=g)
    pred, counts = ops.head_upsample_argmax(lo.to(dev), labels.to(dev), B, h, h, C, S, ops.INTERP_BICUBIC)
    assert torch.equal(counts.cpu().long(), R.counts(pred.cpu(), labels, C, IGN))
    arg, gap = R.ref_argmax(lo, B, h, h, C, S, "bicubic")
    sure = gap > R.MARGIN * lo[:, :C].abs().max().item()
    assert 1.0 - sure.double().mean().item() <= R.MAX_EXCLUDED and int((pred.cpu().long() != arg)[sure].sum()) == 0


# ---- modules, on the tiny model the OHEM and Dice tests build ----
def _tiny(dev):
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


def _tiny_batch(dev, fx):
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev).clone()
    labels[:, :3] = IGN
    labels[:, 5, ::2] = 151   # not counted: >= K
    return inputs, labels


def _check_pred_against_logits(pred, logits):
    top2 = logits.double().topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > R.MARGIN * logits.abs().max().item()
    excluded = 1.0 - sure.double().mean().item()
    bad = int((pred.long() != logits.argmax(1))[sure].sum())
    print("head argmax figures predict: excluded", excluded, "differ", bad)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (logits.shape[0],) + tuple(logits.shape[2:])
    assert excluded <= R.MAX_EXCLUDED and bad == 0


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _zero(m):
    for p in m.parameters():
        p.grad = None


def test_predict_and_forward_loss_seg_counts(dev):
    m, fx = _tiny(dev)
    inputs, labels = _tiny_batch(dev, fx)
    K = 151
    with torch.no_grad():
        logits = m(inputs)["outputs"]
    pred = m.predict(inputs)
    _check_pred_against_logits(pred, logits)
    assert not pred.requires_grad
    want = R.counts(pred.cpu(), labels.cpu(), K, IGN).sum(0)
    assert int(want[2].sum()) == int(R.counted(labels.cpu(), K, IGN).sum()) > 0
    # the loss and the gradients keep their bits; the buffer takes += counts.sum(0)
    loss0 = m.forward_loss(inputs, labels)
    loss0.backward()
    g0 = _grads(m)
    _zero(m)
    buf = torch.zeros(3, K, dtype=torch.int64, device=dev)
    loss1 = m.forward_loss(inputs, labels, seg_counts=buf)
    loss1.backward()
    g1 = _grads(m)
    _zero(m)
    assert torch.equal(loss0, loss1) and g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert torch.equal(buf.cpu(), want)
    m.forward_loss(inputs, labels, seg_counts=buf).backward()
    _zero(m)
    assert torch.equal(buf.cpu(), 2 * want)
    # under ohem= the counts are those of the ORIGINAL labels, and the loss is the OHEM loss unchanged
    ohem = (0.7, 16)
    la = m.forward_loss(inputs, labels, ohem=ohem)
    la.backward()
    ga = _grads(m)
    _zero(m)
    seen = m.last_ohem[0].clone()
    buf.zero_()
    lb = m.forward_loss(inputs, labels, ohem=ohem, seg_counts=buf)
    lb.backward()
    gb = _grads(m)
    _zero(m)
    assert torch.equal(la, lb) and all(torch.equal(ga[k], gb[k]) for k in ga) and torch.equal(m.last_ohem[0], seen)
    assert int((seen != labels).sum()) > 0                       # the selection did relabel pixels
    assert torch.equal(buf.cpu(), want)
    # Dice + CE, and CE with options
    for kw in (dict(dice=(1.0, 3.0, 1.0, True)), dict(label_smoothing=0.1, reduction="sum")):
        lc = m.forward_loss(inputs, labels, **kw).detach().clone()
        _zero(m)
        buf.zero_()
        ld = m.forward_loss(inputs, labels, seg_counts=buf, **kw).detach()
        _zero(m)
        assert torch.equal(lc, ld) and torch.equal(buf.cpu(), want)
    # ignore_index = 0 reaches the counts
    buf.zero_()
    m.forward_loss(inputs, labels, 0, seg_counts=buf)
    assert torch.equal(buf.cpu(), R.counts(pred.cpu(), labels.cpu(), K, 0).sum(0))


def test_score_map_tail_predict_and_seg_counts(dev):
    import lc2is_amd.nn as N
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(-1, K + 2, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    tail = N.ScoreMapTail(4)
    with torch.no_grad():
        logits = tail(ve, te)
    pred = tail.predict(ve, te)
    _check_pred_against_logits(pred, logits)
    want = R.counts(pred.cpu(), labels.cpu(), K, IGN).sum(0)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    l1 = tail.loss(v1, t1, labels)
    l1.backward()
    buf = torch.zeros(3, K, dtype=torch.int64, device=dev)
    for kw in ({}, dict(ohem=(0.7, 64))):
        va, ta = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
        la = tail.loss(va, ta, labels, **kw)
        la.backward()
        v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
        buf.zero_()
        l2 = tail.loss(v2, t2, labels, seg_counts=buf, **kw)
        l2.backward()
        assert torch.equal(la, l2) and torch.equal(va.grad, v2.grad) and torch.equal(ta.grad, t2.grad)
        assert torch.equal(buf.cpu(), want)


def _criterion(name):
    import lc2is_amd.nn as N
    return {"plain": lambda: None, "opts": lambda: N.CrossEntropyLoss(label_smoothing=0.1),
            "ohem": lambda: N.OhemCrossEntropyLoss(0.7, 16), "dice": lambda: N.DiceCrossEntropyLoss(dice_weight=3.0)}[name]()


@pytest.mark.parametrize("crit", ["plain", "opts", "ohem", "dice"])
def test_train_step_seg_metrics(dev, crit):
    """Three steps: parameters and losses bitwise those of a twin without seg_metrics; the buffer is the sum of the per-step counts
    of the class maps the twin predicts in front of each step."""
    from lc2is_amd.step import TrainStep
    K = 151
    m_a, fx = _tiny(dev)
    m_b, _ = _tiny(dev)
    inputs, labels = _tiny_batch(dev, fx)
    ts_a = TrainStep(m_a, optimizer="sgd", lr=1e-2, momentum=0.9, criterion=_criterion(crit), seg_metrics=True)
    ts_b = TrainStep(m_b, optimizer="sgd", lr=1e-2, momentum=0.9, criterion=_criterion(crit))
    assert ts_a.seg_counts.dtype == torch.int64 and tuple(ts_a.seg_counts.shape) == (3, K) and not ts_a.seg_counts.any()
    with pytest.raises(RuntimeError, match="seg_metrics"):
        ts_b.seg_counts
    buf = ts_a.seg_counts
    want = torch.zeros(3, K, dtype=torch.int64)
    for _ in range(3):
        want += R.counts(m_b.predict(inputs).cpu(), labels.cpu(), K, IGN).sum(0)
        la, lb = ts_a.step(inputs, labels).clone(), ts_b.step(inputs, labels).clone()
        assert torch.equal(la, lb)
    assert torch.equal(ts_a.arena.flat, ts_b.arena.flat)
    assert ts_a.seg_counts is buf and torch.equal(buf.cpu(), want)
    assert int(want[2].sum()) == 3 * int(R.counted(labels.cpu(), K, IGN).sum())
    met = ts_a.seg_metrics()
    assert all(met[k].is_cuda and met[k].dtype == torch.float64 for k in ("aAcc", "mAcc", "mIoU", "IoU")) and tuple(met["IoU"].shape) == (K,)
    assert met["aAcc"].item() == (want[0].sum().double() / want[2].sum().double()).item()
    assert torch.equal(buf.cpu(), want)                      # reading does not reset
    met2 = ts_a.seg_metrics(reset=True)
    assert torch.equal(met2["aAcc"], met["aAcc"]) and ts_a.seg_counts is buf and not buf.any()


def test_seg_metrics_leaves_the_ignored_class_out_of_the_means(dev):
    import lc2is_amd.nn as N
    from lc2is_amd.metrics import dataset_iou
    from lc2is_amd.step import TrainStep
    m, fx = _tiny(dev)
    inputs, labels = _tiny_batch(dev, fx)
    ts = TrainStep(m, optimizer="sgd", lr=1e-2, criterion=N.CrossEntropyLoss(ignore_index=0), seg_metrics=True)
    want = R.counts(m.predict(inputs).cpu(), labels.cpu(), 151, 0).sum(0)
    ts.step(inputs, labels)
    assert torch.equal(ts.seg_counts.cpu(), want) and int(want[2, 0]) == 0
    met, ref = ts.seg_metrics(), dataset_iou(want, 0)
    assert all(torch.equal(met[k].cpu(), ref[k]) or (k == "IoU" and torch.equal(met[k].cpu().nan_to_num(-1), ref[k].nan_to_num(-1)))
               for k in ("aAcc", "mAcc", "mIoU", "IoU"))
    assert torch.isnan(met["IoU"][0])


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    lab = torch.randint(0, 151, (2, 16, 16), generator=g)
    lab[:, seed % 5] = IGN
    return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
             "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}, lab.to(dev))


def test_captured_step_keeps_counting_across_replays(dev):
    """A captured step replayed on three new batches gives the counts (and losses, parameters) of three eager steps; the buffer exists
    before the capture, reading and resetting happen outside the graph."""
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(4)]
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    ts_e = TrainStep(m_e, optimizer="sgd", lr=1e-3, seg_metrics=True)
    ts_g = TrainStep(m_g, optimizer="sgd", lr=1e-3, seg_metrics=True)
    buf = ts_g.seg_counts
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(*batches[0])
    torch.cuda.synchronize()
    assert ts_g.seg_counts is buf and torch.equal(ts_e.seg_counts, buf)     # the two warm-up steps are real steps and count
    ts_e.seg_metrics(reset=True)
    ts_g.seg_metrics(reset=True)
    assert not buf.any()
    total = 0
    for inp, lab in batches[1:]:
        le = ts_e.step(inp, lab).clone()
        lg = run(inp, lab).clone()
        total += int((lab != IGN).sum())
        assert torch.equal(le, lg) and torch.equal(ts_e.seg_counts, buf)
        assert int(buf[2].sum()) == int(buf[1].sum()) == total
    torch.cuda.synchronize()
    assert torch.equal(ts_e.arena.flat, ts_g.arena.flat)
    assert torch.equal(ts_e.seg_metrics()["mIoU"], ts_g.seg_metrics()["mIoU"])
    run.release()
