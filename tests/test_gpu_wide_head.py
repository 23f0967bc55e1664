"""The fused head past 192 classes on the HIP path: the chunked cross-entropy against fp64 (with the online softmax's edge cases), the
wide kernels against the narrow ones at C <= 192, the chunked argmax and its counts against fp64, bitwise repeatability, and the
model layer (ScoreMapTail, BaseModelWithText, TrainStep: eager, captured, accumulated) against its own materialised logits.

Bounds: tests/wide_head_ref.py (the project's loss 1e-4 / weight sum 1e-5 / gradient 2e-5 of this head, the first and the last times
ld / 192); 1e-6 wide against narrow (the gamma = 0 focal-vs-CE bound); 1e-5 / 1e-3 for a model against its own materialised logits;
8e-2 / 2e-2 for parameter changes and the loss of a step.  Every measured figure is printed before it is asserted."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_argmax_ref as A  # noqa: E402
import wide_head_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = R.IGN
GRAD_KEYS = ("class_prototypes", "vision_decoder.layers.0.linear2.weight")
STEP_KEYS = GRAD_KEYS + ("pixel_patch.visual.weight", "vision_encoder.enc.embeddings.patch_embedding.weight",
                         "text_encoder.enc.embeddings.token_embedding.weight")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _mode(ops, mode):
    return ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR


def _figures(loss, dlo, C, ref):
    ref_loss, ref_wsum, ref_grad = ref
    return dict(loss=abs(loss[0].item() - ref_loss) / abs(ref_loss), wsum=abs(loss[1].item() - ref_wsum) / ref_wsum,
                grad=_rel(dlo[:, :C], ref_grad), pad=dlo[:, C:].abs().max().item() if dlo.shape[1] > C else 0.0)


def _within(fig, ld):
    lb, wb, gb = R.bounds(ld)
    return fig["loss"] <= lb and fig["wsum"] <= wb and fig["grad"] <= gb and fig["pad"] == 0


# ---- 1. cross-entropy against fp64 ----
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("case", range(len(R.CASES)), ids=R.IDS)
def test_head_upsample_ce_wide_vs_fp64(dev, case, weighted):
    from lc2is_amd import ops
    B, h, w, mode, C = R.CASES[case]
    lo, labels, w64, ref = R.case_ref(case, weighted)
    cw = w64.float().to(dev) if weighted else None
    lod, lab = lo.to(dev), labels.to(dev)
    loss, dlo = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, _mode(ops, mode), want_grad=True, class_weight=cw)
    fig = _figures(loss, dlo, C, ref)
    print("wide head figures ce", R.CASES[case], "weighted" if weighted else "plain", "ld", lo.shape[1], fig)
    assert bool(torch.isfinite(dlo).all()) and tuple(dlo.shape) == tuple(lo.shape)
    assert _within(fig, lo.shape[1]), (fig, R.bounds(lo.shape[1]))
    if not weighted:
        assert loss[1].item() == float(A.counted(labels, C, IGN).sum())          # the integer count, exactly
    # a loss-only call (one sweep, no gradient slabs in the workspace) gives the same two sums
    loss0, none = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, _mode(ops, mode), class_weight=cw)
    assert none is None and torch.equal(loss0, loss)


def test_grad_scale_ignore_index_and_wider_pad(dev):
    from lc2is_amd import ops
    B, h, w, mode, C = R.CASES[3]   # (2, 9, 9, bicubic, 384)
    lo, labels = R.case_inputs(B, h, w, mode, C)
    lod, lab = lo.to(dev), labels.to(dev)
    l1, d1 = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, want_grad=True)
    l2, d2 = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, want_grad=True, grad_scale=0.25)
    assert torch.equal(l1, l2) and torch.equal(d2, d1 * 0.25)                    # a power of two: exact
    l3, _ = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, ignore_index=0)
    assert l3[1].item() == float(((labels != 0) & (labels >= 0) & (labels < C)).sum())
    wide = torch.full((lo.shape[0], 1024), A.PAD_SCORE)                           # ld need not be the smallest pad
    wide[:, :C] = lo[:, :C]
    l4, d4 = ops.head_upsample_ce_wide(wide.to(dev), lab, B, h, w, C, 4, want_grad=True)
    assert torch.equal(l4, l1) and torch.equal(d4[:, :C], d1[:, :C]) and not d4[:, C:].any()


# ---- 2. online-softmax edge cases ----
@pytest.mark.parametrize("name", R.EDGE_NAMES)
def test_online_softmax_edge_cases(dev, name):
    from lc2is_amd import ops
    e = R.EDGE
    lo, labels, w64, ref = R.edge_ref(name)
    loss, dlo = ops.head_upsample_ce_wide(lo.to(dev), labels.to(dev), e["B"], e["h"], e["w"], e["C"], 4, _mode(ops, e["mode"]),
                                          want_grad=True, class_weight=w64.float().to(dev))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dlo).all())
    fig = _figures(loss, dlo, e["C"], ref)
    print("wide head figures edge", name, fig, ref[0])
    assert _within(fig, lo.shape[1]), (fig, R.bounds(lo.shape[1]))


def test_all_labels_ignored(dev):
    from lc2is_amd import ops
    e = R.EDGE
    lo, labels = R.edge_case("huge_scores")
    none = torch.full_like(labels, IGN)
    loss, dlo = ops.head_upsample_ce_wide(lo.to(dev), none.to(dev), e["B"], e["h"], e["w"], e["C"], 4, _mode(ops, e["mode"]),
                                          want_grad=True)
    assert loss.tolist() == [0.0, 0.0] and not dlo.any() and not bool(torch.isnan(dlo).any())


# ---- 3. wide against narrow at C <= 192 ----
@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("C", [151, 192])
def test_wide_matches_narrow_up_to_192_classes(dev, C, mode):
    from lc2is_amd import ops
    B, h, w = (2, 9, 9) if mode == "bicubic" else (2, 5, 5)
    lo, labels = A.case_inputs(B, h, w, 4, mode, C)
    assert lo.shape[1] == 192
    lod, lab = lo.to(dev), labels.to(dev)
    cw = R.weights(C, 3).float().to(dev)
    m = _mode(ops, mode)
    l0, d0, _ = ops.head_upsample_ce(lod, lab, B, h, w, C, 4, m, want_grad=True, grad_scale=0.25, class_weight=cw)
    l1, d1 = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, m, want_grad=True, grad_scale=0.25, class_weight=cw)
    print("wide head figures wide vs narrow", (mode, C), abs(l1[0].item() - l0[0].item()) / abs(l0[0].item()), _rel(d1, d0))
    assert abs(l1[0].item() - l0[0].item()) <= 1e-6 * abs(l0[0].item())
    assert abs(l1[1].item() - l0[1].item()) <= 1e-6 * abs(l0[1].item())
    assert _rel(d1, d0) <= 1e-6
    p0, c0 = ops.head_upsample_argmax(lod, lab, B, h, w, C, 4, m)
    p1, c1 = ops.head_upsample_argmax_wide(lod, lab, B, h, w, C, 4, m)
    _, sure, _ = A.case_ref(B, h, w, 4, mode, C)
    assert p1.dtype == torch.int16 and torch.equal(p1.cpu().long()[sure], p0.cpu().long()[sure])
    assert torch.equal(c1.cpu().long(), A.counts(p1.cpu(), labels, C, IGN))


# ---- 4. argmax against fp64 ----
@pytest.mark.parametrize("case", range(len(R.CASES)), ids=R.IDS)
def test_head_upsample_argmax_wide_vs_fp64(dev, case):
    from lc2is_amd import _lib, ops
    B, h, w, mode, C = R.CASES[case]
    lo, labels = R.case_inputs(B, h, w, mode, C)
    arg, sure, _ = A.case_ref(B, h, w, 4, mode, C)
    lod, lab = lo.to(dev), labels.to(dev)
    pred, counts = ops.head_upsample_argmax_wide(lod, lab, B, h, w, C, 4, _mode(ops, mode))
    assert pred.dtype == torch.int16 and tuple(pred.shape) == (B, 4 * h, 4 * w)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, 3, C)
    p = pred.cpu().long()
    excluded = 1.0 - sure.double().mean().item()
    bad = int((p != arg)[sure].sum())
    print("wide head figures argmax", R.CASES[case], "excluded", excluded, "differ", bad, "differ inside margin",
          int((p != arg).sum()) - bad)
    assert excluded <= A.MAX_EXCLUDED
    assert int(p.min()) >= 0 and int(p.max()) < C and bad == 0
    assert torch.equal(counts.cpu().long(), A.counts(p, labels, C, IGN))
    # pred pre-filled with -1 in a guarded buffer, no labels, no workspace: every pixel is written and nothing else
    n, G = labels.numel(), 2048
    buf = torch.full((n + 2 * G,), -1, dtype=torch.int16, device=dev)
    out = buf[G:G + n]
    _lib.check(ops._fn("lc2is_head_upsample_argmax_wide")(lod.data_ptr(), lod.shape[1], None, out.data_ptr(), None, B, h, w, C, 4,
                                                          _mode(ops, mode), IGN, None, 0, torch.cuda.current_stream().cuda_stream),
               "argmax_wide")
    assert not (out == -1).any() and torch.equal(out.view(pred.shape), pred)
    assert bool((buf[:G] == -1).all()) and bool((buf[G + n:] == -1).all())
    pred1, none = ops.head_upsample_argmax_wide(lod, None, B, h, w, C, 4, _mode(ops, mode), want_counts=False)
    assert none is None and torch.equal(pred1, pred)
    none, counts1 = ops.head_upsample_argmax_wide(lod, lab, B, h, w, C, 4, _mode(ops, mode), want_pred=False)
    assert none is None and torch.equal(counts1, counts)


def test_exact_ties_across_chunks_go_to_the_lowest_class(dev):
    from lc2is_amd import ops
    B, h, w, mode, C = R.CASES[4]   # (2, 9, 9, bicubic, 847)
    lo, labels = R.case_inputs(B, h, w, mode, C)
    lo = lo.clone()
    lo[:, 800] = lo[:, 200] = lo[:, 3]
    lo[:, [3, 200, 800]] += 10
    pred, counts = ops.head_upsample_argmax_wide(lo.to(dev), labels.to(dev), B, h, w, C, 4, _mode(ops, mode))
    assert bool((pred == 3).all())
    assert int(counts[:, 1, 3].sum()) == int(A.counted(labels, C, IGN).sum()) == int(counts[:, 1].sum())


def test_seg_counts_add_dispatches_on_the_class_count(dev):
    from lc2is_amd import ops
    for case in (0, 16):   # C = 193 and C = 847
        B, h, w, mode, C = R.CASES[case]
        lo, labels = R.case_inputs(B, h, w, mode, C)
        lod, lab = lo.to(dev), labels.to(dev)
        seg = torch.zeros(3, C, dtype=torch.int64, device=dev)
        ops.seg_counts_add(seg, lod, lab, B, h, w, C, 4, _mode(ops, mode), IGN)
        _, counts = ops.head_upsample_argmax_wide(lod, lab, B, h, w, C, 4, _mode(ops, mode), want_pred=False)
        assert torch.equal(seg, counts.long().sum(0))


# ---- 5. bitwise repeatability ----
@pytest.mark.parametrize("case", [4, 16], ids=[R.IDS[4], R.IDS[16]])   # 847 classes, bicubic and bilinear
def test_bitwise_reproducible(dev, case):
    from lc2is_amd import ops
    B, h, w, mode, C = R.CASES[case]
    lo, labels = R.case_inputs(B, h, w, mode, C)
    lod, lab = lo.to(dev), labels.to(dev)
    cw = R.weights(C, 1).float().to(dev)
    m = _mode(ops, mode)
    a = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, m, want_grad=True, class_weight=cw)
    pa = ops.head_upsample_argmax_wide(lod, lab, B, h, w, C, 4, m)
    b = ops.head_upsample_ce_wide(lod, lab, B, h, w, C, 4, m, want_grad=True, class_weight=cw)
    pb = ops.head_upsample_argmax_wide(lod, lab, B, h, w, C, 4, m)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[1].any())
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]) and bool(pa[1].any())


# ---- 6. ScoreMapTail ----
def _sure(logits):
    top2 = logits.double().topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > A.MARGIN * logits.abs().max().item()


@pytest.mark.parametrize("K", [200, 300])
def test_score_map_tail_past_192_classes(dev, K):
    import lc2is_amd.nn as N
    B, h, C = 2, 8, 64
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    w = R.weights(K, 13).to(dev)
    tail = N.ScoreMapTail(4)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    logits = tail(v1, t1)
    assert tuple(logits.shape) == (B, K, 4 * h, 4 * h)
    loss_u = F.cross_entropy(logits.double(), labels, weight=w, ignore_index=IGN)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, weight=w.float())
    loss_f.backward()
    print("wide head figures score tail", K, loss_f.item(), loss_u.item(), _rel(v2.grad, v1.grad), _rel(t2.grad, t1.grad))
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert bool(v1.grad.any()) and bool(t1.grad.any())
    assert _rel(v2.grad, v1.grad) <= 1e-3 and _rel(t2.grad, t1.grad) <= 1e-3
    pred = tail.predict(ve, te)
    sure = _sure(logits.detach())
    assert pred.dtype == torch.int16 and tuple(pred.shape) == (B, 4 * h, 4 * h)
    assert 1.0 - sure.double().mean().item() <= A.MAX_EXCLUDED
    assert torch.equal(pred.long()[sure], logits.detach().argmax(1)[sure])
    assert N.ScoreMapTail(4).predict(ve, te[:, :150]).dtype == torch.uint8        # up to 192 classes: as it was


# ---- 7. BaseModelWithText and the step ----
K_WIDE = 200


def _tiny(dev):
    import lc2is_amd.nn as N
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    sd = {k: v for k, v in fx["state_dict"].items() if k != "class_prototypes"}
    protos = torch.randn(K_WIDE, fx["state_dict"]["class_prototypes"].shape[1], generator=torch.Generator().manual_seed(5))
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64, prototypes=protos)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert missing == ["class_prototypes"] and not unexpected
    return m.to(dev).train(), fx


def _batch(dev, seed, fx=None):
    g = torch.Generator().manual_seed(seed)
    if fx is not None:
        inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    else:
        ids = torch.randint(1, 500, (2, 8), generator=g)
        ids[:, 0], ids[:, -1] = 510, 511
        inputs = {"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
                  "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    labels = torch.randint(0, K_WIDE, (inputs["pixel_values"].shape[0], 16, 16), generator=g)
    labels[:, :3] = IGN
    return inputs, labels.to(dev)


def _ref_loss(logits, labels, weight=None, reduction="mean"):
    return F.cross_entropy(logits.double(), labels, weight=None if weight is None else weight.double(), ignore_index=IGN,
                           reduction=reduction)


@pytest.mark.parametrize("weighted,reduction", [(True, "mean"), (False, "sum")])
def test_forward_loss_matches_materialised_logits(dev, weighted, reduction):
    m, fx = _tiny(dev)
    inputs, labels = _batch(dev, 3, fx)
    w = R.weights(K_WIDE, 12).float().to(dev) if weighted else None
    logits = m(inputs)["outputs"]
    assert tuple(logits.shape) == (labels.shape[0], K_WIDE, 16, 16)
    loss_u = _ref_loss(logits, labels, w, reduction)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    loss_f = m.forward_loss(inputs, labels, weight=w, reduction=reduction)
    loss_f.backward()
    named = dict(m.named_parameters())
    rels = {k: _rel(named[k].grad, g_u[k]) for k in GRAD_KEYS}
    print("wide head figures forward_loss", weighted, reduction, loss_f.item(), loss_u.item(), rels)
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert all(bool(g.any()) for g in g_u.values())
    assert all(r <= 1e-3 for r in rels.values()), rels
    with torch.no_grad():
        pred = m.predict(inputs)
        sure = _sure(logits.detach())
    assert pred.dtype == torch.int16 and torch.equal(pred.long()[sure], logits.detach().argmax(1)[sure])


def test_forward_loss_beside_seg_counts(dev):
    from lc2is_amd import metrics
    m, fx = _tiny(dev)
    inputs, labels = _batch(dev, 3, fx)
    with torch.no_grad():
        plain = m.forward_loss(inputs, labels)
        counts = torch.zeros(3, K_WIDE, dtype=torch.int64, device=dev)
        with_counts = m.forward_loss(inputs, labels, seg_counts=counts)
        assert torch.equal(plain, with_counts) and int(counts[2].sum()) == int((labels != IGN).sum())
        pred = m.predict(inputs)
    assert torch.equal(counts.cpu(), A.counts(pred.cpu(), labels.cpu(), K_WIDE, IGN).sum(0))
    iou = metrics.dataset_iou(counts)
    assert 0.0 <= float(iou["aAcc"]) <= 1.0


def test_train_step_past_192_classes(dev):
    """One SGD step of TrainStep moves the parameters as the reference composition on the materialised logits plus -lr * gradient
    does; seg_metrics=True leaves the step's bytes alone."""
    from lc2is_amd.step import TrainStep
    lr = 1e-2
    m1, fx = _tiny(dev)
    m2, _ = _tiny(dev)
    m3, _ = _tiny(dev)
    inputs, labels = _batch(dev, 3, fx)
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    loss_ts = TrainStep(m1, optimizer="sgd", lr=lr).step(inputs, labels)
    loss_h = _ref_loss(m2(inputs)["outputs"], labels)
    loss_h.backward()
    named1, named2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    rels = {k: _rel(named1[k].detach() - start[k], -lr * named2[k].grad) for k in STEP_KEYS}
    print("wide head figures train step", loss_ts.item(), loss_h.item(), rels)
    assert abs(loss_ts.item() - loss_h.item()) <= 1e-4 * abs(loss_h.item())
    assert all(r < 8e-2 for r in rels.values()), rels
    ts3 = TrainStep(m3, optimizer="sgd", lr=lr, seg_metrics=True)
    assert torch.equal(ts3.step(inputs, labels), loss_ts)
    named3 = dict(m3.named_parameters())
    assert all(torch.equal(named1[k], named3[k]) for k in named1), "seg_metrics=True changed the step"
    assert tuple(ts3.seg_counts.shape) == (3, K_WIDE) and int(ts3.seg_counts[2].sum()) == int((labels != IGN).sum())


def test_train_step_with_weighted_criterion_captured(dev):
    """A captured step replayed on another batch gives bitwise the loss and the parameters of the eager step."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(2)]
    w = R.weights(K_WIDE, 15).float()
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    ts_e = TrainStep(m_e, optimizer="sgd", lr=1e-3, criterion=N.CrossEntropyLoss(weight=w).to(dev))
    ts_g = TrainStep(m_g, optimizer="sgd", lr=1e-3, criterion=N.CrossEntropyLoss(weight=w).to(dev))
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(*batches[0])
    torch.cuda.synchronize()
    assert torch.equal(ts_e.step(*batches[1]).clone(), run(*batches[1]).clone())
    torch.cuda.synchronize()
    assert torch.equal(ts_e.arena.flat, ts_g.arena.flat)
    run.release()


def test_accumulate_two_micro_batches_equal_one_step(dev):
    """accumulate=2 over two B = 1 micro-batches (one with most rows ignored) against one step on the B = 2 batch: parameter changes
    within relative L2 8e-2, loss within 2e-2 (tests/test_gpu_accum.py)."""
    from lc2is_amd.step import TrainStep
    lr = 0.05
    inputs, labels = _batch(dev, 41)
    labels[0, :12] = IGN
    m_a, _ = _tiny(dev)
    m_b, _ = _tiny(dev)
    start = {k: p.detach().clone() for k, p in m_a.named_parameters() if k in STEP_KEYS}
    ts_a = TrainStep(m_a, optimizer="sgd", lr=lr, accumulate=2)
    ts_b = TrainStep(m_b, optimizer="sgd", lr=lr)
    for i in range(2):
        ts_a.step({k: v[i:i + 1] for k, v in inputs.items()}, labels[i:i + 1])
    loss_b = ts_b.step(inputs, labels)
    na, nb = dict(m_a.named_parameters()), dict(m_b.named_parameters())
    rels = {k: _rel(na[k].detach() - start[k], nb[k].detach() - start[k]) for k in STEP_KEYS}
    err = abs(ts_a.accum_loss.item() - loss_b.item())
    print("wide head figures accumulate", rels, err, ts_a.accum_count.item())
    assert all(r <= 8e-2 for r in rels.values()), rels
    assert err <= 2e-2
    assert ts_a.accum_count.item() == float((labels != IGN).sum())


# ---- 8. refusals on the device path ----
def test_refusals_on_the_device_path(dev):
    from lc2is_amd import ops
    m, fx = _tiny(dev)
    inputs, labels = _batch(dev, 3, fx)
    for kw in (dict(focal=(2.0, 0.0)), dict(dice=(1.0, 1.0, 1.0, True)), dict(ohem=(0.7, 100)), dict(sigmoid=(2.0, 0.25, "elements")),
               dict(label_smoothing=0.1)):
        with pytest.raises(NotImplementedError, match="192"):
            m.forward_loss(inputs, labels, **kw)
    B, h, w, mode, C = R.CASES[0]   # C = 193
    lo, lab = R.case_inputs(B, h, w, mode, C)
    with pytest.raises(RuntimeError):
        ops.head_upsample_ce(lo.to(dev), lab.to(dev), B, h, w, C, 4, _mode(ops, mode))
    with pytest.raises(RuntimeError, match="192"):
        ops.head_upsample_argmax(lo.to(dev), lab.to(dev), B, h, w, C, 4, _mode(ops, mode))
