"""Self-training on the HIP path: ops.head_upsample_conf (class map, confidence, pseudo-labels, counts), ops.head_upsample_ce_pw
(cross-entropy with a per-pixel weight) and what is built on them — forward_loss(pixel_weight=), predict_confidence,
TrainStep.step(pixel_weight=), selftrain.PseudoLabeler — against the fp64 torch references of tests/selftrain_ref.py.

Gates (tests/selftrain_ref.py says where each comes from): pred is byte for byte ops.head_upsample_argmax's and equals the fp64
argmax outside the near-tie margin; |log conf - log conf64| <= 1e-4; pseudo equals the reference outside the tie margin and the
1e-4 band round the threshold, at most 1 % of a case's pixels excluded; counts are EXACTLY the recount of the kernel's own pseudo;
pixel-weighted CE: loss 1e-4, sum of w_y 1e-5, gradient 2e-5 relative; identities 1e-6 or bitwise."""
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_argmax_ref as A  # noqa: E402
import selftrain_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = R.IGN
GRAD_KEYS = ("class_prototypes", "vision_decoder.layers.0.linear2.weight")
STEP_KEYS = GRAD_KEYS + ("pixel_patch.visual.weight", "vision_encoder.enc.embeddings.patch_embedding.weight",
                         "text_encoder.enc.embeddings.token_embedding.weight")


def _mode(ops, mode):
    return ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR


def _raw_conf(ops, lod, geom, thresh, pred=None, conf=None, pseudo=None, counts=None, ignore_index=IGN):
    """The C entry point on the caller's buffers (None = not written)."""
    from lc2is_amd import _lib
    B, h, w, C, S, md = geom
    nbytes = ops._fn("lc2is_head_upsample_conf_workspace_bytes")(B, h, w, C, S, md) if counts is not None else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=lod.device)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _lib.check(ops._fn("lc2is_head_upsample_conf")(lod.data_ptr(), lod.shape[1], ptr(pred), ptr(conf), ptr(pseudo), ptr(counts), B, h,
                                                   w, C, S, md, thresh, ignore_index, ws.data_ptr() if nbytes else None, nbytes,
                                                   torch.cuda.current_stream().cuda_stream), "conf")


# ---- 1. confidence, pseudo-labels and counts against fp64 ----
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_confidence_and_pseudo_labels_vs_fp64(dev, case):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    H, W = h * S, w * S
    lo, _, _ = R.case_inputs(*case)
    ref = R.conf_ref(*case)
    lod = lo.to(dev)
    geom = (B, h, w, C, S, _mode(ops, mode))
    thresh = ref["thresh"]
    pred, conf, pseudo, counts = ops.head_upsample_conf(lod, *geom, thresh=thresh, want_counts=True)
    assert pred.dtype == torch.uint8 and conf.dtype == torch.float32 and pseudo.dtype == torch.int64 and counts.dtype == torch.int32
    assert tuple(pred.shape) == tuple(conf.shape) == tuple(pseudo.shape) == (B, H, W) and tuple(counts.shape) == (B, 2)
    same, _ = ops.head_upsample_argmax(lod, None, *geom, want_counts=False)
    p, c, ps = pred.cpu().long(), conf.cpu().double(), pseudo.cpu()
    ex_tie, ex_all = R.excluded_share(ref["sure"]), R.excluded_share(ref["sure_t"])
    bad = int((p != ref["arg"])[ref["sure"]].sum())
    err = (c.log() - ref["conf"].log()).abs().max().item()
    bad_ps = int((ps != ref["pseudo"])[ref["sure_t"]].sum())
    print("selftrain figures conf", case, "thresh", thresh, "excluded", ex_tie, ex_all, "pred differ", bad, "log conf err", err,
          "pseudo differ", bad_ps, "pseudo differ inside the margins", int((ps != ref["pseudo"]).sum()) - bad_ps,
          "counts", counts.tolist())
    assert ex_tie <= ex_all <= R.MAX_EXCLUDED
    assert torch.equal(pred, same)                                   # every pixel: the bytes of head_upsample_argmax
    assert int(p.max()) < C and bad == 0
    assert bool((c > 0).all()) and bool((c <= 1).all()) and err <= R.CONF_TOL
    assert bad_ps == 0
    # pseudo is the kernel's own class where its own confidence passes the threshold; counts recount it
    kept = conf >= thresh
    assert torch.equal(pseudo, torch.where(kept, pred.long(), torch.full_like(pseudo, IGN)))
    assert torch.equal(counts[:, 0].long(), (pseudo != IGN).flatten(1).sum(1))
    assert bool((counts[:, 1] == H * W).all())
    assert 0 < int(counts[:, 0].sum()) < B * H * W                  # both sides of the threshold are populated
    # each output alone, in guarded buffers pre-filled with -1: the same bytes, every pixel written, nothing beyond
    n, G = B * H * W, 1024
    bufs = dict(pred=torch.full((n + 2 * G,), 255, dtype=torch.uint8, device=dev),
                conf=torch.full((n + 2 * G,), -1.0, dtype=torch.float32, device=dev),
                pseudo=torch.full((n + 2 * G,), -1, dtype=torch.int64, device=dev),
                counts=torch.full((2 * B + 2 * G,), -1, dtype=torch.int32, device=dev))
    want = dict(pred=pred, conf=conf, pseudo=pseudo, counts=counts)
    for name, buf in bufs.items():
        body = buf[G:G + want[name].numel()]
        _raw_conf(ops, lod, geom, thresh, **{name: body})
        assert torch.equal(body.view(want[name].shape), want[name]), name
        assert bool((buf[:G] == buf[0]).all()) and bool((buf[G + body.numel():] == buf[0]).all()) and float(buf[0]) in (255.0, -1.0), name
    # the wrapper's subsets, another ignore_index, and a second run
    assert torch.equal(ops.head_upsample_conf(lod, *geom, want_conf=False)[0], pred)
    none, conf1, none2, none3 = ops.head_upsample_conf(lod, *geom, want_pred=False)
    assert none is None and none2 is None and none3 is None and torch.equal(conf1, conf)
    out = ops.head_upsample_conf(lod, *geom, thresh=thresh, ignore_index=255, want_pred=False, want_conf=False)
    assert out[0] is None and out[1] is None and out[3] is None
    assert torch.equal(out[2], torch.where(kept, pred.long(), torch.full_like(pseudo, 255)))
    again = ops.head_upsample_conf(lod, *geom, thresh=thresh, want_counts=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (pred, conf, pseudo, counts)))


def test_confidence_sums_many_tiles_in_the_finish_launch(dev):
    """B = 3, 20 x 20 cells, S = 4: 36 tiles per image; the counts are the recount of the kernel's own pseudo."""
    from lc2is_amd import ops
    B, h, S, C = 3, 20, 4, 151
    g = torch.Generator().manual_seed(0)
    lo = torch.full((B * h * h, 192), A.PAD_SCORE)
    lo[:, :C] = torch.randn(B * h * h, C, generator=g)
    pred, conf, pseudo, counts = ops.head_upsample_conf(lo.to(dev), B, h, h, C, S, ops.INTERP_BICUBIC, thresh=0.1, want_counts=True)
    assert torch.equal(counts[:, 0].long(), (pseudo != IGN).flatten(1).sum(1)) and bool((counts[:, 1] == (h * S) ** 2).all())
    assert 0 < int(counts[:, 0].sum()) < B * (h * S) ** 2


# ---- 2. edges ----
@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[10], R.CASES[18]], ids=R.case_id)
def test_confidence_edges(dev, case):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    H, W = h * S, w * S
    lo, _, _ = R.case_inputs(*case)
    geom = (B, h, w, C, S, _mode(ops, mode))
    # thresh = 0 keeps every pixel
    pred, conf, pseudo, counts = ops.head_upsample_conf(lo.to(dev), *geom, thresh=0.0, want_counts=True)
    assert torch.equal(pseudo, pred.long()) and bool((counts[:, 0] == H * W).all())
    # thresh = 1 with one channel at +1e4 in the first image: its pixels are kept with conf == 1, class 3
    hot = lo.clone()
    hot[:h * w, 3] = 1e4
    pred, conf, pseudo, counts = ops.head_upsample_conf(hot.to(dev), *geom, thresh=1.0, want_counts=True)
    assert bool((conf[0] == 1.0).all()) and bool((pseudo[0] == 3).all()) and bool((pred[0] == 3).all())
    assert counts[0].tolist() == [H * W, H * W]
    if B > 1:
        assert torch.equal(counts[1:, 0].long(), (conf[1:] >= 1.0).flatten(1).sum(1)) and int(counts[1:, 0].sum()) < (B - 1) * H * W
    # scores of +-1e4, cells whose every channel is -inf, a NaN cell: conf finite in (0, 1], the class inside [0, C)
    g = torch.Generator().manual_seed(3)
    wild = lo.clone()
    wild[:, :C] = torch.where(torch.rand(lo.shape[0], C, generator=g) < 0.5, 1e4, -1e4)
    wild[::4] = float("-inf")
    wild[1, :C] = float("nan")
    pred, conf, pseudo, _ = ops.head_upsample_conf(wild.to(dev), *geom, thresh=0.5)
    assert bool(torch.isfinite(conf).all()) and bool((conf > 0).all()) and bool((conf <= 1).all()) and int(pred.max()) < C
    assert torch.equal(pseudo, torch.where(conf >= 0.5, pred.long(), torch.full_like(pseudo, IGN)))
    assert torch.equal(pred, ops.head_upsample_argmax(wild.to(dev), None, *geom, want_counts=False)[0])
    ninf = torch.full_like(lo, float("-inf"))
    pred, conf, _, _ = ops.head_upsample_conf(ninf.to(dev), *geom)
    assert not pred.any() and bool((conf == 1.0 / C).all())          # the documented value: class 0, conf = 1 / C


# ---- 3. cross-entropy with a per-pixel weight against fp64 ----
def _variant_dev(variant, C, dev, dyadic=False):
    weight, eps = R.variant_options(variant, C)
    if weight is not None and dyadic:
        weight = R.class_weights(C, dyadic=True)
    return weight, eps, None if weight is None else weight.float().to(dev)


@pytest.mark.parametrize("variant", R.CE_VARIANTS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_pixel_weighted_ce_vs_fp64(dev, case, variant):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, labels, pw = R.case_inputs(*case)
    weight, eps, wdev = _variant_dev(variant, C, dev)
    ref_loss, ref_wsum, ref_grad = R.ce_pw_ref(lo, labels, pw, B, h, w, C, S, mode, None if weight is None else weight.float(), eps)
    geom = (B, h, w, C, S, _mode(ops, mode))
    lod, lab, pwd = lo.to(dev), labels.to(dev), pw.to(dev)
    loss2, dlo = ops.head_upsample_ce_pw(lod, lab, pwd, *geom, want_grad=True, class_weight=wdev, label_smoothing=eps)
    assert loss2.dtype == torch.float32 and tuple(loss2.shape) == (2,) and tuple(dlo.shape) == tuple(lo.shape)
    e_loss = abs(loss2[0].item() - ref_loss.item()) / abs(ref_loss.item())
    e_wsum = abs(loss2[1].item() - ref_wsum.item()) / abs(ref_wsum.item())
    e_grad = R.rel(dlo[:, :C], ref_grad)
    pad = dlo[:, C:].abs().max().item() if dlo.shape[1] > C else 0.0
    print("selftrain figures ce_pw", case, variant, "loss", e_loss, "wsum", e_wsum, "grad", e_grad, "pad", pad)
    assert e_loss <= R.LOSS_TOL and e_wsum <= R.WSUM_TOL and e_grad <= R.GRAD_TOL
    assert pad == 0.0
    only, none = ops.head_upsample_ce_pw(lod, lab, pwd, *geom, class_weight=wdev, label_smoothing=eps)
    assert none is None and torch.equal(only, loss2)


# ---- 4. identities ----
@pytest.mark.parametrize("variant", R.CE_VARIANTS)
@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[7], R.CASES[9], R.CASES[15], R.CASES[18], R.CASES[23], R.CASES[27]], ids=R.case_id)
def test_pixel_weight_identities(dev, case, variant):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, labels, pw = R.case_inputs(*case)
    weight, eps, wdev = _variant_dev(variant, C, dev, dyadic=True)   # (weight sums exact in fp32: they are compared for equality)
    geom = (B, h, w, C, S, _mode(ops, mode))
    lod, lab = lo.to(dev), labels.to(dev)
    kw = dict(want_grad=True, class_weight=wdev, label_smoothing=eps)
    ones = torch.ones(labels.shape, device=dev)
    l1, d1 = ops.head_upsample_ce_pw(lod, lab, ones, *geom, **kw)
    # pw == 1 is the existing loss
    l0, d0, _ = ops.head_upsample_ce(lod, lab, *geom, **kw)
    e_loss, e_grad = abs(l1[0].item() - l0[0].item()) / abs(l0[0].item()), R.rel(d1, d0)
    # pw == 1/2 is exactly half (a power of two)
    lh, dh = ops.head_upsample_ce_pw(lod, lab, 0.5 * ones, *geom, **kw)
    # pw == 0 on a set of pixels against ignore_index on the same set
    drop = torch.rand(labels.shape, generator=torch.Generator().manual_seed(9)) < 0.3
    la, da = ops.head_upsample_ce_pw(lod, lab, (~drop).float().to(dev), *geom, **kw)
    lb, db = ops.head_upsample_ce_pw(lod, torch.where(drop, IGN, labels).to(dev), ones, *geom, **kw)
    wc = torch.ones(C, dtype=torch.float64) if weight is None else weight
    set_wsum = wc[labels.clamp(0, C - 1)][drop & R.counted(labels, C)].sum().item()
    e_loss0, e_grad0 = abs(la[0].item() - lb[0].item()) / abs(lb[0].item()), R.rel(da, db)
    print("selftrain figures identities", case, variant, "vs head_upsample_ce", e_loss, e_grad, "counts", l1[1].item(), l0[1].item(),
          "pw 0 vs ignore", e_loss0, e_grad0, "counts", la[1].item(), lb[1].item(), "set", set_wsum)
    assert e_loss <= 1e-6 and e_grad <= 1e-6 and l1[1].item() == l0[1].item()
    assert torch.equal(2.0 * lh[0], l1[0]) and torch.equal(lh[1], l1[1]) and torch.equal(2.0 * dh, d1)
    assert e_loss0 <= 1e-6 and e_grad0 <= 1e-6
    assert set_wsum > 0 and la[1].item() == l1[1].item() and la[1].item() - lb[1].item() == set_wsum
    # two runs give the same bytes
    pwd = pw.to(dev)
    r1, r2 = ops.head_upsample_ce_pw(lod, lab, pwd, *geom, **kw), ops.head_upsample_ce_pw(lod, lab, pwd, *geom, **kw)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


# ---- 5. the model layer, on the tiny golden model (K = 151) ----
def _tiny(dev):
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


def _batch(dev, seed, fx=None):
    """(inputs, labels, pixel_weight): the fixture's inputs or random ones; three rows IGN, some labels >= K; weights in [0, 2], a
    fifth exactly 0."""
    g = torch.Generator().manual_seed(seed)
    if fx is not None:
        inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    else:
        ids = torch.randint(1, 500, (2, 8), generator=g)
        ids[:, 0], ids[:, -1] = 510, 511
        inputs = {"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
                  "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    n = inputs["pixel_values"].shape[0]
    labels = torch.randint(0, 151, (n, 16, 16), generator=g)
    labels[:, seed % 5:seed % 5 + 3] = IGN
    pw = 2.0 * torch.rand(n, 16, 16, generator=g)
    pw[torch.rand(n, 16, 16, generator=g) < 0.2] = 0.0
    return inputs, labels.to(dev), pw.to(dev)


def _ref_loss(logits, labels, pw, weight=None, eps=0.0, reduction="mean"):
    """(F.cross_entropy(reduction='none') * pw).sum() / sum of w_y over the counted pixels, in fp64 on the materialised logits."""
    K = logits.shape[1]
    wd = None if weight is None else weight.double()
    li = F.cross_entropy(logits.double(), labels, weight=wd, ignore_index=IGN, reduction="none", label_smoothing=eps)
    total = (li * pw.double()).sum()
    if reduction == "sum":
        return total
    ok = labels != IGN
    wy = torch.ones_like(li) if wd is None else wd[labels.clamp(0, K - 1)]
    return total / wy[ok].sum()


def _check_conf_against_logits(out, logits, thresh):
    pred, conf, pseudo, counts = out
    prob, arg = logits.double().softmax(1).max(1)
    top2 = logits.double().topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > A.MARGIN * logits.abs().max().item()
    sure_t = sure & ((prob.log() - math.log(thresh)).abs() > R.CONF_TOL)
    err = (conf.double().log() - prob.log()).abs().max().item()
    want = torch.where(prob >= thresh, arg, torch.full_like(arg, IGN))
    bad, bad_ps = int((pred.long() != arg)[sure].sum()), int((pseudo != want)[sure_t].sum())
    print("selftrain figures predict_confidence: excluded", R.excluded_share(sure), R.excluded_share(sure_t), "pred differ", bad,
          "log conf err", err, "pseudo differ", bad_ps, "counts", counts.tolist())
    assert R.excluded_share(sure_t) <= R.MAX_EXCLUDED and bad == 0 and bad_ps == 0 and err <= R.CONF_TOL
    assert torch.equal(counts[:, 0].long(), (pseudo != IGN).flatten(1).sum(1))
    assert bool((counts[:, 1] == pred.shape[1] * pred.shape[2]).all())
    assert not any(t.requires_grad for t in out)


@pytest.mark.parametrize("variant,reduction", [("plain", "mean"), ("smooth", "mean"), ("weighted", "sum")])
def test_forward_loss_pixel_weight_matches_materialised_logits(dev, variant, reduction):
    m, fx = _tiny(dev)
    inputs, labels, pw = _batch(dev, 3, fx)
    weight, eps, wdev = _variant_dev(variant, 151, dev)
    loss_u = _ref_loss(m(inputs)["outputs"], labels, pw, wdev, eps, reduction)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    counts = torch.zeros(3, 151, dtype=torch.int64, device=dev)
    loss_f = m.forward_loss(inputs, labels, weight=wdev, label_smoothing=eps, reduction=reduction, pixel_weight=pw, seg_counts=counts)
    loss_f.backward()
    named = dict(m.named_parameters())
    rels = {k: R.rel(named[k].grad, g_u[k]) for k in GRAD_KEYS}
    print("selftrain figures forward_loss", variant, reduction, loss_f.item(), loss_u.item(), rels)
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert all(bool(g.any()) for g in g_u.values()) and all(r <= 1e-3 for r in rels.values()), rels
    # the seg counts ignore the pixel weights; an all-ones weight is the call without one
    plain = torch.zeros_like(counts)
    with torch.no_grad():
        l0 = m.forward_loss(inputs, labels, weight=wdev, label_smoothing=eps, reduction=reduction, seg_counts=plain)
        l1 = m.forward_loss(inputs, labels, weight=wdev, label_smoothing=eps, reduction=reduction, pixel_weight=torch.ones_like(pw))
    assert torch.equal(counts, plain) and int(counts[2].sum()) == int((labels != IGN).sum())
    assert abs(l1.item() - l0.item()) <= 1e-6 * abs(l0.item())


def test_predict_confidence_matches_materialised_logits(dev):
    m, fx = _tiny(dev)
    inputs, _, _ = _batch(dev, 3, fx)
    with torch.no_grad():
        logits = m(inputs)["outputs"]
    thresh = float(logits.double().softmax(1).max(1).values.flatten().median().float())
    pred, conf = m.predict_confidence(inputs)
    assert torch.equal(pred, m.predict(inputs)) and conf.dtype == torch.float32
    out = m.predict_confidence(inputs, thresh)
    assert torch.equal(out[0], pred) and torch.equal(out[1], conf)
    _check_conf_against_logits(out, logits, thresh)
    assert 0 < int(out[3][:, 0].sum()) < pred.numel()


def test_score_map_tail_pixel_weight_and_confidence(dev):
    import lc2is_amd.nn as N
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    pw = 2.0 * torch.rand(labels.shape, generator=g)
    pw[torch.rand(labels.shape, generator=g) < 0.2] = 0.0
    labels, pw = labels.to(dev), pw.to(dev)
    tail = N.ScoreMapTail(4)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_u = _ref_loss(tail(v1, t1), labels, pw)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, pixel_weight=pw)
    loss_f.backward()
    print("selftrain figures score tail", loss_f.item(), loss_u.item(), R.rel(v2.grad, v1.grad), R.rel(t2.grad, t1.grad))
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert R.rel(v2.grad, v1.grad) <= 1e-3 and R.rel(t2.grad, t1.grad) <= 1e-3
    with torch.no_grad():
        logits = tail(ve, te)
    thresh = float(logits.double().softmax(1).max(1).values.flatten().median().float())
    out = tail.predict_confidence(ve, te, thresh)
    assert torch.equal(out[0], tail.predict(ve, te))
    _check_conf_against_logits(out, logits, thresh)


# ---- 6. TrainStep ----
def test_train_step_with_pixel_weight(dev):
    """One SGD step with a pixel weight moves the parameters as the reference composition on the materialised logits does."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    lr = 1e-2
    m1, fx = _tiny(dev)
    m2, _ = _tiny(dev)
    inputs, labels, pw = _batch(dev, 3, fx)
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    loss_ts = TrainStep(m1, optimizer="sgd", lr=lr).step(inputs, labels, pw)
    loss_h = _ref_loss(m2(inputs)["outputs"], labels, pw)
    loss_h.backward()
    named1, named2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    rels = {k: R.rel(named1[k].detach() - start[k], -lr * named2[k].grad) for k in STEP_KEYS}
    print("selftrain figures train step", loss_ts.item(), loss_h.item(), rels)
    assert abs(loss_ts.item() - loss_h.item()) <= 1e-4 * abs(loss_h.item())
    assert all(r < 8e-2 for r in rels.values()), rels
    # refused with a criterion it does not combine with, before anything runs
    for crit in (N.OhemCrossEntropyLoss(0.7, 16), N.DiceCrossEntropyLoss(), N.FocalLoss(), N.SigmoidFocalLoss()):
        ts = TrainStep(_tiny(dev)[0], optimizer="sgd", lr=lr, criterion=crit)
        with pytest.raises(ValueError, match="pixel_weight"):
            ts.step(inputs, labels, pw)
        with pytest.raises(ValueError, match="pixel_weight"):
            ts.capture(inputs, labels, pixel_weight=pw)


def test_captured_step_with_pixel_weight_replays_bitwise(dev):
    """A step captured with a pixel weight, replayed on another batch and another weight, is bitwise the eager step; seg_metrics
    rides along."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(3)]
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    mk = lambda m: TrainStep(m, optimizer="sgd", lr=1e-3, criterion=N.CrossEntropyLoss(label_smoothing=0.1), seg_metrics=True)   # noqa: E731
    ts_e, ts_g = mk(m_e), mk(m_g)
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(batches[0][0], batches[0][1], pixel_weight=batches[0][2])
    torch.cuda.synchronize()
    for b in batches[1:]:
        assert torch.equal(ts_e.step(*b).clone(), run(*b).clone())
    torch.cuda.synchronize()
    assert torch.equal(ts_e.arena.flat, ts_g.arena.flat) and torch.equal(ts_e.seg_counts, ts_g.seg_counts)
    assert torch.equal(run.static_pixel_weight, batches[2][2])
    with pytest.raises(ValueError, match="pixel weight"):
        run(batches[1][0], batches[1][1])
    run.release()


def test_accumulate_two_weighted_micro_batches_equal_one_step(dev):
    """accumulate=2 over two weighted B = 1 micro-batches (one with most rows ignored) against one weighted step on the B = 2 batch:
    parameter changes within relative L2 8e-2, loss within 2e-2 (tests/test_gpu_accum.py); the count is the unweighted one."""
    from lc2is_amd.step import TrainStep
    lr = 0.05
    inputs, labels, pw = _batch(dev, 41)
    labels[0, :12] = IGN
    m_a, _ = _tiny(dev)
    m_b, _ = _tiny(dev)
    start = {k: p.detach().clone() for k, p in m_a.named_parameters() if k in STEP_KEYS}
    ts_a = TrainStep(m_a, optimizer="sgd", lr=lr, accumulate=2)
    ts_b = TrainStep(m_b, optimizer="sgd", lr=lr)
    for i in range(2):
        ts_a.step({k: v[i:i + 1] for k, v in inputs.items()}, labels[i:i + 1], pw[i:i + 1].contiguous())
    loss_b = ts_b.step(inputs, labels, pw)
    na, nb = dict(m_a.named_parameters()), dict(m_b.named_parameters())
    rels = {k: R.rel(na[k].detach() - start[k], nb[k].detach() - start[k]) for k in STEP_KEYS}
    err = abs(ts_a.accum_loss.item() - loss_b.item())
    print("selftrain figures accumulate", rels, err, ts_a.accum_count.item())
    assert all(r <= 8e-2 for r in rels.values()), rels
    assert err <= 2e-2
    assert ts_a.accum_count.item() == float((labels != IGN).sum())


# ---- 7. one self-training cycle ----
def test_one_self_training_cycle(dev):
    from lc2is_amd.selftrain import PseudoLabeler
    from lc2is_amd.step import TrainStep
    m, fx = _tiny(dev)
    inputs, labels, _ = _batch(dev, 3, fx)
    weak, _, _ = _batch(dev, 11)
    step = TrainStep(m, optimizer="sgd", lr=1e-2, ema_decay=0.99)
    for _ in range(2):
        step.step(inputs, labels)
    student = step.arena.flat.clone()
    with step.ema_weights():
        assert not torch.equal(step.arena.flat, student)             # the teacher's weights
        with torch.no_grad():
            logits = m(weak)["outputs"]
        thresh = float(logits.double().softmax(1).max(1).values.flatten().median().float())
        labeler = PseudoLabeler(m, threshold=thresh, weight="quality")
        labels_u, pw_u, counts = labeler(weak)
        conf_w = PseudoLabeler(m, threshold=thresh, weight="confidence")(weak)
        out = m.predict_confidence(weak, thresh)
    assert torch.equal(step.arena.flat, student)                     # leaving the block restores the student bitwise
    _check_conf_against_logits((out[0], out[1], labels_u, counts), logits, thresh)
    assert labels_u.dtype == torch.int64 and torch.equal(labels_u, out[2]) and torch.equal(counts, out[3])
    share = counts[:, 0].float() / counts[:, 1].float()
    assert pw_u.dtype == torch.float32 and pw_u.is_contiguous() and torch.equal(pw_u, share.view(-1, 1, 1).expand_as(pw_u))
    assert 0.0 < share.min().item() and share.max().item() < 1.0
    assert torch.equal(conf_w[0], labels_u) and torch.equal(conf_w[1], torch.where(labels_u != IGN, out[1], torch.zeros_like(out[1])))
    batch = labeler.combine(labelled=(inputs, labels), pseudo=(weak, labels_u, pw_u))
    assert batch[1].shape[0] == labels.shape[0] + labels_u.shape[0] and bool((batch[2][:labels.shape[0]] == 1).all())
    loss = step.step(*batch)
    assert bool(torch.isfinite(loss)) and not torch.equal(step.arena.flat, student)
    # the labeler makes no host read: it captures into a graph (student weights), and the replay gives the eager call's tensors
    m.overlap_text = False
    eager = labeler(weak)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        labeler(weak)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = labeler(weak)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    del graph
