"""Focal / poly-1 cross-entropy on the HIP path against the fp64 reference of tests/focal_ref.py: the fused upsample + loss head
(op, saturated pixels, the (0, 0) case against the weighted CE head, bitwise repeat), the NCHW kernels and the FocalLoss module,
and the models and the train step (eager, captured, accumulated, beside the metric counts and the hard-pixel selection).

Bounds are the project's own for this head (tests/test_gpu_ce_options.py): loss 1e-4 relative, weighted count 1e-5 relative,
gradient relative L2 2e-5, padding columns exactly 0; 1e-5 for the NCHW kernels; 1e-5 / 1e-3 for a model against its own
materialised logits (tests/test_gpu_dice.py, tests/test_gpu_ohem.py); 8e-2 / 2e-2 for parameter changes and the loss of a step
(tests/test_gpu_accum.py).  Every measured figure is printed before it is asserted."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import focal_ref as R  # noqa: E402

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


# ---- 1. the op against fp64 ----
@pytest.mark.parametrize("gamma,eps", R.PARAMS)
@pytest.mark.parametrize("case", range(len(R.CASES)), ids=["-".join(map(str, c)) for c in R.CASES])
def test_head_upsample_focal_vs_fp64(dev, case, gamma, eps):
    from lc2is_amd import ops
    mode, S, C, h, w = R.CASES[case]
    B = 2
    lo, labels, w64, (ref_loss, ref_wsum, ref_grad) = R.case_ref(case, gamma, eps)
    loss, dlo = ops.head_upsample_focal(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode), want_grad=True,
                                        class_weight=w64.float().to(dev), gamma=gamma, poly_eps=eps)
    fig = dict(loss=abs(loss[0].item() - ref_loss) / abs(ref_loss), wsum=abs(loss[1].item() - ref_wsum) / ref_wsum,
               grad=_rel(dlo[:, :C], ref_grad), pad=dlo[:, C:].abs().sum().item())
    print("focal figures op", R.CASES[case], (gamma, eps), fig)
    assert bool(torch.isfinite(dlo).all())
    assert fig["loss"] <= 1e-4 and fig["wsum"] <= 1e-5 and fig["grad"] <= 2e-5 and fig["pad"] == 0
    # a loss-only call (no gradient slabs in the workspace) gives the same two sums
    loss0, none = ops.head_upsample_focal(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode),
                                          class_weight=w64.float().to(dev), gamma=gamma, poly_eps=eps)
    assert none is None and torch.equal(loss0, loss)


def test_grad_scale_and_ignore_index(dev):
    from lc2is_amd import ops
    mode, S, C, h, w = R.CASES[0]
    lo, labels, _ = R.head_case(2, h, w, C, S, 3)
    lo, labels = lo.to(dev), labels.to(dev)
    l1, d1 = ops.head_upsample_focal(lo, labels, 2, h, w, C, S, want_grad=True, gamma=1.5, poly_eps=2.0)
    l2, d2 = ops.head_upsample_focal(lo, labels, 2, h, w, C, S, want_grad=True, gamma=1.5, poly_eps=2.0, grad_scale=0.25)
    assert torch.equal(l1, l2) and torch.equal(d2, d1 * 0.25)                 # a power of two: exact
    assert l1[1].item() == float(((labels != IGN) & (labels < C)).sum())      # no weights: the count of the CE head
    l3, _ = ops.head_upsample_focal(lo, labels, 2, h, w, C, S, gamma=1.5, poly_eps=2.0, ignore_index=0)
    assert l3[1].item() == float(((labels != 0) & (labels >= 0) & (labels < C)).sum())


# ---- 2. saturated pixels ----
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("eps", [0.0, 1.0])
def test_saturated_pixels(dev, gamma, eps):
    """q underflows to exactly 0 on the upper half (the label leads by 120) and p is 0 on the lower half (the label trails by
    120): loss and gradient are finite and match fp64 to the bounds of the op test."""
    from lc2is_amd import ops
    s = R.SAT
    lo, labels = R.saturated_case()
    w64 = R.weights(s["C"], 1)
    ref_loss, ref_wsum, ref_grad = R.head_loss(lo, labels, s["B"], s["h"], s["w"], s["C"], s["S"], s["mode"], gamma, eps, w64)
    loss, dlo = ops.head_upsample_focal(lo.to(dev), labels.to(dev), s["B"], s["h"], s["w"], s["C"], s["S"], _mode(ops, s["mode"]),
                                        want_grad=True, class_weight=w64.float().to(dev), gamma=gamma, poly_eps=eps)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dlo).all())
    fig = dict(loss=abs(loss[0].item() - ref_loss) / abs(ref_loss), wsum=abs(loss[1].item() - ref_wsum) / ref_wsum,
               grad=_rel(dlo[:, :s["C"]], ref_grad), pad=dlo[:, s["C"]:].abs().sum().item())
    print("focal figures saturated", (gamma, eps), fig, ref_loss)
    assert fig["loss"] <= 1e-4 and fig["wsum"] <= 1e-5 and fig["grad"] <= 2e-5 and fig["pad"] == 0
    # the upper half alone (every label leads by 120): the loss and every gradient element are exactly what q == 0 gives
    top = labels.clone()
    top[:, s["h"] * s["S"] // 2 - 4:] = IGN
    lt, dt = ops.head_upsample_focal(lo.to(dev), top.to(dev), s["B"], s["h"], s["w"], s["C"], s["S"], _mode(ops, s["mode"]),
                                     want_grad=True, class_weight=w64.float().to(dev), gamma=gamma, poly_eps=eps)
    assert lt[0].item() == 0.0 and lt[1].item() > 0 and not dt.any()


# ---- 3. (gamma, eps) = (0, 0) is the weighted CE head ----
@pytest.mark.parametrize("mode,S,C", [("bicubic", 4, 151), ("bilinear", 8, 150), ("bicubic", 16, 37)])
def test_gamma_0_eps_0_matches_the_weighted_ce_head(dev, mode, S, C):
    from lc2is_amd import ops
    B, h = 2, 8
    lo, labels, _ = R.head_case(B, h, h, C, S, 9)
    lo, labels = lo.to(dev), labels.to(dev)
    cw = R.weights(C, 2).float().to(dev)
    m = _mode(ops, mode)
    l0, d0, _ = ops.head_upsample_ce(lo, labels, B, h, h, C, S, m, want_grad=True, grad_scale=0.25, class_weight=cw)
    l1, d1 = ops.head_upsample_focal(lo, labels, B, h, h, C, S, m, want_grad=True, grad_scale=0.25, class_weight=cw, gamma=0.0,
                                     poly_eps=0.0)
    print("focal figures (0,0) vs CE", (mode, S, C), abs(l1[0].item() - l0[0].item()) / abs(l0[0].item()), _rel(d1, d0))
    assert abs(l1[0].item() - l0[0].item()) <= 1e-6 * abs(l0[0].item())
    assert l1[1].item() == l0[1].item()
    assert _rel(d1, d0) <= 1e-6


# ---- 4. bitwise reproducible ----
@pytest.mark.parametrize("mode,S", [("bicubic", 4), ("bilinear", 16)])
def test_bitwise_reproducible(dev, mode, S):
    from lc2is_amd import ops
    B, h, C = 3, 16, 151
    lo, labels, _ = R.head_case(B, h, h, C, S, 5)
    lo, labels = lo.to(dev), labels.to(dev)
    cw = R.weights(C, 1).float().to(dev)
    m = _mode(ops, mode)
    a = ops.head_upsample_focal(lo, labels, B, h, h, C, S, m, want_grad=True, class_weight=cw, gamma=2.0, poly_eps=1.0)
    b = ops.head_upsample_focal(lo, labels, B, h, h, C, S, m, want_grad=True, class_weight=cw, gamma=2.0, poly_eps=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[1].any())


# ---- 5. the NCHW kernels and the module ----
def _nchw_case(shape=(2, 151, 24, 20), over=0):
    """Labels from [0, C + over): those >= C are not counted."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g) * 2
    labels = torch.randint(0, C + over, (B, H, W), generator=g)
    labels[:, ::4] = IGN
    gpx = torch.rand(B, H, W, generator=g, dtype=torch.float64) + 0.5   # non-uniform upstream gradient
    return x, labels, gpx


@pytest.mark.parametrize("gamma,eps", R.PARAMS)
def test_focal_nchw_kernels_vs_fp64(dev, gamma, eps):
    _focal_nchw_vs_fp64(dev, _nchw_case(), gamma, eps)


def test_focal_nchw_past_the_grid_cap(dev):
    """2 099 601 pixels: more than 8192 blocks of 256, and no multiple of 256 or 64 — the strided walk of the forward and of the
    backward.  The count to the 1e-6 of test_ce_nchw_fwd_sums_are_ordered at this size."""
    _focal_nchw_vs_fp64(dev, _nchw_case((1, 2, 1449, 1449), over=2), 1.5, 2, wsum_tol=1e-6)


@pytest.mark.parametrize("gamma,eps", [(2, 0), (0, 1)])
def test_focal_nchw_one_class(dev, gamma, eps):
    """C = 1: p = 1 and q = 0, so every loss and every gradient is 0 in exact arithmetic and a relative error has no meaning (the
    fp64 reference forms 0 * inf).  The bound is the 1e-5 of the NCHW tests relative to the size of the factors: w for a loss, w g
    for a gradient.  lse and the weighted count as usual."""
    from lc2is_amd import ops
    x, labels, gpx = _nchw_case((1, 1, 5, 7), over=2)
    valid = labels == 0
    w = R.weights(1, 2)[0].item()
    kw = dict(class_weight=R.weights(1, 2).float().to(dev), gamma=gamma, poly_eps=eps)
    xd, ld = x.to(dev), labels.to(dev)
    loss2, lse, lpx = ops.focal_nchw_fwd(xd, ld, IGN, per_pixel=True, **kw)
    assert _rel(lse, x[:, 0]) <= 1e-5 and abs(loss2[1].item() - w * int(valid.sum())) <= 1e-5 * w * int(valid.sum())
    assert lpx.abs().max().item() <= 1e-5 * w and abs(loss2[0].item()) <= 1e-5 * w * int(valid.sum())
    for d, gmax in ((ops.focal_nchw_bwd(xd, ld, lse, None, 1.0, IGN, grad_px=gpx.float().to(dev), **kw), gpx.max().item()),
                    (ops.focal_nchw_bwd(xd, ld, lse, torch.full((1,), 0.25, device=dev), 2.0, IGN, **kw), 0.5)):
        assert d.abs().max().item() <= 1e-5 * w * gmax and not d.cpu()[:, 0][~valid].any()


def _focal_nchw_vs_fp64(dev, case, gamma, eps, wsum_tol=1e-5):
    from lc2is_amd import ops
    x, labels, gpx = case
    w64 = R.weights(x.shape[1], 2)
    kw = dict(class_weight=w64.float().to(dev), gamma=gamma, poly_eps=eps)
    xd, ld = x.to(dev), labels.to(dev)
    loss2, lse, lpx = ops.focal_nchw_fwd(xd, ld, IGN, per_pixel=True, **kw)
    x64 = x.double().requires_grad_(True)
    ref, wy = R.loss_px(x64, labels, gamma, eps, w64)
    fig = dict(px=_rel(lpx, ref.detach()), loss=abs(loss2[0].item() - ref.sum().item()) / abs(ref.sum().item()),
               wsum=abs(loss2[1].item() - wy.sum().item()) / wy.sum().item(),
               lse=_rel(lse, torch.logsumexp(x.double(), 1)))
    ref.backward(gpx)
    d = ops.focal_nchw_bwd(xd, ld, lse, None, 1.0, IGN, grad_px=gpx.float().to(dev), **kw)
    fig["grad_px"] = _rel(d, x64.grad)
    x64.grad = None
    R.loss_px(x64, labels, gamma, eps, w64)[0].sum().backward(torch.tensor(0.5, dtype=torch.float64))
    d2 = ops.focal_nchw_bwd(xd, ld, lse, torch.full((1,), 0.25, device=dev), 2.0, IGN, **kw)   # device scalar times host scalar
    fig["grad_scalar"] = _rel(d2, x64.grad)
    print("focal figures nchw", (gamma, eps), fig)
    assert all(v <= 1e-5 for v in fig.values()) and fig["wsum"] <= wsum_tol, fig
    loss2b, _ = ops.focal_nchw_fwd(xd, ld, IGN, **kw)
    assert torch.equal(loss2b, loss2)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("poly1", [False, True])
def test_focal_loss_module(dev, reduction, poly1):
    import lc2is_amd.nn as N
    x, labels, gpx = _nchw_case()
    w64 = R.weights(151, 4)
    if poly1:
        crit, (gamma, eps) = N.Poly1CrossEntropyLoss(2.0, weight=w64.float(), reduction=reduction).to(dev), (0.0, 2.0)
    else:
        crit, (gamma, eps) = N.FocalLoss(2.0, 0.5, weight=w64.float(), reduction=reduction).to(dev), (2.0, 0.5)
    xd = x.to(dev).requires_grad_(True)
    loss = crit(xd, labels.to(dev))
    x64 = x.double().requires_grad_(True)
    ref = R.reduce(*R.loss_px(x64, labels, gamma, eps, w64), reduction)
    assert loss.shape == ref.shape
    up = gpx if reduction == "none" else torch.tensor(1.5, dtype=torch.float64)
    loss.backward(up.float().to(dev))
    ref.backward(up)
    print("focal figures module", reduction, poly1, _rel(loss.detach(), ref.detach()), _rel(xd.grad, x64.grad))
    assert _rel(loss.detach(), ref.detach()) <= 1e-5 and _rel(xd.grad, x64.grad) <= 1e-5


def test_focal_loss_module_mean_is_the_pixel_mean_without_weights_and_ignored_pixels(dev):
    """'mean' divides by the sum of w_y: with no weights and no ignored pixel that is kornia's / MONAI's mean over the pixels."""
    import lc2is_amd.nn as N
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 19, 8, 8, generator=g)
    labels = torch.randint(0, 19, (2, 8, 8), generator=g)
    loss = N.FocalLoss(2.0)(x.to(dev), labels.to(dev))
    ref = R.loss_px(x.double(), labels, 2.0, 0.0)[0].mean()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())


# ---- 6. models and the step ----
def _tiny(dev):
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


def _ref_loss(logits, labels, focal, weight, reduction="mean"):
    """The reference composition on materialised logits, fp64 on the device."""
    return R.reduce(*R.loss_px(logits.double(), labels, focal[0], focal[1], None if weight is None else weight.double()), reduction)


@pytest.mark.parametrize("focal,reduction", [((2.0, 0.0), "mean"), ((0.5, 1.0), "sum")])
def test_forward_loss_focal_matches_materialised_logits(dev, focal, reduction):
    m, fx = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev).clone()
    labels[:, :3] = IGN
    w = R.weights(151, 12).float().to(dev)
    loss_u = _ref_loss(m(inputs)["outputs"], labels, focal, w, reduction)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    loss_f = m.forward_loss(inputs, labels, weight=w, reduction=reduction, focal=focal)
    loss_f.backward()
    named = dict(m.named_parameters())
    rels = {k: _rel(named[k].grad, g_u[k]) for k in GRAD_KEYS}
    print("focal figures forward_loss", focal, reduction, loss_f.item(), loss_u.item(), rels)
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert all(r <= 1e-3 for r in rels.values()), rels


def test_forward_loss_focal_beside_seg_counts_and_ohem(dev):
    """seg_counts= leaves the loss's bytes alone; under ohem= the selection is the plain-CE one and the loss is the focal loss of
    the relabelled call, bit for bit."""
    m, fx = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev)
    w = R.weights(151, 12).float().to(dev)
    f = (2.0, 0.0)
    with torch.no_grad():
        plain = m.forward_loss(inputs, labels, weight=w, focal=f)
        counts = torch.zeros(3, 151, dtype=torch.int64, device=dev)
        with_counts = m.forward_loss(inputs, labels, weight=w, focal=f, seg_counts=counts)
        assert torch.equal(plain, with_counts) and int(counts[2].sum()) == int(((labels >= 0) & (labels < 151)).sum())
        ohem = (1e-6, 100)   # the threshold never binds on this untrained model: the 100 hardest pixels per image by plain CE
        m.forward_loss(inputs, labels, ohem=ohem)
        kept_ce = m.last_ohem[0].clone()
        hard = m.forward_loss(inputs, labels, weight=w, focal=f, ohem=ohem)
        kept = m.last_ohem[0]
        assert torch.equal(kept, kept_ce) and 0 < int((kept != IGN).sum()) < labels.numel()
        assert torch.equal(hard, m.forward_loss(inputs, kept, weight=w, focal=f)) and not torch.equal(hard, plain)


def test_score_map_tail_focal_matches_materialised_logits(dev):
    import lc2is_amd.nn as N
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    w = R.weights(K, 13).float().to(dev)
    f = (1.5, 2.0)
    tail = N.ScoreMapTail(4)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_u = _ref_loss(tail(v1, t1), labels, f, w)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, weight=w, focal=f)
    loss_f.backward()
    print("focal figures score tail", loss_f.item(), loss_u.item(), _rel(v2.grad, v1.grad), _rel(t2.grad, t1.grad))
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert _rel(v2.grad, v1.grad) <= 1e-3 and _rel(t2.grad, t1.grad) <= 1e-3
    v3, t3 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    assert torch.equal(tail.loss(v3, t3, labels, weight=w, focal=f), loss_f)


def test_prompt_ftn_forward_loss_focal_matches_materialised_logits(dev):
    """The compose model of tests/test_gpu_compose.py (its golden weights and 512 x 512 input): forward_loss(focal=) against the
    reference composition on the score map the same model materialises."""
    import lc2is_amd.nn as N
    from golden_util import make_weights, prompt_ftn_inputs
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "prompt_ftn.pt", weights_only=True)
    m = N.PromptFTN(swin_arch=N.SwinArch(32, (1, 1, 1, 1), (1, 2, 4, 8), 7, drop_path_rate=0.0),
                    text_arch=N.ClipArch(512, 8, 1, 128, vocab=512, max_pos=16, eos_token_id=511), prompt_layers=2, dropout=0.0)
    m.load_state_dict(make_weights({k: v.tolist() for k, v in fx["shapes"].items()}, int(fx["wseed"])), strict=True)
    m = m.to(dev).train()
    inputs, labels = prompt_ftn_inputs(int(fx["iseed"]))
    inputs, labels = {k: v.to(dev) for k, v in inputs.items()}, labels.to(dev)
    w = R.weights(6, 17).float().to(dev)   # (the fixture's six classes: the score map is [1, 6, 512, 512])
    f = (2.0, 1.0)
    with torch.no_grad():
        loss_u = _ref_loss(m(inputs)[1], labels, f, w, "sum")
        loss_f = m.forward_loss(inputs, labels, weight=w, reduction="sum", focal=f)
    print("focal figures prompt_ftn", loss_f.item(), loss_u.item())
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())


def test_train_step_with_focal_criterion(dev):
    """One SGD step of TrainStep(criterion=FocalLoss(2.0, weight=w)) moves the parameters as the reference composition on the
    materialised logits plus -lr * gradient does; seg_metrics=True leaves the step's bytes alone."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    lr = 1e-2
    m1, fx = _tiny(dev)
    m2, _ = _tiny(dev)
    m3, _ = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev)
    w = R.weights(151, 14).float()
    crit = N.FocalLoss(2.0, weight=w).to(dev)
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    loss_ts = TrainStep(m1, optimizer="sgd", lr=lr, criterion=crit).step(inputs, labels)
    loss_h = _ref_loss(m2(inputs)["outputs"], labels, crit.focal, w.to(dev))
    loss_h.backward()
    named1, named2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    rels = {k: _rel(named1[k].detach() - start[k], -lr * named2[k].grad) for k in STEP_KEYS}
    print("focal figures train step", loss_ts.item(), loss_h.item(), rels)
    assert abs(loss_ts.item() - loss_h.item()) <= 1e-4 * abs(loss_h.item())
    assert all(r < 8e-2 for r in rels.values()), rels
    ts3 = TrainStep(m3, optimizer="sgd", lr=lr, criterion=N.FocalLoss(2.0, weight=w).to(dev), seg_metrics=True)
    assert torch.equal(ts3.step(inputs, labels), loss_ts)
    named3 = dict(m3.named_parameters())
    assert all(torch.equal(named1[k], named3[k]) for k in named1), "seg_metrics=True changed the step"
    assert int(ts3.seg_counts[2].sum()) == int(((labels >= 0) & (labels < 151)).sum())


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
             "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)},
            torch.randint(0, 151, (2, 16, 16), generator=g).to(dev))


def test_captured_step_with_focal_criterion(dev):
    """A captured step replayed on different batches gives bitwise the losses and parameters of the eager steps."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(3)]
    w = R.weights(151, 15).float()
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    ts_e = TrainStep(m_e, optimizer="sgd", lr=1e-3, criterion=N.FocalLoss(2.0, 1.0, weight=w).to(dev))
    ts_g = TrainStep(m_g, optimizer="sgd", lr=1e-3, criterion=N.FocalLoss(2.0, 1.0, weight=w).to(dev))
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(*batches[0])
    torch.cuda.synchronize()
    for inp, lab in batches[1:]:
        assert torch.equal(ts_e.step(inp, lab).clone(), run(inp, lab).clone())
    torch.cuda.synchronize()
    assert torch.equal(ts_e.arena.flat, ts_g.arena.flat)
    run.release()


def test_accumulate_two_micro_batches_equal_one_step(dev):
    """accumulate=2 over two B = 1 micro-batches (one with most rows ignored: the micro-batch means differ from the batch mean)
    against one step on the B = 2 batch: parameter changes within relative L2 8e-2, loss within 2e-2 (tests/test_gpu_accum.py)."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    lr = 0.05
    inputs, labels = _batch(dev, 41)
    labels[0, :12] = IGN
    w = R.weights(151, 16).float()
    m_a, _ = _tiny(dev)
    m_b, _ = _tiny(dev)
    start = {k: p.detach().clone() for k, p in m_a.named_parameters() if k in STEP_KEYS}
    ts_a = TrainStep(m_a, optimizer="sgd", lr=lr, criterion=N.FocalLoss(2.0, weight=w).to(dev), accumulate=2)
    ts_b = TrainStep(m_b, optimizer="sgd", lr=lr, criterion=N.FocalLoss(2.0, weight=w).to(dev))
    for i in range(2):
        ts_a.step({k: v[i:i + 1] for k, v in inputs.items()}, labels[i:i + 1])
    loss_b = ts_b.step(inputs, labels)
    na, nb = dict(m_a.named_parameters()), dict(m_b.named_parameters())
    rels = {k: _rel(na[k].detach() - start[k], nb[k].detach() - start[k]) for k in STEP_KEYS}
    err = abs(ts_a.accum_loss.item() - loss_b.item())
    print("focal figures accumulate", rels, err, ts_a.accum_count.item())
    assert all(r <= 8e-2 for r in rels.values()), rels
    assert err <= 2e-2
    want = w.double()[labels[labels != IGN].cpu()].sum().item()
    assert abs(ts_a.accum_count.item() - want) <= 1e-5 * want
