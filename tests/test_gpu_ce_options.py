"""Cross-entropy with class weights, label smoothing and the 'sum' / 'none' reductions on the HIP path, against
torch.nn.functional.cross_entropy in fp64 on the CPU: the fused upsample + CE head (op, module, model, train step, captured
step) and the unfused NCHW drop-in."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_cases  # noqa: E402
from head_cases import head_case as _head_case  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = -100


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _weights(C, seed):
    return torch.rand(C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 1.5 + 0.25


# head_cases.HEAD_CASES, and behind it every (mode, S, TN) instantiation of head_ce_grp_kernel that the list does not reach
HEAD_CASES = head_cases.HEAD_CASES_ALL


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mode,S,C,h,w", HEAD_CASES)
def test_head_upsample_ce_weighted_smoothed(dev, mode, S, C, h, w, eps):
    from lc2is_amd import ops
    B = 2
    lo, labels, ref_labels = _head_case(B, h, w, C, S, 31 * C + S)
    w64 = _weights(C, C)
    m = ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR
    loss, dlo, _ = ops.head_upsample_ce(lo.to(dev), labels.to(dev), B, h, w, C, S, m, want_grad=True,
                                        class_weight=w64.float().to(dev), label_smoothing=eps)
    lod = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = F.interpolate(lod, scale_factor=S, mode=mode)
    ref = F.cross_entropy(up, ref_labels, weight=w64, label_smoothing=eps, reduction="sum")
    ref.backward()
    assert abs(loss[0].item() - ref.item()) <= 1e-4 * abs(ref.item())
    wsum = w64[ref_labels[ref_labels != IGN]].sum().item()
    assert abs(loss[1].item() - wsum) <= 1e-5 * wsum
    assert _rel(dlo[:, :C], lod.grad.permute(0, 2, 3, 1).reshape(B * h * w, C)) <= 2e-5
    assert dlo[:, C:].abs().sum().item() == 0


@pytest.mark.parametrize("mode,S", [("bicubic", 4), ("bilinear", 16)])
def test_head_upsample_ce_options_bitwise_reproducible(dev, mode, S):
    from lc2is_amd import ops
    B, h, C = 3, 16, 151
    lo, labels, _ = _head_case(B, h, h, C, S, 5)
    lo, labels = lo.to(dev), labels.to(dev)
    w = _weights(C, 1).float().to(dev)
    m = ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR
    a = ops.head_upsample_ce(lo, labels, B, h, h, C, S, m, want_grad=True, class_weight=w, label_smoothing=0.1)
    b = ops.head_upsample_ce(lo, labels, B, h, h, C, S, m, want_grad=True, class_weight=w, label_smoothing=0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode,S,C", [("bicubic", 4, 151), ("bilinear", 8, 150), ("bicubic", 16, 37)])
def test_head_upsample_ce_unit_weights_match_default(dev, mode, S, C):
    from lc2is_amd import ops
    B, h = 2, 8
    lo, labels, _ = _head_case(B, h, h, C, S, 9)
    lo, labels = lo.to(dev), labels.to(dev)
    m = ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR
    l0, d0, _ = ops.head_upsample_ce(lo, labels, B, h, h, C, S, m, want_grad=True, grad_scale=0.25)
    l1, d1, _ = ops.head_upsample_ce(lo, labels, B, h, h, C, S, m, want_grad=True, grad_scale=0.25,
                                     class_weight=torch.ones(C, device=dev), label_smoothing=0.0)
    assert abs(l1[0].item() - l0[0].item()) <= 1e-6 * abs(l0[0].item())
    assert l1[1].item() == l0[1].item()
    assert _rel(d1, d0) <= 1e-6


def test_head_upsample_ce_options_refused_on_the_atomic_path(dev):
    from lc2is_amd import ops
    B, h, C, S = 1, 4, 50, 32
    lo = torch.zeros(B * h * h, 64, device=dev)
    labels = torch.zeros(B, h * S, h * S, dtype=torch.long, device=dev)
    with pytest.raises(RuntimeError, match="refused"):
        ops.head_upsample_ce(lo, labels, B, h, h, C, S, ops.INTERP_BILINEAR, class_weight=torch.ones(C, device=dev))
    with pytest.raises(RuntimeError, match="weight tensor should be defined either for all"):
        ops.head_upsample_ce(lo, labels, B, h, h, C, 4, ops.INTERP_BILINEAR, class_weight=torch.ones(C + 1, device=dev))


def _ce_nchw_vs_torch(dev, shape, weighted, eps, over=0, count_tol=1e-5):
    """ops.ce_nchw_fwd / ce_nchw_bwd at one shape.  Labels are drawn from [0, C + over): those >= C are not counted (the reference
    ignores them)."""
    from lc2is_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g) * 2
    dev_labels = torch.randint(0, C + over, (B, H, W), generator=g)
    dev_labels[:, ::4] = IGN
    labels = torch.where(dev_labels < C, dev_labels, torch.full_like(dev_labels, IGN))
    w64 = _weights(C, 2) if weighted else None
    kw = dict(class_weight=None if w64 is None else w64.float().to(dev), label_smoothing=eps)
    xd, ld = x.to(dev), dev_labels.to(dev)
    loss2, lse, lpx = ops.ce_nchw_fwd(xd, ld, IGN, per_pixel=True, **kw)
    x64 = x.double().requires_grad_(True)
    ref = F.cross_entropy(x64, labels, weight=w64, label_smoothing=eps, reduction="none")
    assert _rel(lpx, ref.detach()) <= 1e-5
    assert abs(loss2[0].item() - ref.sum().item()) <= 1e-5 * abs(ref.sum().item())
    wsum = (w64[labels[labels != IGN]].sum() if weighted else (labels != IGN).sum()).item()
    assert abs(loss2[1].item() - wsum) <= count_tol * wsum
    gpx = torch.rand(B, H, W, generator=g, dtype=torch.float64) + 0.5   # non-uniform upstream gradient
    ref.backward(gpx)
    d = ops.ce_nchw_bwd(xd, ld, lse, None, 1.0, IGN, grad_px=gpx.float().to(dev), **kw)
    assert _rel(d, x64.grad) <= 1e-5
    # scalar scale ('sum' / 'mean'): device scalar times host scalar
    x64.grad = None
    F.cross_entropy(x64, labels, weight=w64, label_smoothing=eps, reduction="sum").backward(torch.tensor(0.5, dtype=torch.float64))
    d2 = ops.ce_nchw_bwd(xd, ld, lse, torch.full((1,), 0.25, device=dev), 2.0, IGN, **kw)
    assert _rel(d2, x64.grad) <= 1e-5


@pytest.mark.parametrize("weighted,eps", [(True, 0.0), (False, 0.2), (True, 0.2)])
def test_ce_nchw_options_vs_torch(dev, weighted, eps):
    _ce_nchw_vs_torch(dev, (2, 151, 24, 20), weighted, eps)


@pytest.mark.parametrize("weighted,eps", [(False, 0.0), (True, 0.2)], ids=["plain", "opts"])
def test_ce_nchw_past_the_grid_cap(dev, weighted, eps):
    """2 099 601 pixels: more than 8192 blocks of 256, and no multiple of 256 or 64 — the strided walk of the forward and of the
    backward, both kernel variants.  The sums to the bounds of test_ce_nchw_fwd_sums_are_ordered (1e-5 / 1e-6 relative)."""
    _ce_nchw_vs_torch(dev, (1, 2, 1449, 1449), weighted, eps, over=2, count_tol=1e-6)


@pytest.mark.parametrize("weighted,eps", [(False, 0.0), (True, 0.2)], ids=["plain", "opts"])
def test_ce_nchw_one_class(dev, weighted, eps):
    """C = 1: the softmax is 1, so every loss and every gradient is 0 in exact arithmetic and a relative error has no meaning.  In
    fp32 the terms that cancel (w lse against w z; (1 - eps) w + eps w against itself) are each rounded, so the bound is the 1e-5 of
    the NCHW tests relative to the size of those terms: w |z| for a loss, w g for a gradient.  lse and the count as usual."""
    from lc2is_amd import ops
    B, C, H, W = 1, 1, 5, 7
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g) * 2
    labels = torch.randint(0, C + 2, (B, H, W), generator=g)
    labels[:, ::4] = IGN
    valid = labels == 0
    w64 = _weights(C, 2) if weighted else torch.ones(1, dtype=torch.float64)
    kw = dict(class_weight=w64.float().to(dev) if weighted else None, label_smoothing=eps)
    xd, ld = x.to(dev), labels.to(dev)
    loss2, lse, lpx = ops.ce_nchw_fwd(xd, ld, IGN, per_pixel=True, **kw)
    assert _rel(lse, x[:, 0]) <= 1e-5
    assert abs(loss2[1].item() - w64[0].item() * int(valid.sum())) <= 1e-5 * w64[0].item() * int(valid.sum())
    size = (w64[0] * x[:, 0].double().abs()) * valid
    ref_labels = torch.where(valid, labels, torch.full_like(labels, IGN))
    ref = F.cross_entropy(x.double(), ref_labels, weight=w64 if weighted else None, label_smoothing=eps, reduction="none")
    assert _rel(lse, torch.logsumexp(x.double(), 1)) <= 1e-5                   # fp64 torch is finite here: lse = z, losses ~ 0
    assert (lpx.double().cpu() - ref).abs().max().item() <= 1e-5 * size.max().item()
    assert lpx.double().abs().max().item() <= 1e-5 * size.max().item() and not lpx.cpu()[~valid].any()
    assert abs(loss2[0].item()) <= 1e-5 * size.sum().item()
    gpx = torch.rand(B, H, W, generator=g) + 0.5
    for d, gmax in ((ops.ce_nchw_bwd(xd, ld, lse, None, 1.0, IGN, grad_px=gpx.to(dev), **kw), gpx.max().item()),
                    (ops.ce_nchw_bwd(xd, ld, lse, torch.full((1,), 0.25, device=dev), 2.0, IGN, **kw), 0.5)):
        assert d.abs().max().item() <= 1e-5 * w64[0].item() * gmax and not d.cpu()[:, 0][~valid].any()


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("weighted,eps,ignore_index", [(True, 0.0, IGN), (False, 0.1, 0), (True, 0.1, IGN)])
def test_cross_entropy_module_options(dev, reduction, weighted, eps, ignore_index):
    import lc2is_amd.nn as N
    B, C, H, W = 2, 151, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g) * 2
    labels = torch.randint(0, C, (B, H, W), generator=g)
    labels[:, 5:9] = ignore_index
    w64 = _weights(C, 4) if weighted else None
    ours = N.CrossEntropyLoss(weight=None if w64 is None else w64.float(), ignore_index=ignore_index, reduction=reduction,
                              label_smoothing=eps).to(dev)
    ref_mod = torch.nn.CrossEntropyLoss(weight=w64, ignore_index=ignore_index, reduction=reduction, label_smoothing=eps)
    xd = x.to(dev).requires_grad_(True)
    loss = ours(xd, labels.to(dev))
    x64 = x.double().requires_grad_(True)
    ref = ref_mod(x64, labels)
    assert loss.shape == ref.shape
    assert _rel(loss.detach(), ref.detach()) <= 1e-5
    up = torch.rand(ref.shape, generator=g, dtype=torch.float64) + 0.5 if reduction == "none" else torch.tensor(
        1.5, dtype=torch.float64)
    loss.backward(up.float().to(dev))
    ref.backward(up)
    assert _rel(xd.grad, x64.grad) <= 1e-5


def test_cross_entropy_module_everything_ignored_gives_nan_mean(dev):
    import lc2is_amd.nn as N
    x = torch.randn(1, 151, 8, 8)
    labels = torch.full((1, 8, 8), IGN, dtype=torch.long)
    w = _weights(151, 6)
    ref = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)(x.double(), labels)
    loss = N.CrossEntropyLoss(weight=w.float(), label_smoothing=0.1).to(dev)(x.to(dev), labels.to(dev))
    assert torch.isnan(ref) and torch.isnan(loss)
    s = N.CrossEntropyLoss(weight=w.float(), label_smoothing=0.1, reduction="sum").to(dev)(x.to(dev), labels.to(dev))
    assert s.item() == 0.0


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("h,S", [(16, 8), (8, 16), (32, 4)])
def test_auxiliary_loss_options(dev, reduction, h, S):
    import lc2is_amd.nn as N
    B, C = 2, 151
    g = torch.Generator().manual_seed(h)
    x = torch.randn(B, C, h, h, generator=g) * 2
    labels = torch.randint(0, C, (B, h * S, h * S), generator=g)
    labels[:, ::7] = IGN
    w64 = _weights(C, 8)
    xd = x.to(dev).requires_grad_(True)
    loss = N.AuxiliaryLoss(weight=w64.float(), label_smoothing=0.1, reduction=reduction).to(dev)(xd, labels.to(dev))
    x64 = x.double().requires_grad_(True)
    up = F.interpolate(x64, size=(h * S, h * S), mode="bilinear", align_corners=False)
    ref = F.cross_entropy(up, labels, weight=w64, label_smoothing=0.1, reduction=reduction)
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    loss.backward()
    ref.backward()
    assert _rel(xd.grad, x64.grad) <= 2e-5


def _tiny(dev):
    import lc2is_amd.nn as N
    from pathlib import Path
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


GRAD_KEYS = ("class_prototypes", "vision_decoder.layers.0.linear2.weight")


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_fused_head_matches_unfused_criterion(dev, reduction):
    import lc2is_amd.nn as N
    m, fx = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev).clone()
    labels[:, :3] = IGN
    w = _weights(151, 12).float().to(dev)
    loss_u = N.CrossEntropyLoss(weight=w, label_smoothing=0.1, reduction=reduction)(m(inputs)["outputs"], labels)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    loss_f = m.forward_loss(inputs, labels, weight=w, label_smoothing=0.1, reduction=reduction)
    loss_f.backward()
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    named = dict(m.named_parameters())
    for k in GRAD_KEYS:
        assert _rel(named[k].grad, g_u[k]) <= 1e-3, k


def test_score_map_tail_options_match_unfused(dev):
    import lc2is_amd.nn as N
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    w = _weights(K, 13).float().to(dev)
    tail = N.ScoreMapTail(4)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_u = N.CrossEntropyLoss(weight=w, label_smoothing=0.1)(tail(v1, t1), labels)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, weight=w, label_smoothing=0.1)
    loss_f.backward()
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert _rel(v2.grad, v1.grad) <= 1e-3 and _rel(t2.grad, t1.grad) <= 1e-3


def test_train_step_with_weighted_smoothed_criterion(dev):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    lr = 1e-2
    m1, fx = _tiny(dev)
    m2, _ = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev)
    crit = N.CrossEntropyLoss(weight=_weights(151, 14).float(), label_smoothing=0.1).to(dev)
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    loss_ts = TrainStep(m1, optimizer="sgd", lr=lr, criterion=crit).step(inputs, labels)
    loss_h = crit(m2(inputs)["outputs"], labels)          # the same step by hand, unfused
    loss_h.backward()
    assert abs(loss_ts.item() - loss_h.item()) <= 1e-4 * abs(loss_h.item())
    named1, named2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    for k in GRAD_KEYS + ("pixel_patch.visual.weight", "vision_encoder.enc.embeddings.patch_embedding.weight",
                          "text_encoder.enc.embeddings.token_embedding.weight"):
        r = _rel(named1[k].detach() - start[k], -lr * named2[k].grad)
        assert r < 8e-2, (k, r)


def test_captured_step_with_weighted_criterion(dev):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(1, 500, (2, 8), generator=g)
        ids[:, 0], ids[:, -1] = 510, 511
        return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
                 "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)},
                torch.randint(0, 151, (2, 16, 16), generator=g).to(dev))

    batches = [batch(s) for s in range(3)]
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    crit = N.CrossEntropyLoss(weight=_weights(151, 15).float(), label_smoothing=0.1).to(dev)
    ts_e = TrainStep(m_e, optimizer="sgd", lr=1e-3, criterion=crit)
    ts_g = TrainStep(m_g, optimizer="sgd", lr=1e-3, criterion=crit)
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(*batches[0])
    torch.cuda.synchronize()
    le, lg = [], []
    for inp, lab in batches[1:]:
        le.append(ts_e.step(inp, lab).item())
        lg.append(run(inp, lab).item())
    torch.cuda.synchronize()
    assert le == pytest.approx(lg, abs=1e-5), (le, lg)
    run.release()
