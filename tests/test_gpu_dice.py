"""Dice + cross-entropy on the HIP path against the fp64 torch reference of tests/dice_ref.py: the fused upsample head (op,
cross-block reduce, empty sets, saturated softmax, the CE-only limit), the unfused NCHW criterion, forward_loss / ScoreMapTail.loss
against the unfused module, and the train step (eager, reproducible, captured).

Gates (fp32 kernels vs fp64 torch, those of the existing head tests): T and n_valid exact; I, P rel-L2 <= 1e-5; CE, Dice and the
total <= 1e-4 relative; gradient rel-L2 <= 2e-5; gradient columns past C exactly 0."""
import sys
from functools import lru_cache
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dice_ref as R  # noqa: E402
import head_cases  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = -100

# head_cases.HEAD_CASES (indices 0-9 are used by name below), and behind it every (mode, S, TN) instantiation of
# head_dice_stats_grp_kernel / head_ce_dice_grp_kernel that the list does not reach
HEAD_CASES = head_cases.HEAD_CASES_ALL
WEIGHTS = [(0.0, 1.0), (1.0, 3.0)]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _head_case(B, h, w, C, S, seed, fold):
    """Labels as test_gpu_ce_options._head_case draws them (values >= C are skipped by the kernel, every fifth row is ignored);
    fold: into C // 3 classes, so that two thirds of the classes are absent."""
    g = torch.Generator().manual_seed(seed)
    ld = 64 if C <= 64 else (128 if C <= 128 else 192)
    lo = torch.zeros(B * h * w, ld)
    lo[:, :C] = torch.randn(B * h * w, C, generator=g) * 3
    labels = torch.randint(0, C + 3, (B, h * S, w * S), generator=g)
    if fold:
        labels = labels % (C // 3)
    labels[:, 1::5] = IGN
    return lo, labels


@lru_cache(maxsize=None)
def _head_ref(mode, S, C, h, w, B, seed, fold, cw, dw, smooth, present_only, scale=1.0, blank=-1):
    """The fp64 reference of a case, computed once and shared."""
    lo, labels = _head_case(B, h, w, C, S, seed, fold)
    lo = lo * scale
    if blank >= 0:
        labels[blank] = IGN
    out, grad = R.head(lo, labels, B, h, w, C, S, mode, ignore_index=IGN, ce_weight=cw, dice_weight=dw, smooth=smooth,
                       present_only=present_only)
    return lo, labels, out, grad


def _check(loss4, stats, dlo, out, grad, C, tag=""):
    l4 = loss4.double().cpu()
    st = stats.double().cpu()
    figures = dict(
        n_valid=(l4[3].item(), out["n_valid"]),
        T=int((st[2, :C] != out["T"]).sum()),
        I=_rel(st[0, :C], out["I"]), P=_rel(st[1, :C], out["P"]),
        ce=abs(l4[1].item() - out["ce"].item()) / max(abs(out["ce"].item()), 1e-30),
        dice=abs(l4[2].item() - out["dice"].item()) / max(abs(out["dice"].item()), 1e-30),
        total=abs(l4[0].item() - out["total"].item()) / max(abs(out["total"].item()), 1e-30),
        grad=_rel(dlo[:, :C], grad) if dlo is not None else 0.0,
        pad=dlo[:, C:].abs().sum().item() if dlo is not None else 0.0)
    print("dice figures", tag, figures)
    assert torch.isfinite(loss4).all() and torch.isfinite(stats).all() and (dlo is None or torch.isfinite(dlo).all())
    assert figures["n_valid"][0] == figures["n_valid"][1] and figures["T"] == 0
    assert st[:, C:].abs().sum().item() == 0
    assert figures["I"] <= 1e-5 and figures["P"] <= 1e-5
    assert figures["ce"] <= 1e-4 and figures["dice"] <= 1e-4 and figures["total"] <= 1e-4
    assert figures["grad"] <= 2e-5 and figures["pad"] == 0


def _mode(ops, mode):
    return ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR


@pytest.mark.parametrize("smooth", [1.0, 0.0])
@pytest.mark.parametrize("present_only", [True, False])
@pytest.mark.parametrize("cw,dw", WEIGHTS)
@pytest.mark.parametrize("mode,S,C,h,w", HEAD_CASES)
def test_head_upsample_ce_dice_vs_fp64(dev, mode, S, C, h, w, cw, dw, present_only, smooth):
    from lc2is_amd import ops
    B = 2
    lo, labels, out, grad = _head_ref(mode, S, C, h, w, B, 31 * C + S, present_only, cw, dw, smooth, present_only)
    if present_only:   # two thirds of the classes are absent
        assert int((out["T"] > 0).sum()) == C // 3
    loss4, stats, dlo = ops.head_upsample_ce_dice(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode), want_grad=True,
                                                  ce_weight=cw, dice_weight=dw, smooth=smooth, present_only=present_only)
    _check(loss4, stats, dlo, out, grad, C, f"{mode} S={S} C={C} cw={cw} dw={dw} po={present_only} s={smooth}")
    # forward only: the same loss block and statistics from the first two launches alone
    l2, s2, d2 = ops.head_upsample_ce_dice(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode), want_grad=False,
                                           ce_weight=cw, dice_weight=dw, smooth=smooth, present_only=present_only)
    assert d2 is None and torch.equal(l2, loss4) and torch.equal(s2, stats)


@pytest.mark.parametrize("cw,dw", WEIGHTS)
def test_grad_scale_scales_the_gradient_only(dev, cw, dw):
    from lc2is_amd import ops
    mode, S, C, h, w = HEAD_CASES[0]
    lo, labels, out, grad = _head_ref(mode, S, C, h, w, 2, 31 * C + S, True, cw, dw, 1.0, True)
    loss4, stats, dlo = ops.head_upsample_ce_dice(lo.to(dev), labels.to(dev), 2, h, w, C, S, _mode(ops, mode), want_grad=True,
                                                  ce_weight=cw, dice_weight=dw, grad_scale=0.25)
    _check(loss4, stats, dlo * 4.0, out, grad, C, "grad_scale")


@pytest.mark.parametrize("cw,dw", WEIGHTS)
def test_cross_block_reduce_and_bitwise_repeat(dev, cw, dw):
    """B = 3, 16 x 16 cells, S = 4: 75 blocks, more than a wave's stride in the slab sums; two runs give the same bytes."""
    from lc2is_amd import ops
    B, h, S, C = 3, 16, 4, 151
    lo, labels, out, grad = _head_ref("bicubic", S, C, h, h, B, 5, True, cw, dw, 1.0, True)
    lod, lab = lo.to(dev), labels.to(dev)
    a = ops.head_upsample_ce_dice(lod, lab, B, h, h, C, S, ops.INTERP_BICUBIC, want_grad=True, ce_weight=cw, dice_weight=dw)
    _check(*a, out, grad, C, f"75 blocks cw={cw} dw={dw}")
    b = ops.head_upsample_ce_dice(lod, lab, B, h, h, C, S, ops.INTERP_BICUBIC, want_grad=True, ce_weight=cw, dice_weight=dw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("smooth", [1.0, 0.0])
@pytest.mark.parametrize("present_only", [True, False])
def test_empty_sets(dev, present_only, smooth):
    from lc2is_amd import ops
    mode, S, C, h, w = "bicubic", 4, 151, 5, 5
    B = 2
    # one image of the batch all ignore_index: equals the reference
    lo, labels, out, grad = _head_ref(mode, S, C, h, w, B, 77, True, 1.0, 3.0, smooth, present_only, 1.0, 1)
    assert out["n_valid"] > 0 and not R.valid_mask(labels[1], C, IGN).any()
    res = ops.head_upsample_ce_dice(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode), want_grad=True,
                                    ce_weight=1.0, dice_weight=3.0, smooth=smooth, present_only=present_only)
    _check(*res, out, grad, C, f"one image ignored po={present_only} s={smooth}")
    # the whole batch ignored: loss block all 0 with n_valid 0, gradient all 0, nothing non-finite
    none = torch.full_like(labels, IGN).to(dev)
    loss4, stats, dlo = ops.head_upsample_ce_dice(lo.to(dev), none, B, h, w, C, S, _mode(ops, mode), want_grad=True,
                                                  ce_weight=1.0, dice_weight=3.0, smooth=smooth, present_only=present_only)
    for t in (loss4, stats, dlo):
        assert torch.isfinite(t).all()
    assert loss4.tolist() == [0.0, 0.0, 0.0, 0.0] and not dlo.any() and not stats.any()


@pytest.mark.parametrize("cw,dw", WEIGHTS)
@pytest.mark.parametrize("mode,S,C,h,w", [HEAD_CASES[0], HEAD_CASES[5]])
def test_saturated_softmax(dev, mode, S, C, h, w, cw, dw):
    from lc2is_amd import ops
    B = 2
    lo, labels, out, grad = _head_ref(mode, S, C, h, w, B, 31 * C + S, True, cw, dw, 1.0, True, 40.0)
    res = ops.head_upsample_ce_dice(lo.to(dev), labels.to(dev), B, h, w, C, S, _mode(ops, mode), want_grad=True,
                                    ce_weight=cw, dice_weight=dw)
    _check(*res, out, grad, C, f"x40 {mode} S={S} cw={cw} dw={dw}")


@pytest.mark.parametrize("mode,S,C,h,w", [HEAD_CASES[0], HEAD_CASES[4], HEAD_CASES[7]])
def test_dice_weight_zero_is_the_mean_ce_head(dev, mode, S, C, h, w):
    from lc2is_amd import ops
    B = 2
    lo, labels = _head_case(B, h, w, C, S, 9, False)
    lo, labels = lo.to(dev), labels.to(dev)
    loss2, d0, _ = ops.head_upsample_ce(lo, labels, B, h, w, C, S, _mode(ops, mode), want_grad=True)
    loss4, _, d1 = ops.head_upsample_ce_dice(lo, labels, B, h, w, C, S, _mode(ops, mode), want_grad=True, ce_weight=1.0,
                                             dice_weight=0.0)
    mean = (loss2[0] / loss2[1]).item()
    assert loss4[3].item() == loss2[1].item()
    assert abs(loss4[0].item() - mean) <= 1e-6 * abs(mean) and abs(loss4[1].item() - mean) <= 1e-6 * abs(mean)
    assert _rel(d1, d0 / loss2[1]) <= 1e-6


@pytest.mark.parametrize("smooth", [1.0, 0.0])
@pytest.mark.parametrize("present_only", [True, False])
@pytest.mark.parametrize("cw,dw", WEIGHTS)
@pytest.mark.parametrize("C", [10, 151])
def test_dice_cross_entropy_module_on_nchw_logits(dev, C, cw, dw, present_only, smooth):
    _dice_nchw_vs_fp64(dev, (2, C, 20, 28), cw, dw, present_only, smooth)


@pytest.mark.parametrize("present_only,smooth", [(True, 1.0), (False, 0.0)])
@pytest.mark.parametrize("C", [5, 192])
def test_dice_nchw_edge_class_counts(dev, C, present_only, smooth):
    """C = 5: the rows of the statistics slab and of the coefficient block are padded to cq = 8; C = 192: the class limit."""
    _dice_nchw_vs_fp64(dev, (1, C, 9, 7), 1.0, 3.0, present_only, smooth)


def test_dice_nchw_past_the_grid_cap(dev):
    """525 625 pixels: more than the 2048 blocks of the statistics pass, and no multiple of 256 or 64 — its block-uniform strided
    loop, the coefficient pass over 2048 slabs, and the backward's walk.  The CE mean (the loss sum over the exact count) also to the
    1e-5 of test_ce_nchw_fwd_sums_are_ordered at this size."""
    loss4, out = _dice_nchw_vs_fp64(dev, (1, 3, 725, 725), 1.0, 3.0, False, 1.0, ld=3)
    assert abs(loss4[1].item() - out["ce"].item()) <= 1e-5 * abs(out["ce"].item())


def _dice_nchw_vs_fp64(dev, shape, cw, dw, present_only, smooth, ld=192):
    """``ld``: the width the gradient is padded to for _check (192 as the head's; C where the map is large)."""
    import lc2is_amd.nn as N
    from lc2is_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, C, H, W, generator=g) * 2
    labels = torch.randint(0, C + 3, (B, H, W), generator=g)
    if present_only:
        labels = labels % (C // 3)
    labels[:, 1::5] = IGN
    out, grad = R.nchw(x, labels, ignore_index=IGN, ce_weight=cw, dice_weight=dw, smooth=smooth, present_only=present_only)
    crit = N.DiceCrossEntropyLoss(cw, dw, smooth, present_only)
    xd = x.to(dev).requires_grad_(True)
    loss = crit(xd, labels.to(dev))
    loss.backward(torch.tensor(1.5, device=dev))
    I, P, T, loss4 = crit.last_stats
    assert torch.equal(loss.detach(), loss4[0])
    stats = torch.zeros(3, 192, device=dev)
    stats[:, :C] = torch.stack([I, P, T])
    pad = torch.zeros(B * H * W, ld, device=dev)
    pad[:, :C] = xd.grad.permute(0, 2, 3, 1).reshape(-1, C) / 1.5
    _check(loss4, stats, pad, out, grad.permute(0, 2, 3, 1).reshape(-1, C), C, f"nchw C={C} cw={cw} dw={dw} po={present_only} s={smooth}")
    # the launchers directly: host scalar times device scalar
    l4, st, lse, coef = ops.ce_dice_nchw_fwd(xd.detach(), labels.to(dev), IGN, ce_weight=cw, dice_weight=dw, smooth=smooth,
                                             present_only=present_only)
    d = ops.ce_dice_nchw_bwd(xd.detach(), labels.to(dev), lse, coef, torch.full((1,), 0.5, device=dev), 3.0, IGN)
    assert torch.equal(l4, loss4) and torch.equal(st[0], I) and torch.equal(d, xd.grad)
    # every pixel ignored: zeros, nothing non-finite
    none = torch.full_like(labels, IGN).to(dev)
    x0 = x.to(dev).requires_grad_(True)
    l0 = crit(x0, none)
    l0.backward()
    assert l0.item() == 0.0 and crit.last_stats[3].tolist() == [0.0, 0.0, 0.0, 0.0] and not x0.grad.any()
    return loss4, out


def _tiny(dev):
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


GRAD_KEYS = ("class_prototypes", "vision_decoder.layers.0.linear2.weight")


def _tiny_unfused_loss(dev, crit):
    m, fx = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev).clone()
    labels[:, :3] = IGN
    loss_u = crit(m(inputs)["outputs"], labels)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    return m, inputs, labels, loss_u, g_u


@pytest.mark.parametrize("cw,dw,present_only", [(0.0, 1.0, True), (1.0, 3.0, True), (1.0, 3.0, False)])
def test_forward_loss_dice_matches_unfused_module(dev, cw, dw, present_only):
    import lc2is_amd.nn as N
    crit = N.DiceCrossEntropyLoss(cw, dw, 1.0, present_only)
    m, inputs, labels, loss_u, g_u = _tiny_unfused_loss(dev, crit)
    loss_f = m.forward_loss(inputs, labels, dice=crit.dice)
    loss_f.backward()
    print("dice figures forward_loss", loss_f.item(), loss_u.item())
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    named = dict(m.named_parameters())
    for k in GRAD_KEYS:
        r = _rel(named[k].grad, g_u[k])
        print("dice figures forward_loss grad", k, r)
        assert r <= 1e-3, k
    I, P, T, loss4 = m.last_dice
    assert torch.equal(loss4[0], loss_f.detach()) and loss4[3].item() == float((labels != IGN).sum())
    assert _rel(T[:151], crit.last_stats[2]) == 0 and _rel(P[:151], crit.last_stats[1]) <= 1e-5


def test_score_map_tail_dice_matches_unfused(dev):
    import lc2is_amd.nn as N
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    crit = N.DiceCrossEntropyLoss(1.0, 3.0)
    tail = N.ScoreMapTail(4)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_u = crit(tail(v1, t1), labels)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, dice=crit.dice)
    loss_f.backward()
    print("dice figures score tail", loss_f.item(), loss_u.item(), _rel(v2.grad, v1.grad), _rel(t2.grad, t1.grad))
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert _rel(v2.grad, v1.grad) <= 1e-3 and _rel(t2.grad, t1.grad) <= 1e-3
    assert torch.equal(tail.last_dice[3][0], loss_f.detach())


def test_train_step_with_dice_criterion(dev):
    """Three eager steps: the first loss is forward_loss(dice=)'s; two fresh TrainSteps give the same bytes; eval() mode of the
    criterion changes nothing."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    crit = N.DiceCrossEntropyLoss(dice_weight=3.0)
    m0, fx = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev)
    first = m0.forward_loss(inputs, labels, dice=crit.dice).detach()
    outs = []
    for variant in range(3):
        m, _ = _tiny(dev)
        c = N.DiceCrossEntropyLoss(dice_weight=3.0)
        if variant == 2:
            c.eval()
        ts = TrainStep(m, optimizer="sgd", lr=1e-2, momentum=0.9, criterion=c)
        assert ts.dice_stats is None
        losses = [ts.step(inputs, labels).clone() for _ in range(3)]
        assert torch.equal(ts.dice_stats[3][0], losses[-1])
        outs.append((losses, ts.arena.flat.clone()))
    assert abs(outs[0][0][0].item() - first.item()) <= 1e-6 * abs(first.item())
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0][0], other[0])) and torch.equal(outs[0][1], other[1])


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
             "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)},
            torch.randint(0, 151, (2, 16, 16), generator=g).to(dev))


@pytest.mark.parametrize("kind,kw", [("sgd", {}), ("adamw", dict(max_grad_norm=1.0, skip_nonfinite=True))])
def test_captured_step_with_dice_criterion(dev, kind, kw):
    """A captured step replayed on three different batches gives bitwise the losses and parameters of three eager steps."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(4)]
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    ts_e = TrainStep(m_e, optimizer=kind, lr=1e-3, criterion=N.DiceCrossEntropyLoss(dice_weight=3.0), **kw)
    ts_g = TrainStep(m_g, optimizer=kind, lr=1e-3, criterion=N.DiceCrossEntropyLoss(dice_weight=3.0), **kw)
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(*batches[0])
    torch.cuda.synchronize()
    for inp, lab in batches[1:]:
        le = ts_e.step(inp, lab).clone()
        lg = run(inp, lab).clone()
        assert torch.equal(le, lg)
        assert all(torch.equal(a, b) for a, b in zip(ts_g.dice_stats, ts_e.dice_stats))
        assert ts_g.dice_stats[3][3].item() == lab.numel()
    torch.cuda.synchronize()
    assert torch.equal(ts_e.arena.flat, ts_g.arena.flat)
    run.release()
