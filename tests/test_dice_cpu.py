"""CPU checks of the Dice + cross-entropy loss: the closed-form gradient the kernels evaluate against fp64 autograd, argument
validation, the refusals of TrainStep / forward_loss / ScoreMapTail.loss that happen before any GPU work, and the host-side
workspace queries and entry-point refusals."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dice_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402

IGN = -100


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("smooth", [1.0, 0.0])
@pytest.mark.parametrize("present_only", [True, False])
@pytest.mark.parametrize("cw,dw", [(0.0, 1.0), (1.0, 3.0)])
@pytest.mark.parametrize("B,C,H,W", [(2, 10, 12, 9), (1, 151, 8, 8), (3, 37, 5, 7)])
def test_closed_form_gradient_equals_autograd(B, C, H, W, cw, dw, present_only, smooth):
    g = torch.Generator().manual_seed(C + H)
    z = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 3
    labels = torch.randint(0, C + 3, (B, H, W), generator=g) % max(C // 3, 1) if present_only else torch.randint(
        0, C + 3, (B, H, W), generator=g)
    labels[:, 1::5] = IGN
    kw = dict(ignore_index=IGN, ce_weight=cw, dice_weight=dw, smooth=smooth, present_only=present_only)
    out, grad = R.nchw(z, labels, **kw)
    assert out["n_valid"] == int(R.valid_mask(labels, C, IGN).sum()) > 0
    assert _rel(R.closed_form_grad(z, labels, **kw), grad) <= 1e-12
    # the loss itself, term by term, against an independent statement of the definition
    p = torch.softmax(z, 1)
    valid = R.valid_mask(labels, C, IGN)
    dice = 0.0
    for c in range(C):
        sel = valid & (labels == c)
        I, P, T = p[:, c][sel].sum(), p[:, c][valid].sum(), sel.sum()
        if (T > 0 or not present_only) and P + T + smooth > 0:
            dice += 1.0 - (2 * I + smooth) / (P + T + smooth)
    assert abs(out["dice"].item() - float(dice) / C) <= 1e-12
    ce = F.cross_entropy(z.permute(0, 2, 3, 1)[valid], labels[valid])
    assert abs(out["ce"].item() - ce.item()) <= 1e-12 * abs(ce.item())
    assert abs(out["total"].item() - (cw * ce.item() + dw * float(dice) / C)) <= 1e-12


def test_reference_empty_set_is_zero():
    z = torch.randn(1, 5, 4, 4, dtype=torch.float64)
    labels = torch.full((1, 4, 4), IGN)
    for po in (True, False):
        for s in (0.0, 1.0):
            out, grad = R.nchw(z, labels, ignore_index=IGN, smooth=s, present_only=po)
            assert out["n_valid"] == 0 and out["total"].item() == 0 and out["dice"].item() == 0 and not grad.any()
            assert not R.closed_form_grad(z, labels, IGN, 1.0, 1.0, s, po).any()


def test_check_dice_and_constructor_validation():
    from lc2is_amd.nn.loss import check_dice
    assert check_dice(1, 3, 0, True) == (1.0, 3.0, 0.0, True)
    c = N.DiceCrossEntropyLoss()
    assert isinstance(c, N.CrossEntropyLoss) and c.dice == (1.0, 1.0, 1.0, True) and c.ignore_index == IGN
    assert c.reduction == "mean" and c.weight is None and c.label_smoothing == 0.0 and c.last_stats is None
    c = N.DiceCrossEntropyLoss(0.0, 3.0, 0.0, False, 255)
    assert c.dice == (0.0, 3.0, 0.0, False) and c.ignore_index == 255
    assert list(c.state_dict().keys()) == list(nn.CrossEntropyLoss().state_dict().keys())
    for name in ("ce_weight", "dice_weight", "smooth"):
        for bad in (-0.1, float("nan"), float("inf"), None, "1", True):
            with pytest.raises(ValueError, match=name):
                N.DiceCrossEntropyLoss(**{name: bad})
    with pytest.raises(ValueError, match="both"):
        N.DiceCrossEntropyLoss(ce_weight=0.0, dice_weight=0.0)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="present_only"):
            N.DiceCrossEntropyLoss(present_only=bad)
    with pytest.raises(ValueError, match="not supported"):
        N.DiceCrossEntropyLoss(weight=torch.ones(3))
    with pytest.raises(ValueError, match="not supported"):
        N.DiceCrossEntropyLoss(label_smoothing=0.1)
    for red in ("sum", "none"):
        with pytest.raises(ValueError, match="not supported"):
            N.DiceCrossEntropyLoss(reduction=red)


def test_module_refuses_cpu_tensors():
    with pytest.raises(RuntimeError):
        N.DiceCrossEntropyLoss()(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError):
        N.DiceCrossEntropyLoss().eval()(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


class _CpuModel(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so reaching that error proves the criterion guards passed."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", ohem=None,
                     dice=None):
        raise AssertionError("not reached")


class _NoDiceModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", ohem=None):
        raise AssertionError("not reached")


def test_trainstep_accepts_the_criterion_and_keeps_its_guards():
    from lc2is_amd.step import TrainStep
    with pytest.raises(RuntimeError):                      # accepted: the arena is what refuses a CPU model
        TrainStep(_CpuModel(), criterion=N.DiceCrossEntropyLoss(dice_weight=3.0))
    with pytest.raises(RuntimeError):                      # eval() mode is still CE + Dice: accepted alike
        TrainStep(_CpuModel(), criterion=N.DiceCrossEntropyLoss().eval())
    with pytest.raises(ValueError, match="ignore_index"):
        TrainStep(_CpuModel(), criterion=N.DiceCrossEntropyLoss(), ignore_index=0)
    with pytest.raises(TypeError, match="dice"):           # a model whose fused head has no Dice term (the compose models)
        TrainStep(_NoDiceModel(), criterion=N.DiceCrossEntropyLoss())
    crit = N.DiceCrossEntropyLoss()
    crit.reduction = "none"
    with pytest.raises(ValueError, match="reduction='none'"):
        TrainStep(_CpuModel(), criterion=crit)


def _tiny_cpu():
    return N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                               text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                               dim_feedforward=128, out_dim=64)


def test_fused_sites_refuse_combinations_before_running():
    import inspect
    assert inspect.signature(N.BaseModelWithText.forward_loss).parameters["dice"].default is None
    assert inspect.signature(N.ScoreMapTail.loss).parameters["dice"].default is None
    m = _tiny_cpu()
    labels = torch.zeros(1, 16, 16, dtype=torch.long)
    d = (1.0, 1.0, 1.0, True)
    for kw in (dict(ohem=(0.7, 4)), dict(weight=torch.ones(151)), dict(label_smoothing=0.1), dict(reduction="sum")):
        with pytest.raises(ValueError, match="cannot be combined"):
            m.forward_loss({}, labels, dice=d, **kw)           # (raised before the inputs are looked at)
    with pytest.raises(NotImplementedError):
        m.forward_loss({}, labels, dice=d, reduction="none")
    with pytest.raises(ValueError, match="dice_weight"):
        m.forward_loss({}, labels, dice=(1.0, -1.0, 1.0, True))
    with pytest.raises(ValueError, match="both"):
        m.forward_loss({}, labels, dice=(0.0, 0.0, 1.0, True))
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    for kw in (dict(ohem=(0.7, 4)), dict(weight=torch.ones(3)), dict(label_smoothing=0.1), dict(reduction="sum")):
        with pytest.raises(ValueError, match="cannot be combined"):
            tail.loss(*args, dice=d, **kw)
    with pytest.raises(ValueError, match="smooth"):
        tail.loss(*args, dice=(1.0, 1.0, -1.0, True))
    with pytest.raises(ValueError, match="present_only"):
        tail.loss(*args, dice=(1.0, 1.0, 1.0, 1))


def test_workspace_queries_are_pure_host_functions():
    from lc2is_amd import ops
    q = ops._fn("lc2is_head_upsample_ce_dice_workspace_bytes")
    for mode in (0, 1):
        for S in (4, 8, 16):
            for grad in (0, 1):
                sizes = [q(B, 8, 8, 151, S, mode, grad) for B in (1, 2, 3, 8, 32)]
                assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (mode, S, grad, sizes)
            assert q(2, 8, 8, 151, S, mode, 1) > q(2, 8, 8, 151, S, mode, 0)
            # the slabs of the gradient pass are head_upsample_ce's: the difference between the two queries is the same
            ce = ops._fn("lc2is_head_upsample_ce_workspace_bytes")
            assert q(2, 8, 8, 151, S, mode, 1) - q(2, 8, 8, 151, S, mode, 0) == ce(2, 8, 8, 151, S, mode, 1) - ce(2, 8, 8, 151, S, mode, 0)
    assert q(2, 8, 8, 151, 32, 0, 1) == 0 and q(2, 8, 8, 151, 5, 0, 1) == 0 and q(2, 8, 8, 151, 4, 7, 1) == 0
    assert q(0, 8, 8, 151, 4, 0, 1) == 0 and q(2, 8, 8, 193, 4, 0, 1) == 0 and q(2, 8, 8, 0, 4, 0, 1) == 0
    n = ops._fn("lc2is_ce_dice_nchw_workspace_bytes")
    sizes = [n(B, 151, 20 * 28) for B in (1, 2, 3, 8)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert n(0, 151, 64) == 0 and n(1, 193, 64) == 0 and n(1, 151, 0) == 0
    assert n(64, 151, 512 * 512) == n(128, 151, 512 * 512)      # the grid is capped: so are the rows


def test_entry_points_refuse_bad_arguments_without_touching_a_gpu():
    from lc2is_amd import ops
    P = 0x1000   # (16-byte aligned; never dereferenced)
    f = ops._fn("lc2is_head_upsample_ce_dice")
    ok = dict(lo=P, ld=192, labels=P, dlo=P, loss=P, stats=P, B=2, h=8, w=8, C=151, S=4, mode=0, cw=1.0, dw=1.0, s=1.0, po=1,
              gs=1.0, ws=P, wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["dlo"], a["loss"], a["stats"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"],
                 IGN, a["cw"], a["dw"], a["s"], a["po"], a["gs"], a["ws"], a["wsb"], None)

    for name in ("lo", "labels", "loss"):
        assert call(**{name: None}) == -2, name
    assert call(S=32) == -3 and call(S=5) == -3 and call(mode=7) == -3
    assert call(s=-1.0) == -1 and call(cw=-1.0) == -1 and call(dw=float("nan")) == -1 and call(cw=float("inf")) == -1
    assert call(cw=0.0, dw=0.0) == -1
    assert call(ld=190) == -1 and call(C=193) == -1 and call(B=0) == -1 and call(lo=P + 4) == -1
    need = ops._fn("lc2is_head_upsample_ce_dice_workspace_bytes")(2, 8, 8, 151, 4, 0, 1)
    assert call(wsb=need - 1) == -4 and call(ws=None) == -4
    fwd = ops._fn("lc2is_ce_dice_nchw_fwd")
    assert fwd(None, P, P, P, P, P, 1, 5, 16, IGN, 1.0, 1.0, 1.0, 1, P, 1 << 20, None) == -2
    assert fwd(P, P, P, P, P, None, 1, 5, 16, IGN, 1.0, 1.0, 1.0, 1, P, 1 << 20, None) == -2
    assert fwd(P, P, P, P, P, P, 1, 193, 16, IGN, 1.0, 1.0, 1.0, 1, P, 1 << 20, None) == -3
    assert fwd(P, P, P, P, P, P, 1, 5, 16, IGN, 0.0, 0.0, 1.0, 1, P, 1 << 20, None) == -1
    assert fwd(P, P, P, P, P, P, 1, 5, 16, IGN, 1.0, 1.0, -2.0, 1, P, 1 << 20, None) == -1
    assert fwd(P, P, P, P, P, P, 1, 5, 16, IGN, 1.0, 1.0, 1.0, 1, P, 8, None) == -4
    bwd = ops._fn("lc2is_ce_dice_nchw_bwd")
    assert bwd(P, P, P, None, None, 1.0, P, 1, 5, 16, IGN, None) == -2
    assert bwd(P, P, P, P, None, 1.0, P, 1, 0, 16, IGN, None) == -1
    assert bwd(P, P, P, P, None, 1.0, P, 1, 193, 16, IGN, None) == -3


def test_python_wrappers_refuse_cpu_tensors_and_bad_settings():
    from lc2is_amd import ops
    lo, lab = torch.zeros(4, 64), torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_ce_dice(lo, lab, 1, 2, 2, 5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ce_dice_nchw_fwd(torch.zeros(1, 5, 8, 8), lab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ce_dice_nchw_bwd(torch.zeros(1, 5, 8, 8), lab, torch.zeros(1, 8, 8), torch.zeros(20), None)
    with pytest.raises(ValueError, match="both"):
        ops.dice_options(0, 0, 1, True)
