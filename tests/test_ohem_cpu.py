"""CPU checks of the OHEM cross-entropy: the loss-space rule against the literal p-space original, constructor validation, the
TrainStep guards, and the refusals of the new entry points that happen before any GPU work."""
import sys
from pathlib import Path

import pytest
import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ohem_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402

IGN = -100


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("thresh,K", [(0.7, 40), (1e-6, 40), (0.02, 0), (1.0, 10**9), (0.3, 1)])
def test_loss_space_rule_matches_the_p_space_original(seed, thresh, K):
    g = torch.Generator().manual_seed(seed)
    n, C = 400, 19
    logits = torch.randn(n, C, generator=g, dtype=torch.float64) * 3
    labels = torch.randint(-1, C + 2, (n,), generator=g)
    labels[::7] = IGN
    loss = R.plain_ce(logits, labels, C, IGN)
    ref = R.ohem_rule(loss, labels, C, IGN, thresh, K)
    # the comparison is meant for inputs whose pivot is untied and that hold no pixel at the threshold itself
    v = loss[R.valid_mask(labels, C, IGN)]
    assert int((v == ref["L"]).sum()) == 1 and float((v - R.tau32(thresh).double()).abs().min()) > 1e-6
    kept = R.ohem_pspace(logits, labels, IGN, thresh, K)
    assert torch.equal(kept, ref["kept"])
    assert torch.equal(ref["labels_out"] != IGN, kept) and torch.equal(ref["labels_out"][kept], labels[kept])
    assert ref["k"] == min(K, ref["n_valid"] - 1)


def test_rule_edge_cases():
    labels = torch.tensor([0, 1, IGN, 5, -3])
    loss = torch.tensor([0.5, 0.5, 9.0, 9.0, 9.0])
    r = R.ohem_rule(loss, labels, 2, IGN, 1e-6, 0)          # the pivot and its tie are dropped
    assert r["n_valid"] == 2 and r["k"] == 0 and not bool(r["kept"].any())
    r = R.ohem_rule(loss, labels, 2, IGN, 0.7, 10)          # the threshold binds: both are above -log(0.7)
    assert r["kept"].tolist() == [True, True, False, False, False] and float(r["L_eff"]) == float(R.tau32(0.7))
    r = R.ohem_rule(loss, torch.full((5,), IGN), 2, IGN, 0.7, 3)
    assert r["n_valid"] == 0 and r["k"] == -1 and float(r["L"]) == float("inf") and not bool(r["kept"].any())


def test_constructor_validation():
    c = N.OhemCrossEntropyLoss()
    assert isinstance(c, N.CrossEntropyLoss) and (c.thresh, c.min_kept, c.ignore_index, c.reduction) == (0.7, 100_000, IGN, "mean")
    assert c.ohem == (0.7, 100_000) and c.last_info is None
    w = torch.rand(7)
    c = N.OhemCrossEntropyLoss(0.9, 0, weight=w, ignore_index=255, reduction="sum", label_smoothing=0.1)
    assert c.weight is w and (c.ignore_index, c.reduction, c.label_smoothing) == (255, "sum", 0.1)
    assert list(c.state_dict().keys()) == list(nn.CrossEntropyLoss(weight=w).state_dict().keys())
    with pytest.raises(ValueError, match="reduction='none'"):
        N.OhemCrossEntropyLoss(reduction="none")
    for bad in (0.0, -0.1, 1.5, float("nan"), None, "0.7", True):
        with pytest.raises(ValueError, match="thresh"):
            N.OhemCrossEntropyLoss(thresh=bad)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="min_kept"):
            N.OhemCrossEntropyLoss(min_kept=bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        N.OhemCrossEntropyLoss(label_smoothing=2.0)


def test_module_refuses_cpu_tensors_while_training():
    c = N.OhemCrossEntropyLoss(min_kept=4)
    with pytest.raises(RuntimeError):
        c(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


class _CpuModel(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so reaching that error proves the criterion guards passed."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", ohem=None):
        raise AssertionError("not reached")


class _NoOhemModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean"):
        raise AssertionError("not reached")


def test_trainstep_accepts_the_criterion_and_keeps_its_guards():
    from lc2is_amd.step import TrainStep
    with pytest.raises(RuntimeError):                      # accepted: the arena is what refuses a CPU model
        TrainStep(_CpuModel(), criterion=N.OhemCrossEntropyLoss(min_kept=16))
    crit = N.OhemCrossEntropyLoss(min_kept=16)
    crit.reduction = "none"
    with pytest.raises(ValueError, match="reduction='none'"):
        TrainStep(_CpuModel(), criterion=crit)
    with pytest.raises(ValueError, match="ignore_index"):
        TrainStep(_CpuModel(), criterion=N.OhemCrossEntropyLoss(), ignore_index=0)
    with pytest.raises(TypeError, match="ohem"):          # a model whose fused head does not select (the compose models)
        TrainStep(_NoOhemModel(), criterion=N.OhemCrossEntropyLoss())


def test_fused_sites_validate_ohem_before_running():
    import inspect
    from lc2is_amd.nn.model import fused_loss_options
    assert fused_loss_options(None, 0.0, "mean") is None    # unchanged without ohem
    assert inspect.signature(N.BaseModelWithText.forward_loss).parameters["ohem"].default is None
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="thresh"):
        tail.loss(*args, ohem=(0.0, 4))
    with pytest.raises(ValueError, match="min_kept"):
        tail.loss(*args, ohem=(0.7, -1))


def test_entry_points_refuse_bad_arguments_without_touching_a_gpu():
    from lc2is_amd import ops
    P = 0x1000   # (16-byte aligned; never dereferenced)
    px = ops._fn("lc2is_head_upsample_px")
    assert px(None, 64, P, P, 1, 2, 2, 5, 4, 0, IGN, None) == -2
    assert px(P, 64, None, P, 1, 2, 2, 5, 4, 0, IGN, None) == -2
    assert px(P, 64, P, None, 1, 2, 2, 5, 4, 0, IGN, None) == -2
    assert px(P, 60, P, P, 1, 2, 2, 5, 4, 0, IGN, None) == -1      # ld not a multiple of 64
    assert px(P, 64, P, P, 1, 2, 2, 65, 4, 0, IGN, None) == -1     # C > ld
    assert px(P, 64, P, P, 0, 2, 2, 5, 4, 0, IGN, None) == -1
    assert px(P, 64, P, P, 1, 2, 2, 5, 5, 0, IGN, None) == -3      # S outside 4 / 8 / 16
    assert px(P, 64, P, P, 1, 2, 2, 5, 32, 0, IGN, None) == -3
    assert px(P, 64, P, P, 1, 2, 2, 5, 4, 7, IGN, None) == -3      # unknown mode
    sel = ops._fn("lc2is_ohem_select")
    ok = dict(loss=P, labels=P, out=P, n=100, C=5, ign=IGN, tau=0.3, K=10, info=P, ws=P, wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return sel(a["loss"], a["labels"], a["out"], a["n"], a["C"], a["ign"], a["tau"], a["K"], a["info"], a["ws"], a["wsb"], None)

    for name in ("loss", "labels", "out", "info", "ws"):
        assert call(**{name: None}) == -2, name
    assert call(n=0) == -1 and call(n=-5) == -1 and call(n=1 << 31) == -1
    assert call(C=0) == -1 and call(K=-1) == -1 and call(tau=-0.5) == -1 and call(tau=float("nan")) == -1
    assert call(loss=P + 4) == -1 and call(out=P + 8) == -1        # 16-byte alignment
    assert call(wsb=ops._fn("lc2is_ohem_select_workspace_bytes")(100) - 1) == -4


def test_workspace_query_is_a_pure_host_function():
    from lc2is_amd import ops
    q = ops._fn("lc2is_ohem_select_workspace_bytes")
    fixed = q(4)
    assert fixed == 64 + 512 * 256 * 4 + 16
    assert q(1) == fixed and q(5) == fixed + 16 and q(32 * 512 * 512) == fixed - 16 + 4 * 32 * 512 * 512
    assert q(0) == 0 and q(-1) == 0 and q(1 << 31) == 0 and q((1 << 31) - 1) > 0


def test_python_wrappers_refuse_cpu_tensors_and_bad_settings():
    from lc2is_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ohem_select(torch.zeros(8), torch.zeros(8, dtype=torch.long), 3, 0.7, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_px(torch.zeros(4, 64), torch.zeros(1, 8, 8, dtype=torch.long), 1, 2, 2, 5, 4)
    with pytest.raises(ValueError, match="thresh"):
        ops.ohem_loss_thresh(0.0)
    assert ops.ohem_loss_thresh(1.0) == 0.0 and ops.ohem_loss_thresh(0.7) == float(R.tau32(0.7))
