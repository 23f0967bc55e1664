"""CPU checks of the cross-entropy options (class weights, label smoothing, reductions): constructors, the legacy
size_average / reduce mapping, state_dict keys against nn.CrossEntropyLoss, and the refusals that happen before any GPU work."""
import pytest
import torch
from torch import nn

import lc2is_amd.nn as N


@pytest.mark.parametrize("cls", [N.CrossEntropyLoss, N.AuxiliaryLoss])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("weighted", [False, True])
def test_constructor_and_state_dict_match_torch(cls, reduction, weighted):
    w = torch.rand(151) + 0.5 if weighted else None
    ref = nn.CrossEntropyLoss(weight=w, ignore_index=3, reduction=reduction, label_smoothing=0.1)
    if cls is N.AuxiliaryLoss and reduction == "none":
        with pytest.raises(NotImplementedError, match="reduction='none'"):
            cls(weight=w, ignore_index=3, reduction=reduction, label_smoothing=0.1)
        return
    m = cls(weight=w, ignore_index=3, reduction=reduction, label_smoothing=0.1)
    assert (m.ignore_index, m.reduction, m.label_smoothing) == (3, reduction, 0.1)
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in ref.named_buffers()]
    if weighted:
        assert m.weight is w and torch.equal(m.state_dict()["weight"], ref.state_dict()["weight"])
    else:
        assert m.weight is None
    # a state_dict of torch's module loads into ours and back
    m.load_state_dict(ref.state_dict())
    ref.load_state_dict(m.state_dict())


@pytest.mark.parametrize("size_average,reduce", [(None, False), (True, None), (False, None), (False, True), (True, False),
                                                 (None, True)])
def test_legacy_reduction_arguments_map_like_torch(size_average, reduce):
    with pytest.warns(UserWarning):
        ref = nn.CrossEntropyLoss(size_average=size_average, reduce=reduce)
    with pytest.warns(UserWarning):   # (torch's own deprecation warning, from the same mapping)
        m = N.CrossEntropyLoss(size_average=size_average, reduce=reduce)
    assert m.reduction == ref.reduction


def test_invalid_arguments_raise_at_construction():
    with pytest.raises(ValueError, match="not a valid value for reduction"):
        N.CrossEntropyLoss(reduction="avg")
    with pytest.raises(ValueError, match="not a valid value for reduction"):
        N.AuxiliaryLoss(reduction="elementwise")
    with pytest.raises(ValueError, match="label_smoothing"):
        N.CrossEntropyLoss(label_smoothing=1.5)
    with pytest.raises(NotImplementedError):
        N.ContrastiveLoss(label_smoothing=0.1)   # (out of scope: probability targets)


def test_default_module_keeps_its_state_dict():
    assert list(N.CrossEntropyLoss().state_dict().keys()) == list(nn.CrossEntropyLoss().state_dict().keys()) == []


def test_fused_heads_refuse_reduction_none_before_running():
    from lc2is_amd.nn.model import fused_loss_options
    assert fused_loss_options(None, 0.0, "mean") is None
    w = torch.ones(3)
    assert fused_loss_options(w, 0.1, "sum") == (w, 0.1, "sum")
    with pytest.raises(NotImplementedError):
        fused_loss_options(None, 0.0, "none")
    with pytest.raises(ValueError):
        fused_loss_options(None, 0.0, "bad")
    with pytest.raises(ValueError):
        fused_loss_options(None, -0.1, "mean")
    tail = N.ScoreMapTail(4)
    with pytest.raises(NotImplementedError):
        tail.loss(torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long), reduction="none")


class _NoArena(nn.Module):
    """A model the ParamArena would be built from: the checks must fire before it is touched."""

    def __init__(self):
        super().__init__()
        self.p = nn.Parameter(torch.zeros(4))
        self.touched = False

    def parameters(self, recurse=True):
        self.touched = True
        return super().parameters(recurse)


def test_trainstep_refuses_criterion_conflicts_before_building_anything():
    from lc2is_amd.step import TrainStep
    m = _NoArena()
    with pytest.raises(ValueError, match="ignore_index"):
        TrainStep(m, criterion=N.CrossEntropyLoss(weight=torch.ones(4)), ignore_index=0)
    with pytest.raises(ValueError, match="reduction='none'"):
        TrainStep(m, criterion=N.CrossEntropyLoss(reduction="none"))
    with pytest.raises(TypeError):
        TrainStep(m, criterion=N.AuxiliaryLoss())
    assert not m.touched


def test_launchers_validate_options_on_the_host():
    from lc2is_amd import ops
    f = ops._fn("lc2is_head_upsample_ce_opts")
    # label smoothing outside [0, 1] is refused before any launch (pointers are never dereferenced)
    assert f(0x1000, 64, 0x1000, None, None, 0x1000, 1, 4, 4, 10, 4, 0, -100, 1.0, None, 1.5, 0x1000, 1 << 20, None) == -1
    # options on the atomic (S >= 32) path: unsupported
    assert f(0x1000, 64, 0x1000, None, None, 0x1000, 1, 4, 4, 10, 32, 0, -100, 1.0, None, 0.1, None, 0, None) == -3
    assert ops._fn("lc2is_ce_nchw_fwd_opts")(0x1000, 0x1000, None, 0x1000, None, 1, 10, 16, -100, None, -0.5, None) == -1
    assert ops._fn("lc2is_ce_nchw_bwd_opts")(0x1000, 0x1000, 0x1000, None, 1.0, None, 0x1000, 1, 10, 16, -100, None,
                                             2.0, None) == -1
