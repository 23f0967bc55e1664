"""CPU checks of the head's class map / accuracy counts: the entry points are declared, bound and exported and refuse bad arguments
before any launch, the workspace formula, the Python refusals that happen before device work, the reference's counting rule on a
hand-counted case, and the condition the GPU comparison rests on: the fp64 reference alone leaves at most 1 % of a case's pixels
inside the near-tie margin."""
import ctypes as C
import inspect
import sys
from pathlib import Path

import pytest
import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_argmax_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402
from lc2is_amd import _lib, ops  # noqa: E402

IGN = R.IGN
NAMES = ("lc2is_head_upsample_argmax", "lc2is_head_upsample_argmax_workspace_bytes")


def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and name in ops._ARGTYPES and hasattr(lib, name)
    assert ops._fn(NAMES[1]).restype is C.c_size_t and ops._fn(NAMES[0]).restype is C.c_int
    assert len(ops._ARGTYPES[NAMES[0]]) == 15 and len(ops._ARGTYPES[NAMES[1]]) == 6
    header = (Path(_lib.__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    assert "replaces: model(inputs)[\"outputs\"].argmax(1)" in header


def test_c_entry_point_refuses_before_launching():
    f = ops._fn(NAMES[0])
    P = 0x1000   # (16-byte aligned; never dereferenced)
    ok = dict(lo=P, ld=64, labels=P, pred=P, counts=P, B=1, h=2, w=2, C=5, S=4, mode=0, ign=IGN, ws=P, wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["pred"], a["counts"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"], a["ign"],
                 a["ws"], a["wsb"], None)

    assert call(lo=None) == -2                                   # LC2IS_ERR_NULL
    assert call(pred=None, counts=None) == -2
    assert call(labels=None) == -2                               # counts without labels
    assert call(C=193, ld=192) == -1                             # LC2IS_ERR_SHAPE
    assert call(C=65) == -1 and call(ld=256, C=200) == -1 and call(ld=256) == -1 and call(ld=60) == -1
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1 and call(**{dim: -3}) == -1, dim
    assert call(lo=P + 4) == -1 and call(lo=P + 8) == -1         # misaligned scores
    for S in (0, 2, 5, 12, 32):
        assert call(S=S) == -3, S                                # LC2IS_ERR_UNSUPPORTED
    assert call(mode=7) == -3 and call(mode=-1) == -3
    need = ops._fn(NAMES[1])(1, 2, 2, 5, 4, 0)
    assert need > 0
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4 and call(wsb=0) == -4   # LC2IS_ERR_WORKSPACE
    # the order of the table: NULL before SHAPE before UNSUPPORTED before WORKSPACE
    assert call(lo=None, C=0, S=5, ws=None) == -2 and call(C=0, S=5, ws=None) == -1 and call(S=5, ws=None) == -3


def test_workspace_size_formula():
    q = ops._fn(NAMES[1])

    def want(B, h, w, Cn, S):
        tiles = -(-(h * S + S // 2) // 16) * -(-(w * S + S // 2) // 16)
        return B * tiles * 3 * ((Cn + 3) // 4 * 4) * 4

    for B, h, w, S, mode, Cn in R.CASES:
        assert q(B, h, w, Cn, S, 0 if mode == "bicubic" else 1) == want(B, h, w, Cn, S)
    assert q(32, 32, 32, 151, 4, 0) == want(32, 32, 32, 151, 4) == 32 * 81 * 3 * 152 * 4          # the headline step: 4.7 MB
    assert q(32, 128, 128, 151, 4, 0) == 32 * 33 * 33 * 3 * 152 * 4                               # 512 x 512 outputs: 63.6 MB
    assert q(2, 9, 9, 5, 4, 0) == q(2, 9, 9, 8, 4, 1) == q(2, 9, 9, 8, 4, 0)                      # cq, and no mode dependence
    for bad in ((0, 2, 2, 5, 4, 0), (1, 0, 2, 5, 4, 0), (1, 2, -1, 5, 4, 0), (1, 2, 2, 0, 4, 0), (1, 2, 2, 193, 4, 0),
                (1, 2, 2, 5, 5, 0), (1, 2, 2, 5, 32, 0), (1, 2, 2, 5, 4, 2)):
        assert q(*bad) == 0, bad


def test_op_refuses_before_allocating():
    lo, lab = torch.zeros(4, 64), torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_argmax(lo, lab, 1, 2, 2, 5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_argmax(lo, None, 1, 2, 2, 5, 4, want_counts=False)
    sig = inspect.signature(ops.head_upsample_argmax).parameters
    assert (sig["ignore_index"].default, sig["want_pred"].default, sig["want_counts"].default) == (-100, True, True)
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("ignore_index", "want_pred", "want_counts"))

    class _Dev(torch.Tensor):   # a tensor that claims to be on the device: the checks behind _chk run, nothing is allocated
        is_cuda = True

    fake = torch.zeros(4, 64).as_subclass(_Dev)
    with pytest.raises(ValueError, match="needs labels"):
        ops.head_upsample_argmax(fake, None, 1, 2, 2, 5, 4)
    with pytest.raises(ValueError, match="both False"):
        ops.head_upsample_argmax(fake, None, 1, 2, 2, 5, 4, want_pred=False, want_counts=False)


def test_seg_counts_argument_is_checked_before_the_towers_run():
    for bad, exc in ((torch.zeros(3, 151), TypeError), ([0], TypeError), (torch.zeros(3, 150, dtype=torch.long), ValueError),
                     (torch.zeros(151, 3, dtype=torch.long), ValueError), (torch.zeros(3, 151, dtype=torch.long), RuntimeError)):
        with pytest.raises(exc, match="seg_counts"):
            ops.check_seg_counts(bad, 151)
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    with pytest.raises(TypeError, match="seg_counts"):
        tail.loss(*args, seg_counts=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="seg_counts"):
        tail.loss(*args, seg_counts=torch.zeros(3, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="seg_counts"):   # a CPU buffer
        tail.loss(*args, seg_counts=torch.zeros(3, 3, dtype=torch.long))
    for cls in (N.BaseModelWithText, N.PromptFTN):
        assert inspect.signature(cls.forward_loss).parameters["seg_counts"].default is None and hasattr(cls, "predict")
    assert inspect.signature(N.ScoreMapTail.loss).parameters["seg_counts"].default is None and hasattr(N.ScoreMapTail, "predict")


class _CpuModel(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so reaching that error proves the seg_metrics guards passed."""

    def __init__(self, protos=True):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))
        if protos:
            self.class_prototypes = nn.Parameter(torch.zeros(7, 4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", seg_counts=None):
        raise AssertionError("not reached")


class _NoSegModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean"):
        raise AssertionError("not reached")


def test_trainstep_guards():
    from lc2is_amd.step import TrainStep
    with pytest.raises(TypeError, match="seg_counts"):      # like the OHEM and Dice guards: at construction
        TrainStep(_NoSegModel(), seg_metrics=True)
    with pytest.raises(RuntimeError):                       # accepted: the arena is what refuses a CPU model
        TrainStep(_CpuModel(), seg_metrics=True)
    with pytest.raises(RuntimeError):
        TrainStep(_CpuModel(protos=False), seg_metrics=True, seg_classes=150)
    with pytest.raises(ValueError, match="seg_classes"):    # no prototypes and no class count
        TrainStep(_CpuModel(protos=False), seg_metrics=True)
    with pytest.raises(ValueError, match="seg_classes"):
        TrainStep(_CpuModel(), seg_metrics=True, seg_classes=500)
    with pytest.raises(ValueError, match="seg_classes"):
        TrainStep(_CpuModel(), seg_classes=7)
    with pytest.raises(TypeError, match="seg_metrics"):
        TrainStep(_CpuModel(), seg_metrics=1)
    with pytest.raises(RuntimeError):                       # seg_metrics=False is today's constructor
        TrainStep(_NoSegModel())


def test_counting_rule_on_a_hand_counted_case():
    pred = torch.tensor([[[0, 0, 1, 1], [2, 2, 1, 0], [0, 1, 2, 2], [1, 1, 0, 0]]])
    lab = torch.tensor([[[0, 1, 1, IGN], [2, 3, -1, 0], [0, 0, 2, 1], [IGN, 1, 0, 2]]])
    c = R.counts(pred, lab, 3, IGN)
    assert c.tolist() == [[[4, 2, 2], [6, 3, 3], [5, 4, 3]]]           # 12 counted pixels: labels IGN, 3 and -1 add nothing
    assert int(c[0, 1].sum()) == int(c[0, 2].sum()) == int(R.counted(lab, 3, IGN).sum()) == 12
    c0 = R.counts(pred, lab, 3, 0)                                     # class 0 ignored: its pixels leave all three rows
    assert c0.tolist() == [[[0, 2, 2], [2, 2, 3], [0, 4, 3]]]
    from lc2is_amd.metrics import dataset_iou
    m = dataset_iou(c[0], None)
    assert float(m["aAcc"]) == 8 / 12 and float(m["mAcc"]) == pytest.approx((4 / 5 + 2 / 4 + 2 / 3) / 3)
    assert float(m["mIoU"]) == pytest.approx((4 / 7 + 2 / 5 + 2 / 4) / 3)


def test_reference_ties_go_to_the_lowest_class():
    lo = torch.zeros(4, 192)
    lo[:, :151] = torch.randn(4, 151, generator=torch.Generator().manual_seed(1))
    lo[:, 100] = lo[:, 3]
    lo[:, [3, 100]] += 10
    arg, gap = R.ref_argmax(lo, 1, 2, 2, 151, 4, "bicubic")
    assert bool((arg == 3).all()) and bool((gap == 0).all())


@pytest.mark.parametrize("B,h,w,S,mode,Cn", R.CASES)
def test_reference_alone_excludes_few_pixels(B, h, w, S, mode, Cn):
    """The GPU test compares only pixels whose fp64 top-2 gap exceeds the margin; for exactly its inputs the excluded share stays
    within the cap (and within 0.4 % at twice the margin)."""
    lo, labels = R.case_inputs(B, h, w, S, mode, Cn)
    arg, sure, gap = R.case_ref(B, h, w, S, mode, Cn)
    assert arg.shape == labels.shape == (B, h * S, w * S) and int(arg.max()) < Cn
    share = 1.0 - sure.double().mean().item()
    share2 = (gap <= 2 * R.MARGIN * lo[:, :Cn].abs().max().item()).double().mean().item()
    print("head argmax reference excluded share", (B, h, w, S, mode, Cn), share, share2)
    assert share <= R.MAX_EXCLUDED and share2 <= 0.004
    # the labels hold every kind the rule names
    assert bool((labels == IGN).any()) and bool((labels < 0).any()) and bool((labels >= Cn).any()) and bool((labels == 0).any())
