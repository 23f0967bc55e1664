"""CPU checks of the distillation pieces: the fp64 reference the GPU tests rest on agrees with autograd of torch's own kl_div and its
KL sums are large against their bounds; the entry point is declared with a `replaces:` note, bound, exported and refuses bad
arguments before any launch; ops, head_criterion, the loss methods and TrainStep refuse what they must before anything runs."""
import inspect
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distill_ref as D  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402
from lc2is_amd import _lib, ops  # noqa: E402
from lc2is_amd.nn.head_loss import Distill, HeadCriterion, head_criterion  # noqa: E402
from lc2is_amd.step import TrainStep  # noqa: E402

IGN = D.IGN
NAME = "lc2is_head_upsample_kd"
P = 0x1000   # (16-byte aligned; never dereferenced)


class _Dev(torch.Tensor):   # a tensor that claims to be on the device: the checks behind _chk run, nothing is allocated
    is_cuda = True


# ---- the reference ----
@pytest.mark.parametrize("temp", D.TEMPS)
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_reference_gradient_is_autograd_of_kl_div(case, temp):
    B, h, w, S, mode, C = case
    lo, t, labels, pw = D.case_inputs(*case)
    for lab, weight in ((None, None), (labels, pw)):
        ref = D.kd_ref(lo, t, lab, weight, B, h, w, C, S, mode, temp)
        loss, grad = D.kd_autograd(lo, t, lab, weight, B, h, w, C, S, mode, temp)
        assert abs(ref["loss"].item() - loss.item()) <= 1e-10 * abs(loss.item())
        assert D.rel(ref["grad"], grad) <= 1e-10
        assert ref["count"] == (B * h * S * w * S if lab is None else int(D.S.counted(labels, C).sum()))


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_reference_kl_is_well_above_its_bound(case):
    """The independent teacher makes the T^2 KL O(1) per pixel (above 0.1 at both temperatures), so the relative figures of the GPU
    tests mean something: the bound is at most 1 % of the sum at T = 1 and at most 10 % at T = 4, where both softmaxes flatten
    towards uniform — the KL itself falls like 1 / T^2 while the two entropies it is the difference of rise towards log C."""
    for temp, factor in zip(D.TEMPS, (100.0, 10.0)):
        for weighted in (False, True):
            ref = D.case_ref(case, temp, weighted)
            assert ref["count"] > 0 and ref["loss"].item() / ref["count"] > 0.1
            assert ref["loss"].item() >= factor * D.LOSS_TOL * ref["scale"].item(), (temp, weighted)


def test_teacher_padding_differs_from_the_students():
    lo, t, _, _ = D.case_inputs(*D.CASES[0])
    C = D.CASES[0][-1]
    assert bool((lo[:, C:] == D.A.PAD_SCORE).all()) and bool((t[:, C:] == -D.A.PAD_SCORE).all()) and not torch.equal(lo[:, :C], t[:, :C])


# ---- the C entry point ----
def test_entry_point_is_declared_bound_and_exported():
    lib = _lib.load()
    assert NAME in _lib.header_symbols() and NAME in ops._ARGTYPES and hasattr(lib, NAME)
    assert len(ops._ARGTYPES[NAME]) == 19
    header = (Path(_lib.__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    sec = header[header.index("distillation on the fused head"):]
    assert "replaces:" in sec and "kl_div" in sec and sec.index("replaces:") < sec.index("int lc2is_head_upsample_kd(")
    src = (Path(_lib.__file__).resolve().parent / "csrc" / "head_distill.hip").read_text()
    assert "replaces:" in src and "head_kd_grp_kernel" in src and "scratch" in src and "VGPRs" in src


def test_entry_point_refuses_before_launching():
    f = ops._fn(NAME)
    ok = dict(lo=P, tlo=P + 64, ld=64, labels=P, pw=P, dlo=P, loss=P, B=1, h=2, w=2, C=5, S=4, mode=0, ign=IGN, temp=1.0, gs=1.0, ws=P,
              wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["tlo"], a["ld"], a["labels"], a["pw"], a["dlo"], a["loss"], a["B"], a["h"], a["w"], a["C"], a["S"],
                 a["mode"], a["ign"], a["temp"], a["gs"], a["ws"], a["wsb"], None)

    for k in ("lo", "tlo", "loss"):
        assert call(**{k: None}) == -2, k                                    # LC2IS_ERR_NULL
    assert call(C=193, ld=192) == -1 and call(C=65) == -1 and call(ld=60) == -1 and call(ld=256) == -1   # LC2IS_ERR_SHAPE
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1, dim
    assert call(lo=P + 4) == -1 and call(tlo=P + 8) == -1 and call(dlo=P + 4) == -1
    for t in (0.0, -1.0, float("nan"), float("inf")):
        assert call(temp=t) == -1, t
    assert call(S=2) == -3 and call(S=5) == -3 and call(mode=3) == -3        # LC2IS_ERR_UNSUPPORTED
    need = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(1, 2, 2, 5, 4, 0, 1)
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4   # LC2IS_ERR_WORKSPACE
    # the documented order: NULL, SHAPE, UNSUPPORTED, WORKSPACE
    assert call(lo=None, temp=0.0, S=2, ws=None) == -2 and call(temp=0.0, S=2, ws=None) == -1 and call(S=2, ws=None) == -3
    assert call(tlo=None, C=0, S=5, ws=None) == -2 and call(C=0, S=5, ws=None) == -1


# ---- ops ----
def test_ops_refuse_before_allocating():
    lo, teacher = torch.zeros(4, 64), torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_kd(lo, teacher, 1, 2, 2, 5, 4)
    fake = lo.as_subclass(_Dev)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="temperature"):
            ops.head_upsample_kd(fake, teacher, 1, 2, 2, 5, 4, temperature=bad)
    for bad, what in ((torch.zeros(4, 128), "shape"), (torch.zeros(5, 64), "shape"), (torch.zeros(4, 64, dtype=torch.float64), "float32"),
                      (torch.zeros(4, 64, requires_grad=True), "require grad"), (torch.zeros(4, 128)[:, ::2], "contiguous"),
                      (None, "float32")):
        with pytest.raises(ValueError, match=what):
            ops.head_upsample_kd(fake, bad, 1, 2, 2, 5, 4)
    with pytest.raises(ValueError, match="pixel_weight"):
        ops.head_upsample_kd(fake, teacher, 1, 2, 2, 5, 4, pixel_weight=torch.ones(1, 8, 7))
    with pytest.raises(RuntimeError, match="S must be"):
        ops.head_upsample_kd(fake, teacher, 1, 2, 2, 5, 2)
    with pytest.raises(RuntimeError, match="labels must be"):
        ops.head_upsample_kd(fake, teacher, 1, 2, 2, 5, 4, labels=torch.zeros(1, 8, 7, dtype=torch.long).as_subclass(_Dev))
    sig = inspect.signature(ops.head_upsample_kd).parameters
    assert list(sig)[:8] == ["scores_lo", "teacher_lo", "B", "h", "w", "C", "S", "mode"]
    keys = ("temperature", "labels", "pixel_weight", "want_grad", "ignore_index", "grad_scale")
    assert [sig[k].default for k in keys] == [1.0, None, None, False, -100, 1.0]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keys)


# ---- head_criterion ----
def test_head_criterion_validates_distill():
    t = torch.zeros(8, 192)
    assert HeadCriterion().distill is None and "distill" not in HeadCriterion._fields and len(HeadCriterion._fields) == 8
    assert Distill(t)[1:] == (1.0, 1.0, "all", None)
    c = head_criterion("t", distill=Distill(t, 0.5, 4, "labelled"))
    assert c.distill.scores is t and c.distill[1:] == (0.5, 4.0, "labelled", None)
    # the term rides beside the criterion's eight fields: the same tuple, the term-less criterion as .base
    assert isinstance(c, HeadCriterion) and tuple(c) == tuple(HeadCriterion()) and type(c.base) is HeadCriterion and c.base.distill is None
    assert c.plain_ce and head_criterion("t").distill is None and type(head_criterion("t")) is HeadCriterion
    assert head_criterion("t", distill=(t, 2)).distill[1:] == (2.0, 1.0, "all", None)     # a plain tuple is taken too
    # the term joins every base criterion
    for kw in (dict(), dict(weight=torch.ones(5), label_smoothing=0.1), dict(ohem=(0.7, 16)), dict(dice=(1.0, 1.0, 1.0, False)),
               dict(focal=(2.0, 0.0)), dict(sigmoid=(2.0, 0.25, "elements")), dict(pixel_weight=torch.ones(1, 8, 8))):
        assert head_criterion("t", distill=Distill(t), **kw).distill is not None
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="temperature"):
            head_criterion("t", distill=Distill(t, 1.0, bad))
    for bad in (-0.5, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="weight"):
            head_criterion("t", distill=Distill(t, bad))
    for bad in ("image", None, 0):
        with pytest.raises(ValueError, match="region"):
            head_criterion("t", distill=Distill(t, 1.0, 1.0, bad))
    with pytest.raises(NotImplementedError, match="accum"):
        head_criterion("t", distill=Distill(t), accum=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="192 classes"):
        head_criterion("t", distill=Distill(torch.zeros(8, 256)), n_classes=193, scale=4)
    assert head_criterion("t", n_classes=193, scale=4).distill is None      # the wide head itself is still taken
    # the teacher's tensor
    for bad, what in ((torch.zeros(8, 192, dtype=torch.float16), "float32"), (torch.zeros(8, 192, requires_grad=True), "require grad"),
                      (torch.zeros(8, 384)[:, ::2], "contiguous"), ([0.0], "float32")):
        with pytest.raises(ValueError, match=what):
            head_criterion("t", distill=Distill(bad))
    with pytest.raises(ValueError, match="contiguous"):
        head_criterion("t", distill=Distill(t), n_classes=151, scale=4, rows=16)                 # 8 rows given, 16 expected
    with pytest.raises(ValueError, match="contiguous"):
        head_criterion("t", distill=Distill(torch.zeros(16, 128)), n_classes=151, scale=4, rows=16)
    with pytest.raises(ValueError, match="must be on"):
        head_criterion("t", distill=Distill(t), n_classes=151, scale=4, rows=8, device=torch.device("meta"))
    with pytest.raises(ValueError, match="pixel_weight"):
        head_criterion("t", distill=Distill(t, pixel_weight=torch.ones(1, 8, 8, dtype=torch.float64)))
    with pytest.raises(ValueError, match="Distill"):
        head_criterion("t", distill=(t, 1.0, 1.0, "all", None, 7))


def test_loss_methods_refuse_before_a_tower_runs():
    """A bad distill= is refused by the three sites before anything of the model is touched (the receivers are bare objects)."""
    t = torch.zeros(8, 192)
    for cls in (N.BaseModelWithText, N.PromptFTN):
        assert "distill" in inspect.signature(cls.forward_loss).parameters
    assert "distill" in inspect.signature(N.ScoreMapTail.loss).parameters
    assert hasattr(N.BaseModelWithText, "head_scores") and hasattr(N.ScoreMapTail, "scores_lo")
    ftn = object.__new__(N.PromptFTN)
    with pytest.raises(ValueError, match="temperature"):
        N.PromptFTN.forward_loss(ftn, {}, None, distill=Distill(t, 1.0, 0.0))
    with pytest.raises(NotImplementedError, match="accum"):
        N.PromptFTN.forward_loss(ftn, {}, None, distill=Distill(t), accum=torch.zeros(4, dtype=torch.float64))
    tail = N.ScoreMapTail(4)
    ve, te = torch.zeros(1, 4, 64), torch.zeros(1, 5, 64)
    with pytest.raises(ValueError, match="region"):
        tail.loss(ve, te, None, distill=Distill(t, 1.0, 1.0, "some"))
    with pytest.raises(ValueError, match="contiguous"):
        tail.loss(ve, te, None, distill=Distill(t))                      # [8, 192] against the tail's [4, 192]
    with pytest.raises(NotImplementedError, match="192 classes"):
        tail.loss(ve, torch.zeros(1, 193, 64), None, distill=Distill(torch.zeros(4, 256)))


# ---- TrainStep ----
class _NoDistill:
    def forward_loss(self, inputs, labels, ignore_index=-100, *, pixel_weight=None):
        raise AssertionError("must not run")


class _Takes:
    def forward_loss(self, inputs, labels, ignore_index=-100, *, accum=None, distill=None):
        raise AssertionError("must not run")


def test_train_step_refuses_before_building_anything():
    sig = inspect.signature(TrainStep.step_distill).parameters
    assert list(sig)[1:] == ["inputs", "labels", "teacher_scores", "teacher_weight", "pixel_weight"]
    assert sig["teacher_scores"].default is inspect.Parameter.empty and sig["teacher_weight"].default is None
    sig = inspect.signature(TrainStep.capture_distill).parameters
    assert list(sig)[1:] == ["inputs", "labels", "teacher_scores", "teacher_weight", "warmup", "pixel_weight"] and sig["warmup"].default == 2
    assert inspect.signature(TrainStep.__init__).parameters["distill"].default is None
    with pytest.raises(NotImplementedError, match="accumulate"):
        TrainStep(_Takes(), distill=(1.0, 1.0, "all"), accumulate=2)
    with pytest.raises(TypeError, match="distill="):
        TrainStep(_NoDistill(), distill=(1.0, 1.0, "all"))
    for bad, what in (((1.0, 0.0, "all"), "temperature"), ((-1.0, 1.0, "all"), "weight"), ((1.0, 1.0, "x"), "region"),
                      ((1.0, 1.0), "distill must be"), (3.0, "distill must be")):
        with pytest.raises(ValueError, match=what):
            TrainStep(_Takes(), distill=bad)
    # the per-step tensors against how the step was built (the check reads nothing else)
    ts = object.__new__(TrainStep)
    ts._distill = (1.0, 1.0, "all")
    with pytest.raises(ValueError, match="teacher_scores"):
        ts._check_teacher("step", None, None)
    ts._check_teacher("step", torch.zeros(8, 192), None)
    ts._distill = None
    with pytest.raises(ValueError, match="distill="):
        ts._check_teacher("step", torch.zeros(8, 192), None)
    ts._check_teacher("step", None, None)
