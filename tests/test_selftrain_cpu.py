"""CPU checks of the self-training pieces: the three entry points are declared with a `replaces:` note, bound and exported and refuse
bad arguments before any launch; the Python layers refuse before a tower runs; the new keywords sit where the issue puts them; and
the fp64 reference the GPU tests rest on is self-consistent and meets the condition on its excluded pixels."""
import ctypes as C
import inspect
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import selftrain_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402
from lc2is_amd import _lib, ops, selftrain  # noqa: E402
from lc2is_amd.nn.head_loss import HeadCriterion, head_criterion  # noqa: E402
from lc2is_amd.step import TrainStep  # noqa: E402

IGN = R.IGN
NAMES = ("lc2is_head_upsample_conf", "lc2is_head_upsample_conf_workspace_bytes", "lc2is_head_upsample_ce_pw")
P = 0x1000   # (16-byte aligned; never dereferenced)


class _Dev(torch.Tensor):   # a tensor that claims to be on the device: the checks behind _chk run, nothing is allocated
    is_cuda = True


def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and name in ops._ARGTYPES and hasattr(lib, name)
    assert ops._fn(NAMES[1]).restype is C.c_size_t and ops._fn(NAMES[0]).restype is C.c_int and ops._fn(NAMES[2]).restype is C.c_int
    assert [len(ops._ARGTYPES[n]) for n in NAMES] == [17, 6, 19]
    header = (Path(_lib.__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    sec = header[header.index("self-training on the fused head"):]
    assert sec.count("replaces:") == 2 and "softmax(1).max(1)" in sec and "reduction='none'" in sec
    assert sec.index("replaces:") < sec.index("size_t lc2is_head_upsample_conf_workspace_bytes(")
    src = (Path(_lib.__file__).resolve().parent / "csrc" / "head_selftrain.hip").read_text()
    assert "replaces:" in src and "head_conf_grp_kernel" in src and "head_ce_pw_grp_kernel" in src


def test_conf_entry_point_refuses_before_launching():
    f = ops._fn(NAMES[0])
    ok = dict(lo=P, ld=64, pred=P, conf=P, pseudo=P, counts=P, B=1, h=2, w=2, C=5, S=4, mode=0, t=0.5, ign=IGN, ws=P, wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["pred"], a["conf"], a["pseudo"], a["counts"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"],
                 a["t"], a["ign"], a["ws"], a["wsb"], None)

    assert call(lo=None) == -2                                               # LC2IS_ERR_NULL
    assert call(pred=None, conf=None, pseudo=None, counts=None) == -2        # nothing requested
    assert call(C=193, ld=192) == -1 and call(C=65) == -1 and call(ld=256) == -1 and call(ld=60) == -1   # LC2IS_ERR_SHAPE
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1 and call(**{dim: -3}) == -1, dim
    assert call(lo=P + 4) == -1
    for t in (-0.1, 1.5, float("nan"), float("inf")):
        assert call(t=t) == -1, t
    for S in (0, 2, 5, 32):
        assert call(S=S) == -3, S                                            # LC2IS_ERR_UNSUPPORTED
    assert call(mode=7) == -3
    need = ops._fn(NAMES[1])(1, 2, 2, 5, 4, 0)
    assert need == 1 * 1 * 2 * 4                                             # one tile, {kept, inside} int32
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4   # LC2IS_ERR_WORKSPACE
    # the ends of the threshold range pass the argument checks (the refusal that follows is the workspace's)
    assert call(t=0.0, ws=None) == -4 and call(t=1.0, ws=None) == -4
    assert call(lo=None, C=0, S=5, ws=None) == -2 and call(C=0, S=5, ws=None) == -1 and call(S=5, ws=None) == -3


def test_conf_workspace_size_formula():
    q = ops._fn(NAMES[1])
    for B, h, w, S, mode, Cn in R.CASES:
        tiles = -(-(h * S + S // 2) // 16) * -(-(w * S + S // 2) // 16)
        assert q(B, h, w, Cn, S, 0 if mode == "bicubic" else 1) == B * tiles * 2 * 4
    for bad in ((0, 2, 2, 5, 4, 0), (1, 2, 2, 0, 4, 0), (1, 2, 2, 193, 4, 0), (1, 2, 2, 5, 5, 0), (1, 2, 2, 5, 4, 2)):
        assert q(*bad) == 0, bad


def test_ce_pw_entry_point_refuses_before_launching():
    f = ops._fn(NAMES[2])
    ok = dict(lo=P, ld=64, labels=P, pw=P, dlo=P, loss=P, B=1, h=2, w=2, C=5, S=4, mode=0, ign=IGN, gs=1.0, cw=None, eps=0.0, ws=P,
              wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["pw"], a["dlo"], a["loss"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"],
                 a["ign"], a["gs"], a["cw"], a["eps"], a["ws"], a["wsb"], None)

    for k in ("lo", "labels", "pw", "loss"):
        assert call(**{k: None}) == -2, k                                    # LC2IS_ERR_NULL
    assert call(C=193, ld=192) == -1 and call(C=65) == -1 and call(ld=60) == -1 and call(B=0) == -1   # LC2IS_ERR_SHAPE
    assert call(lo=P + 4) == -1 and call(dlo=P + 8) == -1
    assert call(eps=-0.1) == -1 and call(eps=1.5) == -1 and call(eps=float("nan")) == -1
    assert call(S=5) == -3 and call(mode=3) == -3                            # LC2IS_ERR_UNSUPPORTED
    need = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(1, 2, 2, 5, 4, 0, 1)
    assert call(ws=None) == -4 and call(wsb=need - 1) == -4                  # LC2IS_ERR_WORKSPACE
    assert call(lo=None, C=0, S=5, ws=None) == -2 and call(C=0, S=5, ws=None) == -1 and call(S=5, ws=None) == -3


def test_ops_refuse_before_allocating():
    lo, lab, pw = torch.zeros(4, 64), torch.zeros(1, 8, 8, dtype=torch.long), torch.ones(1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_conf(lo, 1, 2, 2, 5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_ce_pw(lo, lab, pw, 1, 2, 2, 5, 4)
    fake = torch.zeros(4, 64).as_subclass(_Dev)
    fake_lab = lab.as_subclass(_Dev)
    for bad in (-0.1, 1.01, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="threshold"):
            ops.head_upsample_conf(fake, 1, 2, 2, 5, 4, thresh=bad)
    with pytest.raises(ValueError, match="nothing requested"):
        ops.head_upsample_conf(fake, 1, 2, 2, 5, 4, want_pred=False, want_conf=False)
    with pytest.raises(ValueError, match="needs thresh"):
        ops.head_upsample_conf(fake, 1, 2, 2, 5, 4, want_counts=True)
    with pytest.raises(RuntimeError, match="S must be"):
        ops.head_upsample_conf(fake, 1, 2, 2, 5, 32)
    with pytest.raises(RuntimeError, match="scores_lo must be"):
        ops.head_upsample_conf(torch.zeros(4, 256).as_subclass(_Dev), 1, 2, 2, 200, 4)
    for bad, what in ((torch.ones(1, 8, 7), "shape"), (torch.ones(8, 8), "shape"), (torch.ones(1, 8, 8, dtype=torch.float64), "float32"),
                      (torch.ones(1, 8, 8, requires_grad=True), "require grad"), (torch.ones(1, 8, 16)[:, :, ::2], "contiguous"),
                      (None, "float32")):
        with pytest.raises(ValueError, match=what):
            ops.head_upsample_ce_pw(fake, fake_lab, bad, 1, 2, 2, 5, 4)
    with pytest.raises(RuntimeError, match="label_smoothing"):
        ops.head_upsample_ce_pw(fake, fake_lab, pw, 1, 2, 2, 5, 4, label_smoothing=1.5)
    sig = inspect.signature(ops.head_upsample_conf).parameters
    assert [sig[k].default for k in ("thresh", "ignore_index", "want_pred", "want_conf", "want_counts")] == [None, -100, True, True, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("thresh", "ignore_index", "want_pred", "want_conf", "want_counts"))
    sig = inspect.signature(ops.head_upsample_ce_pw).parameters
    assert list(sig)[:3] == ["scores_lo", "labels", "pixel_weight"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("want_grad", "ignore_index", "grad_scale", "class_weight",
                                                                        "label_smoothing"))


def test_head_criterion_validates_pixel_weight():
    pw = torch.ones(1, 8, 8)
    for kw in (dict(ohem=(0.7, 16)), dict(dice=(1.0, 1.0, 1.0, True)), dict(focal=(2.0, 0.0)), dict(sigmoid=(2.0, 0.25, "elements"))):
        with pytest.raises(ValueError, match="pixel_weight"):
            head_criterion("test", pixel_weight=pw, n_classes=151, scale=4, **kw)
    with pytest.raises(ValueError, match="require grad"):
        head_criterion("test", pixel_weight=torch.ones(1, 8, 8, requires_grad=True), n_classes=151, scale=4)
    with pytest.raises(ValueError, match="float32"):
        head_criterion("test", pixel_weight=torch.ones(1, 8, 8, dtype=torch.float16), n_classes=151, scale=4)
    with pytest.raises(NotImplementedError, match="192"):
        head_criterion("test", pixel_weight=pw, n_classes=193, scale=4)
    with pytest.raises(NotImplementedError, match="192"):
        head_criterion("test", pixel_weight=pw, n_classes=lambda: 193, scale=4)
    with pytest.raises(NotImplementedError, match="reduction='none'"):
        head_criterion("test", pixel_weight=pw, n_classes=151, scale=4, reduction="none")
    crit = head_criterion("test", pixel_weight=pw, n_classes=192, scale=4, label_smoothing=0.1, reduction="sum")
    assert crit.pixel_weight is pw and not crit.plain_ce and crit[-1] is pw
    assert not head_criterion("test", pixel_weight=pw).plain_ce and head_criterion("test").plain_ce
    # the default criterion keeps its first seven fields, and positional constructions keep working
    assert tuple(HeadCriterion())[:7] == (None, 0.0, "mean", None, None, None, None) and HeadCriterion().pixel_weight is None
    assert HeadCriterion._fields[-1] == "pixel_weight" and len(HeadCriterion._fields) == 8
    assert HeadCriterion(None, 0.1, "sum", None, None, (2.0, 0.0), None).focal == (2.0, 0.0)


def test_loss_methods_refuse_before_a_tower_runs():
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="pixel_weight"):
        tail.loss(*args, pixel_weight=torch.ones(1, 8, 8), focal=(2.0, 0.0))
    with pytest.raises(ValueError, match="float32"):
        tail.loss(*args, pixel_weight=torch.ones(1, 8, 8, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="192"):
        tail.loss(torch.zeros(1, 4, 64), torch.zeros(1, 193, 64), args[2], pixel_weight=torch.ones(1, 8, 8))
    with pytest.raises(NotImplementedError, match="192"):
        tail.predict_confidence(torch.zeros(1, 4, 64), torch.zeros(1, 193, 64))
    with pytest.raises(ValueError, match="threshold"):
        tail.predict_confidence(args[0], args[1], thresh=2.0)
    for cls, name in ((N.BaseModelWithText, "forward_loss"), (N.ScoreMapTail, "loss"), (N.PromptFTN, "forward_loss")):
        par = inspect.signature(getattr(cls, name)).parameters["pixel_weight"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None, cls
    for cls in (N.BaseModelWithText, N.ScoreMapTail):
        sig = inspect.signature(cls.predict_confidence).parameters
        assert sig["thresh"].default is None and sig["ignore_index"].default == -100


def test_train_step_signatures():
    sig = inspect.signature(TrainStep.step).parameters
    assert list(sig) == ["self", "inputs", "labels", "pixel_weight"] and sig["pixel_weight"].default is None
    sig = inspect.signature(TrainStep.capture).parameters
    assert list(sig) == ["self", "inputs", "labels", "warmup", "pixel_weight"]
    assert sig["warmup"].default == 2 and sig["pixel_weight"].default is None


class _NoPw:
    def forward_loss(self, inputs, labels, ignore_index=-100):
        raise AssertionError("never reached")


def test_train_step_refuses_pixel_weight_it_cannot_honour():
    from lc2is_amd.step import _accepts
    assert _accepts(N.BaseModelWithText, "pixel_weight") and _accepts(N.PromptFTN, "pixel_weight") and not _accepts(_NoPw(), "pixel_weight")
    ts = object.__new__(TrainStep)   # the refusal reads the model and the criterion only
    ts.model, ts.criterion, ts._ohem, ts._dice = _NoPw(), None, False, False
    with pytest.raises(TypeError, match="pixel_weight"):
        ts._check_pixel_weight("step")
    ts.model = N.ScoreMapTail(4)   # (no forward_loss either)
    with pytest.raises(TypeError, match="pixel_weight"):
        ts._check_pixel_weight("capture")

    class _Takes:
        def forward_loss(self, inputs, labels, ignore_index=-100, *, pixel_weight=None):
            raise AssertionError("never reached")

    ts.model = _Takes()
    ts._check_pixel_weight("step")
    for crit, ohem, dice in ((N.FocalLoss(), False, False), (N.SigmoidFocalLoss(), False, False),
                             (N.OhemCrossEntropyLoss(0.7, 16), True, False), (N.DiceCrossEntropyLoss(), False, True)):
        ts.criterion, ts._ohem, ts._dice = crit, ohem, dice
        with pytest.raises(ValueError, match="pixel_weight"):
            ts._check_pixel_weight("step")
    ts.criterion, ts._ohem, ts._dice = N.CrossEntropyLoss(label_smoothing=0.1), False, False
    ts._check_pixel_weight("step")


def test_pseudo_labeler_arguments_and_combine():
    class _M:
        def predict_confidence(self, inputs, thresh=None, ignore_index=-100):
            conf = torch.tensor([[[0.99, 0.5], [0.97, 0.2]], [[0.1, 0.2], [0.3, 0.98]]])
            pred = torch.tensor([[[3, 1], [2, 0]], [[1, 1], [4, 5]]], dtype=torch.uint8)
            kept = conf >= thresh
            pseudo = torch.where(kept, pred.long(), torch.full_like(pred, 0, dtype=torch.long) + ignore_index)
            counts = torch.stack([kept.flatten(1).sum(1), torch.full((2,), 4)], 1).int()
            return pred, conf, pseudo, counts

    with pytest.raises(TypeError, match="predict_confidence"):
        selftrain.PseudoLabeler(object())
    with pytest.raises(ValueError, match="weight"):
        selftrain.PseudoLabeler(_M(), weight="soft")
    with pytest.raises(ValueError, match="threshold"):
        selftrain.PseudoLabeler(_M(), threshold=1.5)
    sig = inspect.signature(selftrain.PseudoLabeler.__init__).parameters
    assert (sig["threshold"].default, sig["weight"].default, sig["ignore_index"].default) == (0.968, "quality", -100)
    lab, pw, counts = selftrain.PseudoLabeler(_M(), weight="quality")(None)
    assert lab.tolist() == [[[3, IGN], [2, IGN]], [[IGN, IGN], [IGN, 5]]] and counts.tolist() == [[2, 4], [1, 4]]
    assert pw.dtype == torch.float32 and pw.is_contiguous() and torch.equal(pw, torch.tensor([0.5, 0.25]).view(2, 1, 1).expand(2, 2, 2))
    lab2, pw2, _ = selftrain.PseudoLabeler(_M(), weight="confidence")(None)
    assert torch.equal(lab2, lab) and pw2.tolist() == [[[pytest.approx(0.99), 0.0], [pytest.approx(0.97), 0.0]],
                                                       [[0.0, 0.0], [0.0, pytest.approx(0.98)]]]
    assert selftrain.PseudoLabeler(_M(), weight=None)(None)[1] is None
    ids = torch.zeros(3, 8, dtype=torch.long)
    a = ({"pixel_values": torch.zeros(1, 3, 4, 4), "input_ids": ids[:1]}, torch.zeros(1, 2, 2, dtype=torch.long))
    b = ({"pixel_values": torch.ones(2, 3, 4, 4), "input_ids": ids[1:]}, lab, pw)
    inputs, labels, weight = selftrain.PseudoLabeler.combine(labelled=a, pseudo=b)
    assert tuple(inputs["pixel_values"].shape) == (3, 3, 4, 4) and tuple(inputs["input_ids"].shape) == (3, 8)
    assert torch.equal(labels[1:], lab) and not labels[0].any()
    assert torch.equal(weight[0], torch.ones(2, 2)) and torch.equal(weight[1:], pw) and weight.is_contiguous()
    assert torch.equal(selftrain.PseudoLabeler.combine(a, (b[0], lab, None))[2], torch.ones(3, 2, 2))
    with pytest.raises(ValueError, match="different inputs"):
        selftrain.PseudoLabeler.combine(a, ({"pixel_values": b[0]["pixel_values"]}, lab, pw))


# ---- the reference ----
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_reference_excludes_at_most_one_percent(case):
    """The condition of the GPU comparison: the tie margin and the threshold band leave out at most 1 % of a case's pixels, and the
    median threshold populates both sides."""
    ref = R.conf_ref(*case)
    ex_tie, ex_all = R.excluded_share(ref["sure"]), R.excluded_share(ref["sure_t"])
    print("selftrain reference figures", case, "thresh", ref["thresh"], "excluded by ties", ex_tie, "with the threshold band", ex_all,
          "kept share", ref["kept"].double().mean().item())
    assert ex_tie <= ex_all <= R.MAX_EXCLUDED
    assert 0.0 < ref["thresh"] < 1.0 and 0.3 <= ref["kept"].double().mean().item() <= 0.7
    assert bool((ref["conf"] > 0).all()) and bool((ref["conf"] <= 1).all())
    assert torch.equal(ref["pseudo"] != IGN, ref["kept"]) and torch.equal(ref["pseudo"][ref["kept"]], ref["arg"][ref["kept"]])


@pytest.mark.parametrize("variant", R.CE_VARIANTS)
@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[5], R.CASES[9], R.CASES[15], R.CASES[18], R.CASES[27]], ids=R.case_id)
def test_reference_is_self_consistent(case, variant):
    B, h, w, S, mode, Cn = case
    lo, labels, pw = R.case_inputs(*case)
    weight, eps = R.variant_options(variant, Cn)
    geom = (B, h, w, Cn, S, mode)
    loss, wsum, grad = R.ce_pw_ref(lo, labels, pw, *geom, weight, eps)
    loss_a, wsum_a, grad_a = R.ce_pw_autograd(lo, labels, pw, *geom, weight, eps)
    print("selftrain reference figures", case, variant, loss.item(), loss_a.item(), wsum.item(), R.rel(grad, grad_a))
    assert abs(loss.item() - loss_a.item()) <= 1e-12 * abs(loss_a.item()) and wsum.item() == wsum_a.item()
    assert R.rel(grad, grad_a) <= 1e-12 and bool(grad.any())
    # pw == 1: F.cross_entropy's sum and (through the weight sum) its mean
    ones = torch.ones_like(pw)
    loss1, wsum1, _ = R.ce_pw_ref(lo, labels, ones, *geom, weight, eps, want_grad=False)
    hi = R.upsample64(lo, *geom)
    lab = torch.where(R.counted(labels, Cn), labels, torch.full_like(labels, -100))
    kw = dict(weight=weight, ignore_index=-100, label_smoothing=eps)
    want_sum, want_mean = F.cross_entropy(hi, lab, reduction="sum", **kw), F.cross_entropy(hi, lab, reduction="mean", **kw)
    assert abs(loss1.item() - want_sum.item()) <= 1e-12 * abs(want_sum.item())
    assert abs((loss1 / wsum1).item() - want_mean.item()) <= 1e-12 * abs(want_mean.item())
    # a fifth of the weights is exactly 0, the rest spread over [0, 2]; the count ignores them
    share0 = (pw == 0).double().mean().item()
    assert 0.15 <= share0 <= 0.25 and 0.0 <= pw.min().item() and 1.5 < pw.max().item() <= 2.0
    assert wsum.item() == wsum1.item() and loss.item() != loss1.item()
