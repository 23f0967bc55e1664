"""CPU checks of the sigmoid cross-entropy / sigmoid focal loss: the entry points are declared, bound and exported and refuse bad
arguments in the stated order before any launch; ops.sigmoid_options, the criteria, forward_loss / ScoreMapTail.loss and TrainStep
raise before device work; and the fp64 reference the GPU tests compare against checks itself (closed form against autograd,
(0, None) against F.binary_cross_entropy_with_logits, finiteness on the saturated case and at z = +-1e4)."""
import ctypes as C
import inspect
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sigmoid_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402
from lc2is_amd import _lib, ops  # noqa: E402

IGN = R.IGN
NAMES = ("lc2is_head_upsample_sigmoid", "lc2is_sigmoid_focal_nchw_fwd", "lc2is_sigmoid_focal_nchw_bwd")
NAN, INF = float("nan"), float("inf")
BAD_GAMMA = (NAN, -0.5, INF, -INF)
BAD_ALPHA = (NAN, 1.5, INF)
BAD_SCALE = (NAN, 0.0, -1.0, INF, -INF)


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and name in ops._ARGTYPES and hasattr(lib, name)
        assert ops._fn(name).restype is C.c_int
    assert [len(ops._ARGTYPES[n]) for n in NAMES] == [20, 15, 15]
    header = (Path(_lib.__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    sec = header[header.index("sigmoid cross-entropy and sigmoid focal loss"):]
    rep = sec[sec.index("replaces:"):sec.index("lc2is_head_upsample_sigmoid:")]
    for named in ("torch.nn.BCEWithLogitsLoss on one-hot targets", "CrossEntropyLoss(use_sigmoid=True)",
                  "torchvision.ops.sigmoid_focal_loss", "mmseg's FocalLoss"):
        assert named in rep, named
    for fn in ("sigmoid_options", "head_upsample_sigmoid", "sigmoid_focal_nchw_fwd", "sigmoid_focal_nchw_bwd"):
        assert callable(getattr(ops, fn))
    assert "SigmoidFocalLoss" in N.__all__ and "SigmoidCrossEntropyLoss" in N.__all__


def test_c_entry_point_refuses_in_the_stated_order():
    f = ops._fn(NAMES[0])
    P = 0x1000   # (16-byte aligned; never dereferenced)
    ok = dict(lo=P, ld=192, labels=P, dlo=P, loss=P, B=2, h=8, w=8, C=151, S=4, mode=0, gs=1.0, cw=P, gamma=2.0, alpha=0.25,
              cs=1.0, ws=P, wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["dlo"], a["loss"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"], IGN,
                 a["gs"], a["cw"], a["gamma"], a["alpha"], a["cs"], a["ws"], a["wsb"], None)

    for name in ("lo", "labels", "loss"):
        assert call(**{name: None}) == -2, name                               # LC2IS_ERR_NULL
    assert call(C=193) == -1 and call(ld=190) == -1 and call(ld=256) == -1 and call(ld=128) == -1     # LC2IS_ERR_SHAPE
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1 and call(**{dim: -3}) == -1, dim
    assert call(lo=P + 4) == -1 and call(dlo=P + 8) == -1                     # misaligned pointers
    for bad in BAD_GAMMA:
        assert call(gamma=bad) == -1, bad
    for bad in BAD_ALPHA:
        assert call(alpha=bad) == -1, bad
    for bad in BAD_SCALE:
        assert call(cs=bad) == -1, bad
    for S in (0, 2, 5, 12, 32):
        assert call(S=S) == -3, S                                             # LC2IS_ERR_UNSUPPORTED
    assert call(mode=7) == -3 and call(mode=-1) == -3
    need = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(2, 8, 8, 151, 4, 0, 1)
    need0 = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(2, 8, 8, 151, 4, 0, 0)
    assert 0 < need0 < need
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4 and call(wsb=0) == -4   # LC2IS_ERR_WORKSPACE
    assert call(dlo=None, wsb=need0 - 1) == -4                                # a loss-only call needs the partials alone
    # NULL before SHAPE before UNSUPPORTED before WORKSPACE
    assert call(lo=None, gamma=NAN, S=5, ws=None) == -2 and call(gamma=NAN, S=5, ws=None) == -1
    assert call(alpha=2.0, S=5) == -1 and call(cs=0.0, mode=9, ws=None) == -1
    assert call(S=5, ws=None) == -3 and call(mode=9, wsb=0) == -3
    # gamma = 0, any negative alpha ("no alpha"), alpha = 0 / 1 and a NULL weight vector are valid: the refusal is the workspace's
    for alpha in (-1.0, -0.25, -INF, 0.0, 1.0):
        assert call(gamma=0.0, alpha=alpha, cw=None, wsb=0) == -4, alpha
    assert call(cs=1.0 / 151, wsb=0) == -4

    fwd, bwd = ops._fn(NAMES[1]), ops._fn(NAMES[2])
    okf = (P, P, P, P, 1, 5, 16, IGN, P)
    big = 1 << 20
    assert fwd(None, P, P, P, 1, 5, 16, IGN, P, 2.0, 0.25, 1.0, P, big, None) == -2
    assert fwd(*okf, 2.0, 0.25, 1.0, None, big, None) == -2
    assert fwd(P, P, P, P, 1, 0, 16, IGN, P, 2.0, 0.25, 1.0, P, big, None) == -1
    bad = [(g, 0.25, 1.0) for g in BAD_GAMMA] + [(2.0, a, 1.0) for a in BAD_ALPHA] + [(2.0, 0.25, s) for s in BAD_SCALE]
    for g, a, s in bad:
        assert fwd(*okf, g, a, s, P, big, None) == -1, (g, a, s)
        assert bwd(P, P, None, 1.0, None, P, 1, 5, 16, IGN, None, g, a, s, None) == -1, (g, a, s)
    assert fwd(*okf, 2.0, -1.0, 1.0, P, ops._fn("lc2is_ce_nchw_fwd_workspace_bytes")(1, 16) - 1, None) == -4
    assert bwd(P, P, None, 1.0, None, None, 1, 5, 16, IGN, None, 2.0, 0.25, 1.0, None) == -2
    assert bwd(None, P, None, 1.0, None, P, 1, 5, 16, IGN, None, 2.0, 0.25, 1.0, None) == -2
    assert bwd(P, P, None, 1.0, None, P, 0, 5, 16, IGN, None, 2.0, 0.25, 1.0, None) == -1


def test_sigmoid_options_validation():
    assert ops.sigmoid_options(2, 0.25, "elements") == (2.0, 0.25, "elements")
    assert ops.sigmoid_options(0, None, "pixels") == (0.0, None, "pixels") and ops.sigmoid_options(1, 1) == (1.0, 1.0, "elements")
    g, a, _ = ops.sigmoid_options(1, 0)
    assert isinstance(g, float) and isinstance(a, float)
    for bad in (-0.1, NAN, INF, None, "2", True, [2.0]):
        with pytest.raises(ValueError, match="gamma"):
            ops.sigmoid_options(bad, 0.25)
    for bad in (-0.1, 1.1, NAN, INF, "0.25", False):
        with pytest.raises(ValueError, match="alpha"):
            ops.sigmoid_options(2.0, bad)
    for bad in ("mean", None, 1, "element"):
        with pytest.raises(ValueError, match="normalize"):
            ops.sigmoid_options(2.0, 0.25, bad)
    assert ops.sigmoid_class_scale("elements", "mean", 4) == 0.25 and ops.sigmoid_class_scale("pixels", "mean", 4) == 1.0
    assert ops.sigmoid_class_scale("elements", "sum", 4) == 1.0 and ops.sigmoid_class_scale("elements", "none", 4) == 1.0


def test_criteria_construction_and_validation():
    c = N.SigmoidFocalLoss()
    assert isinstance(c, N.CrossEntropyLoss) and c.sigmoid == (2.0, 0.25, "elements") and c.ignore_index == IGN
    assert c.reduction == "mean" and c.weight is None and c.label_smoothing == 0.0 and not isinstance(c, N.FocalLoss)
    sig = inspect.signature(N.SigmoidFocalLoss.__init__).parameters
    assert list(sig)[1:7] == ["gamma", "alpha", "weight", "ignore_index", "reduction", "normalize"]
    sig = inspect.signature(N.SigmoidCrossEntropyLoss.__init__).parameters
    assert list(sig)[1:5] == ["weight", "ignore_index", "reduction", "normalize"]
    w = torch.rand(5)
    c = N.SigmoidFocalLoss(0.5, None, w, 255, "sum", "pixels")
    assert c.sigmoid == (0.5, None, "pixels") and c.ignore_index == 255 and c.reduction == "sum" and torch.equal(c.weight, w)
    assert list(c.state_dict().keys()) == ["weight"]
    b = N.SigmoidCrossEntropyLoss(w, 0, "none", "pixels")
    assert isinstance(b, N.SigmoidFocalLoss) and b.sigmoid == (0.0, None, "pixels") and b.reduction == "none" and b.ignore_index == 0
    assert N.SigmoidCrossEntropyLoss().sigmoid == (0.0, None, "elements")
    for bad in (-1.0, NAN, INF, None, "2"):
        with pytest.raises(ValueError, match="gamma"):
            N.SigmoidFocalLoss(gamma=bad)
    for bad in (-0.01, 1.01, NAN, INF):
        with pytest.raises(ValueError, match="alpha"):
            N.SigmoidFocalLoss(alpha=bad)
    for cls in (N.SigmoidFocalLoss, N.SigmoidCrossEntropyLoss):
        with pytest.raises(ValueError, match="normalize"):
            cls(normalize="batch")
        with pytest.raises(ValueError, match="label_smoothing"):
            cls(label_smoothing=0.1)
        with pytest.raises(ValueError, match="reduction"):
            cls(reduction="avg")
    doc = N.SigmoidFocalLoss.__doc__
    assert "count" in doc.lower() and "weight sum" in doc and "torchvision" in doc and "mmseg" in doc


def test_module_and_ops_refuse_cpu_tensors():
    x, lab = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    for crit in (N.SigmoidFocalLoss(), N.SigmoidCrossEntropyLoss(), N.SigmoidFocalLoss().eval()):
        with pytest.raises(RuntimeError):
            crit(x, lab)
    crit = N.SigmoidFocalLoss()
    crit.label_smoothing = 0.1                                               # set behind the constructor's back
    with pytest.raises((ValueError, RuntimeError)):
        crit(x, lab)
    lo = torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_sigmoid(lo, torch.zeros(1, 8, 8, dtype=torch.long), 1, 2, 2, 5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sigmoid_focal_nchw_fwd(x, lab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sigmoid_focal_nchw_bwd(x, lab, None)

    class _Dev(torch.Tensor):   # a tensor that claims to be on the device: the checks behind _chk run, nothing is allocated
        is_cuda = True

    fake = lo.as_subclass(_Dev)
    flab = torch.zeros(1, 8, 8, dtype=torch.long).as_subclass(_Dev)
    with pytest.raises(ValueError, match="gamma"):
        ops.head_upsample_sigmoid(fake, flab, 1, 2, 2, 5, 4, gamma=-1.0)
    with pytest.raises(ValueError, match="alpha"):
        ops.head_upsample_sigmoid(fake, flab, 1, 2, 2, 5, 4, alpha=NAN)
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="class_scale"):
            ops.head_upsample_sigmoid(fake, flab, 1, 2, 2, 5, 4, class_scale=bad)
    with pytest.raises(RuntimeError, match="S must be 4, 8 or 16"):
        ops.head_upsample_sigmoid(torch.zeros(1, 64).as_subclass(_Dev), torch.zeros(1, 32, 32, dtype=torch.long).as_subclass(_Dev),
                                  1, 1, 1, 5, 32)


def _tiny_cpu():
    return N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                               text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                               dim_feedforward=128, out_dim=64)


def test_fused_sites_refuse_combinations_before_running():
    for fn in (N.BaseModelWithText.forward_loss, N.PromptFTN.forward_loss, N.ScoreMapTail.loss):
        par = inspect.signature(fn).parameters["sigmoid"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY
    m = _tiny_cpu()
    labels = torch.zeros(1, 16, 16, dtype=torch.long)
    s = (2.0, 0.25, "elements")
    with pytest.raises(ValueError, match="cannot be combined"):
        m.forward_loss({}, labels, sigmoid=s, dice=(1.0, 1.0, 1.0, True))      # (raised before the inputs are looked at)
    with pytest.raises(ValueError, match="cannot be combined"):
        m.forward_loss({}, labels, sigmoid=s, focal=(2.0, 0.0))
    with pytest.raises(ValueError, match="cannot be combined"):
        m.forward_loss({}, labels, sigmoid=s, label_smoothing=0.1)
    with pytest.raises(NotImplementedError):
        m.forward_loss({}, labels, sigmoid=s, reduction="none")
    with pytest.raises(ValueError, match="gamma"):
        m.forward_loss({}, labels, sigmoid=(-1.0, 0.25, "elements"))
    with pytest.raises(ValueError, match="alpha"):
        m.forward_loss({}, labels, sigmoid=(2.0, 3.0, "elements"))
    with pytest.raises(ValueError, match="normalize"):
        m.forward_loss({}, labels, sigmoid=(2.0, None, "classes"))
    with pytest.raises(ValueError, match="thresh"):
        m.forward_loss({}, labels, sigmoid=s, ohem=(1.5, 4))                   # ohem= combines: its own checks still run
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="cannot be combined"):
        tail.loss(*args, sigmoid=s, dice=(1.0, 1.0, 1.0, True))
    with pytest.raises(ValueError, match="cannot be combined"):
        tail.loss(*args, sigmoid=s, focal=(2.0, 0.0))
    with pytest.raises(ValueError, match="cannot be combined"):
        tail.loss(*args, sigmoid=s, label_smoothing=0.5)
    with pytest.raises(ValueError, match="gamma"):
        tail.loss(*args, sigmoid=(NAN, None, "pixels"))
    with pytest.raises(RuntimeError):                                          # accepted with weight / sum: the CPU tensors are refused
        tail.loss(*args, sigmoid=s, weight=torch.ones(3), reduction="sum")
    class _Towers:   # a PromptFTN whose towers must not run: a refusal that came after them would be this AssertionError
        def _embeddings(self, inputs):
            raise AssertionError("the towers ran before the refusal")

    with pytest.raises(ValueError, match="gamma"):
        N.PromptFTN.forward_loss(_Towers(), {}, labels, sigmoid=(-1.0, 0.25, "elements"))
    with pytest.raises(ValueError, match="cannot be combined"):
        N.PromptFTN.forward_loss(_Towers(), {}, labels, sigmoid=s, label_smoothing=0.1)
    with pytest.raises(AssertionError, match="towers ran"):                    # (and an accepted call does reach them)
        N.PromptFTN.forward_loss(_Towers(), {}, labels, sigmoid=s)
    with pytest.raises(ValueError, match="cannot be combined"):
        N.PromptFTN.forward_loss(None, {}, labels, sigmoid=s, focal=(2.0, 0.0))   # (before ``self`` is touched)
    with pytest.raises(ValueError, match="cannot be combined"):
        N.PromptFTN.forward_loss(None, {}, labels, sigmoid=s, label_smoothing=0.1)


class _CpuModel(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so reaching that error proves the criterion guards passed."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", seg_counts=None,
                     accum=None, focal=None, sigmoid=None):
        raise AssertionError("not reached")


class _NoSigmoidModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", ohem=None,
                     dice=None, seg_counts=None, accum=None, focal=None):
        raise AssertionError("not reached")


def test_trainstep_accepts_the_criterion_and_keeps_its_guards():
    from lc2is_amd.step import TrainStep, _accepts
    assert _accepts(_CpuModel(), "sigmoid") and not _accepts(_NoSigmoidModel(), "sigmoid") and not _accepts(nn.Linear(2, 2), "sigmoid")
    assert _accepts(_tiny_cpu(), "sigmoid")
    for crit in (N.SigmoidFocalLoss(2.0, weight=torch.ones(151)), N.SigmoidCrossEntropyLoss(), N.SigmoidFocalLoss(reduction="sum"),
                 N.SigmoidFocalLoss(normalize="pixels")):
        with pytest.raises(RuntimeError):                       # accepted: the arena is what refuses a CPU model
            TrainStep(_CpuModel(), criterion=crit)
        with pytest.raises(RuntimeError):                       # and under accumulation
            TrainStep(_CpuModel(), criterion=crit, accumulate=2)
        with pytest.raises(TypeError, match="sigmoid="):        # a model whose fused head has no sigmoid keyword
            TrainStep(_NoSigmoidModel(), criterion=crit)
    with pytest.raises(ValueError, match="ignore_index"):
        TrainStep(_CpuModel(), criterion=N.SigmoidFocalLoss(), ignore_index=0)
    with pytest.raises(ValueError, match="reduction='none'"):
        TrainStep(_CpuModel(), criterion=N.SigmoidFocalLoss(reduction="none"))


# ---- the reference checks itself ----
@pytest.mark.parametrize("gamma,alpha", R.PARAMS)
@pytest.mark.parametrize("B,Cn,H,W", [(2, 10, 12, 9), (1, 151, 8, 8), (3, 37, 5, 7)])
def test_closed_form_gradient_equals_autograd(B, Cn, H, W, gamma, alpha):
    g = torch.Generator().manual_seed(Cn + H)
    z = (torch.randn(B, Cn, H, W, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    labels = torch.randint(0, Cn + 3, (B, H, W), generator=g)
    labels[:, 1::5] = IGN
    w = R.weights(Cn, Cn)
    lpx, valid = R.loss_px(z, labels, gamma, alpha, w)
    lpx.sum().backward()
    assert int(valid.sum()) == int(((labels != IGN) & (labels < Cn)).sum()) > 0
    assert _rel(R.closed_form_grad(z.detach(), labels, gamma, alpha, w), z.grad) <= 1e-12
    # the loss against an independent statement of the definition (torchvision's sigmoid_focal_loss, written out)
    zd = z.detach().permute(0, 2, 3, 1)[valid]
    t = F.one_hot(labels[valid], Cn).double()
    p = torch.sigmoid(zd)
    p_t = p * t + (1 - p) * (1 - t)
    want = F.binary_cross_entropy_with_logits(zd, t, reduction="none") * (1 - p_t) ** gamma
    if alpha is not None:
        want = (alpha * t + (1 - alpha) * (1 - t)) * want
    want = (want * w).sum()
    assert abs(lpx.sum().item() - want.item()) <= 1e-12 * abs(want.item())
    assert R.reduce(lpx, valid, "mean", "elements", Cn).item() == pytest.approx(want.item() / (int(valid.sum()) * Cn), rel=1e-12)
    assert R.reduce(lpx, valid, "mean", "pixels", Cn).item() == pytest.approx(want.item() / int(valid.sum()), rel=1e-12)


@pytest.mark.parametrize("weighted", [True, False])
def test_gamma_0_no_alpha_is_bce_with_logits(weighted):
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 151, 9, 7, generator=g, dtype=torch.float64) * 3
    labels = torch.randint(0, 151, (2, 9, 7), generator=g)
    labels[:, ::4] = IGN
    w = R.weights(151, 3) if weighted else None
    lpx, valid = R.loss_px(z, labels, 0, None, w)
    zd = z.permute(0, 2, 3, 1)[valid]
    t = F.one_hot(labels[valid], 151).double()
    ref = F.binary_cross_entropy_with_logits(zd, t, weight=w, reduction="sum")
    assert abs(lpx.sum().item() - ref.item()) <= 1e-12 * abs(ref.item())
    if not weighted:   # torch's elementwise mean is the 'mean' of normalize='elements'
        ref_mean = F.binary_cross_entropy_with_logits(zd, t)
        assert abs(R.reduce(lpx, valid, "mean", "elements", 151).item() - ref_mean.item()) <= 1e-12 * abs(ref_mean.item())


@pytest.mark.parametrize("gamma,alpha", R.PARAMS + [(0.5, None), (2, 1.0)])
def test_reference_is_finite_on_the_saturated_case_and_at_huge_scores(gamma, alpha):
    s = R.SAT
    lo, labels = R.saturated_case()
    loss, count, grad = R.head_loss(lo, labels, s["B"], s["h"], s["w"], s["C"], s["S"], s["mode"], gamma, alpha, R.weights(s["C"], 1))
    assert torch.isfinite(torch.tensor(loss)) and loss > 0 and count > 0 and bool(torch.isfinite(grad).all())
    # the case is what it says: in fp32 every term of region A underflows, and region B is confidently wrong
    lod = lo[:, :s["C"]].double().reshape(s["B"], s["h"], s["w"], s["C"]).permute(0, 3, 1, 2)
    up = F.interpolate(lod, scale_factor=s["S"], mode=s["mode"])
    H = s["h"] * s["S"]
    top = up[:, :, : H // 2 - 4]
    assert bool((top[:, s["A"]] >= 119.9).all()) and bool((top.sum(1) - top[:, s["A"]] <= -119.9 * 150).all())
    assert float(torch.exp(torch.tensor(-119.9)).float()) == 0.0
    bot = up[:, :, H // 2 + 4:]
    assert bool((bot[:, s["Bc"]] <= -119.9).all()) and bool((bot[:, s["Wr"]] >= 119.9).all())
    la, ca, ga = R.head_loss(lo, R.region_a_only(labels), s["B"], s["h"], s["w"], s["C"], s["S"], s["mode"], gamma, alpha)
    assert ca > 0 and 0.0 <= la < 1e-45 and float(ga.abs().max()) < 1e-45      # below the smallest fp32 subnormal
    # z = +-1e4, as the label's score and as another class's
    z = torch.tensor([1e4, -1e4, 1e4, -1e4], dtype=torch.float64).reshape(1, 4, 1, 1).repeat(1, 1, 1, 4).requires_grad_(True)
    lab = torch.tensor([[[0, 1, 2, 3]]])
    lpx, _ = R.loss_px(z, lab, gamma, alpha)
    lpx.sum().backward()
    assert bool(torch.isfinite(lpx).all()) and bool(torch.isfinite(z.grad).all())
    assert bool(torch.isfinite(R.closed_form_grad(z.detach(), lab, gamma, alpha)).all())
    assert _rel(R.closed_form_grad(z.detach(), lab, gamma, alpha), z.grad) <= 1e-12
