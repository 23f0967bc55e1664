"""CPU checks of the focal / poly-1 cross-entropy: the entry points are declared, bound and exported and refuse bad arguments in the
stated order before any launch; ops.focal_options, the criteria, forward_loss / ScoreMapTail.loss and TrainStep raise before device
work; and the fp64 reference the GPU tests compare against checks itself (closed form against autograd, (0, 0) against
F.cross_entropy, finiteness on the saturated case)."""
import ctypes as C
import inspect
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import focal_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402
from lc2is_amd import _lib, ops  # noqa: E402

IGN = R.IGN
NAMES = ("lc2is_head_upsample_focal", "lc2is_focal_nchw_fwd", "lc2is_focal_nchw_bwd")
NAN, INF = float("nan"), float("inf")


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and name in ops._ARGTYPES and hasattr(lib, name)
        assert ops._fn(name).restype is C.c_int
    assert [len(ops._ARGTYPES[n]) for n in NAMES] == [19, 15, 15]
    header = (Path(_lib.__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    assert "replaces: kornia.losses.FocalLoss" in header
    for fn in ("focal_options", "head_upsample_focal", "focal_nchw_fwd", "focal_nchw_bwd"):
        assert callable(getattr(ops, fn))
    assert "FocalLoss" in N.__all__ and "Poly1CrossEntropyLoss" in N.__all__


def test_c_entry_point_refuses_in_the_stated_order():
    f = ops._fn(NAMES[0])
    P = 0x1000   # (16-byte aligned; never dereferenced)
    ok = dict(lo=P, ld=192, labels=P, dlo=P, loss=P, B=2, h=8, w=8, C=151, S=4, mode=0, gs=1.0, cw=P, gamma=2.0, eps=0.0, ws=P,
              wsb=1 << 30)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["dlo"], a["loss"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"], IGN,
                 a["gs"], a["cw"], a["gamma"], a["eps"], a["ws"], a["wsb"], None)

    for name in ("lo", "labels", "loss"):
        assert call(**{name: None}) == -2, name                               # LC2IS_ERR_NULL
    assert call(C=193) == -1 and call(ld=190) == -1 and call(ld=256) == -1 and call(ld=128) == -1     # LC2IS_ERR_SHAPE
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1 and call(**{dim: -3}) == -1, dim
    assert call(lo=P + 4) == -1 and call(dlo=P + 8) == -1                     # misaligned pointers
    for bad in (NAN, -0.5, INF, -INF):
        assert call(gamma=bad) == -1, bad
    for bad in (NAN, -1.5, INF, -INF):
        assert call(eps=bad) == -1, bad
    for S in (0, 2, 5, 12, 32):
        assert call(S=S) == -3, S                                             # LC2IS_ERR_UNSUPPORTED
    assert call(mode=7) == -3 and call(mode=-1) == -3
    need = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(2, 8, 8, 151, 4, 0, 1)
    need0 = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(2, 8, 8, 151, 4, 0, 0)
    assert 0 < need0 < need
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4 and call(wsb=0) == -4   # LC2IS_ERR_WORKSPACE
    assert call(dlo=None, wsb=need0 - 1) == -4                                # a loss-only call needs the partials alone
    # NULL before SHAPE before UNSUPPORTED before WORKSPACE
    assert call(lo=None, gamma=NAN, S=5, ws=None) == -2 and call(gamma=NAN, S=5, ws=None) == -1 and call(eps=-2.0, S=5) == -1
    assert call(S=5, ws=None) == -3 and call(mode=9, wsb=0) == -3
    # gamma = 0, eps = -1 and a NULL weight vector are valid: the refusal of such a call is the workspace's
    assert call(gamma=0.0, eps=-1.0, cw=None, wsb=0) == -4

    fwd, bwd = ops._fn(NAMES[1]), ops._fn(NAMES[2])
    okf = (P, P, P, P, P, 1, 5, 16, IGN, P)
    assert fwd(None, P, P, P, P, 1, 5, 16, IGN, P, 2.0, 0.0, P, 1 << 20, None) == -2
    assert fwd(*okf, 2.0, 0.0, None, 1 << 20, None) == -2
    assert fwd(P, P, P, P, P, 1, 0, 16, IGN, P, 2.0, 0.0, P, 1 << 20, None) == -1
    for g, e in ((NAN, 0.0), (-1.0, 0.0), (INF, 0.0), (2.0, -1.5), (2.0, NAN), (2.0, INF)):
        assert fwd(*okf, g, e, P, 1 << 20, None) == -1, (g, e)
        assert bwd(P, P, P, None, 1.0, None, P, 1, 5, 16, IGN, None, g, e, None) == -1, (g, e)
    assert fwd(*okf, 2.0, 0.0, P, ops._fn("lc2is_ce_nchw_fwd_workspace_bytes")(1, 16) - 1, None) == -4
    assert bwd(P, P, None, None, 1.0, None, P, 1, 5, 16, IGN, None, 2.0, 0.0, None) == -2
    assert bwd(P, P, P, None, 1.0, None, P, 0, 5, 16, IGN, None, 2.0, 0.0, None) == -1


def test_focal_options_validation():
    assert ops.focal_options(2, 0) == (2.0, 0.0) and ops.focal_options(0.0, -1) == (0.0, -1.0)
    assert all(isinstance(v, float) for v in ops.focal_options(1, 1))
    for bad in (-0.1, NAN, INF, None, "2", True, [2.0]):
        with pytest.raises(ValueError, match="gamma"):
            ops.focal_options(bad, 0.0)
    for bad in (-1.5, NAN, INF, -INF, None, "1", False):
        with pytest.raises(ValueError, match="poly_eps"):
            ops.focal_options(2.0, bad)


def test_criteria_construction_and_validation():
    c = N.FocalLoss()
    assert isinstance(c, N.CrossEntropyLoss) and c.focal == (2.0, 0.0) and c.ignore_index == IGN and c.reduction == "mean"
    assert c.weight is None and c.label_smoothing == 0.0
    sig = inspect.signature(N.FocalLoss.__init__).parameters
    assert list(sig)[1:6] == ["gamma", "poly_eps", "weight", "ignore_index", "reduction"]
    w = torch.rand(5)
    c = N.FocalLoss(0.5, 1.0, w, 255, "sum")
    assert c.focal == (0.5, 1.0) and c.ignore_index == 255 and c.reduction == "sum" and torch.equal(c.weight, w)
    assert list(c.state_dict().keys()) == ["weight"]                          # the alpha vector is CrossEntropyLoss's buffer
    for e in (1.0, 0.0, -1.0, 2.5):
        p = N.Poly1CrossEntropyLoss(e)
        assert isinstance(p, N.FocalLoss) and p.focal == (0.0, e) and p.epsilon == e
    assert N.Poly1CrossEntropyLoss().focal == (0.0, 1.0)
    assert N.Poly1CrossEntropyLoss(2.0, weight=w, ignore_index=0, reduction="none").reduction == "none"
    for bad in (-1.0, NAN, INF, None, "2"):
        with pytest.raises(ValueError, match="gamma"):
            N.FocalLoss(gamma=bad)
    for bad in (-1.01, NAN, INF, None):
        with pytest.raises(ValueError, match="poly_eps"):
            N.FocalLoss(poly_eps=bad)
        with pytest.raises(ValueError, match="poly_eps"):
            N.Poly1CrossEntropyLoss(bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        N.FocalLoss(label_smoothing=0.1)
    with pytest.raises(ValueError, match="label_smoothing"):
        N.Poly1CrossEntropyLoss(label_smoothing=0.1)
    with pytest.raises(ValueError, match="reduction"):
        N.FocalLoss(reduction="avg")
    doc = N.FocalLoss.__doc__
    assert "kornia" in doc and "MONAI" in doc and "number of pixels" in doc


def test_module_and_ops_refuse_cpu_tensors():
    x, lab = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    for crit in (N.FocalLoss(), N.Poly1CrossEntropyLoss(), N.FocalLoss().eval()):
        with pytest.raises(RuntimeError):
            crit(x, lab)
    crit = N.FocalLoss()
    crit.label_smoothing = 0.1                                               # set behind the constructor's back
    with pytest.raises((ValueError, RuntimeError)):
        crit(x, lab)
    lo = torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_focal(lo, torch.zeros(1, 8, 8, dtype=torch.long), 1, 2, 2, 5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.focal_nchw_fwd(x, lab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.focal_nchw_bwd(x, lab, torch.zeros(1, 4, 4), None)

    class _Dev(torch.Tensor):   # a tensor that claims to be on the device: the checks behind _chk run, nothing is allocated
        is_cuda = True

    fake = lo.as_subclass(_Dev)
    flab = torch.zeros(1, 8, 8, dtype=torch.long).as_subclass(_Dev)
    with pytest.raises(ValueError, match="gamma"):
        ops.head_upsample_focal(fake, flab, 1, 2, 2, 5, 4, gamma=-1.0)
    with pytest.raises(ValueError, match="poly_eps"):
        ops.head_upsample_focal(fake, flab, 1, 2, 2, 5, 4, poly_eps=NAN)
    with pytest.raises(RuntimeError, match="S must be 4, 8 or 16"):
        ops.head_upsample_focal(torch.zeros(1, 64).as_subclass(_Dev), torch.zeros(1, 32, 32, dtype=torch.long).as_subclass(_Dev),
                                1, 1, 1, 5, 32)


def _tiny_cpu():
    return N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                               text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                               dim_feedforward=128, out_dim=64)


def test_fused_sites_refuse_combinations_before_running():
    for fn in (N.BaseModelWithText.forward_loss, N.PromptFTN.forward_loss, N.ScoreMapTail.loss):
        par = inspect.signature(fn).parameters["focal"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY
    m = _tiny_cpu()
    labels = torch.zeros(1, 16, 16, dtype=torch.long)
    f = (2.0, 0.0)
    with pytest.raises(ValueError, match="cannot be combined"):
        m.forward_loss({}, labels, focal=f, dice=(1.0, 1.0, 1.0, True))        # (raised before the inputs are looked at)
    with pytest.raises(ValueError, match="cannot be combined"):
        m.forward_loss({}, labels, focal=f, label_smoothing=0.1)
    with pytest.raises(NotImplementedError):
        m.forward_loss({}, labels, focal=f, reduction="none")
    with pytest.raises(ValueError, match="gamma"):
        m.forward_loss({}, labels, focal=(-1.0, 0.0))
    with pytest.raises(ValueError, match="poly_eps"):
        m.forward_loss({}, labels, focal=(2.0, -3.0))
    with pytest.raises(ValueError, match="thresh"):
        m.forward_loss({}, labels, focal=f, ohem=(1.5, 4))                     # ohem= combines: its own checks still run
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 3, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="cannot be combined"):
        tail.loss(*args, focal=f, dice=(1.0, 1.0, 1.0, True))
    with pytest.raises(ValueError, match="cannot be combined"):
        tail.loss(*args, focal=f, label_smoothing=0.5)
    with pytest.raises(ValueError, match="gamma"):
        tail.loss(*args, focal=(NAN, 0.0))
    with pytest.raises(RuntimeError):                                          # accepted with weight / sum: the CPU tensors are refused
        tail.loss(*args, focal=f, weight=torch.ones(3), reduction="sum")
    class _Towers:   # a PromptFTN whose towers must not run: a refusal that came after them would be this AssertionError
        def _embeddings(self, inputs):
            raise AssertionError("the towers ran before the refusal")

    with pytest.raises(ValueError, match="gamma"):
        N.PromptFTN.forward_loss(_Towers(), {}, labels, focal=(-1.0, 0.0))
    with pytest.raises(ValueError, match="cannot be combined"):
        N.PromptFTN.forward_loss(_Towers(), {}, labels, focal=f, label_smoothing=0.1)
    with pytest.raises(AssertionError, match="towers ran"):                    # (and an accepted call does reach them)
        N.PromptFTN.forward_loss(_Towers(), {}, labels, focal=f)


class _CpuModel(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so reaching that error proves the criterion guards passed."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", seg_counts=None,
                     accum=None, focal=None):
        raise AssertionError("not reached")


class _NoFocalModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))

    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", ohem=None,
                     dice=None, seg_counts=None, accum=None):
        raise AssertionError("not reached")


def test_trainstep_accepts_the_criterion_and_keeps_its_guards():
    from lc2is_amd.step import TrainStep, _accepts
    assert _accepts(_CpuModel(), "focal") and not _accepts(_NoFocalModel(), "focal") and not _accepts(nn.Linear(2, 2), "focal")
    assert _accepts(_tiny_cpu(), "focal")
    for crit in (N.FocalLoss(2.0, weight=torch.ones(151)), N.Poly1CrossEntropyLoss(1.0), N.FocalLoss(reduction="sum")):
        with pytest.raises(RuntimeError):                       # accepted: the arena is what refuses a CPU model
            TrainStep(_CpuModel(), criterion=crit)
        with pytest.raises(RuntimeError):                       # and under accumulation / with the metric counts
            TrainStep(_CpuModel(), criterion=crit, accumulate=2)
        with pytest.raises(TypeError, match="focal"):           # a model whose fused head has no focal keyword
            TrainStep(_NoFocalModel(), criterion=crit)
    with pytest.raises(ValueError, match="ignore_index"):
        TrainStep(_CpuModel(), criterion=N.FocalLoss(), ignore_index=0)
    with pytest.raises(ValueError, match="reduction='none'"):
        TrainStep(_CpuModel(), criterion=N.FocalLoss(reduction="none"))


# ---- the reference checks itself ----
@pytest.mark.parametrize("gamma,eps", R.PARAMS)
@pytest.mark.parametrize("B,Cn,H,W", [(2, 10, 12, 9), (1, 151, 8, 8), (3, 37, 5, 7)])
def test_closed_form_gradient_equals_autograd(B, Cn, H, W, gamma, eps):
    g = torch.Generator().manual_seed(Cn + H)
    z = (torch.randn(B, Cn, H, W, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    labels = torch.randint(0, Cn + 3, (B, H, W), generator=g)
    labels[:, 1::5] = IGN
    w = R.weights(Cn, Cn)
    lpx, wy = R.loss_px(z, labels, gamma, eps, w)
    lpx.sum().backward()
    assert int((wy > 0).sum()) == int(((labels != IGN) & (labels < Cn)).sum()) > 0
    assert _rel(R.closed_form_grad(z.detach(), labels, gamma, eps, w), z.grad) <= 1e-12
    # the loss against an independent statement of the definition
    p = torch.softmax(z.detach(), 1)
    valid = (labels != IGN) & (labels < Cn)
    py = p.permute(0, 2, 3, 1)[valid].gather(1, labels[valid][:, None])[:, 0]
    want = (w[labels[valid]] * ((1 - py) ** gamma * -py.log() + eps * (1 - py))).sum()
    assert abs(lpx.sum().item() - want.item()) <= 1e-12 * abs(want.item())
    assert R.reduce(lpx, wy, "mean").item() == pytest.approx(want.item() / w[labels[valid]].sum().item(), rel=1e-12)


@pytest.mark.parametrize("weighted", [True, False])
def test_gamma_0_eps_0_is_the_weighted_cross_entropy(weighted):
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 151, 9, 7, generator=g, dtype=torch.float64) * 3
    labels = torch.randint(0, 151, (2, 9, 7), generator=g)
    labels[:, ::4] = IGN
    w = R.weights(151, 3) if weighted else None
    lpx, wy = R.loss_px(z, labels, 0, 0, w)
    ref = F.cross_entropy(z, labels, weight=w, reduction="sum")
    assert abs(lpx.sum().item() - ref.item()) <= 1e-12 * abs(ref.item())
    ref_mean = F.cross_entropy(z, labels, weight=w)
    assert abs(R.reduce(lpx, wy, "mean").item() - ref_mean.item()) <= 1e-12 * abs(ref_mean.item())
    assert bool((R.closed_form_c(z, labels, 0, 0)[labels != IGN] == 1.0).all())


@pytest.mark.parametrize("gamma,eps", R.PARAMS + [(0.5, 1), (2, -1)])
def test_reference_is_finite_on_the_saturated_case(gamma, eps):
    s = R.SAT
    lo, labels = R.saturated_case()
    loss, wsum, grad = R.head_loss(lo, labels, s["B"], s["h"], s["w"], s["C"], s["S"], s["mode"], gamma, eps, R.weights(s["C"], 1))
    assert torch.isfinite(torch.tensor(loss)) and wsum > 0 and bool(torch.isfinite(grad).all())
    # the case is what it says: in fp32 q is exactly 0 on the upper rows and p exactly 0 on the lower rows
    lod = lo[:, :s["C"]].double().reshape(s["B"], s["h"], s["w"], s["C"]).permute(0, 3, 1, 2)
    p = torch.softmax(F.interpolate(lod, scale_factor=s["S"], mode=s["mode"]), 1).float()
    H = s["h"] * s["S"]
    assert bool((p[:, s["A"], : H // 2 - 4] == 1.0).all()) and bool((p[:, s["Bc"], H // 2 + 4:] == 0.0).all())
    c = R.closed_form_c(F.interpolate(lod, scale_factor=s["S"], mode=s["mode"]), labels, gamma, eps)
    assert bool(torch.isfinite(c).all())
