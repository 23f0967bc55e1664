"""CPU checks of the fused head past 192 classes: the entry points are declared, bound and exported and refuse bad arguments in the
stated order before any launch; the workspace queries equal their documented formula; ops.class_pad; the model layer accepts up to
1024 classes and refuses the criteria that keep the 192-class limit before device work; and the fp64 reference the GPU tests compare
against checks itself."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_argmax_ref as A  # noqa: E402
import wide_head_ref as R  # noqa: E402

import lc2is_amd.nn as N  # noqa: E402
from lc2is_amd import _lib, ops  # noqa: E402

IGN = R.IGN
NAMES = ("lc2is_head_upsample_ce_wide_workspace_bytes", "lc2is_head_upsample_ce_wide",
         "lc2is_head_upsample_argmax_wide_workspace_bytes", "lc2is_head_upsample_argmax_wide")
P = 0x1000   # (16-byte aligned stand-in pointer; never dereferenced)


def test_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and name in ops._ARGTYPES and hasattr(lib, name)
    assert [len(ops._ARGTYPES[n]) for n in NAMES] == [8, 17, 6, 15]
    assert ops._fn(NAMES[0]).restype is C.c_size_t and ops._fn(NAMES[2]).restype is C.c_size_t
    assert ops._fn(NAMES[1]).restype is C.c_int and ops._fn(NAMES[3]).restype is C.c_int
    header = (Path(_lib.__file__).resolve().parent.parent / "include" / "lc2is_hip.h").read_text()
    assert "#define LC2IS_HEAD_WIDE_CMAX 1024" in header
    assert ops.HEAD_CMAX == 192 and ops.HEAD_WIDE_CMAX == 1024
    for fn in ("class_pad", "head_upsample_ce_wide", "head_upsample_argmax_wide"):
        assert callable(getattr(ops, fn))


def test_class_pad():
    assert [ops.class_pad(k) for k in (1, 64, 151, 192)] == [192] * 4
    assert [ops.class_pad(k) for k in (193, 256, 257, 459, 847, 919, 1024)] == [256, 256, 320, 512, 896, 960, 1024]
    assert all(ops.class_pad(k) % 64 == 0 and k <= ops.class_pad(k) < k + 64 for k in range(193, 1025))


def _tiles(h, w):
    return ((4 * h + 2 + 15) // 16) * ((4 * w + 2 + 15) // 16)


def test_workspace_queries_equal_their_formula():
    ce, am = ops._fn(NAMES[0]), ops._fn(NAMES[2])
    for (B, h, w, mode, Cn) in R.CASES + [(32, 32, 32, "bicubic", 847), (3, 8, 8, "bilinear", 151), (1, 1, 1, "bicubic", 1)]:
        md = 0 if mode == "bicubic" else 1
        f, cq, t = (7 if md == 0 else 5), (Cn + 3) // 4 * 4, _tiles(h, w)
        part = (B * t * 2 * 4 + 255) // 256 * 256
        assert ce(B, h, w, Cn, R.ld_of(Cn), 4, md, 0) == part
        assert ce(B, h, w, Cn, R.ld_of(Cn), 4, md, 1) == part + B * t * f * f * cq * 4
        assert ce(B, h, w, Cn, 1024, 4, md, 1) == part + B * t * f * f * cq * 4        # ld need not be the smallest pad
        assert am(B, h, w, Cn, 4, md) == B * t * 3 * cq * 4
    # 0 for a call that would be refused
    for bad in (dict(B=0), dict(h=0), dict(w=-1), dict(C=0), dict(C=1025), dict(ld=1088), dict(ld=832), dict(ld=900), dict(S=8),
                dict(S=16), dict(S=2), dict(mode=2), dict(mode=-1)):
        a = {**dict(B=2, h=9, w=9, C=847, ld=896, S=4, mode=0), **bad}
        assert ce(a["B"], a["h"], a["w"], a["C"], a["ld"], a["S"], a["mode"], 1) == 0, bad
        if "ld" not in bad:
            assert am(a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"]) == 0, bad


def test_ce_entry_point_refuses_in_the_stated_order():
    f = ops._fn(NAMES[1])
    ok = dict(lo=P, ld=896, labels=P, dlo=P, loss=P, B=2, h=9, w=9, C=847, S=4, mode=0, gs=1.0, cw=P, ws=P, wsb=1 << 40)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["dlo"], a["loss"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"], IGN,
                 a["gs"], a["cw"], a["ws"], a["wsb"], None)

    for name in ("lo", "labels", "loss"):
        assert call(**{name: None}) == -2, name                                  # LC2IS_ERR_NULL
    assert call(C=1025, ld=1088) == -1 and call(ld=1088) == -1 and call(ld=832) == -1 and call(ld=900) == -1     # LC2IS_ERR_SHAPE
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1 and call(**{dim: -3}) == -1, dim
    assert call(lo=P + 4) == -1 and call(dlo=P + 8) == -1                        # misaligned pointers
    for S in (0, 2, 5, 8, 16, 32):
        assert call(S=S) == -3, S                                                # LC2IS_ERR_UNSUPPORTED
    assert call(mode=7) == -3 and call(mode=-1) == -3
    need = ops._fn(NAMES[0])(2, 9, 9, 847, 896, 4, 0, 1)
    need0 = ops._fn(NAMES[0])(2, 9, 9, 847, 896, 4, 0, 0)
    assert 0 < need0 < need
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4 and call(wsb=0) == -4   # LC2IS_ERR_WORKSPACE
    assert call(dlo=None, wsb=need0 - 1) == -4                                   # a loss-only call needs the partials alone
    # NULL before SHAPE before UNSUPPORTED before WORKSPACE
    assert call(lo=None, C=0, S=8, ws=None) == -2 and call(C=0, S=8, ws=None) == -1 and call(S=8, ws=None) == -3
    assert call(mode=9, wsb=0) == -3
    # C <= 192, a wider pad than needed and a NULL weight vector are valid: the refusal of such a call is the workspace's
    assert call(C=151, ld=192, wsb=0) == -4 and call(C=193, ld=1024, cw=None, wsb=0) == -4 and call(C=1024, ld=1024, wsb=0) == -4


def test_argmax_entry_point_refuses_in_the_stated_order():
    f = ops._fn(NAMES[3])
    ok = dict(lo=P, ld=896, labels=P, pred=P, counts=P, B=2, h=9, w=9, C=847, S=4, mode=0, ws=P, wsb=1 << 40)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["ld"], a["labels"], a["pred"], a["counts"], a["B"], a["h"], a["w"], a["C"], a["S"], a["mode"], IGN,
                 a["ws"], a["wsb"], None)

    assert call(lo=None) == -2 and call(pred=None, counts=None) == -2 and call(labels=None) == -2     # counts without labels
    assert call(C=1025, ld=1088) == -1 and call(ld=832) == -1 and call(ld=900) == -1 and call(lo=P + 8) == -1
    for dim in ("B", "h", "w", "C"):
        assert call(**{dim: 0}) == -1, dim
    for S in (0, 2, 8, 16):
        assert call(S=S) == -3, S
    assert call(mode=2) == -3
    need = ops._fn(NAMES[2])(2, 9, 9, 847, 4, 0)
    assert call(ws=None) == -4 and call(ws=P + 4) == -4 and call(wsb=need - 1) == -4
    assert call(lo=None, C=0, S=8, ws=None) == -2 and call(C=0, S=8, ws=None) == -1 and call(S=8, ws=None) == -3


def test_existing_entry_points_still_stop_at_192():
    f = ops._fn("lc2is_head_upsample_focal")
    assert f(P, 256, P, P, P, 2, 8, 8, 193, 4, 0, IGN, 1.0, P, 2.0, 0.0, P, 1 << 30, None) == -1
    g = ops._fn("lc2is_head_upsample_argmax")
    assert g(P, 256, P, P, P, 2, 8, 8, 193, 4, 0, IGN, P, 1 << 30, None) == -1
    assert ops._fn("lc2is_head_upsample_argmax_workspace_bytes")(2, 8, 8, 193, 4, 0) == 0


class _Dev(torch.Tensor):   # a tensor that claims to be on the device: the checks behind _chk run, nothing is allocated
    is_cuda = True


def test_ops_wrappers_check_before_device_work():
    lo = torch.zeros(4, 256)
    lab = torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_ce_wide(lo, lab, 1, 2, 2, 200, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_upsample_argmax_wide(lo, lab, 1, 2, 2, 200, 4)
    flo, flab = lo.as_subclass(_Dev), lab.as_subclass(_Dev)
    for fn in (ops.head_upsample_ce_wide, ops.head_upsample_argmax_wide):
        with pytest.raises(RuntimeError, match="S must be 4"):
            fn(torch.zeros(1, 256).as_subclass(_Dev), torch.zeros(1, 8, 8, dtype=torch.long).as_subclass(_Dev), 1, 1, 1, 200, 8)
        with pytest.raises(RuntimeError, match="ld % 64 == 0"):
            fn(flo, flab, 1, 2, 2, 257, 4)                                       # C > ld
        with pytest.raises(RuntimeError, match="ld % 64 == 0"):
            fn(torch.zeros(4, 1088).as_subclass(_Dev), flab, 1, 2, 2, 1030, 4)   # past the cap
        with pytest.raises(RuntimeError, match="labels must be contiguous"):
            fn(flo, torch.zeros(1, 8, 4, dtype=torch.long).as_subclass(_Dev), 1, 2, 2, 200, 4)
    with pytest.raises(RuntimeError, match="weight tensor should be defined"):
        ops.head_upsample_ce_wide(flo, flab, 1, 2, 2, 200, 4, class_weight=torch.ones(199))
    with pytest.raises(ValueError, match="both False"):
        ops.head_upsample_argmax_wide(flo, flab, 1, 2, 2, 200, 4, want_pred=False, want_counts=False)
    with pytest.raises(ValueError, match="needs labels"):
        ops.head_upsample_argmax_wide(flo, None, 1, 2, 2, 200, 4)
    # the narrow wrappers keep their message
    with pytest.raises(RuntimeError, match="C <= ld <= 192"):
        ops.head_upsample_argmax(flo, flab, 1, 2, 2, 200, 4)
    with pytest.raises(RuntimeError, match="C <= ld <= 192"):
        ops.head_upsample_focal(flo, flab, 1, 2, 2, 200, 4)


def _tiny_cpu(K):
    g = torch.Generator().manual_seed(K)
    return N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                               text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                               dim_feedforward=128, out_dim=64, prototypes=torch.randn(K, 64, generator=g))


def test_model_layer_accepts_1024_classes_and_refuses_more():
    m = _tiny_cpu(200)
    assert m.class_prototypes.shape == (200, 64)
    assert _tiny_cpu(1024).class_prototypes.shape[0] == 1024
    with pytest.raises(ValueError, match="1024"):
        _tiny_cpu(1025)
    labels = torch.zeros(1, 16, 16, dtype=torch.long)
    for kw in (dict(label_smoothing=0.1), dict(ohem=(0.7, 100)), dict(dice=(1.0, 1.0, 1.0, True)), dict(focal=(2.0, 0.0)),
               dict(sigmoid=(2.0, 0.25, "elements"))):
        with pytest.raises(NotImplementedError, match="192"):
            m.forward_loss({}, labels, **kw)                                     # (raised before the inputs are looked at)
        if "dice" not in kw:                                                     # (dice= with weight= is a ValueError of its own)
            with pytest.raises(NotImplementedError, match="192"):
                m.forward_loss({}, labels, weight=torch.ones(200), reduction="sum", **kw)
    with pytest.raises(ValueError, match="thresh"):                             # an option's own checks still come first
        m.forward_loss({}, labels, ohem=(1.5, 4))
    with pytest.raises(ValueError, match="seg_counts"):
        m.forward_loss({}, labels, seg_counts=torch.zeros(3, 192, dtype=torch.long))
    # 192 classes keep every option: the same calls get past the option checks and fail on the missing inputs instead
    m192 = _tiny_cpu(192)
    with pytest.raises(KeyError):
        m192.forward_loss({}, labels, focal=(2.0, 0.0))


def test_score_map_tail_refusals_past_192():
    tail = N.ScoreMapTail(4)
    args = (torch.zeros(1, 4, 64), torch.zeros(1, 200, 64), torch.zeros(1, 8, 8, dtype=torch.long))
    for kw in (dict(label_smoothing=0.1), dict(ohem=(0.7, 100)), dict(dice=(1.0, 1.0, 1.0, True)), dict(focal=(2.0, 0.0)),
               dict(sigmoid=(2.0, 0.25, "elements"))):
        with pytest.raises(NotImplementedError, match="192"):
            tail.loss(*args, **kw)
    with pytest.raises(RuntimeError):                                            # accepted with weight / sum: the CPU tensors are refused
        tail.loss(*args, weight=torch.ones(200), reduction="sum")
    with pytest.raises(NotImplementedError, match="upsamples by 4"):
        N.ScoreMapTail(8).loss(*args)
    with pytest.raises(NotImplementedError, match="1024"):
        tail.loss(torch.zeros(1, 4, 64), torch.zeros(1, 1025, 64), args[2])


def test_trainstep_takes_a_wide_class_count():
    from lc2is_amd.step import TrainStep

    class _CpuModel(torch.nn.Module):
        """A CPU model: ParamArena refuses it with a RuntimeError, so reaching that error proves the seg_metrics guards passed."""

        def __init__(self, K=None):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(4))
            if K:
                self.class_prototypes = torch.nn.Parameter(torch.zeros(K, 4))

        def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean",
                         seg_counts=None):
            raise AssertionError("not reached")

    with pytest.raises(RuntimeError):
        TrainStep(_CpuModel(847), seg_metrics=True)
    with pytest.raises(RuntimeError):
        TrainStep(_CpuModel(), seg_metrics=True, seg_classes=1024)
    with pytest.raises(ValueError, match="seg_classes"):
        TrainStep(_CpuModel(), seg_metrics=True, seg_classes=1025)
    with pytest.raises(ValueError, match="seg_classes"):
        TrainStep(_CpuModel(847), seg_metrics=True, seg_classes=500)


# ---- the reference checks itself ----
def test_case_list_and_label_overrides():
    assert len(R.CASES) == 18 and all(C > 192 for *_, C in R.CASES)
    for (B, h, w, mode, Cn) in R.CASES:
        lo, labels = R.case_inputs(B, h, w, mode, Cn)
        base_lo, base_labels = A.case_inputs(B, h, w, 4, mode, Cn)
        assert lo is base_lo and tuple(lo.shape) == (B * h * w, R.ld_of(Cn)) and bool((lo[:, Cn:] == A.PAD_SCORE).all())
        assert {0, 191, 192, Cn - 1} <= set(labels[:, 0, :4].reshape(-1).tolist())
        assert int((labels != base_labels).sum()) <= 8 * B and bool((labels[:, 1::5] == IGN).all())


@pytest.mark.parametrize("case", [0, 10, 17])
def test_reference_gradient_is_the_closed_form(case):
    B, h, w, mode, Cn = R.CASES[case]
    lo, labels, w64, (loss, wsum, grad) = R.case_ref(case, True)
    assert int((w64 == 0).sum()) >= 2
    x = lo[:, :Cn].double().reshape(B, h, w, Cn).permute(0, 3, 1, 2)
    hi = F.interpolate(x, scale_factor=4, mode=mode, align_corners=False).requires_grad_(True)
    valid = A.counted(labels, Cn, IGN)
    p = torch.softmax(hi.detach(), 1)
    onehot = F.one_hot(labels.clamp(0, Cn - 1), Cn).permute(0, 3, 1, 2).double()
    wy = torch.where(valid, w64[labels.clamp(0, Cn - 1)], torch.zeros((), dtype=torch.float64))
    dhi = wy[:, None] * (p - onehot)
    xg = x.clone().requires_grad_(True)
    F.interpolate(xg, scale_factor=4, mode=mode, align_corners=False).backward(dhi)   # U^T of the closed-form dlogits
    got = xg.grad.permute(0, 2, 3, 1).reshape(B * h * w, Cn)
    assert ((got - grad).norm() / grad.norm()).item() <= 1e-12
    lse = torch.logsumexp(hi.detach(), 1)
    zy = hi.detach().gather(1, labels.clamp(0, Cn - 1)[:, None])[:, 0]
    assert abs((wy * (lse - zy)).sum().item() - loss) <= 1e-12 * abs(loss) and abs(wy.sum().item() - wsum) <= 1e-12 * wsum


def test_edge_cases_are_what_they_say():
    e = R.EDGE
    for name in R.EDGE_NAMES:
        lo, labels, w64, (loss, wsum, grad) = R.edge_ref(name)
        assert torch.isfinite(torch.tensor(loss)) and wsum > 0 and bool(torch.isfinite(grad).all())
        x = lo[:, :e["C"]].double().reshape(e["B"], e["h"], e["w"], e["C"]).permute(0, 3, 1, 2)
        arg = F.interpolate(x, scale_factor=4, mode=e["mode"], align_corners=False).argmax(1)
        lab = labels[labels != IGN]
        if name == "max_last_label_first":
            assert bool((arg >= 4 * R.CHUNK).float().mean() > 0.9) and bool((lab < R.CHUNK).all())
        elif name == "max_first_label_last":
            assert bool((arg < R.CHUNK).float().mean() > 0.9) and bool((lab >= 4 * R.CHUNK).all())
        else:
            assert lo[:, :e["C"]].max().item() == 1e4 and lo[:, :e["C"]].min().item() == -1e4


def test_margin_excludes_at_most_one_percent_of_every_case():
    worst = 0.0
    for (B, h, w, mode, Cn) in R.CASES:
        _, sure, _ = A.case_ref(B, h, w, 4, mode, Cn)
        worst = max(worst, 1.0 - sure.double().mean().item())
    assert worst <= A.MAX_EXCLUDED, worst
