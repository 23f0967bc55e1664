"""Distillation on the HIP path: ops.head_upsample_kd (per-pixel KL(teacher || student) of the upsampled scores at a temperature)
and what is built on it — forward_loss(distill=), ScoreMapTail.loss(distill=), head_scores / scores_lo, TrainStep(distill=) —
against the fp64 torch references of tests/distill_ref.py.

Gates (tests/distill_ref.py says where each comes from): |loss sum - fp64| <= 1e-4 * sum_i pw_i T^2 (H(p_t, p_s) + H(p_t))_i, the
gradient 2e-5 relative L2, the count exact; identities exact or bitwise; the model layer to test_gpu_selftrain's tolerances."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distill_ref as D  # noqa: E402
import selftrain_ref as R  # noqa: E402
from test_gpu_selftrain import GRAD_KEYS, STEP_KEYS, _batch, _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = D.IGN


def _mode(ops, mode):
    return ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR


def _check(tag, loss2, dlo, ref, C):
    """The three gates of a call against its fp64 reference; prints the figures first."""
    e_loss = abs(loss2[0].item() - ref["loss"].item())
    bound = D.LOSS_TOL * ref["scale"].item()
    e_grad = D.rel(dlo[:, :C], ref["grad"])
    print("distill figures", tag, "loss", loss2[0].item(), ref["loss"].item(), "err", e_loss, "bound", bound, "grad", e_grad,
          "count", loss2[1].item(), ref["count"])
    assert bool(torch.isfinite(loss2).all()) and bool(torch.isfinite(dlo).all())
    assert e_loss <= bound and e_grad <= D.GRAD_TOL and loss2[1].item() == ref["count"]


# ---- 1. against fp64 ----
@pytest.mark.parametrize("weighted", [False, True], ids=["all", "labels+pw"])
@pytest.mark.parametrize("temp", D.TEMPS)
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_kd_vs_fp64(dev, case, temp, weighted):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, t, labels, pw = D.case_inputs(*case)
    ref = D.case_ref(case, temp, weighted)
    geom = (B, h, w, C, S, _mode(ops, mode))
    kw = dict(temperature=temp, labels=labels.to(dev), pixel_weight=pw.to(dev)) if weighted else dict(temperature=temp)
    lod, td = lo.to(dev), t.to(dev)
    loss2, dlo = ops.head_upsample_kd(lod, td, *geom, want_grad=True, **kw)
    assert loss2.dtype == torch.float32 and tuple(loss2.shape) == (2,) and tuple(dlo.shape) == tuple(lo.shape)
    _check((case, temp, weighted), loss2, dlo, ref, C)
    assert dlo.shape[1] == C or dlo[:, C:].abs().max().item() == 0.0
    only, none = ops.head_upsample_kd(lod, td, *geom, **kw)
    assert none is None and torch.equal(only, loss2)                  # the loss-only call: the bytes of the gradient call


# ---- 2. identity ----
@pytest.mark.parametrize("temp", D.TEMPS)
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_teacher_equal_to_student_gives_exact_zero(dev, case, temp):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, _, labels, pw = D.case_inputs(*case)
    lod = lo.to(dev)
    geom = (B, h, w, C, S, _mode(ops, mode))
    for kw in (dict(), dict(labels=labels.to(dev), pixel_weight=pw.to(dev))):
        loss2, dlo = ops.head_upsample_kd(lod, lod.clone(), *geom, temperature=temp, want_grad=True, **kw)
        assert loss2[0].item() == 0.0 and not dlo.any()
        assert loss2[1].item() == (B * h * S * w * S if not kw else int(R.counted(labels, C).sum()))


# ---- 3. a one-hot teacher is the cross-entropy ----
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_one_hot_teacher_is_cross_entropy(dev, case):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, _, _, _ = D.case_inputs(*case)
    ys = [(7 * b + 3) % C for b in range(B)]
    t = torch.zeros(B, h * w, lo.shape[1])
    labels = torch.empty(B, h * S, w * S, dtype=torch.long)
    for b, y in enumerate(ys):
        t[b, :, y] = 1e4
        labels[b] = y
    geom = (B, h, w, C, S, _mode(ops, mode))
    lod = lo.to(dev)
    kd2, kd_d = ops.head_upsample_kd(lod, t.reshape(lo.shape).contiguous().to(dev), *geom, temperature=1.0, want_grad=True)
    ce2, ce_d, _ = ops.head_upsample_ce(lod, labels.to(dev), *geom, want_grad=True)
    e_loss, e_grad = abs(kd2[0].item() - ce2[0].item()) / abs(ce2[0].item()), D.rel(kd_d, ce_d)
    print("distill figures one-hot", case, kd2.tolist(), ce2.tolist(), e_loss, e_grad)
    assert e_loss <= 2 * D.LOSS_TOL and e_grad <= 2 * D.GRAD_TOL
    assert kd2[1].item() == ce2[1].item() == B * h * S * w * S


# ---- 4. pixel-weight and region rules ----
@pytest.mark.parametrize("case", [D.CASES[1], D.CASES[6], D.CASES[10], D.CASES[15], D.CASES[17], D.CASES[22], D.CASES[27]], ids=D.case_id)
def test_pixel_weight_and_region_rules(dev, case):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, t, labels, pw = D.case_inputs(*case)
    lod, td, lab = lo.to(dev), t.to(dev), labels.to(dev)
    geom = (B, h, w, C, S, _mode(ops, mode))
    kw = dict(temperature=4.0, want_grad=True)
    l1, d1 = ops.head_upsample_kd(lod, td, *geom, **kw)
    # pw == 2^-3 is exactly an eighth, with the same count; pw == 1 is the call without a weight
    ones = torch.ones(labels.shape, device=dev)
    l8, d8 = ops.head_upsample_kd(lod, td, *geom, pixel_weight=0.125 * ones, **kw)
    assert torch.equal(8.0 * l8[0], l1[0]) and torch.equal(l8[1], l1[1]) and torch.equal(8.0 * d8, d1)
    lo1, do1 = ops.head_upsample_kd(lod, td, *geom, pixel_weight=ones, **kw)
    assert torch.equal(lo1, l1) and torch.equal(do1, d1)
    # pw == 0 on a set of pixels adds nothing to the loss or the gradient and one each to the count: it is the labelled region
    # of labels that ignore the same set, but for the count
    drop = torch.rand(labels.shape, generator=torch.Generator().manual_seed(9)) < 0.3
    la, da = ops.head_upsample_kd(lod, td, *geom, pixel_weight=(~drop).float().to(dev), **kw)
    region = torch.where(drop, IGN, torch.zeros_like(labels)).to(dev)
    lb, db = ops.head_upsample_kd(lod, td, *geom, labels=region, **kw)
    e_loss, e_grad = abs(la[0].item() - lb[0].item()) / abs(lb[0].item()), D.rel(da, db)
    print("distill figures pw 0 vs region", case, la.tolist(), lb.tolist(), e_loss, e_grad)
    assert e_loss <= 1e-6 and e_grad <= 1e-6
    assert la[1].item() == l1[1].item() == B * h * S * w * S and lb[1].item() == int((~drop).sum())
    # region semantics: with labels the count is that of the pixels the cross-entropy counts, another ignore_index included
    lc, _ = ops.head_upsample_kd(lod, td, *geom, labels=lab, **kw)
    assert lc[1].item() == int(R.counted(labels, C).sum())
    lab255 = torch.where(labels == IGN, 255, labels)
    lc255, _ = ops.head_upsample_kd(lod, td, *geom, labels=lab255.to(dev), ignore_index=255, **kw)
    assert lc255[1].item() == int(R.counted(lab255, C, 255).sum()) and (C > 255 or torch.equal(lc255, lc))
    # grad_scale multiplies the gradient, not the loss
    lg, dg = ops.head_upsample_kd(lod, td, *geom, grad_scale=0.25, **kw)
    assert torch.equal(lg, l1) and torch.equal(4.0 * dg, d1)


# ---- 5. extremes ----
@pytest.mark.parametrize("temp", D.TEMPS)
@pytest.mark.parametrize("case", [D.CASES[0], D.CASES[10], D.CASES[27]], ids=D.case_id)   # TN = 4, 10, 12
def test_scores_of_1e4_stay_finite_and_inside_the_bounds(dev, case, temp):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, t, labels, pw = D.case_inputs(*case)
    lo, t = lo.clone(), t.clone()
    lo[:, :C] *= 1e4 / lo[:, :C].abs().max()
    t[:, :C] *= 1e4 / t[:, :C].abs().max()
    assert lo[:, :C].abs().max().item() == 1e4 and t[:, :C].abs().max().item() == 1e4
    ref = D.kd_ref(lo, t, labels, pw, B, h, w, C, S, mode, temp)
    loss2, dlo = ops.head_upsample_kd(lo.to(dev), t.to(dev), B, h, w, C, S, _mode(ops, mode), temperature=temp, labels=labels.to(dev),
                                      pixel_weight=pw.to(dev), want_grad=True)
    _check(("extremes", case, temp), loss2, dlo, ref, C)


# ---- 6. padding ----
@pytest.mark.parametrize("case", [D.CASES[0], D.CASES[5], D.CASES[10], D.CASES[12], D.CASES[18], D.CASES[20], D.CASES[26]], ids=D.case_id)
def test_padding_is_never_read_into_a_result(dev, case):
    from lc2is_amd import ops
    B, h, w, S, mode, C = case
    lo, t, labels, pw = D.case_inputs(*case)
    assert lo.shape[1] > C
    geom = (B, h, w, C, S, _mode(ops, mode))
    kw = dict(temperature=4.0, labels=labels.to(dev), pixel_weight=pw.to(dev), want_grad=True)
    l0, d0 = ops.head_upsample_kd(lo.to(dev), t.to(dev), *geom, **kw)
    assert not d0[:, C:].any()
    g = torch.Generator().manual_seed(2)
    for which in (0, 1):
        maps = [lo.clone(), t.clone()]
        maps[which][:, C:] = 1e4 * torch.randn(lo.shape[0], lo.shape[1] - C, generator=g)
        l1, d1 = ops.head_upsample_kd(maps[0].to(dev), maps[1].to(dev), *geom, **kw)
        assert torch.equal(l1, l0) and torch.equal(d1, d0), which


# ---- 7. many tiles, determinism ----
def test_many_tiles_sum_in_a_fixed_order(dev):
    """B = 2, 32 x 32 cells, S = 4, C = 151: 81 tiles per image through the finish launch's fixed-order sums; two runs, the same bytes."""
    from lc2is_amd import ops
    B, h, S, C, temp = 2, 32, 4, 151, 2.0
    g = torch.Generator().manual_seed(0)
    lo, t = torch.full((B * h * h, 192), D.A.PAD_SCORE), torch.full((B * h * h, 192), -D.A.PAD_SCORE)
    lo[:, :C] = torch.randn(B * h * h, C, generator=g)
    t[:, :C] = torch.randn(B * h * h, C, generator=g)
    labels = torch.randint(0, C, (B, h * S, h * S), generator=g)
    labels[:, 100:] = IGN
    pw = 2.0 * torch.rand(labels.shape, generator=g)
    ref = D.kd_ref(lo, t, labels, pw, B, h, h, C, S, "bicubic", temp)
    args = (lo.to(dev), t.to(dev), B, h, h, C, S, ops.INTERP_BICUBIC)
    kw = dict(temperature=temp, labels=labels.to(dev), pixel_weight=pw.to(dev), want_grad=True)
    l1, d1 = ops.head_upsample_kd(*args, **kw)
    l2, d2 = ops.head_upsample_kd(*args, **kw)
    _check("many tiles", l1, d1, ref, C)
    assert torch.equal(l1, l2) and torch.equal(d1, d2)


# ---- 8. the C entry point refuses in the documented order and writes nothing ----
def test_entry_point_refusals_leave_the_outputs_untouched(dev):
    from lc2is_amd import ops
    B, h, w, C, S, ld = 1, 2, 2, 5, 4, 64
    f = ops._fn("lc2is_head_upsample_kd")
    lo, t = torch.randn(B * h * w + 1, ld, device=dev), torch.randn(B * h * w + 1, ld, device=dev)
    labels = torch.zeros(B, h * S, w * S, dtype=torch.long, device=dev)
    pw = torch.ones(B, h * S, w * S, device=dev)
    dlo, loss = torch.full((B * h * w + 1, ld), -7.0, device=dev), torch.full((2,), -7.0, device=dev)
    need = ops._fn("lc2is_head_upsample_ce_workspace_bytes")(B, h, w, C, S, 0, 1)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=dev)
    ok = dict(lo=lo.data_ptr(), tlo=t.data_ptr(), ld=ld, labels=labels.data_ptr(), pw=pw.data_ptr(), dlo=dlo.data_ptr(),
              loss=loss.data_ptr(), B=B, h=h, w=w, C=C, S=S, mode=0, temp=1.0, ws=ws.data_ptr(), wsb=need)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["lo"], a["tlo"], a["ld"], a["labels"], a["pw"], a["dlo"], a["loss"], a["B"], a["h"], a["w"], a["C"], a["S"],
                 a["mode"], IGN, a["temp"], 1.0, a["ws"], a["wsb"], torch.cuda.current_stream().cuda_stream)

    assert call(lo=None) == call(tlo=None) == call(loss=None) == -2                                   # LC2IS_ERR_NULL
    assert call(lo=ok["lo"] + 4) == call(tlo=ok["tlo"] + 8) == call(dlo=ok["dlo"] + 4) == -1          # unaligned: LC2IS_ERR_SHAPE
    assert call(ld=60) == call(ld=96) == call(ld=256) == call(C=193, ld=192) == call(C=65) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(temp=bad) == -1, bad
    assert call(S=2) == call(mode=5) == -3                                                             # LC2IS_ERR_UNSUPPORTED
    assert call(ws=None) == call(ws=ok["ws"] + 4) == call(wsb=need - 1) == -4                          # LC2IS_ERR_WORKSPACE
    assert call(lo=None, temp=0.0, S=2, wsb=0) == -2 and call(temp=0.0, S=2, wsb=0) == -1 and call(S=2, wsb=0) == -3
    torch.cuda.synchronize()
    assert bool((dlo == -7.0).all()) and bool((loss == -7.0).all()) and bool((ws == 0x5A).all())
    # and the good call writes every channel of its rows and nothing behind them
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and loss[1].item() == h * S * w * S
    assert not (dlo[:B * h * w] == -7.0).any() and bool((dlo[B * h * w:] == -7.0).all()) and bool((ws[need:] == 0x5A).all())


# ---- 9. the model layer, on the tiny golden model (K = 151) ----
def _kl_mean64(student_logits, teacher_logits, temp, ok=None, pw=None):
    """weightless mean over the counted pixels of pw_i T^2 KL(teacher || student) on materialised logits, fp64."""
    kl = temp * temp * F.kl_div((student_logits.double() / temp).log_softmax(1), (teacher_logits.double() / temp).softmax(1),
                                reduction="none").sum(1)
    if pw is not None:
        kl = kl * pw.double()
    return kl.mean() if ok is None else kl[ok].sum() / ok.sum()


def _teacher_hi(ts, B, g, K, mode):
    from lc2is_amd.nn.model import head_scores_hi
    return head_scores_hi(ts, B, g, g, K, 4, mode)


def _noisy(inputs, seed=17):
    g = torch.Generator().manual_seed(seed)
    pv = inputs["pixel_values"]
    return {**inputs, "pixel_values": pv + 0.5 * torch.randn(pv.shape, generator=g).to(pv.device)}


def _focal64(logits, labels, gamma):
    lp = logits.double().log_softmax(1)
    ok = labels != IGN
    lpy = lp.gather(1, labels.clamp_min(0)[:, None]).squeeze(1)
    return (((1.0 - lpy.exp()) ** gamma) * -lpy)[ok].sum() / ok.sum()


@pytest.mark.parametrize("base", ["ce", "focal"])
def test_forward_loss_distill_matches_materialised_logits(dev, base):
    from lc2is_amd import ops
    from lc2is_amd.nn.head_loss import Distill
    m, fx = _tiny(dev)
    inputs, labels, pw = _batch(dev, 3, fx)
    labels = labels.clamp_max(150)
    B = labels.shape[0]
    ts = m.head_scores(_noisy(inputs))
    assert ts.dtype == torch.float32 and tuple(ts.shape) == (B * 16, 192) and not ts.requires_grad and ts.is_contiguous()
    weight, temp = 0.7, 2.0
    t_hi = _teacher_hi(ts, B, 4, 151, ops.INTERP_BICUBIC)
    ok = labels != IGN
    kw = dict(focal=(2.0, 0.0)) if base == "focal" else {}

    logits = m(inputs)["outputs"]
    base_u = _focal64(logits, labels, 2.0) if base == "focal" else F.cross_entropy(logits.double(), labels, ignore_index=IGN)
    loss_u = base_u + weight * _kl_mean64(logits, t_hi, temp, ok, pw)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    loss_f = m.forward_loss(inputs, labels, distill=Distill(ts, weight, temp, "labelled", pw), **kw)
    loss_f.backward()
    named = dict(m.named_parameters())
    rels = {k: D.rel(named[k].grad, g_u[k]) for k in GRAD_KEYS}
    print("distill figures forward_loss", base, loss_f.item(), loss_u.item(), base_u.item(), rels)
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert loss_u.item() - base_u.item() > 1e-3 * base_u.item()               # the term is a visible part of the loss
    assert all(bool(g.any()) for g in g_u.values()) and all(r <= 1e-3 for r in rels.values()), rels
    with torch.no_grad():
        # region 'all' without a pixel weight, against the same composition
        l_all = m.forward_loss(inputs, labels, distill=Distill(ts, weight, temp), **kw)
        want = base_u + weight * _kl_mean64(logits, t_hi, temp)
        assert abs(l_all.item() - want.item()) <= 1e-5 * abs(want.item())
        # weight 0 is the base loss; the call without distill gives the same bytes every time, a distill call in between or not
        l0 = m.forward_loss(inputs, labels, **kw)
        lz = m.forward_loss(inputs, labels, distill=Distill(ts, 0.0, temp), **kw)
        assert abs(lz.item() - l0.item()) <= 1e-6 * abs(l0.item())
        assert torch.equal(m.forward_loss(inputs, labels, **kw), l0)
    for p in m.parameters():
        p.grad = None
    g0 = []
    for _ in range(2):
        m.forward_loss(inputs, labels, **kw).backward()
        g0.append({k: named[k].grad.clone() for k in GRAD_KEYS})
        for p in m.parameters():
            p.grad = None
    assert all(torch.equal(g0[0][k], g0[1][k]) for k in GRAD_KEYS)
    # refused on the device too: a teacher of another shape, before a tower runs
    with pytest.raises(ValueError, match="teacher"):
        m.forward_loss(inputs, labels, distill=Distill(ts[:-16].contiguous()))
    with pytest.raises(ValueError, match="teacher"):
        m.forward_loss(inputs, labels, distill=Distill(ts.cpu()))


# ---- 10. the score-map tail (bilinear) ----
def test_score_map_tail_distill(dev):
    import lc2is_amd.nn as N
    from lc2is_amd import ops
    from lc2is_amd.nn.head_loss import Distill
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    tail = N.ScoreMapTail(4)
    ts = tail.scores_lo(ve + 2.0 * torch.randn(ve.shape, generator=g).to(dev), te)
    assert ts.dtype == torch.float32 and tuple(ts.shape) == (B * h * h, 192) and not ts.requires_grad
    weight, temp = 15.0, 0.5   # (the cosine scores lie in [-1, 1] and their KL is small: the weight makes the term visible)
    t_hi = _teacher_hi(ts, B, h, K, ops.INTERP_BILINEAR)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    logits = tail(v1, t1)
    base_u = F.cross_entropy(logits.double(), labels, ignore_index=IGN)
    loss_u = base_u + weight * _kl_mean64(logits, t_hi, temp)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, distill=Distill(ts, weight, temp))
    loss_f.backward()
    print("distill figures score tail", loss_f.item(), loss_u.item(), base_u.item(), D.rel(v2.grad, v1.grad), D.rel(t2.grad, t1.grad))
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert loss_u.item() - base_u.item() > 1e-2 * base_u.item()               # the term is a visible part of the loss
    assert D.rel(v2.grad, v1.grad) <= 1e-3 and D.rel(t2.grad, t1.grad) <= 1e-3
    # the call without distill: the same bytes as before and after
    v3, t3 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    v4, t4 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    la, lb = tail.loss(v3, t3, labels), tail.loss(v4, t4, labels)
    la.backward(); lb.backward()
    assert torch.equal(la, lb) and torch.equal(v3.grad, v4.grad) and torch.equal(t3.grad, t4.grad)


# ---- 11. TrainStep ----
def _teacher_scores(dev, batches):
    """A fixed teacher (the golden model with its class prototypes moved) on each batch's inputs."""
    teacher, _ = _tiny(dev)
    with torch.no_grad():
        g = torch.Generator().manual_seed(4)
        teacher.class_prototypes.add_(0.3 * torch.randn(teacher.class_prototypes.shape, generator=g).to(dev))
    return [teacher.head_scores(b[0]) for b in batches]


def test_train_step_with_distill(dev):
    """One SGD step with distill moves the parameters as the reference composition on the materialised logits does."""
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep
    lr, weight, temp = 1e-2, 0.5, 2.0
    m1, fx = _tiny(dev)
    m2, _ = _tiny(dev)
    inputs, labels, pw = _batch(dev, 3, fx)
    labels = labels.clamp_max(150)
    (ts,) = _teacher_scores(dev, [(inputs,)])
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    step = TrainStep(m1, optimizer="sgd", lr=lr, distill=(weight, temp, "all"))
    loss_ts = step.step_distill(inputs, labels, ts, pw)
    logits = m2(inputs)["outputs"]
    t_hi = _teacher_hi(ts, labels.shape[0], 4, 151, ops.INTERP_BICUBIC)
    loss_h = F.cross_entropy(logits.double(), labels, ignore_index=IGN) + weight * _kl_mean64(logits, t_hi, temp, None, pw)
    loss_h.backward()
    named1, named2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    rels = {k: D.rel(named1[k].detach() - start[k], -lr * named2[k].grad) for k in STEP_KEYS}
    print("distill figures train step", loss_ts.item(), loss_h.item(), rels)
    assert abs(loss_ts.item() - loss_h.item()) <= 1e-4 * abs(loss_h.item())
    assert all(r < 8e-2 for r in rels.values()), rels
    # refusals, before anything runs
    with pytest.raises(NotImplementedError, match="accumulate"):
        TrainStep(m2, optimizer="sgd", lr=lr, distill=(weight, temp, "all"), accumulate=2)
    with pytest.raises(ValueError, match="teacher_scores"):
        step.step(inputs, labels)
    with pytest.raises(ValueError, match="teacher_scores"):
        step.capture(inputs, labels)
    with pytest.raises(ValueError, match="distill="):
        TrainStep(m2, optimizer="sgd", lr=lr).step_distill(inputs, labels, ts)


def test_captured_step_with_distill_replays_bitwise(dev):
    """A step captured with teacher scores, replayed on two other batches and teachers, is bitwise the eager step; seg_metrics
    rides along; a replay that omits the teacher is refused."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(3)]
    teachers = _teacher_scores(dev, batches)
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    mk = lambda m: TrainStep(m, optimizer="sgd", lr=1e-3, criterion=N.CrossEntropyLoss(label_smoothing=0.1), seg_metrics=True,   # noqa: E731
                             distill=(0.5, 2.0, "labelled"))
    ts_e, ts_g = mk(m_e), mk(m_g)
    for _ in range(2):
        ts_e.step_distill(batches[0][0], batches[0][1], teachers[0])
    run = ts_g.capture_distill(batches[0][0], batches[0][1], teachers[0])
    torch.cuda.synchronize()
    for b, t in zip(batches[1:], teachers[1:]):
        eager = ts_e.step_distill(b[0], b[1], t).clone()
        assert torch.equal(eager, run(b[0], b[1], teacher_scores=t).clone())
    torch.cuda.synchronize()
    assert torch.equal(ts_e.arena.flat, ts_g.arena.flat) and torch.equal(ts_e.seg_counts, ts_g.seg_counts)
    assert torch.equal(run.static_teacher_scores, teachers[2]) and run.static_teacher_weight is None
    with pytest.raises(ValueError, match="teacher_scores"):
        run(batches[1][0], batches[1][1])
    with pytest.raises(ValueError, match="teacher_weight"):
        run(batches[1][0], batches[1][1], teacher_scores=teachers[1], teacher_weight=batches[1][2])
    run.release()


# ---- 12. one soft mean-teacher cycle ----
def test_one_soft_mean_teacher_cycle(dev):
    """with step.ema_weights(): ts = model.head_scores(weak); step.step_distill(inputs, labels, ts): a finite loss, the
    parameters move, and leaving the block restores the student bitwise.
    Which assertion: the finite step ONLY.  The EMA's warm-up weight is max(1 - decay, 9 / (10 + updates)) < 1, so after the first
    update the EMA is a blend of the initial and the updated weights, not the student: the bookkeeping does not make 'teacher ==
    student, KD term exactly 0' hold, and that identity is asserted at the kernel level instead
    (test_teacher_equal_to_student_gives_exact_zero), and here with the student's own scores as the teacher's."""
    from lc2is_amd.step import TrainStep
    m, fx = _tiny(dev)
    inputs, labels, _ = _batch(dev, 3, fx)
    labels = labels.clamp_max(150)
    step = TrainStep(m, optimizer="sgd", lr=1e-2, ema_decay=0.99, ema_warmup=True, distill=(1.0, 1.0, "all"))
    ts0 = m.head_scores(inputs)
    step.step_distill(inputs, labels, ts0)
    student = step.arena.flat.clone()
    with step.ema_weights():
        assert not torch.equal(step.arena.flat, student)             # the teacher's weights: a blend, not the student
        ts = m.head_scores(_noisy(inputs))                           # the teacher sees the weak view
    assert torch.equal(step.arena.flat, student)
    loss = step.step_distill(inputs, labels, ts)
    assert bool(torch.isfinite(loss)) and not torch.equal(step.arena.flat, student)
    # the student's own scores as the teacher's: the KD term is exactly 0 and the step is the step without distill, bitwise
    m_a, _ = _tiny(dev)
    m_b, _ = _tiny(dev)
    s_a = TrainStep(m_a, optimizer="sgd", lr=1e-2, distill=(1.0, 2.0, "all"))
    s_b = TrainStep(m_b, optimizer="sgd", lr=1e-2)
    l_a = s_a.step_distill(inputs, labels, m_a.head_scores(inputs))
    l_b = s_b.step(inputs, labels)
    assert torch.equal(l_a, l_b) and torch.equal(s_a.arena.flat, s_b.arena.flat)
