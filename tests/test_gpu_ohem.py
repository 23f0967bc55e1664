"""OHEM cross-entropy on the HIP path: the exact device-side selection against torch.sort on the same values, the per-pixel loss of
the fused head against fp64, the fused and unfused OHEM losses against fp64 with the GPU's own mask as an input of the oracle (as for
dropout), the model heads against the unfused module, and the train step (eager, captured, bitwise reproducible).

Band rule (tests 3 and 4): the GPU's per-pixel losses are within e = 1e-4 of fp64 (test 2's max-abs bound: about 20 fp32 roundings
at |value| <= 32, 4e-5), so the pivot moves by at most e and every pixel with |l64 - L_eff64| > 2e must be classified exactly as
the fp64 rule classifies it; the reference alone must hold at most 4 valid pixels inside the band."""
import functools
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ohem_ref as R  # noqa: E402
from head_cases import head_case as _head_case  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = -100
BAND_E = 1e-4


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _weights(C, seed):
    return torch.rand(C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 1.5 + 0.25


# ---- 1. the selection is exact ---------------------------------------------------------------------------------------
def _values(family, n, g):
    if family == "continuous":
        return torch.rand(n, generator=g) * 5 + 1e-3
    if family == "quantised":
        return torch.randint(0, 8, (n,), generator=g).float() * 0.37
    if family == "equal":
        return torch.full((n,), 1.25)
    if family == "ulps":      # consecutive bit patterns above 1.0: only the low digits differ
        return (0x3F800000 + torch.randint(0, 300, (n,), generator=g, dtype=torch.int32)).view(torch.float32)
    if family == "exponents":  # one value per exponent: only the high digits differ
        return (torch.randint(1, 255, (n,), generator=g, dtype=torch.int32) << 23).view(torch.float32)
    assert family == "mixed"
    pool = torch.tensor([0.0, -0.0, -1e-7, 1e-45, 1e-40, float("inf"), 0.5, 2.0, 3e-39, 1e-7])
    return pool[torch.randint(0, pool.numel(), (n,), generator=g)]


def _sel_labels(n, C, g):
    labels = torch.randint(0, C, (n,), generator=g)
    r = torch.rand(n, generator=g)
    labels[r < 0.15] = IGN
    labels[(r >= 0.15) & (r < 0.22)] = -1
    labels[(r >= 0.22) & (r < 0.30)] = C + 2
    return labels


def _check_select(ops, dev, v, labels, C, thresh, K):
    out, info = ops.ohem_select(v.to(dev), labels.to(dev), C, thresh, K, IGN)
    got = ops.ohem_info_fields(info)
    ref = R.ohem_rule(v, labels, C, IGN, thresh, K)
    ctx = (v.numel(), thresh, K, got, ref["n_valid"], ref["k"], float(ref["L"]), float(ref["L_eff"]))
    assert got["n_valid"] == ref["n_valid"] and got["k"] == ref["k"], ctx
    assert got["L"] == float(ref["L"]) and got["L_eff"] == float(ref["L_eff"]), ctx
    assert torch.equal(out.cpu(), ref["labels_out"]), ctx
    return out, info


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 100003])
@pytest.mark.parametrize("family", ["continuous", "quantised", "equal", "ulps", "exponents", "mixed"])
def test_selection_is_exact(dev, family, n):
    from lc2is_amd import ops
    C = 7
    g = torch.Generator().manual_seed(1000 * n % 9973 + len(family))
    v = _values(family, n, g)
    labels = _sel_labels(n, C, g)
    nv = int(R.valid_mask(labels, C, IGN).sum())
    for K in sorted({0, 1, nv // 3, max(nv - 1, 0), nv, 10 * n}):
        for thresh in (1.0, 0.7, 1e-6):
            _check_select(ops, dev, v, labels, C, thresh, K)
    a = ops.ohem_select(v.to(dev), labels.to(dev), C, 0.7, nv // 3, IGN)
    b = ops.ohem_select(v.to(dev), labels.to(dev), C, 0.7, nv // 3, IGN)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])   # (the info block as int64 words: the same bytes)


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_selection_with_no_or_one_valid_pixel(dev, n):
    from lc2is_amd import ops
    g = torch.Generator().manual_seed(n)
    v = torch.rand(n, generator=g) + 0.5
    none = torch.full((n,), IGN)
    none[::3] = -2
    one = none.clone()
    one[n // 2] = 3
    for labels in (none, one):
        for K in (0, 1, 10 * n):
            for thresh in (1.0, 0.7, 1e-6):
                out, info = _check_select(ops, dev, v, labels, 5, thresh, K)
    f = ops.ohem_info_fields(ops.ohem_select(v.to(dev), none.to(dev), 5, 0.7, 3, IGN)[1])
    assert f["n_valid"] == 0 and f["k"] == -1 and f["L"] == float("inf")


def test_selection_refuses_bad_arguments(dev):
    from lc2is_amd import ops
    v = torch.rand(16, device=dev)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.ohem_select(v, torch.zeros(8, dtype=torch.long, device=dev), 3, 0.7, 2)
    with pytest.raises(ValueError, match="thresh"):
        ops.ohem_select(v, torch.zeros(16, dtype=torch.long, device=dev), 3, 0.0, 2)
    with pytest.raises(ValueError, match="min_kept"):
        ops.ohem_select(v, torch.zeros(16, dtype=torch.long, device=dev), 3, 0.7, -2)


# ---- 2 / 3. per-pixel loss of the fused head, and fused OHEM at op level ---------------------------------------------
HEAD_CASES = [("bicubic", 4, 151, 5, 5), ("bilinear", 4, 150, 12, 7), ("bicubic", 8, 37, 7, 5), ("bilinear", 16, 64, 5, 5),
              ("bicubic", 16, 150, 3, 5), ("bilinear", 8, 192, 4, 6)]
# behind them, the (mode, S, TN) instantiations of head_px_grp_kernel that the six do not reach
HEAD_CASES += [
    ("bicubic", 4, 10, 5, 7), ("bicubic", 4, 100, 5, 7), ("bicubic", 4, 192, 5, 7), ("bicubic", 8, 100, 5, 4),
    ("bicubic", 8, 151, 5, 4), ("bicubic", 8, 192, 5, 4), ("bicubic", 16, 10, 3, 4), ("bicubic", 16, 100, 3, 4),
    ("bicubic", 16, 192, 3, 4), ("bilinear", 4, 10, 5, 7), ("bilinear", 4, 100, 5, 7), ("bilinear", 4, 192, 5, 7),
    ("bilinear", 8, 10, 5, 4), ("bilinear", 8, 100, 5, 4), ("bilinear", 8, 151, 5, 4), ("bilinear", 16, 100, 3, 4),
    ("bilinear", 16, 151, 3, 4), ("bilinear", 16, 192, 3, 4)]
HEAD_B = 2


@functools.lru_cache(maxsize=None)
def _head_ref(mode, S, C, h, w):
    """Inputs and the fp64 reference of one case, computed once: upsampled logits [B,C,H,W] and per-pixel plain CE [B,H,W]."""
    lo, labels, ref_labels = _head_case(HEAD_B, h, w, C, S, 31 * C + S)
    lod = lo[:, :C].double().reshape(HEAD_B, h, w, C).permute(0, 3, 1, 2).contiguous()
    up = F.interpolate(lod, scale_factor=S, mode=mode)
    l64 = F.cross_entropy(up, ref_labels, reduction="none")
    return lo, labels, ref_labels, lod, l64


def _mode(ops, mode):
    return ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR


@pytest.mark.parametrize("mode,S,C,h,w", HEAD_CASES)
def test_head_upsample_px_vs_fp64(dev, mode, S, C, h, w):
    from lc2is_amd import ops
    lo, labels, ref_labels, _, l64 = _head_ref(mode, S, C, h, w)
    lod, lbd = lo.to(dev), labels.to(dev)
    lpx = ops.head_upsample_px(lod, lbd, HEAD_B, h, w, C, S, _mode(ops, mode))
    again = ops.head_upsample_px(lod, lbd, HEAD_B, h, w, C, S, _mode(ops, mode))
    assert lpx.shape == l64.shape and lpx.dtype == torch.float32
    rel, mab = _rel(lpx, l64), (lpx.cpu().double() - l64).abs().max().item()
    print(f"head_upsample_px {mode} S={S} C={C} {h}x{w}: rel-L2 {rel:.3e} max-abs {mab:.3e}")
    assert rel <= 2e-5 and mab <= 1e-4
    assert bool((lpx.cpu()[ref_labels == IGN] == 0).all())   # not counted: 0
    assert torch.equal(lpx.view(torch.int32), again.view(torch.int32))


def _band_check(l64, labels, C, thresh, K, kept_gpu):
    """The band rule; returns the fp64 rule's result.  kept_gpu: bool, labels' shape (CPU)."""
    ref = R.ohem_rule(l64, labels, C, IGN, thresh, K)
    valid = R.valid_mask(labels, C, IGN)
    outside = valid & ((l64 - ref["L_eff"]).abs() > 2 * BAND_E)
    inside = int((valid & ~outside).sum())
    assert inside <= 4, f"the reference holds {inside} valid pixels inside the band"
    assert torch.equal(kept_gpu[outside], ref["kept"][outside])
    assert not bool(kept_gpu[~valid].any())
    return ref, inside


OHEM_SETTINGS = [(0.7, 4), (1e-6, 4), (0.02, 0)]   # (thresh, HW / min_kept per image; 0 = min_kept 0)


@pytest.mark.parametrize("mode,S,C,h,w", HEAD_CASES)
def test_fused_ohem_op_level_vs_fp64(dev, mode, S, C, h, w):
    from lc2is_amd import ops
    lo, labels, ref_labels, lod64, l64 = _head_ref(mode, S, C, h, w)
    B, H, W = HEAD_B, h * S, w * S
    lod, lbd = lo.to(dev), labels.to(dev)
    for thresh, div in OHEM_SETTINGS:
        min_kept = H * W // div if div else 0
        kept_lab, info = ops.ohem_labels(lod, lbd, B, h, w, C, S, _mode(ops, mode), IGN, (thresh, min_kept))
        kl = kept_lab.cpu()
        kept_gpu = kl != IGN
        assert torch.equal(kl[kept_gpu], labels[kept_gpu])
        ref, inside = _band_check(l64, labels, C, thresh, min_kept * B, kept_gpu)
        rank_binding = bool(ref["L"] < R.tau32(thresh).double())
        assert rank_binding == (thresh == 1e-6), (thresh, float(ref["L"]))   # both branches occur across the settings
        f = ops.ohem_info_fields(info)
        assert f["n_valid"] == ref["n_valid"] and f["k"] == ref["k"] and abs(f["L_eff"] - float(ref["L_eff"])) <= BAND_E
        # loss and gradient against fp64 CE on the GPU's own labels
        loss, dlo, _ = ops.head_upsample_ce(lod, kept_lab, B, h, w, C, S, _mode(ops, mode), want_grad=True)
        x = lod64.clone().requires_grad_(True)
        r = F.cross_entropy(F.interpolate(x, scale_factor=S, mode=mode), kl, reduction="sum")
        r.backward()
        assert int(kept_gpu.sum()) > 0 and loss[1].item() == float(kept_gpu.sum())
        assert abs(loss[0].item() - r.item()) <= 1e-4 * abs(r.item())
        assert _rel(dlo[:, :C], x.grad.permute(0, 2, 3, 1).reshape(B * h * w, C)) <= 2e-5


# ---- 4. the module on materialised logits ----------------------------------------------------------------------------
@pytest.mark.parametrize("thresh,div", [(1e-6, 4), (0.004, 0)])
def test_ohem_module_on_nchw_logits(dev, thresh, div):
    import lc2is_amd.nn as N
    from lc2is_amd import ops
    B, C, H, W = 2, 151, 24, 20
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g) * 2
    labels = torch.randint(0, C, (B, H, W), generator=g)
    labels[:, ::4] = IGN
    w64 = _weights(C, 2)
    min_kept = H * W // div if div else 0
    crit = N.OhemCrossEntropyLoss(thresh, min_kept, weight=w64.float(), label_smoothing=0.1).to(dev)
    xd = x.to(dev).requires_grad_(True)
    loss = crit(xd, labels.to(dev))
    kl = crit.last_labels.cpu()
    kept_gpu = kl != IGN
    x64 = x.double().requires_grad_(True)
    l64 = F.cross_entropy(x64.detach(), labels, reduction="none")
    ref, inside = _band_check(l64, labels, C, thresh, min_kept * B, kept_gpu)
    assert bool(ref["L"] < R.tau32(thresh).double()) == (thresh == 1e-6)   # one rank-binding, one threshold-binding setting
    assert 0 < int(kept_gpu.sum()) < ref["n_valid"] and ops.ohem_info_fields(crit.last_info)["n_valid"] == ref["n_valid"]
    r = F.cross_entropy(x64, kl, weight=w64, label_smoothing=0.1)
    assert _rel(loss.detach(), r.detach()) <= 1e-5
    loss.backward()
    r.backward()
    assert _rel(xd.grad, x64.grad) <= 1e-5
    # the selection never sees the weights or the smoothing
    plain = N.OhemCrossEntropyLoss(thresh, min_kept).to(dev)
    plain(x.to(dev), labels.to(dev))
    assert torch.equal(plain.last_labels, crit.last_labels) and torch.equal(plain.last_info, crit.last_info)
    # eval(): the plain criterion, bit for bit
    e = crit.eval()(x.to(dev), labels.to(dev))
    p = N.CrossEntropyLoss(weight=w64.float(), label_smoothing=0.1).to(dev)(x.to(dev), labels.to(dev))
    assert torch.equal(e, p)


# ---- 5. model level ---------------------------------------------------------------------------------------------------
def _tiny(dev):
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    fx = torch.load(Path(__file__).resolve().parent / "golden" / "base_tiny.pt", weights_only=True)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


GRAD_KEYS = ("class_prototypes", "vision_decoder.layers.0.linear2.weight")


def _thresh_in_a_gap(logits, labels, C):
    """A threshold (with min_kept = 0) no pixel is close to: the middle of the widest gap between neighbouring per-pixel losses, the
    lowest and the highest hundredth of their sorted order left out (so that some pixels are kept and some dropped).  Asserts that no valid pixel lies within 1e-3 of tau."""
    import math
    from lc2is_amd import ops
    _, _, lpx = ops.ce_nchw_fwd(logits.detach().float().contiguous(), labels.contiguous(), IGN, per_pixel=True)
    v = lpx[R.valid_mask(labels, C, IGN)].double().cpu().sort().values
    q = v[v.numel() // 100 + 1: v.numel() - v.numel() // 100 - 1]
    i = int((q[1:] - q[:-1]).argmax())
    thresh = math.exp(-0.5 * (float(q[i]) + float(q[i + 1])))
    tau = float(R.tau32(thresh))
    assert float((v - tau).abs().min()) > 1e-3 and float(v[0]) < tau < float(v[-1])
    return thresh


def test_forward_loss_ohem_matches_unfused_module(dev):
    import lc2is_amd.nn as N
    m, fx = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev).clone()
    labels[:, :3] = IGN
    with torch.no_grad():
        thresh = _thresh_in_a_gap(m(inputs)["outputs"], labels, 151)
    crit = N.OhemCrossEntropyLoss(thresh, 0).to(dev)
    loss_u = crit(m(inputs)["outputs"], labels)
    loss_u.backward()
    g_u = {k: p.grad.clone() for k, p in m.named_parameters() if k in GRAD_KEYS}
    for p in m.parameters():
        p.grad = None
    loss_f = m.forward_loss(inputs, labels, ohem=(thresh, 0))
    loss_f.backward()
    kept_f, info_f = m.last_ohem
    assert torch.equal(kept_f, crit.last_labels) and 0 < int((kept_f != IGN).sum()) < int((labels != IGN).sum())
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    named = dict(m.named_parameters())
    for k in GRAD_KEYS:
        assert _rel(named[k].grad, g_u[k]) <= 1e-3, k


def test_score_map_tail_ohem_matches_unfused_module(dev):
    import lc2is_amd.nn as N
    B, h, C, K = 2, 8, 64, 150
    g = torch.Generator().manual_seed(21)
    ve = torch.randn(B, h * h, C, generator=g).to(dev)
    te = torch.randn(B, K, C, generator=g).to(dev)
    labels = torch.randint(0, K, (B, 4 * h, 4 * h), generator=g)
    labels[:, ::6] = IGN
    labels = labels.to(dev)
    tail = N.ScoreMapTail(4)
    with torch.no_grad():
        thresh = _thresh_in_a_gap(tail(ve, te), labels, K)
    crit = N.OhemCrossEntropyLoss(thresh, 0).to(dev)
    v1, t1 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_u = crit(tail(v1, t1), labels)
    loss_u.backward()
    v2, t2 = ve.clone().requires_grad_(True), te.clone().requires_grad_(True)
    loss_f = tail.loss(v2, t2, labels, ohem=(thresh, 0))
    loss_f.backward()
    assert torch.equal(tail.last_ohem[0], crit.last_labels)
    assert 0 < int((crit.last_labels != IGN).sum()) < int((labels != IGN).sum())
    assert abs(loss_f.item() - loss_u.item()) <= 1e-5 * abs(loss_u.item())
    assert _rel(v2.grad, v1.grad) <= 1e-3 and _rel(t2.grad, t1.grad) <= 1e-3


# ---- 6. train step ----------------------------------------------------------------------------------------------------
def test_train_step_with_ohem_criterion(dev):
    import lc2is_amd.nn as N
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep
    lr = 1e-2
    m1, fx = _tiny(dev)
    m2, _ = _tiny(dev)
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev)
    with torch.no_grad():
        thresh = _thresh_in_a_gap(m2(inputs)["outputs"], labels, 151)
    crit = N.OhemCrossEntropyLoss(thresh, 0, weight=_weights(151, 14).float(), label_smoothing=0.1).to(dev)
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    ts = TrainStep(m1, optimizer="sgd", lr=lr, criterion=crit)
    assert ts.ohem_info is None
    loss_ts = ts.step(inputs, labels)
    kept_ts, info_ts = ts.ohem_labels.clone(), ts.ohem_info.clone()
    loss_h = crit(m2(inputs)["outputs"], labels)          # the same step by hand, unfused
    loss_h.backward()
    assert torch.equal(kept_ts, crit.last_labels) and 0 < int((kept_ts != IGN).sum()) < int(R.valid_mask(labels, 151, IGN).sum())
    assert ops.ohem_info_fields(info_ts)["n_valid"] == int(R.valid_mask(labels, 151, IGN).sum())
    assert abs(loss_ts.item() - loss_h.item()) <= 1e-4 * abs(loss_h.item())
    named1, named2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    for k in GRAD_KEYS + ("pixel_patch.visual.weight", "vision_encoder.enc.embeddings.patch_embedding.weight",
                          "text_encoder.enc.embeddings.token_embedding.weight"):
        r = _rel(named1[k].detach() - start[k], -lr * named2[k].grad)
        assert r < 8e-2, (k, r)
    # criterion.eval(): the step runs the plain criterion
    crit.eval()
    m3, _ = _tiny(dev)
    m4, _ = _tiny(dev)
    plain = N.CrossEntropyLoss(weight=_weights(151, 14).float(), label_smoothing=0.1).to(dev)
    a = TrainStep(m3, optimizer="sgd", lr=lr, criterion=crit).step(inputs, labels)
    b = TrainStep(m4, optimizer="sgd", lr=lr, criterion=plain).step(inputs, labels)
    assert torch.equal(a, b)


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
             "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)},
            torch.randint(0, 151, (2, 16, 16), generator=g).to(dev))


@pytest.mark.parametrize("kind,kw", [("sgd", {}), ("adamw", dict(max_grad_norm=1.0, skip_nonfinite=True))])
def test_captured_step_with_ohem_criterion(dev, kind, kw):
    """Capture and replay over two new batches equals eager; the kept count differs between the batches: the selection is
    data-driven inside the graph.  The second case runs the device-held optimizer path."""
    import lc2is_amd.nn as N
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep
    batches = [_batch(dev, s) for s in range(3)]
    m_e, _ = _tiny(dev)
    m_g, _ = _tiny(dev)
    mk = lambda: N.OhemCrossEntropyLoss(0.0067, 32, weight=_weights(151, 15).float(), label_smoothing=0.1).to(dev)
    ts_e = TrainStep(m_e, optimizer=kind, lr=1e-3, criterion=mk(), **kw)
    ts_g = TrainStep(m_g, optimizer=kind, lr=1e-3, criterion=mk(), **kw)
    for _ in range(2):
        ts_e.step(*batches[0])
    run = ts_g.capture(*batches[0])
    torch.cuda.synchronize()
    le, lg, kept = [], [], []
    for inp, lab in batches[1:]:
        le.append(ts_e.step(inp, lab).item())
        lg.append(run(inp, lab).item())
        assert torch.equal(ts_g.ohem_labels, ts_e.ohem_labels) and torch.equal(ts_g.ohem_info, ts_e.ohem_info)
        kept.append(int((ts_g.ohem_labels != IGN).sum()))
        assert ops.ohem_info_fields(ts_g.ohem_info)["n_valid"] == lab.numel()
    torch.cuda.synchronize()
    assert le == pytest.approx(lg, abs=1e-5), (le, lg)
    assert kept[0] != kept[1] and all(0 < c < 512 for c in kept), kept
    run.release()


def test_ohem_step_is_bitwise_reproducible(dev):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    inp, lab = _batch(dev, 7)
    outs = []
    for _ in range(2):
        m, _ = _tiny(dev)
        crit = N.OhemCrossEntropyLoss(0.0067, 32, weight=_weights(151, 15).float(), label_smoothing=0.1).to(dev)
        ts = TrainStep(m, optimizer="sgd", lr=1e-2, momentum=0.9, criterion=crit)
        losses = [ts.step(inp, lab).clone() for _ in range(2)]
        outs.append((losses, ts.arena.flat.clone(), ts.ohem_labels.clone(), ts.ohem_info.clone()))
    (l0, p0, k0, i0), (l1, p1, k1, i1) = outs
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    assert torch.equal(p0, p1) and torch.equal(k0, k1) and torch.equal(i0, i1)
