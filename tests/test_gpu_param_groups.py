"""Parameter groups at the op level (lc2is_amd/csrc/optim.hip: sgd_groups_kernel / adamw_groups_kernel): one launch over an
arena-like buffer with a learning-rate factor and a weight decay per 64-element granule.

The yardstick for the bits is the EXISTING pair ops.sgd_step_ctrl / ops.adamw_step_ctrl run range by range with the control
block's lr word overwritten by fp32(lr) * fp32(scale) and the range's decay as the argument; torch.optim with param_groups is
the yardstick for the arithmetic.

Step level (TrainStep(param_groups=...)): tiny BaseModelWithText twins; the step is bitwise reproducible, which is what makes
these comparisons exact."""
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
G = ROOT / "tests" / "golden"
MAX_NORM = 0.05                              # below every gradient norm these tiny random-init models produce (asserted)

SKIP = 255
N_BITS = 64 * (4096 * 16 * 3 + 77)           # more than one grid-stride round of 4096 blocks x 256 lanes x 4 elements, ragged


def _ctrl(dev):
    from lc2is_amd import ops
    c = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32, device=dev)
    return c, c.view(torch.float32)


def _update(ctrl, gr, table, **kw):
    from lc2is_amd import ops
    partials, flags = ops.grad_sumsq(gr)
    ops.optim_ctrl_update(ctrl, partials, flags, table, **kw)


def _random_map(granules, ngroups, seed):
    """Runs of 1-300 granules of one group each, about one run in six carrying the skip id.  Returns the uint8 CPU map and the
    runs as (first granule, end granule, id)."""
    g = torch.Generator().manual_seed(seed)
    ids, runs, at = torch.empty(granules, dtype=torch.uint8), [], 0
    while at < granules:
        length = min(int(torch.randint(1, 301, (1,), generator=g)), granules - at)
        gid = SKIP if int(torch.randint(0, 6, (1,), generator=g)) == 0 else int(torch.randint(0, ngroups, (1,), generator=g))
        if runs and runs[-1][2] == gid:
            gid = (gid + 1) % ngroups
        ids[at:at + length] = gid
        runs.append((at, at + length, gid))
        at += length
    return ids, runs


def _run_kind(kind, n, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev)
    s1 = torch.zeros(n, device=dev) if kind in ("sgd_mom", "adamw") else None
    s2 = torch.zeros(n, device=dev) if kind == "adamw" else None
    return p, s1, s2


def _launch_groups(kind, p, gr, s1, s2, ctrl, gmap, table, reverse=False):
    from lc2is_amd import ops
    if kind == "adamw":
        ops.adamw_step_groups(p, gr, s1, s2, ctrl, gmap, table, 0.9, 0.999, 1e-8, reverse=reverse)
    else:
        ops.sgd_step_groups(p, gr, s1, ctrl, gmap, table, 0.9 if kind == "sgd_mom" else 0.0, reverse=reverse)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "sgd_mom", "adamw"])
def test_grouped_launch_gives_the_bits_of_the_ctrl_kernels_range_by_range(dev, kind, reverse):
    from lc2is_amd import ops
    n = N_BITS
    scales = [1.0, 0.1, 0.0, 0.37, 2.5]
    decays = [0.01, 0.0, 0.05, 0.1, 0.003]
    table_cpu = torch.tensor(list(zip(scales, decays)), dtype=torch.float32)
    ids, runs = _random_map(n // 64, len(scales), seed=17)
    assert {r[2] for r in runs} == set(range(len(scales))) | {SKIP} and len(runs) > 300
    gmap, table = ids.to(dev), table_cpu.to(dev)
    lr_table = torch.tensor([0.07, 0.05, 0.03], device=dev)
    p_new, s1_new, s2_new = _run_kind(kind, n, dev)
    p_ref, s1_ref, s2_ref = p_new.clone(), None if s1_new is None else s1_new.clone(), None if s2_new is None else s2_new.clone()
    start = p_new.clone()
    ctrl, ctrl_f = _ctrl(dev)
    g = torch.Generator().manual_seed(23)
    for step in range(3):
        gr = torch.randn(n, generator=g).to(dev)
        assert bool(torch.isfinite(gr).all())
        _update(ctrl, gr, lr_table, grad_scale=0.5, max_norm=1.0, beta1=0.9, beta2=0.999)
        assert ctrl_f[ops.CTRL_CLIP_COEF].item() < 1.0                      # clipping is active
        _launch_groups(kind, p_new, gr, s1_new, s2_new, ctrl, gmap, table, reverse=reverse)
        # the reference: the existing kernels, one launch per run, lr word = fp32(lr) * fp32(scale) formed in fp32 on the host
        lr = torch.tensor(ctrl_f[ops.CTRL_LR].item(), dtype=torch.float32)
        rates = [(lr * table_cpu[k, 0]).item() for k in range(len(scales))]       # one fp32 multiplication each, on the host
        ctrl_r = ctrl.clone()
        ctrl_rf = ctrl_r.view(torch.float32)
        for lo, hi, gid in runs:
            if gid == SKIP:
                continue
            sl = slice(lo * 64, hi * 64)
            ctrl_rf[ops.CTRL_LR] = rates[gid]
            if kind == "adamw":
                ops.adamw_step_ctrl(p_ref[sl], gr[sl], s1_ref[sl], s2_ref[sl], ctrl_r, 0.9, 0.999, 1e-8, decays[gid])
            else:
                ops.sgd_step_ctrl(p_ref[sl], gr[sl], None if s1_ref is None else s1_ref[sl], ctrl_r,
                                  0.9 if kind == "sgd_mom" else 0.0, decays[gid])
    assert torch.equal(p_new, p_ref)
    for a, b in ((s1_new, s1_ref), (s2_new, s2_ref)):
        if a is not None:
            assert torch.equal(a, b)
    assert not torch.equal(p_new, start)
    skipped = (ids == SKIP).to(dev).repeat_interleave(64)
    assert torch.equal(p_new[skipped], start[skipped]) and int(skipped.sum()) > 0


@pytest.mark.parametrize("kind", ["sgd", "sgd_mom", "adamw"])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_grouped_optimizers_vs_torch_param_groups(dev, clip, kind):
    """test_optimizers_ctrl_vs_torch's cases with the vector split into three torch.optim param groups (lr = base * scale, own
    weight_decay), with and without clip_grad_norm_ over all three; the project's tolerance for the same arithmetic."""
    from lc2is_amd import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    n = 4096 * 3
    p0 = torch.randn(n, generator=g).to(dev)
    cuts = [(0, 4096 + 640), (4096 + 640, 2 * 4096 + 64), (2 * 4096 + 64, n)]
    scales, decays = [1.0, 0.1, 0.5], [0.01, 0.0, 0.1]
    ids = torch.empty(n // 64, dtype=torch.uint8)
    for k, (lo, hi) in enumerate(cuts):
        ids[lo // 64:hi // 64] = k
    gmap = ids.to(dev)
    table = torch.tensor(list(zip(scales, decays)), dtype=torch.float32, device=dev)
    p = p0.clone()
    pts = [torch.nn.Parameter(p0[lo:hi].clone()) for lo, hi in cuts]
    ctrl, ctrl_f = _ctrl(dev)
    base = 1e-2 if kind == "adamw" else 0.1
    pg = [dict(params=[pt], lr=base * s, weight_decay=w) for pt, s, w in zip(pts, scales, decays)]
    if kind == "sgd":
        opt, s1, s2 = torch.optim.SGD(pg, lr=base), None, None
    elif kind == "sgd_mom":
        opt, s1, s2 = torch.optim.SGD(pg, lr=base, momentum=0.9), torch.zeros(n, device=dev), None
    else:
        opt = torch.optim.AdamW(pg, lr=base, betas=(0.9, 0.999), eps=1e-8)
        s1, s2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr_table = torch.tensor([base], device=dev)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g).to(dev)
        for pt, (lo, hi) in zip(pts, cuts):
            pt.grad = gr[lo:hi].clone()
        if clip is not None:
            total = torch.nn.utils.clip_grad_norm_(pts, clip)
            assert total.item() > clip
        else:
            total = torch.linalg.vector_norm(gr)
        opt.step()
        _update(ctrl, gr, lr_table, max_norm=float("inf") if clip is None else clip, beta1=0.9, beta2=0.999)
        _launch_groups(kind, p, gr, s1, s2, ctrl, gmap, table)
        assert (ctrl_f[ops.CTRL_CLIP_COEF].item() < 1.0) == (clip is not None)
        assert ctrl_f[ops.CTRL_GRAD_NORM].item() == pytest.approx(total.item(), rel=1e-5)      # one norm over all three groups
    want = torch.cat([pt.data for pt in pts])
    assert torch.allclose(p, want, atol=2e-6, rtol=1e-5), (kind, clip, (p - want).abs().max().item())


@pytest.mark.parametrize("kind", ["sgd_mom", "adamw"])
def test_skipped_step_and_skipped_granules_touch_nothing(dev, kind):
    from lc2is_amd import ops
    n = 64 * (16 * 300 + 2)
    ids, runs = _random_map(n // 64, 3, seed=29)
    gmap = ids.to(dev)
    dead = (ids == SKIP).to(dev).repeat_interleave(64)
    assert 0 < int(dead.sum()) < n
    table = torch.tensor([[1.0, 0.05], [0.5, 0.01], [0.25, 0.1]], device=dev)       # weight decay > 0 in every group
    p = torch.randn(n, device=dev)
    s1, s2 = torch.randn(n, device=dev), (torch.rand(n, device=dev) if kind == "adamw" else None)
    state = [t for t in (p, s1, s2) if t is not None]
    gr = torch.randn(n, device=dev)
    lr_table = torch.tensor([0.1], device=dev)
    ctrl, _ = _ctrl(dev)
    start = [t.clone() for t in state]

    def run(grad_for_launch=None):
        _update(ctrl, gr, lr_table, max_norm=1.0, skip_nonfinite=True, beta1=0.9, beta2=0.999)
        _launch_groups(kind, p, gr if grad_for_launch is None else grad_for_launch, s1, s2, ctrl, gmap, table)

    run()                                                    # an applied step: the id-255 granules keep their bits
    assert ctrl[ops.CTRL_APPLIED].item() == 1
    for t, b in zip(state, start):
        assert torch.equal(t[dead], b[dead]) and not torch.equal(t[~dead], b[~dead])
    # they are not read either: norm and verdict from the clean gradient, NaN in the id-255 slots of what the launch sees
    poisoned = gr.clone()
    poisoned[dead] = float("nan")
    run(poisoned)
    assert ctrl[ops.CTRL_APPLIED].item() == 2
    for t, b in zip(state, start):
        assert torch.equal(t[dead], b[dead]) and bool(torch.isfinite(t[~dead]).all())
    before = [t.clone() for t in state]
    gr[int((~dead).nonzero()[-1])] = float("inf")            # a skipped step: nothing moves anywhere
    run()
    assert ctrl[ops.CTRL_SKIPPED].item() == 1 and ctrl[ops.CTRL_APPLIED].item() == 2
    for t, b in zip(state, before):
        assert torch.equal(t, b)


# ---------------------------------------------------------------------------------------------------------------------
# step level
# ---------------------------------------------------------------------------------------------------------------------
def _model(dev):
    import lc2is_amd.nn as N
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 4, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    return m.to(dev).train()


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
             "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)},
            torch.randint(0, 151, (2, 16, 16), generator=g).to(dev))


def _twins(dev, k=2):
    ms = [_model(dev) for _ in range(k)]
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    return ms


def _state(ts):
    return [ts.arena.flat] + ([ts.m, ts.v] if ts.kind == "adamw" else [] if ts.mom is None else [ts.mom])


def _mask(ts, names):
    """Boolean mask over the arena of the elements of the named parameters."""
    named = dict(ts.model.named_parameters())
    mask = torch.zeros(ts.arena.numel, dtype=torch.bool, device=ts.arena.flat.device)
    for n in names:
        lo, hi = ts.arena.ranges[id(named[n])]
        mask[lo:hi] = True
    return mask


@pytest.mark.parametrize("kw", [dict(optimizer="sgd", momentum=0.9, lr_schedule=[0.4, 0.8, 0.6], max_grad_norm=MAX_NORM),
                                dict(optimizer="adamw", lr_schedule=[2e-4, 4e-4, 3e-4], max_grad_norm=MAX_NORM)],
                         ids=["sgd_mom", "adamw"])
def test_one_group_is_the_ungrouped_device_path(dev, kw):
    from lc2is_amd.step import TrainStep
    w = 0.05
    m_a, m_b = _twins(dev)
    every = [n for n, _ in m_a.named_parameters()]
    ts_a = TrainStep(m_a, device_state=True, weight_decay=w, **kw)
    ts_b = TrainStep(m_b, param_groups=[dict(params=every, lr_scale=1.0, weight_decay=w)], **kw)
    assert len(ts_b.param_groups) == 1 and ts_b.param_groups[0]["numel"] == sum(p.numel() for p in m_b.parameters())
    post = _mask(ts_b, [n for n in every if "post_layernorm" in n])
    start = ts_b.arena.flat.clone()
    for s_ in range(3):
        la, lb = ts_a.step(*_batch(dev, s_)), ts_b.step(*_batch(dev, s_))
        assert torch.equal(la, lb)
    for a, b in zip(_state(ts_a), _state(ts_b)):
        assert torch.equal(a, b)
    assert torch.equal(ts_a._ctrl, ts_b._ctrl) and ts_b.last_clip_coef.item() < 1.0
    # post_layernorm never receives a gradient: the skip id keeps its bits although w > 0
    assert len(ts_b.arena.dead) > 0 and int(post.sum()) > 0
    assert torch.equal(ts_b.arena.flat[post], start[post]) and not torch.equal(ts_b.arena.flat, start)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_selectivity_is_exact(dev, kind):
    """ONE step from one state and one batch.  A = {G1: decay 0.1, scale 1; G2 (all 1-D parameters): decay 0, scale 0.25};
    B = no groups, decay 0.1; C = no groups, decay 0, rates x 0.25 (a power of two: lr * 0.25 is exact either way)."""
    from lc2is_amd.step import TrainStep
    m_a, m_b, m_c = _twins(dev, 3)
    rate = 0.4 if kind == "sgd" else 2e-4
    kw = dict(optimizer=kind, max_grad_norm=MAX_NORM)
    g2 = [n for n, p in m_a.named_parameters() if p.dim() == 1]
    g1 = [n for n, p in m_a.named_parameters() if p.dim() != 1]
    ts_a = TrainStep(m_a, lr_schedule=[rate], param_groups=[dict(params=g1, weight_decay=0.1, lr_scale=1.0),
                                                            dict(params=g2, weight_decay=0.0, lr_scale=0.25)], **kw)
    ts_b = TrainStep(m_b, lr_schedule=[rate], weight_decay=0.1, **kw)
    ts_c = TrainStep(m_c, lr_schedule=[rate * 0.25], weight_decay=0.0, **kw)
    mask2 = _mask(ts_a, g2)
    ids = ts_a.arena._group_ids
    assert sum(ids[i] != ids[i + 1] for i in range(len(ids) - 1)) >= 40      # the two groups interleave in the arena
    start = ts_a.arena.flat.clone()
    batch = _batch(dev, 3)
    for ts in (ts_a, ts_b, ts_c):
        ts.step(*batch)
    for word in (4, 5):                                                      # grad_norm, clip_coef
        assert ts_a._ctrl[word].item() == ts_b._ctrl[word].item() == ts_c._ctrl[word].item()
    assert ts_a.last_clip_coef.item() < 1.0
    for a, b, c in zip(_state(ts_a), _state(ts_b), _state(ts_c)):
        assert torch.equal(a[~mask2], b[~mask2])
        assert torch.equal(a[mask2], c[mask2])
    moved = ts_a.arena.flat != start
    assert bool(moved[mask2].any()) and bool(moved[~mask2].any())
    assert not torch.equal(ts_b.arena.flat[mask2], ts_c.arena.flat[mask2])  # the comparison can tell B from C


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_lr_scale_zero_keeps_the_bits(dev, kind):
    from lc2is_amd.step import TrainStep
    m = _model(dev)
    frozen = [n for n, _ in m.named_parameters() if n.startswith("vision_decoder.")]
    ts = TrainStep(m, optimizer=kind, lr=0.1 if kind == "sgd" else 1e-3, weight_decay=0.05,
                   param_groups=[dict(params=frozen, lr_scale=0.0)])
    assert len(ts.param_groups) == 2 and ts.param_groups[1]["lr_scale"] == 1.0 and ts.param_groups[1]["weight_decay"] == 0.05
    mask = _mask(ts, frozen)
    start = ts.arena.flat.clone()
    for s_ in range(3):
        ts.step(*_batch(dev, s_))
    assert torch.equal(ts.arena.flat[mask], start[mask])
    assert not torch.equal(ts.arena.flat[~mask], start[~mask])
    if kind == "adamw":
        assert bool((ts.m[mask] != 0).any()) and bool((ts.v[mask] != 0).any())


def test_make_param_groups_trains_in_one_launch(dev, monkeypatch):
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep, make_param_groups
    m_g, m_u = _twins(dev)
    groups = make_param_groups(m_g, weight_decay=0.05, lr_scales={"vision_encoder": 0.1}, layer_decay=0.75)
    rate = 3e-4
    ts_g = TrainStep(m_g, optimizer="adamw", lr=rate, weight_decay=0.05, param_groups=groups)
    ts_u = TrainStep(m_u, optimizer="adamw", lr=rate, weight_decay=0.05, device_state=True)
    calls = {"groups": 0, "other": 0}
    real = ops.adamw_step_groups

    def counted(*a, **k):
        calls["groups"] += 1
        return real(*a, **k)

    def other(*a, **k):
        calls["other"] += 1
        raise AssertionError("the grouped step launched an ungrouped optimizer")

    batch = _batch(dev, 0)
    losses_u = [ts_u.step(*batch).item() for _ in range(5)]
    monkeypatch.setattr(ops, "adamw_step_groups", counted)
    monkeypatch.setattr(ops, "adamw_step_ctrl", other)
    monkeypatch.setattr(ops, "adamw_step", other)
    losses_g = [ts_g.step(*batch).item() for _ in range(5)]
    print(f"grouped losses {losses_g}, ungrouped {losses_u}, groups {len(groups)}")
    assert calls == {"groups": 5, "other": 0}
    assert losses_u[-1] < losses_u[0] and losses_g[-1] < losses_g[0]
    assert all(bool(torch.isfinite(t).all()) for t in _state(ts_g)) and all(l == l and abs(l) != float("inf") for l in losses_g)


def test_capture_with_groups_schedule_and_clipping(dev):
    """Groups + a moving schedule + clipping, captured: 4 replays against 4 eager steps on a twin."""
    from lc2is_amd.step import TrainStep, make_param_groups
    rates = [2e-4, 6e-4, 1e-3, 8e-4, 6e-4, 4e-4, 2e-4]
    m_e, m_g = _twins(dev)
    kw = dict(optimizer="adamw", weight_decay=0.01, lr_schedule=rates, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    ts_e = TrainStep(m_e, param_groups=make_param_groups(m_e, weight_decay=0.01, lr_scales={"vision_encoder": 0.25}), **kw)
    ts_g = TrainStep(m_g, param_groups=make_param_groups(m_g, weight_decay=0.01, lr_scales={"vision_encoder": 0.25}), **kw)
    first = _batch(dev, 0)
    for _ in range(2):
        ts_e.step(*first)
    run = ts_g.capture(*first)
    torch.cuda.synchronize()
    assert ts_g._ctrl[0].item() == 2 and len(ts_g.arena._group_maps) == 1      # the warm-up established the one map
    for s_ in range(1, 5):
        inp, lab = _batch(dev, s_)
        le, lg = ts_e.step(inp, lab), run(inp, lab)
        print(f"replay {s_}: eager loss {le.item()!r} captured {lg.item()!r} max |d arena| "
              f"{(ts_e.arena.flat - ts_g.arena.flat).abs().max().item():.3e}")
    torch.cuda.synchronize()
    assert torch.equal(ts_g._ctrl[:3], ts_e._ctrl[:3]) and ts_g._ctrl[0].item() == 6
    for a, b in zip(_state(ts_e), _state(ts_g)):
        assert torch.equal(a, b)
    run.release()


def test_capture_refuses_a_live_set_the_warmup_did_not_see(dev):
    from lc2is_amd.step import TrainStep
    m = _model(dev)
    ts = TrainStep(m, optimizer="sgd", lr=1e-3, param_groups=[dict(params=["class_prototypes"], lr_scale=0.5)])
    real = ts.arena.finalize_grads
    n = {"calls": 0}

    def finalize():
        live = real()
        n["calls"] += 1
        if n["calls"] == 3:                                   # the recorded step (after 2 warm-up steps) sees another dead set
            ts.arena.dead = ts.arena.dead + (0,) if 0 not in ts.arena.dead else ts.arena.dead[1:]
        return live

    ts.arena.finalize_grads = finalize
    with pytest.raises(RuntimeError, match="differs"):
        ts.capture(*_batch(dev, 0))


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")                             # gloo: both ranks share the one GPU of the test box
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import lc2is_amd.nn as N
    from lc2is_amd.dp import GradReducer
    from lc2is_amd.step import TrainStep, make_param_groups
    fx = torch.load(G / "base_tiny.pt", weights_only=True)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    m.load_state_dict(fx["state_dict"], strict=True)
    m = m.to(dev).train()
    red = GradReducer(bucket_elems=100_000)
    groups = make_param_groups(m, weight_decay=0.01, lr_scales={"vision_encoder": 0.1}, layer_decay=0.75)
    ts = TrainStep(m, optimizer="adamw", weight_decay=0.01, lr_schedule=[1e-3, 2e-3, 1e-3, 5e-4], max_grad_norm=MAX_NORM,
                   skip_nonfinite=True, reducer=red, param_groups=groups)
    red.broadcast_params(ts.arena.flat, src=0)
    start = ts.arena.flat.clone()
    base = {k: fx[k][rank:rank + 1].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"][rank:rank + 1].to(dev)
    ctrls = []
    for s_ in range(3):                                      # different batches on the two ranks
        g = torch.Generator().manual_seed(100 + 10 * s_ + rank)
        inputs = dict(base, pixel_values=torch.randn(base["pixel_values"].shape, generator=g).to(dev) * (1 + rank))
        ts.step(inputs, labels)
        ctrls.append(ts._ctrl.clone().cpu())
    torch.cuda.synchronize()
    torch.save(dict(ctrls=torch.stack(ctrls), flat=ts.arena.flat.cpu(), m=ts.m.cpu(), v=ts.v.cpu(),
                    moved=not torch.equal(ts.arena.flat, start), ngroups=len(ts.param_groups)),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_stay_bit_identical_with_groups(dev, tmp_path):
    from lc2is_amd import ops
    ctx = mp.get_context("spawn")
    port = 29560 + os.getpid() % 100
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    hung = False
    for p in procs:
        p.join(timeout=300)
        if p.is_alive():                                     # never leave a rank holding the GPU behind a failed test
            hung = True
            p.terminate()
            p.join(30)
            if p.is_alive():
                p.kill()
                p.join()
    assert not hung, "a DP worker did not finish within 300 s"
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert torch.equal(r0["ctrls"], r1["ctrls"])
    c = r0["ctrls"]
    assert bool((c[:, ops.CTRL_CLIP_COEF].view(torch.float32) < 1.0).all()) and c[:, ops.CTRL_APPLIED].tolist() == [1, 2, 3]
    for k in ("flat", "m", "v"):
        assert torch.equal(r0[k], r1[k]), f"replicas diverged in {k} after 3 grouped, clipped AdamW steps"
    assert r0["moved"] and r0["ngroups"] > 3
