"""The weight EMA held on the device (lc2is_amd/csrc/optim.hip: ema_ctrl_kernel, swap_f32_kernel; TrainStep's ema_decay /
ema_warmup / ema_every, ema_weights(), ema_state_dict()).

Op level against fp64 PyTorch on the same data, with the control block set by hand; step level against the fp64 recurrence run
over snapshots of the parameters, against a twin without EMA (training is not disturbed), captured against eager, and two gloo
ranks on the one GPU.  The tiny model and the 2-image batches are those of test_gpu_optim_ctrl.py."""
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

SIZES = [4, 1020, 5 * 1024 * 4096 + 1024 * 77 + 4]     # one float4; one ragged block; > one full grid stride (4096 x 256 float4s), ragged
IDS = ["one_float4", "ragged_block", "grid_stride_ragged"]
U = 2.0 ** -24
MAX_NORM = 0.05


def _ctrl(dev, apply=1, applied=1):
    from lc2is_amd import ops
    c = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32, device=dev)
    c[ops.CTRL_APPLY], c[ops.CTRL_APPLIED] = apply, applied
    return c


def _heavy(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, device=dev, generator=g) * torch.exp(2.0 * torch.randn(n, device=dev, generator=g))


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _bits(t):
    return t.view(torch.int32)


def _model(dev, dropout=0.0):
    import lc2is_amd.nn as N
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 4, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64, **({"dropout": dropout} if dropout else {}))
    return m.to(dev).train()


def _batch(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    return ({"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
             "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)},
            torch.randint(0, 151, (2, 16, 16), generator=g).to(dev))


def _nan_batch(dev, seed):
    inp, lab = _batch(dev, seed)
    inp["pixel_values"][1, 1, 20, 33] = float("nan")     # arithmetic, not a fault: the NaN spreads through the forward
    return inp, lab


def _twins(dev):
    a, b = _model(dev), _model(dev)
    b.load_state_dict(a.state_dict())
    return a, b


# ---------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES, ids=IDS)
@pytest.mark.parametrize("w", [0.5, 1e-4])
def test_ema_update_ctrl_vs_fp64(dev, n, w):
    """e' = e + fp32(w) * (p - e) against fp64 on the same data.  Bound per element: 5 * 2^-24 * max(|p|, |e|, |e'|) — the worst
    case (1 + 4w) * 2^-24 * M of three fp32 roundings with w <= 1 (the kernel's fma makes it two); a CPU emulation of the
    non-contracted form measured <= 1.0 * 2^-24 * M.  Forward and reverse walks give the same bits."""
    from lc2is_amd import ops
    p, e0 = _heavy(n, dev, 1 + n % 1000), _heavy(n, dev, 2 + n % 1000)
    ctrl = _ctrl(dev)
    p_before = p.clone()
    e_f, e_r = e0.clone(), e0.clone()
    ops.ema_update_ctrl(e_f, p, ctrl, w)
    ops.ema_update_ctrl(e_r, p, ctrl, w, reverse=True)
    ref = e0.double() + _f32(w) * (p.double() - e0.double())
    M = torch.maximum(torch.maximum(p.abs(), e0.abs()), e_f.abs()).double()
    ratio = ((e_f.double() - ref).abs() / (U * M).clamp_min(1e-300)).max().item()
    print(f"ema_update_ctrl n={n} w={w}: max |e' - fp64| / (2^-24 * M) = {ratio:.3f} (bound 5)")
    assert bool(((e_f.double() - ref).abs() <= 5 * U * M).all()), ratio
    assert torch.equal(_bits(e_f), _bits(e_r))
    assert torch.equal(_bits(p), _bits(p_before))                  # the parameters are read only
    assert not torch.equal(e_f, e0)
    moved = (e_f != e0).sum().item()
    assert moved >= n - max(2, n // 100), (moved, n)               # every element was visited (a few may round back onto themselves)


def _specials(dev, n=1024):
    """Random fp32 bit patterns with the edge cases up front: +-0, denormals, +-inf, quiet and signalling NaNs with payloads."""
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    edge = [0x00000000, -0x80000000, 0x00000001, 0x007fffff, -0x80000000 + 0x00000001, -0x80000000 + 0x00400000,
            0x7f800000, -0x80000000 + 0x7f800000, 0x7fc00000, 0x7fc12345, 0x7f800001, 0x7fa55aa5,
            -0x80000000 + 0x7fc00001, -0x80000000 + 0x7f923456, 0x3f800000, -0x80000000 + 0x3f800000]
    bits[:len(edge)] = torch.tensor(edge, dtype=torch.int64).to(torch.int32)
    return bits.to(dev)


def test_fixed_points_and_early_returns(dev):
    from lc2is_amd import ops
    pb = _specials(dev)
    p = pb.view(torch.float32)
    # 1. e a bit-copy of p: every pattern is a fixed point, whatever the weight and the walk
    for w in (0.5, 1e-4, 1.0):
        for rev in (False, True):
            e = pb.clone().view(torch.float32)
            ops.ema_update_ctrl(e, p, _ctrl(dev), w, reverse=rev)
            assert torch.equal(_bits(e), pb), (w, rev)
    # 2. apply = 0: a skipped step leaves the EMA's bits alone (here e differs from p everywhere)
    e0 = _heavy(1024, dev, 9)
    q = _heavy(1024, dev, 10)
    e = e0.clone()
    ops.ema_update_ctrl(e, q, _ctrl(dev, apply=0, applied=1), 0.5)
    assert torch.equal(_bits(e), _bits(e0))
    ops.ema_update_ctrl(e, q, _ctrl(dev, apply=1, applied=1), 0.5)
    assert not torch.equal(_bits(e), _bits(e0))                    # the same launch with apply = 1 does move it
    # 3. every = 3: changed only when applied is a multiple of 3
    for applied, moves in ((1, False), (2, False), (3, True), (4, False), (6, True)):
        e = e0.clone()
        ops.ema_update_ctrl(e, q, _ctrl(dev, applied=applied), 0.5, every=3)
        assert torch.equal(_bits(e), _bits(e0)) != moves, applied


def test_warmup_weight_and_its_host_mirror(dev):
    """Warm-up: the j-th EMA update (j = applied / every) takes max(w, 9 / (10 + j)).  An element with e = 0, p = 1 comes back as
    the weight itself (fma(w, 1, 0) = w, exact): that is compared bit for bit with the host mirror step.ema_weight_at."""
    from lc2is_amd import ops
    from lc2is_amd.step import ema_weight_at
    decay = 0.9999
    w = 1.0 - decay
    n = 2048
    p, e0 = _heavy(n, dev, 21), _heavy(n, dev, 22)
    p[0], e0[0] = 1.0, 0.0
    plain = e0.clone()
    ops.ema_update_ctrl(plain, p, _ctrl(dev), w)
    assert plain[0].item() == _f32(w) == ema_weight_at(1, decay)
    for applied, every in ((1, 1), (5, 1), (91, 1), (10, 2), (89_999, 1)):
        j = applied // every
        e = e0.clone()
        ops.ema_update_ctrl(e, p, _ctrl(dev, applied=applied), w, warmup=True, every=every)
        wj = max(_f32(w), _f32(9.0 / (10.0 + j)))
        assert e[0].item() == wj == ema_weight_at(j, decay, True), (applied, every, e[0].item(), wj)
        ref = e0.double() + wj * (p.double() - e0.double())
        M = torch.maximum(torch.maximum(p.abs(), e0.abs()), e.abs()).double()
        ratio = ((e.double() - ref).abs() / (U * M)).max().item()
        print(f"warm-up applied={applied} every={every}: weight {wj!r}, max error / (2^-24 * M) = {ratio:.3f}")
        assert bool(((e.double() - ref).abs() <= 5 * U * M).all()), (applied, ratio)
        if j == 89_999:                                            # 9 / 90 009 < 1e-4: the weight is w itself, the bits the plain launch's
            assert wj == _f32(w) and torch.equal(_bits(e), _bits(plain))
        else:
            assert wj > _f32(w) and not torch.equal(_bits(e), _bits(plain))


@pytest.mark.parametrize("n", SIZES, ids=IDS)
def test_swap_f32(dev, n):
    from lc2is_amd import ops
    g = torch.Generator(device=dev).manual_seed(n % 977)
    ab = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, n), generator=g, device=dev, dtype=torch.int64).to(torch.int32)
    ab[0, 0], ab[1, 0] = 0x7fc12345, -0x80000000                   # a NaN with a payload against -0.0
    ab[0, n - 1], ab[1, n - 1] = 0x7f800001, 0x00000001            # a signalling NaN against the smallest denormal
    a, b = ab[0].clone().view(torch.float32), ab[1].clone().view(torch.float32)
    ops.swap_f32(a, b)
    assert torch.equal(_bits(a), ab[1]) and torch.equal(_bits(b), ab[0])
    ops.swap_f32(a, b)
    assert torch.equal(_bits(a), ab[0]) and torch.equal(_bits(b), ab[1])


def test_swap_refuses_overlapping_and_misaligned_views(dev):
    from lc2is_amd import ops
    x = torch.arange(4096, device=dev, dtype=torch.float32)
    before = x.clone()
    for a, b in ((x[0:1024], x[512:1536]), (x[512:1536], x[0:1024]), (x[0:1024], x[0:1024]), (x[1:1025], x[2048:3072]),
                 (x[0:1024], x[2050:3074]), (x[0:1022], x[2048:3070])):
        with pytest.raises(RuntimeError, match="refused"):
            ops.swap_f32(a, b)
    with pytest.raises(RuntimeError, match="elements"):
        ops.swap_f32(x[0:1024], x[2048:2052])
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                  # nothing was launched
    ops.swap_f32(x[0:1024], x[1024:2048])                          # adjacent is not overlapping
    assert torch.equal(x[0:1024], before[1024:2048]) and torch.equal(x[1024:2048], before[0:1024])
    e = torch.zeros(1024, device=dev)
    with pytest.raises(RuntimeError, match="refused"):
        ops.ema_update_ctrl(e[4:1024], x[1:1021], _ctrl(dev), 0.5)
    assert not e.any().item()


# ---------------------------------------------------------------------------------------------------------------------
# step level
# ---------------------------------------------------------------------------------------------------------------------
RATES = [2e-4, 6e-4, 1e-3, 8e-4, 6e-4, 4e-4, 2e-4]
ADAMW = dict(optimizer="adamw", weight_decay=0.01, lr_schedule=RATES, max_grad_norm=MAX_NORM)


def test_ema_does_not_disturb_training(dev):
    from lc2is_amd.step import TrainStep
    m_a, m_b = _twins(dev)
    ts_a, ts_b = TrainStep(m_a, **ADAMW), TrainStep(m_b, ema_decay=0.9, **ADAMW)
    assert ts_a.ema is None and ts_b.ema is not None and ts_b.ema.data_ptr() != ts_b.arena.flat.data_ptr()
    assert torch.equal(ts_b.ema, ts_b.arena.flat)                  # initialised as a copy
    for s in range(6):
        la, lb = ts_a.step(*_batch(dev, s)), ts_b.step(*_batch(dev, s))
        assert torch.equal(la, lb), s
    for x, y in ((ts_a.arena.flat, ts_b.arena.flat), (ts_a.m, ts_b.m), (ts_a.v, ts_b.v), (ts_a._ctrl, ts_b._ctrl)):
        assert torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)
    assert not torch.equal(ts_b.ema, ts_b.arena.flat)
    with pytest.raises(RuntimeError, match="no EMA"):
        ts_a.ema_state_dict()
    with pytest.raises(RuntimeError, match="no EMA"):
        with ts_a.ema_weights():
            pass


def _param_mask(ts, pred):
    """Boolean mask over the arena of the elements of the parameters whose name satisfies pred."""
    mask = torch.zeros(ts.arena.numel, dtype=torch.bool, device=ts.arena.flat.device)
    names = {id(p): n for n, p in ts.model.named_parameters()}
    for p in ts.arena.params:
        if pred(names[id(p)]):
            lo, hi = ts.arena.ranges[id(p)]
            mask[lo:hi] = True
    return mask


@pytest.mark.parametrize("warmup,every", [(False, 1), (True, 1), (True, 2)], ids=["plain", "warmup", "warmup_every2"])
def test_ema_tracks_the_fp64_recurrence(dev, warmup, every):
    """Snapshots of arena.flat after every step, the recurrence e += w_j * (p - e) on them in fp64 with the host mirror's weights;
    the device EMA is within 5 * n_updates * 2^-24 * M elementwise, M the running maximum magnitude of p and e.  The frozen text
    tower, CLIP's unreached post_layernorm and the alignment padding never move: their EMA keeps the parameters' bits."""
    from lc2is_amd.step import TrainStep, ema_weight_at
    decay, steps = 0.9, 6
    m = _model(dev)
    for p in m.text_encoder.parameters():
        p.requires_grad = False
    ts = TrainStep(m, ema_decay=decay, ema_warmup=warmup, ema_every=every, **ADAMW)
    e64 = ts.arena.flat.double()
    M = e64.abs()
    start = ts.arena.flat.clone()
    n_updates = 0
    for s in range(steps):
        ts.step(*_batch(dev, s))
        p64 = ts.arena.flat.double()
        M = torch.maximum(M, p64.abs())
        if (s + 1) % every == 0:
            n_updates += 1
            e64 = e64 + ema_weight_at(n_updates, decay, warmup) * (p64 - e64)
            M = torch.maximum(M, e64.abs())
    assert n_updates == steps // every and ts.applied_steps.item() == steps
    err = (ts.ema.double() - e64).abs()
    ratio = (err / (U * M).clamp_min(1e-300)).max().item()
    print(f"EMA tracking warmup={warmup} every={every}: {n_updates} updates, max error / (2^-24 * M) = {ratio:.3f} "
          f"(bound {5 * n_updates})")
    assert bool((err <= 5 * n_updates * U * M).all()), ratio
    # it follows the parameters, and it lags them
    moved = ts.arena.flat != start
    assert moved.sum().item() > ts.arena.numel // 4
    assert not torch.equal(ts.ema[moved], ts.arena.flat[moved]) and not torch.equal(ts.ema[moved], start[moved])
    still = _param_mask(ts, lambda n: n.startswith("text_encoder.") or "post_layernorm" in n)
    assert still.sum().item() > 1000 and not moved[still].any().item()
    pad = torch.ones(ts.arena.numel, dtype=torch.bool, device=dev)
    for lo, hi in ts.arena.ranges.values():
        pad[lo:hi] = False
    for mask in (still, pad):                                      # (this model's sizes are multiples of 64: its padding is empty)
        assert torch.equal(_bits(ts.ema)[mask], _bits(ts.arena.flat)[mask])
    # reset_ema restarts from the current parameters
    ts.reset_ema()
    assert torch.equal(_bits(ts.ema), _bits(ts.arena.flat))


def test_skipped_step_leaves_the_ema_alone_and_warmup_follows_applied(dev):
    from lc2is_amd.step import TrainStep, ema_weight_at
    decay = 0.99
    batches = [_batch(dev, 0), _batch(dev, 1), _nan_batch(dev, 2), _batch(dev, 3), _batch(dev, 4)]
    ts = TrainStep(_model(dev), ema_decay=decay, ema_warmup=True, skip_nonfinite=True, **ADAMW)
    by_applied = ts.arena.flat.double()
    by_calls = by_applied.clone()
    M = by_applied.abs()
    applied = 0
    for s, b in enumerate(batches):
        before = ts.ema.clone()
        loss = ts.step(*b)
        if s == 2:
            assert not torch.isfinite(loss).item()
            assert torch.equal(_bits(ts.ema), _bits(before))       # bitwise unchanged across the skipped step
            assert ts.skipped_steps.item() == 1
            continue
        assert not torch.equal(ts.ema, before)
        applied += 1
        p64 = ts.arena.flat.double()
        by_applied = by_applied + ema_weight_at(applied, decay, True) * (p64 - by_applied)
        by_calls = by_calls + ema_weight_at(s + 1, decay, True) * (p64 - by_calls)
        M = torch.maximum(torch.maximum(M, p64.abs()), by_applied.abs())
    assert applied == 4 and ts.applied_steps.item() == 4 and ts._ctrl[0].item() == 5
    bound = 5 * applied * U * M
    err = (ts.ema.double() - by_applied).abs()
    wrong = (ts.ema.double() - by_calls).abs()
    print(f"skip: max error / (2^-24 * M) with j = applied {(err / (U * M).clamp_min(1e-300)).max().item():.3f}, "
          f"with j = calls {(wrong / (U * M).clamp_min(1e-300)).max().item():.1f} (bound {5 * applied})")
    assert bool((err <= bound).all())
    assert not bool((wrong <= bound).all())                        # the index is 'applied': counting calls is told apart


def test_captured_ema_equals_eager(dev):
    """SGD + schedule + EMA: the EMA launch is captured with the step and follows the device counter across replays."""
    from lc2is_amd.step import TrainStep
    kw = dict(optimizer="sgd", momentum=0.9, lr_schedule=[1e-3, 2e-3, 3e-3, 2e-3, 1e-3, 5e-4, 2e-4], ema_decay=0.9,
              ema_warmup=True)
    m_e, m_g = _twins(dev)
    ts_e, ts_g = TrainStep(m_e, **kw), TrainStep(m_g, **kw)
    first = _batch(dev, 0)
    for _ in range(2):                                             # capture() runs 2 real warm-up steps, then records one
        ts_e.step(*first)
    run = ts_g.capture(*first)
    torch.cuda.synchronize()
    try:
        assert ts_g.applied_steps.item() == 2                      # the recorded step did not run
        assert torch.equal(_bits(ts_g.ema), _bits(ts_e.ema))       # the same warm-up steps on both
        ema_ptr = ts_g.ema.data_ptr()
        for s in range(1, 5):
            before = ts_g.ema.clone()
            ts_e.step(*_batch(dev, s))
            run(*_batch(dev, s))
            assert not torch.equal(ts_g.ema, before), s            # it advances on every replay
        torch.cuda.synchronize()
        assert ts_g.applied_steps.item() == ts_e.applied_steps.item() == 6 and ts_g.ema.data_ptr() == ema_ptr
        n_diff = (_bits(ts_g.ema) != _bits(ts_e.ema)).sum().item()
        p_diff = (_bits(ts_g.arena.flat) != _bits(ts_e.arena.flat)).sum().item()
        print(f"captured vs eager after 4 replays: {n_diff} EMA elements and {p_diff} parameter elements differ of {ts_g.arena.numel}; "
              f"max |EMA difference| {(ts_g.ema - ts_e.ema).abs().max().item():.3e}")
        assert torch.equal(_bits(ts_g.ema), _bits(ts_e.ema))
    finally:
        run.release()


def _ema_eval(dev, ts, inputs):
    """Inside ema_weights(): the model's own output in eval mode, and its parameters."""
    ts.model.eval()
    try:
        with torch.no_grad():
            out = ts.model(inputs)["outputs"].clone()
        sd = {k: v.detach().clone() for k, v in ts.model.state_dict().items()}
    finally:
        ts.model.train()
    return out, sd


def test_ema_weights_context(dev):
    from lc2is_amd.step import TrainStep
    kw = dict(ema_decay=0.9, **ADAMW)
    m_a, m_b = _twins(dev)
    ts_a, ts_b = TrainStep(m_a, **kw), TrainStep(m_b, **kw)         # b never enters the context
    for s in range(3):
        ts_a.step(*_batch(dev, s))
        ts_b.step(*_batch(dev, s))
    inputs, _ = _batch(dev, 50)
    flat0, ema0 = ts_a.arena.flat.clone(), ts_a.ema.clone()
    flat_ptr, ema_ptr = ts_a.arena.flat.data_ptr(), ts_a.ema.data_ptr()
    ema_sd = ts_a.ema_state_dict()
    assert list(ema_sd) == list(m_a.state_dict()) and all(v.device.type == "cpu" for v in ema_sd.values())
    assert all(ema_sd[k].shape == v.shape for k, v in m_a.state_dict().items())
    fresh = _model(dev)
    fresh.load_state_dict(ema_sd, strict=True)
    fresh.eval()
    with torch.no_grad():
        want = fresh(inputs)["outputs"]
    with ts_a.ema_weights():
        out, sd_in = _ema_eval(dev, ts_a, inputs)
        assert torch.equal(_bits(ts_a.arena.flat), _bits(ema0)) and torch.equal(_bits(ts_a.ema), _bits(flat0))
        inside_sd = ts_a.ema_state_dict()                          # still the averaged model, wherever its bytes are
        with pytest.raises(RuntimeError, match="already inside"):
            with ts_a.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            ts_a.step(*_batch(dev, 3))
    assert torch.equal(out, want) and out.abs().sum().item() > 0
    for k, v in sd_in.items():
        assert torch.equal(v.cpu(), ema_sd[k]) and torch.equal(inside_sd[k], ema_sd[k]), k
    assert any(not torch.equal(ema_sd[k], v.cpu()) for k, v in m_a.state_dict().items())   # the EMA is not the parameters
    # after exit: both buffers hold their own bits again, at their own addresses
    assert torch.equal(_bits(ts_a.arena.flat), _bits(flat0)) and torch.equal(_bits(ts_a.ema), _bits(ema0))
    assert ts_a.arena.flat.data_ptr() == flat_ptr and ts_a.ema.data_ptr() == ema_ptr
    # the same when the body raises
    with pytest.raises(KeyError, match="boom"):
        with ts_a.ema_weights():
            assert torch.equal(_bits(ts_a.arena.flat), _bits(ema0))
            raise KeyError("boom")
    assert torch.equal(_bits(ts_a.arena.flat), _bits(flat0)) and torch.equal(_bits(ts_a.ema), _bits(ema0))
    with ts_a.ema_weights():                                       # and it can be entered again
        pass
    # the next step equals, bit for bit, the step of the twin that never entered
    la, lb = ts_a.step(*_batch(dev, 3)), ts_b.step(*_batch(dev, 3))
    assert torch.equal(la, lb)
    for x, y in ((ts_a.arena.flat, ts_b.arena.flat), (ts_a.ema, ts_b.ema), (ts_a.m, ts_b.m), (ts_a.v, ts_b.v)):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(ts_a._ctrl, ts_b._ctrl)


def test_captured_replay_inside_ema_weights_raises(dev):
    from lc2is_amd.step import TrainStep
    ts = TrainStep(_model(dev), optimizer="sgd", lr_schedule=[1e-3], ema_decay=0.9)
    run = ts.capture(*_batch(dev, 0))
    try:
        run(*_batch(dev, 1))
        torch.cuda.synchronize()
        state = [t.clone() for t in (ts.arena.flat, ts.ema, ts._ctrl)]
        with ts.ema_weights():
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                run(*_batch(dev, 2))
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                ts.capture(*_batch(dev, 2))
        torch.cuda.synchronize()
        for t, b in zip((ts.arena.flat, ts.ema, ts._ctrl), state):
            assert torch.equal(t.view(torch.int32), b.view(torch.int32))       # nothing ran
        before = ts.ema.clone()
        run(*_batch(dev, 2))                                       # the captured step is still valid afterwards
        torch.cuda.synchronize()
        assert ts.applied_steps.item() == 4 and not torch.equal(ts.ema, before)
    finally:
        run.release()


# ---------------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on the one GPU
# ---------------------------------------------------------------------------------------------------------------------
def _build(dev):
    import lc2is_amd.nn as N
    fx = torch.load(G / "base_tiny.pt", weights_only=True)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")                             # gloo: both ranks share the one GPU of the test box
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lc2is_amd.dp import GradReducer
    from lc2is_amd.step import TrainStep
    m, fx = _build(dev)
    red = GradReducer(bucket_elems=100_000)
    ts = TrainStep(m, optimizer="adamw", weight_decay=0.01, lr_schedule=[1e-3, 2e-3, 1e-3, 5e-4], max_grad_norm=MAX_NORM,
                   skip_nonfinite=True, reducer=red, ema_decay=0.9, ema_warmup=True)
    red.broadcast_params(ts.arena.flat, src=0)
    ts.reset_ema()                                           # the parameters changed under the EMA (rank 0's were broadcast)
    base = {k: fx[k][rank:rank + 1].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"][rank:rank + 1].to(dev)
    for s in range(3):                                       # different batches on the two ranks
        g = torch.Generator().manual_seed(100 + 10 * s + rank)
        inputs = dict(base, pixel_values=torch.randn(base["pixel_values"].shape, generator=g).to(dev) * (1 + rank))
        ts.step(inputs, labels)
    torch.cuda.synchronize()
    torch.save(dict(ema=ts.ema.cpu(), flat=ts.arena.flat.cpu(), ctrl=ts._ctrl.cpu()), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_ema(dev, tmp_path):
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
    assert r0["ctrl"][ops.CTRL_APPLIED].item() == 3 and torch.equal(r0["ctrl"], r1["ctrl"])
    assert torch.equal(_bits(r0["flat"]), _bits(r1["flat"]))
    assert torch.equal(_bits(r0["ema"]), _bits(r1["ema"])), "the EMA diverged between the ranks"
    assert not torch.equal(r0["ema"], r0["flat"])
