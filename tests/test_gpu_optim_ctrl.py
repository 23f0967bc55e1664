"""The device-held optimizer path (lc2is_amd/csrc/optim.hip; TrainStep's lr_schedule / max_grad_norm / skip_nonfinite /
device_state): what the reference's loop has around optimizer.step() — GradScaler's skip on non-finite gradients
(engine.py:89-91), lr_scheduler.step() after every iteration (engine.py:103-104) — plus clip_grad_norm_, with every
step-dependent scalar held in a control block on the device.

Op level against fp64 PyTorch on the same data, step level against references built from the OLD launchers (ops.sgd_step /
ops.adamw_step with host scalars), captured against eager, and two gloo ranks on the one GPU."""
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

ARENA_N = (157_090_000 + 63) // 64 * 64     # the flagship model's 157 M parameters rounded to the arena's 64-element alignment
MAX_NORM = 0.05                              # below every gradient norm these tiny random-init models produce (asserted, printed)


def _ctrl(dev):
    from lc2is_amd import ops
    c = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32, device=dev)
    return c, c.view(torch.float32)


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
# op level: the norm
# ---------------------------------------------------------------------------------------------------------------------
def _data(kind, n, dev):
    g = torch.Generator(device=dev).manual_seed(n % 1000 + len(kind))
    x = torch.randn(n, device=dev, generator=g)
    if kind == "heavy":                                   # log-normal scales: a few elements carry most of the sum
        x *= torch.exp(2.0 * torch.randn(n, device=dev, generator=g))
    elif kind == "inf":
        x[n - 3] = float("inf")
    elif kind == "nan":
        x[n // 2 + 1] = float("nan")
    elif kind == "big":
        x[::max(1, n // 7)] = 1e30                          # finite, but 1e60 is not an fp32
    return x


@pytest.mark.parametrize("n", [1024, 37 * 1024 + 516, ARENA_N], ids=["one_block", "ragged_last_block", "arena_157M"])
@pytest.mark.parametrize("kind", ["normal", "heavy", "inf", "nan", "big"])
def test_grad_sumsq_norm_and_flags(dev, n, kind):
    """Geometry (the issue's): min(4096, ceil(n / 1024)) blocks of 256 lanes, grid-stride, one fp32 accumulator per lane — 152
    additions per lane at 157 M elements — then an 8-level tree per block and an fp64 sum of the <= 4096 partials.  Worst-case
    relative bound ~ 161 * 2^-24 ~ 1e-5 on the sum (half on the norm); a CPU emulation of this order measured 7.5e-10 (normal)
    and 4.7e-9 (heavy-tailed).  Asserted: relative error <= 1e-6 against torch's fp64 norm of the same buffer.
    'big' (elements of 1e30): finite = 1 — the verdict comes from the exponent bits — while the fp32 sum of squares overflows,
    so the norm field holds +inf (and a finite max_norm then gives clip_coef 0: the update runs on a zeroed gradient)."""
    from lc2is_amd import ops
    x = _data(kind, n, dev)
    ctrl, ctrl_f = _ctrl(dev)
    table = torch.tensor([0.5], device=dev)
    partials, flags = ops.grad_sumsq(x)
    assert partials.numel() == flags.numel() == min(4096, -(-n // 1024))
    ops.optim_ctrl_update(ctrl, partials, flags, table, max_norm=1.0, skip_nonfinite=True)
    p1, f1, c1 = partials.clone(), flags.clone(), ctrl.clone()
    norm, finite = ctrl_f[ops.CTRL_GRAD_NORM].item(), ctrl[ops.CTRL_FINITE].item()
    if kind in ("normal", "heavy"):
        ref = torch.linalg.vector_norm(x, dtype=torch.float64).item()
        rel = abs(norm - ref) / ref
        print(f"grad_sumsq {kind} n={n}: norm {norm!r} fp64 {ref!r} rel {rel:.3e}")
        assert finite == 1 and int(flags.sum()) == 0
        assert rel <= 1e-6, (norm, ref, rel)
        assert ctrl[ops.CTRL_APPLY].item() == 1 and ctrl[ops.CTRL_APPLIED].item() == 1
    elif kind == "big":
        assert finite == 1 and int(flags.sum()) == 0
        assert norm == float("inf") and ctrl_f[ops.CTRL_CLIP_COEF].item() == 0.0
        assert ctrl[ops.CTRL_APPLY].item() == 1
    else:
        assert finite == 0 and int(flags.sum()) == 1          # exactly the one block that read the element
        assert ctrl[ops.CTRL_APPLY].item() == 0 and ctrl[ops.CTRL_SKIPPED].item() == 1 and ctrl[ops.CTRL_APPLIED].item() == 0
    # a second launch on the same buffer: the same bits (fixed grid, fixed order, no atomics)
    ctrl2, _ = _ctrl(dev)
    partials, flags = ops.grad_sumsq(x)
    ops.optim_ctrl_update(ctrl2, partials, flags, table, max_norm=1.0, skip_nonfinite=True)
    assert torch.equal(partials.view(torch.int32), p1.view(torch.int32)) and torch.equal(flags, f1) and torch.equal(ctrl2, c1)


def test_grad_sumsq_sees_every_element(dev):
    """A dropped block, a wrong tail or a skipped unrolled load would lose elements: each position counts, exactly."""
    from lc2is_amd import ops
    for n in (4, 1020, 4 * 1024 * 4096 + 8, 5 * 1024 * 4096 + 1024 * 77 + 4):
        x = torch.ones(n, device=dev)
        partials, _ = ops.grad_sumsq(x)
        assert partials.double().sum().item() == n, n     # integers below 2^24 per lane and per block: exact in fp32
        x.zero_()
        x[n - 1] = 3.0
        x[0] = 4.0
        partials, _ = ops.grad_sumsq(x)
        assert partials.double().sum().item() == 25.0, n


# ---------------------------------------------------------------------------------------------------------------------
# op level: the control update
# ---------------------------------------------------------------------------------------------------------------------
def _hand(dev, values, bad=None):
    p = torch.tensor(values, dtype=torch.float32, device=dev)
    f = torch.zeros(len(values), dtype=torch.int32, device=dev)
    if bad is not None:
        f[bad] = 1
    return p, f


def test_ctrl_update_clip_coefficient(dev):
    from lc2is_amd import ops
    table = torch.tensor([0.1], device=dev)
    x = torch.randn(50_000, device=dev) * 3
    for gscale, max_norm in ((1.0, 1.0), (0.5, 2.5), (1.0, 100.0), (0.25, 1e-3)):
        ctrl, ctrl_f = _ctrl(dev)
        partials, flags = ops.grad_sumsq(x)
        ops.optim_ctrl_update(ctrl, partials, flags, table, grad_scale=gscale, max_norm=max_norm)
        norm, coef = ctrl_f[ops.CTRL_GRAD_NORM].item(), ctrl_f[ops.CTRL_CLIP_COEF].item()
        ref = gscale * torch.linalg.vector_norm(x, dtype=torch.float64).item()
        assert abs(norm - ref) <= 1e-6 * ref                                     # grad_scale goes into the norm
        want = min(1.0, max_norm / (norm + 1e-6))                                # fp64, from the kernel's own norm
        assert coef == pytest.approx(want, rel=1e-6), (coef, want)
        assert (coef < 1.0) == (max_norm < norm)
        mul = ctrl_f[ops.CTRL_GRAD_MUL].item()
        assert mul == torch.tensor(gscale, dtype=torch.float32).mul(torch.tensor(coef, dtype=torch.float32)).item()
    # exactly 1.0f: no clipping requested, and a norm under max_norm
    for max_norm in (float("inf"), 1e4):
        ctrl, ctrl_f = _ctrl(dev)
        ops.optim_ctrl_update(ctrl, partials, flags, table, max_norm=max_norm)
        assert ctrl_f[ops.CTRL_CLIP_COEF].item() == 1.0 and ctrl_f[ops.CTRL_GRAD_MUL].item() == 1.0
    ctrl, ctrl_f = _ctrl(dev)
    p, f = _hand(dev, [9.0, 16.0])
    ops.optim_ctrl_update(ctrl, p, f, table, max_norm=float("inf"), grad_scale=0.5)
    assert ctrl_f[ops.CTRL_GRAD_NORM].item() == 2.5 and ctrl_f[ops.CTRL_CLIP_COEF].item() == 1.0
    assert ctrl_f[ops.CTRL_GRAD_MUL].item() == 0.5


def test_ctrl_update_table_indexing_counters_and_bias_corrections(dev):
    from lc2is_amd import ops
    rates = [0.1, 0.2, 0.3]
    table = torch.tensor(rates, device=dev)
    ctrl, ctrl_f = _ctrl(dev)
    good, bad = _hand(dev, [1.0, 3.0]), _hand(dev, [1.0, float("nan")], bad=1)
    b1, b2 = 0.9, 0.999
    seq = [good, bad, good, good, bad, good]        # calls 1..6; applied 1, -, 2, 3, -, 4
    applied = skipped = 0
    for i, (p, f) in enumerate(seq):
        bc_before = (ctrl_f[ops.CTRL_BC1].item(), ctrl_f[ops.CTRL_BC2].item())
        ops.optim_ctrl_update(ctrl, p, f, table, max_norm=1.0, skip_nonfinite=True, beta1=b1, beta2=b2)
        is_bad = p is bad[0]
        applied += not is_bad
        skipped += is_bad
        assert ctrl_f[ops.CTRL_LR].item() == table[min(i, 2)].item()          # first entry on the first call, clamped at the end
        assert ctrl[ops.CTRL_CALLS].item() == i + 1                            # calls advance on a skipped step too
        assert ctrl[ops.CTRL_APPLIED].item() == applied and ctrl[ops.CTRL_SKIPPED].item() == skipped
        assert ctrl[ops.CTRL_FINITE].item() == (0 if is_bad else 1) and ctrl[ops.CTRL_APPLY].item() == (0 if is_bad else 1)
        if is_bad:
            assert (ctrl_f[ops.CTRL_BC1].item(), ctrl_f[ops.CTRL_BC2].item()) == bc_before
        else:                                        # 1 - fp32(beta^t) in fp32, as lc2is_adamw_step forms it on the host;
            for word, beta in ((ops.CTRL_BC1, b1), (ops.CTRL_BC2, b2)):       # one fp32 ulp of beta^t is 6e-8
                want = (1.0 - (torch.tensor(beta, dtype=torch.float32).double() ** applied).float()).item()
                assert ctrl_f[word].item() == pytest.approx(want, abs=6e-8), (applied, beta)
            assert ctrl_f[ops.CTRL_GRAD_NORM].item() == 2.0
    # skipping disabled: the verdict is recorded, the step is applied
    ctrl, ctrl_f = _ctrl(dev)
    ops.optim_ctrl_update(ctrl, *bad, table, skip_nonfinite=False)
    assert ctrl[ops.CTRL_FINITE].item() == 0 and ctrl[ops.CTRL_APPLY].item() == 1
    assert ctrl[ops.CTRL_APPLIED].item() == 1 and ctrl[ops.CTRL_SKIPPED].item() == 0


# ---------------------------------------------------------------------------------------------------------------------
# op level: the optimizers
# ---------------------------------------------------------------------------------------------------------------------
def _update(ctrl, gr, table, **kw):
    from lc2is_amd import ops
    partials, flags = ops.grad_sumsq(gr)
    ops.optim_ctrl_update(ctrl, partials, flags, table, **kw)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("reverse", [False, True])
def test_sgd_step_ctrl_gives_the_bits_of_sgd_step(dev, momentum, reverse):
    """Coefficient 1 and a constant table: torch.equal to ops.sgd_step on the same inputs (weight decay and a 1/world scale on)."""
    from lc2is_amd import ops
    g = torch.Generator().manual_seed(11)
    n = 1024 * 4096 + 1024 * 3 + 64                    # more than one grid-stride round, ragged
    p_old = torch.randn(n, generator=g).to(dev)
    p_new = p_old.clone()
    m_old = torch.zeros(n, device=dev) if momentum else None
    m_new = torch.zeros(n, device=dev) if momentum else None
    ctrl, ctrl_f = _ctrl(dev)
    table = torch.tensor([0.1], device=dev)
    for _ in range(3):
        gr = torch.randn(n, generator=g).to(dev)
        ops.sgd_step(p_old, gr, m_old, 0.1, momentum, 0.01, 0.5)
        _update(ctrl, gr, table, grad_scale=0.5)
        ops.sgd_step_ctrl(p_new, gr, m_new, ctrl, momentum, 0.01, reverse=reverse)
        assert ctrl_f[ops.CTRL_CLIP_COEF].item() == 1.0
    assert torch.equal(p_new, p_old)
    if momentum:
        assert torch.equal(m_new, m_old)


@pytest.mark.parametrize("clip", [None, 1.0])
def test_optimizers_ctrl_vs_torch(dev, clip):
    """test_gpu_misc.py::test_optimizers' cases and tolerance (atol 2e-6, rtol 1e-5: the same arithmetic), the scalars now coming
    from the control block; with clip: torch's clip_grad_norm_ followed by the torch optimizer."""
    from lc2is_amd import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    n = 4096 * 3
    p0 = torch.randn(n, generator=g).to(dev)
    for kind in ("sgd", "sgd_mom", "adamw"):
        p = p0.clone()
        pt = torch.nn.Parameter(p0.clone())
        ctrl, ctrl_f = _ctrl(dev)
        if kind == "sgd":
            opt = torch.optim.SGD([pt], lr=0.1, weight_decay=0.01)
            buf = None
        elif kind == "sgd_mom":
            opt = torch.optim.SGD([pt], lr=0.1, momentum=0.9, weight_decay=0.01)
            buf = torch.zeros(n, device=dev)
        else:
            opt = torch.optim.AdamW([pt], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
            m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        table = torch.tensor([1e-2 if kind == "adamw" else 0.1], device=dev)
        for step in range(1, 4):
            gr = torch.randn(n, generator=g).to(dev)
            pt.grad = gr.clone()
            if clip is not None:
                total = torch.nn.utils.clip_grad_norm_([pt], clip)
                assert total.item() > clip                                   # clipping is active
            opt.step()
            kw = dict(max_norm=float("inf") if clip is None else clip)
            if kind == "adamw":
                _update(ctrl, gr, table, beta1=0.9, beta2=0.999, **kw)
                ops.adamw_step_ctrl(p, gr, m, v, ctrl, 0.9, 0.999, 1e-8, 0.05)
            else:
                _update(ctrl, gr, table, **kw)
                ops.sgd_step_ctrl(p, gr, buf, ctrl, 0.9 if buf is not None else 0.0, 0.01)
            assert (ctrl_f[ops.CTRL_CLIP_COEF].item() < 1.0) == (clip is not None)
        assert ctrl[ops.CTRL_APPLIED].item() == 3
        assert torch.allclose(p, pt.data, atol=2e-6, rtol=1e-5), (kind, clip)


@pytest.mark.parametrize("kind", ["sgd_mom", "adamw"])
def test_skipped_step_touches_nothing(dev, kind):
    from lc2is_amd import ops
    n = 1024 * 300 + 128
    p = torch.randn(n, device=dev)
    s1, s2 = torch.randn(n, device=dev), torch.rand(n, device=dev)
    gr = torch.randn(n, device=dev)
    table = torch.tensor([0.1], device=dev)
    ctrl, _ = _ctrl(dev)

    def run():
        _update(ctrl, gr, table, max_norm=1.0, skip_nonfinite=True, beta1=0.9, beta2=0.999)
        if kind == "adamw":
            ops.adamw_step_ctrl(p, gr, s1, s2, ctrl, 0.9, 0.999, 1e-8, 0.05)
        else:
            ops.sgd_step_ctrl(p, gr, s1, ctrl, 0.9, 0.05)

    run()                                                    # a good step first: state is live
    before = [t.clone() for t in (p, s1, s2)]
    gr[n - 1] = float("inf")
    run()
    assert ctrl[ops.CTRL_SKIPPED].item() == 1 and ctrl[ops.CTRL_APPLIED].item() == 1
    for t, b in zip((p, s1, s2), before):
        assert torch.equal(t, b)
    gr[n - 1] = 0.5
    run()                                                    # and the next good step moves again
    assert ctrl[ops.CTRL_APPLIED].item() == 2 and not torch.equal(p, before[0])


# ---------------------------------------------------------------------------------------------------------------------
# step level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(optimizer="sgd", lr=1e-3, momentum=0.9, weight_decay=0.01), dict(optimizer="sgd", lr=1e-3)])
def test_device_state_alone_is_the_default_arithmetic(dev, kw):
    """device_state=True with nothing that clips, skips or schedules: parameters torch.equal to the plain step's after 3 steps."""
    from lc2is_amd.step import TrainStep
    m_a, m_b = _twins(dev)
    ts_a, ts_b = TrainStep(m_a, **kw), TrainStep(m_b, device_state=True, **kw)
    for s in range(3):
        la, lb = ts_a.step(*_batch(dev, s)), ts_b.step(*_batch(dev, s))
        assert torch.equal(la, lb)
    assert torch.equal(ts_a.arena.flat, ts_b.arena.flat)
    if ts_a.mom is not None:
        assert torch.equal(ts_a.mom, ts_b.mom)
    assert ts_b.applied_steps.item() == 3 and ts_b.skipped_steps.item() == 0 and ts_b.t == 3
    assert ts_b.last_lr.item() == torch.tensor(1e-3, dtype=torch.float32).item()
    assert ts_b.last_grad_norm.is_cuda and ts_b.last_grad_norm.item() > 0
    with pytest.raises(RuntimeError, match="device-held"):
        ts_a.last_grad_norm


def _reference_step(ts, inputs, labels, lr, max_norm, t):
    """One clipped step built from the OLD launchers on a plain TrainStep's model and arena: gradient as the step forms it, norm
    in fp64 with torch, gradient scaled by torch's coefficient, ops.sgd_step / ops.adamw_step with the host's table entry."""
    from lc2is_amd import ops
    arena = ts.arena
    arena.zero_grad(set_to_none=True)
    loss = ts.model.forward_loss(inputs, labels, ts.ignore_index)
    loss.backward()
    live = arena.finalize_grads()
    norm = torch.linalg.vector_norm(arena.grad, dtype=torch.float64).item()
    coef = min(1.0, max_norm / (norm + 1e-6))
    arena.grad.mul_(coef)
    segs = [(0, arena.numel)] if (ts.weight_decay == 0.0 or live == [(0, arena.numel)]) else live
    for lo, hi in segs:
        sl = slice(lo, hi)
        if ts.kind == "sgd":
            ops.sgd_step(arena.flat[sl], arena.grad[sl], None if ts.mom is None else ts.mom[sl], lr, ts.momentum, ts.weight_decay)
        else:
            ops.adamw_step(arena.flat[sl], arena.grad[sl], ts.m[sl], ts.v[sl], lr, ts.betas[0], ts.betas[1], ts.eps,
                           ts.weight_decay, t)
    for m in ts.model.modules():
        if hasattr(m, "invalidate_shadows"):
            m.invalidate_shadows()
    return norm, coef, loss.detach()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipping_and_schedule_eager(dev, kind):
    """4 steps, a rate that changes every step, max_grad_norm below the observed norms.  The step is bitwise reproducible, so both
    sides see the same gradient bits; the only difference is the coefficient's rounding: UPDATES agree to rel-L2 <= 1e-5."""
    from lc2is_amd.step import TrainStep
    m_new, m_ref = _twins(dev)
    # Rates in the regime training runs in (test_gpu_graph.py: SGD at lr * |g| ~ 0.02 on this model; here |clipped g| = MAX_NORM, so
    # lr * MAX_NORM = 0.01 ... 0.04).  A first try at 30x these rates diverged (loss 7.3 -> 10.9 in 4 steps) and a diverging
    # trajectory amplifies last-bit differences (4e-3 on the updates) and says nothing about the step.
    rates = [0.4, 0.8, 0.6, 0.2] if kind == "sgd" else [2e-4, 4e-4, 3e-4, 1e-4]
    kw = dict(optimizer=kind, **({"momentum": 0.9, "weight_decay": 1e-4} if kind == "sgd" else {"weight_decay": 0.01}))
    ts_new = TrainStep(m_new, lr_schedule=rates, max_grad_norm=MAX_NORM, **kw)
    ts_ref = TrainStep(m_ref, lr=rates[0], **kw)
    table = torch.tensor(rates, dtype=torch.float64).to(torch.float32)
    start = ts_new.arena.flat.clone()
    for i in range(4):
        inputs, labels = _batch(dev, i)
        loss_new = ts_new.step(inputs, labels)
        norm, coef, loss_ref = _reference_step(ts_ref, inputs, labels, table[i].item(), MAX_NORM, i + 1)
        got = ts_new.last_grad_norm.item()
        # fp64 norm of the very gradient the kernel read (arena.grad is left as the step formed it).  From the second step on the
        # reference's gradient is not that one to the bit: its parameters differ in last bits (g * coef rounded before the update
        # there, fused into it here), and bf16 activations turn that into ~1e-6 of the gradient.
        own = torch.linalg.vector_norm(ts_new.arena.grad, dtype=torch.float64).item()
        print(f"{kind} step {i}: fp64 norm {norm!r} (own gradient {own!r}) kernel {got!r} coef {coef!r} kernel "
              f"{ts_new.last_clip_coef.item()!r} loss {loss_new.item()!r} reference {loss_ref.item()!r}")
        assert norm > MAX_NORM and coef < 1.0 and ts_new.last_clip_coef.item() < 1.0      # clipping is active on every step
        assert abs(got - own) <= 1e-6 * own
        if i == 0:                                           # the same parameters, so the same loss and gradient bits
            assert own == norm and loss_new.item() == loss_ref.item()
        assert ts_new.last_lr.item() == table[i].item()
    upd_new, upd_ref = ts_new.arena.flat - start, ts_ref.arena.flat - start
    rel = ((upd_new - upd_ref).norm() / upd_ref.norm()).item()
    print(f"{kind}: update rel-L2 {rel:.3e}, |update| / |params| {(upd_ref.norm() / start.norm()).item():.3e}")
    assert upd_ref.norm().item() > 0 and rel <= 1e-5, rel
    assert ts_new.applied_steps.item() == 4 and ts_new.t == 4


def test_norm_covers_what_clip_grad_norm_covers(dev):
    """Frozen text tower + CLIP's unreached post_layernorm: the norm over the WHOLE arena (zeroed segments, untouched alignment
    padding) is clip_grad_norm_'s over the parameters that have a gradient; and the per-segment _ctrl launches under weight decay
    leave the parameters without a gradient bit-identical."""
    from lc2is_amd.step import TrainStep
    m_new, m_ref = _twins(dev)
    for m in (m_new, m_ref):
        for p in m.text_encoder.parameters():
            p.requires_grad = False
    inputs, labels = _batch(dev, 3)
    # the reference: one backward on the twin, the parameters autograd reached, their gradient views, fp64
    ts_ref = TrainStep(m_ref, optimizer="adamw", lr=1e-3, weight_decay=0.1)
    ts_ref.arena.zero_grad(set_to_none=True)
    m_ref.forward_loss(inputs, labels, ts_ref.ignore_index).backward()
    with_grad = [p for p in m_ref.parameters() if p.grad is not None]
    without = [n for n, p in m_ref.named_parameters() if p.grad is None]
    assert any(n.startswith("text_encoder.") for n in without) and any("post_layernorm" in n for n in without)
    assert 0 < len(with_grad) < len(list(m_ref.parameters()))
    want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in with_grad)).item()
    ts_new = TrainStep(m_new, optimizer="adamw", lr=1e-3, weight_decay=0.1, max_grad_norm=MAX_NORM)
    before = {k: v.detach().clone() for k, v in m_new.state_dict().items()}
    ts_new.step(inputs, labels)
    got = ts_new.last_grad_norm.item()
    print(f"norm over the arena {got!r}, clip_grad_norm_ over {len(with_grad)} parameters {want!r}")
    assert abs(got - want) <= 1e-6 * want
    after = m_new.state_dict()
    for k in before:
        if k in without:
            assert torch.equal(after[k], before[k]), k
    assert sum(not torch.equal(after[k], before[k]) for k in before) > 10


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_nonfinite_step_is_skipped(dev, kind):
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep
    rates = [1e-3, 2e-3, 3e-3, 4e-3]
    batches = [_batch(dev, 0), _nan_batch(dev, 1), _batch(dev, 2)]
    kw = dict(optimizer=kind, weight_decay=0.01, **({"momentum": 0.9} if kind == "sgd" else {}))
    ts = TrainStep(_model(dev), lr_schedule=rates, skip_nonfinite=True, **kw)
    state = [ts.arena.flat] + ([ts.m, ts.v] if kind == "adamw" else [ts.mom])
    ts.step(*batches[0])
    before = [t.clone() for t in state]
    loss = ts.step(*batches[1])
    assert not torch.isfinite(loss).item()                   # the caller is told: a NaN loss, and the counter below
    for t, b in zip(state, before):
        assert torch.equal(t, b)                             # parameters and every state buffer bit-identical across the step
    assert ts.skipped_steps.item() == 1 and ts.applied_steps.item() == 1
    assert not torch.isfinite(ts.last_grad_norm).item()
    ts.step(*batches[2])
    assert ts.skipped_steps.item() == 1 and ts.applied_steps.item() == 2 and ts.t == 3
    assert ts.last_lr.item() == torch.tensor(rates[2], dtype=torch.float32).item()    # the schedule advanced regardless
    if kind == "adamw":                                      # bias corrections for t = 2, not 3
        bc1, bc2 = ts._ctrl_f[ops.CTRL_BC1].item(), ts._ctrl_f[ops.CTRL_BC2].item()
        assert bc1 == pytest.approx(1 - 0.9 ** 2, rel=1e-6) and bc2 == pytest.approx(1 - 0.999 ** 2, rel=1e-4)
    assert all(torch.isfinite(t).all().item() for t in state) and not torch.equal(state[0], before[0])
    # the same run without the guard ends with non-finite parameters: the test would notice a guard that does nothing
    ts2 = TrainStep(_model(dev), lr_schedule=rates, skip_nonfinite=False, **kw)
    for b in batches:
        ts2.step(*b)
    assert not torch.isfinite(ts2.arena.flat).all().item()
    assert ts2.skipped_steps.item() == 0 and ts2.applied_steps.item() == 3


def test_capture_adamw_with_schedule_clipping_and_skip(dev):
    """AdamW, a warm-up-and-decay table, clipping and skip, captured; 4 replays against the eager device-held step on a twin.
    Tolerances of test_gpu_graph.py::test_graph_replay_matches_eager (the weight-gradient plan differs under capture)."""
    from lc2is_amd.step import TrainStep
    rates = [2e-4, 6e-4, 1e-3, 8e-4, 6e-4, 4e-4, 2e-4]       # held at 2e-4 from the 7th call on
    kw = dict(optimizer="adamw", weight_decay=0.01, lr_schedule=rates, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    m_e, m_g = _twins(dev)
    ts_e, ts_g = TrainStep(m_e, **kw), TrainStep(m_g, **kw)
    start = ts_e.arena.flat.clone()
    first = _batch(dev, 0)
    for _ in range(2):                                        # capture() runs 2 real warm-up steps, then records one
        ts_e.step(*first)
    run = ts_g.capture(*first)
    torch.cuda.synchronize()
    assert ts_g._ctrl[0].item() == 2 and ts_g.t == 2          # the recorded step did not run
    losses_e, losses_g = [], []
    for s in range(1, 5):
        inp, lab = _batch(dev, s)
        losses_e.append(ts_e.step(inp, lab).item())
        losses_g.append(run(inp, lab).item())
        assert ts_g.last_lr.item() == ts_e.last_lr.item() == torch.tensor(rates[s + 1], dtype=torch.float32).item()
        assert ts_g.last_clip_coef.item() < 1.0
        assert ts_g.last_grad_norm.item() == pytest.approx(ts_e.last_grad_norm.item(), rel=1e-4)
    torch.cuda.synchronize()
    assert losses_e == pytest.approx(losses_g, abs=1e-5), (losses_e, losses_g)
    upd_e, upd_g = ts_e.arena.flat - start, ts_g.arena.flat - start
    rel = ((upd_e - upd_g).norm() / upd_e.norm()).item()
    print(f"capture vs eager: losses {losses_e} / {losses_g}, update rel-L2 {rel:.3e}")
    assert upd_e.norm().item() > 0 and rel < 1e-4
    assert torch.equal(ts_g._ctrl[:3], ts_e._ctrl[:3])        # calls, applied, skipped
    assert ts_g._ctrl[0].item() == 6 and ts_g.applied_steps.item() == 6 and ts_g.t == ts_e.t == 6
    # one replay with a NaN batch: skipped inside the graph, parameters and moments bit-identical across it
    before = [t.clone() for t in (ts_g.arena.flat, ts_g.m, ts_g.v)]
    loss = run(*_nan_batch(dev, 9))
    assert not torch.isfinite(loss).item()
    for t, b in zip((ts_g.arena.flat, ts_g.m, ts_g.v), before):
        assert torch.equal(t, b)
    assert ts_g.skipped_steps.item() == 1 and ts_g.applied_steps.item() == 6 and ts_g._ctrl[0].item() == 7
    loss = run(*_batch(dev, 10))                              # the next replay proceeds, at the held last rate
    assert torch.isfinite(loss).item() and ts_g.applied_steps.item() == 7 and ts_g.skipped_steps.item() == 1
    assert ts_g.last_lr.item() == torch.tensor(rates[-1], dtype=torch.float32).item()
    assert not torch.equal(ts_g.arena.flat, before[0]) and torch.isfinite(ts_g.arena.flat).all().item()
    run.release()


def test_capture_on_the_old_path_still_refuses_adamw(dev):
    from lc2is_amd.step import TrainStep
    ts = TrainStep(_model(dev), optimizer="adamw", lr=1e-3)
    with pytest.raises(RuntimeError, match="AdamW bias correction is step-dependent"):
        ts.capture(*_batch(dev, 0))


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
                   skip_nonfinite=True, reducer=red)
    red.broadcast_params(ts.arena.flat, src=0)
    base = {k: fx[k][rank:rank + 1].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"][rank:rank + 1].to(dev)
    ctrls = []
    for s in range(3):                                       # different batches on the two ranks
        g = torch.Generator().manual_seed(100 + 10 * s + rank)
        inputs = dict(base, pixel_values=torch.randn(base["pixel_values"].shape, generator=g).to(dev) * (1 + rank))
        ts.step(inputs, labels)
        ctrls.append(ts._ctrl.clone().cpu())
    flat3 = ts.arena.flat.clone()
    state3 = [t.clone() for t in (ts.arena.flat, ts.m, ts.v)]
    inputs = dict(base, pixel_values=base["pixel_values"].clone())
    if rank == 1:                                            # the NaN on ONE rank only: the all-reduce carries it to both
        inputs["pixel_values"][0, 0, 5, 5] = float("nan")
    ts.step(inputs, labels)
    torch.cuda.synchronize()
    unchanged = all(torch.equal(a, b) for a, b in zip((ts.arena.flat, ts.m, ts.v), state3))
    torch.save(dict(ctrls=torch.stack(ctrls), flat3=flat3.cpu(), ctrl4=ts._ctrl.cpu(), unchanged=unchanged),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reach_the_same_clip_and_skip_decisions(dev, tmp_path):
    from lc2is_amd import ops
    ctx = mp.get_context("spawn")
    port = 29450 + os.getpid() % 100
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
    # the whole control block — grad_norm and clip_coef among it — is bit-identical across the ranks at every step
    assert torch.equal(r0["ctrls"], r1["ctrls"])
    c = r0["ctrls"]
    coefs, norms = c[:, ops.CTRL_CLIP_COEF].view(torch.float32), c[:, ops.CTRL_GRAD_NORM].view(torch.float32)
    print(f"DP norms {norms.tolist()} coefficients {coefs.tolist()}")
    assert bool((coefs < 1.0).all()) and bool((norms > MAX_NORM).all())
    assert c[:, ops.CTRL_APPLIED].tolist() == [1, 2, 3]
    assert torch.equal(r0["flat3"], r1["flat3"]), "replicas diverged after 3 clipped AdamW steps"
    for r in (r0, r1):                                       # the NaN step: both ranks skip, nothing moved on either
        assert r["ctrl4"][ops.CTRL_SKIPPED].item() == 1 and r["ctrl4"][ops.CTRL_APPLIED].item() == 3
        assert r["ctrl4"][ops.CTRL_FINITE].item() == 0 and r["ctrl4"][ops.CTRL_CALLS].item() == 4
        assert r["unchanged"]
