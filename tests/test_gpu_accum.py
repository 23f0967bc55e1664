"""Gradient accumulation with the exact large-batch mean: TrainStep(accumulate=N), ops.accum_add and
ops.optim_ctrl_update_accum (lc2is_amd/csrc/optim.hip).

N calls of step() are one optimizer update whose gradient is (sum of the pixel losses of all N micro-batches) / (count of all
their non-ignored pixels) — one step on the concatenated batch — and not the mean of the micro-batch means.  The tiny model and
the 2-image 64 x 64 batches are those of test_gpu_optim_ctrl.py / test_gpu_train_state.py; a micro-batch is B = 2.

Bounds: the project's stated ones (tests/test_gpu_modules.py): relative L2 of any parameter gradient <= 8e-2, loss within 2e-2
absolute.  A single SGD step without momentum or decay moves a parameter by -lr * gradient, so the bound on gradients is the
bound on parameter CHANGES, which is what the step-level tests compare.  Every measured figure is printed; the maxima are also
written to accum_parity.json in the directory LC2IS_REPORT_DIR names (no file when it is unset)."""
import json
import math
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

MAX_NORM = 0.05
COSINE = [0.5e-3 * (1.0 + math.cos(math.pi * i / 8)) for i in range(8)]
GRAD_BOUND, LOSS_BOUND = 8e-2, 2e-2
IGNORE = 255
LR = 0.05
KEYS = ("class_prototypes", "pixel_patch.visual.weight", "vision_encoder.enc.embeddings.patch_embedding.weight",
        "text_encoder.enc.embeddings.token_embedding.weight")
REPORT = {}


def _note(k, v):
    REPORT[k] = v
    where = os.environ.get("LC2IS_REPORT_DIR")
    if not where:
        return
    out = Path(where)
    try:
        out.mkdir(parents=True, exist_ok=True)
        (out / "accum_parity.json").write_text(json.dumps(REPORT, indent=1))
    except OSError:
        pass


def _model(dev):
    import lc2is_amd.nn as N
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 4, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    return m.to(dev).train()


def _batch(dev, seed, ignore_rows=0):
    """The 2-image batch of test_gpu_optim_ctrl.py; the first ``ignore_rows`` of the 16 label rows are set to IGNORE."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    inputs = {"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
              "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    labels = torch.randint(0, 151, (2, 16, 16), generator=g)
    labels[:, :ignore_rows] = IGNORE
    return inputs, labels.to(dev)


def _cat(batches):
    return ({k: torch.cat([b[0][k] for b in batches]) for k in batches[0][0]}, torch.cat([b[1] for b in batches]))


def _named(ts):
    return {k: p.detach().clone() for k, p in ts.model.named_parameters() if k in KEYS}


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _bits(ts):
    out = {"flat": ts.arena.flat}
    for k in ("mom", "m", "v", "ema", "_ctrl"):
        t = getattr(ts, k, None)
        if t is not None:
            out[k] = t
    return {k: v.clone() for k, v in out.items()}


def _same_bits(a, b, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k in skip:
            continue
        x, y = a[k].view(torch.int32), b[k].view(torch.int32)
        assert torch.equal(x, y), f"{k}: {(x != y).sum().item()} of {x.numel()} elements differ"


def _device_kw(model):
    from lc2is_amd.step import make_param_groups
    return dict(optimizer="adamw", lr_schedule=COSINE, max_grad_norm=MAX_NORM, ema_decay=0.99, ema_warmup=True,
                param_groups=make_param_groups(model, weight_decay=0.05, layer_decay=0.9))


# ---------------------------------------------------------------------------------------------------------------------
# 1. op level: the control arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _ctrl(dev):
    from lc2is_amd import ops
    c = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32, device=dev)
    return c, c.view(torch.float32)


def _block(dev, loss_sum=0.0, denom=0.0):
    b = torch.zeros(4, dtype=torch.float64, device=dev)
    b[0], b[1] = loss_sum, denom
    return b


def _f32(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


def test_ctrl_update_accum_arithmetic(dev):
    """grad_mul, grad_norm, clip_coef, last_loss, last_denom restated on the CPU: scale64 = grad_scale / denom in fp64,
    norm = fp32(scale64 * sqrt(sum)), coef = fp32(min(1, max_norm / (norm64 + 1e-6))), grad_mul = fp32(scale64) * coef in fp32."""
    from lc2is_amd import ops
    table = torch.tensor([0.1, 0.2], device=dev)
    x = torch.randn(50_000, device=dev) * 3
    tot = torch.linalg.vector_norm(x, dtype=torch.float64).item()
    for gscale, max_norm, denom, loss_sum in ((1.0, 1.0, 576.0, 3000.5), (0.5, 2.5, 1088.0, 7.25), (1.0, float("inf"), 3.0, 1.0),
                                              (0.25, 1e-3, 16777217.0, 5e7)):
        ctrl, ctrl_f = _ctrl(dev)
        block = _block(dev, loss_sum, denom)
        block.view(torch.int32)[ops.ACCUM_MICRO] = 3
        partials, flags = ops.grad_sumsq(x)
        ops.optim_ctrl_update_accum(ctrl, block, True, partials, flags, table, grad_scale=gscale, max_norm=max_norm, beta1=0.9,
                                    beta2=0.999)
        scale64 = _f32(gscale) / denom
        norm64 = scale64 * tot
        norm, coef, mul = ctrl_f[ops.CTRL_GRAD_NORM].item(), ctrl_f[ops.CTRL_CLIP_COEF].item(), ctrl_f[ops.CTRL_GRAD_MUL].item()
        assert abs(norm - norm64) <= 1e-6 * norm64, (norm, norm64)         # the kernel's fixed-order fp32 partials against fp64
        want = 1.0 if math.isinf(max_norm) else min(1.0, max_norm / (norm64 + 1e-6))
        assert coef == pytest.approx(want, rel=1e-6), (coef, want)
        assert mul == torch.tensor(_f32(scale64)).mul(torch.tensor(coef)).item()       # fp32(scale64) * coef, one fp32 product
        f = block.view(torch.float32)
        assert f[ops.ACCUM_LAST_LOSS].item() == _f32(loss_sum / denom) and f[ops.ACCUM_LAST_DENOM].item() == _f32(denom)
        assert block[0].item() == 0.0 and block[1].item() == 0.0 and block.view(torch.int32)[ops.ACCUM_MICRO].item() == 0
        assert ctrl[ops.CTRL_CALLS].item() == 1 and ctrl[ops.CTRL_APPLIED].item() == 1 and ctrl_f[ops.CTRL_LR].item() == _f32(0.1)
    # use_denom = 0: the sums are reported and cleared, the scale is grad_scale alone
    ctrl, ctrl_f = _ctrl(dev)
    block = _block(dev, 12.5, 40.0)
    ops.optim_ctrl_update_accum(ctrl, block, False, partials, flags, table, grad_scale=0.5)
    assert ctrl_f[ops.CTRL_GRAD_MUL].item() == 0.5
    f = block.view(torch.float32)
    assert f[ops.ACCUM_LAST_LOSS].item() == 12.5 and f[ops.ACCUM_LAST_DENOM].item() == 40.0 and block[1].item() == 0.0


@pytest.mark.parametrize("case", ["use_denom_0", "denom_1"])
def test_ctrl_update_accum_equals_the_plain_update_bit_for_bit(dev, case):
    from lc2is_amd import ops
    table = torch.tensor([0.1, 0.2, 0.3], device=dev)
    g = torch.Generator().manual_seed(5)
    c_old, _ = _ctrl(dev)
    c_new, _ = _ctrl(dev)
    for i, (gscale, max_norm, skip) in enumerate(((1.0, 1.0, True), (0.5, float("inf"), False), (0.3, 0.01, True),
                                                  (1.0, 2.0, True))):
        x = torch.randn(40_000 + 4 * i, generator=g).to(dev) * (i + 1)
        if i == 3:
            x[17] = float("nan")                                          # a skipped update: counters, verdict, kept bc1 / bc2
        partials, flags = ops.grad_sumsq(x)
        kw = dict(grad_scale=gscale, max_norm=max_norm, skip_nonfinite=skip, beta1=0.9, beta2=0.999)
        ops.optim_ctrl_update(c_old, partials, flags, table, **kw)
        block = _block(dev, 3.5, 1.0 if case == "denom_1" else 77.0)
        ops.optim_ctrl_update_accum(c_new, block, case == "denom_1", partials, flags, table, **kw)
        assert torch.equal(c_new, c_old), (i, c_new.tolist(), c_old.tolist())
    assert c_old[ops.CTRL_SKIPPED].item() == 1 and c_old[ops.CTRL_APPLIED].item() == 3


def test_zero_denominator_gives_scale_one_and_a_nan_loss(dev):
    from lc2is_amd import ops
    table = torch.tensor([0.1], device=dev)
    ctrl, ctrl_f = _ctrl(dev)
    block = _block(dev)
    ops.accum_add(block, torch.zeros(2, device=dev))                      # an all-ignored micro-batch: [0, 0]
    partials, flags = ops.grad_sumsq(torch.zeros(4096, device=dev))
    ops.optim_ctrl_update_accum(ctrl, block, True, partials, flags, table, grad_scale=1.0, max_norm=1.0)
    assert ctrl_f[ops.CTRL_GRAD_MUL].item() == 1.0 and ctrl_f[ops.CTRL_GRAD_NORM].item() == 0.0
    assert ctrl[ops.CTRL_FINITE].item() == 1 and ctrl[ops.CTRL_APPLY].item() == 1
    f = block.view(torch.float32)
    assert math.isnan(f[ops.ACCUM_LAST_LOSS].item()) and f[ops.ACCUM_LAST_DENOM].item() == 0.0


def test_accum_add_counts_exactly_past_two_to_the_24(dev):
    """3 x 2^24 + 1 in three adds of 2^24 and a fourth of 1: exact in fp64; an fp32 accumulator would lose the 1."""
    from lc2is_amd import ops
    block = _block(dev)
    big = torch.tensor([0.5, 2.0 ** 24], device=dev)
    for _ in range(3):
        ops.accum_add(block, big)
    ops.accum_add(block, torch.tensor([0.25, 1.0], device=dev))
    assert block[ops.ACCUM_DENOM].item() == 3 * 2.0 ** 24 + 1 and block[ops.ACCUM_LOSS_SUM].item() == 1.75
    assert block.view(torch.int32)[ops.ACCUM_MICRO].item() == 4
    assert (torch.tensor(3 * 2.0 ** 24) + torch.tensor(1.0)).item() != 3 * 2.0 ** 24 + 1     # what fp32 would have given
    ctrl, ctrl_f = _ctrl(dev)
    partials, flags = ops.grad_sumsq(torch.ones(4096, device=dev))
    ops.optim_ctrl_update_accum(ctrl, block, True, partials, flags, torch.tensor([0.1], device=dev))
    assert ctrl_f[ops.CTRL_GRAD_MUL].item() == _f32(1.0 / (3 * 2.0 ** 24 + 1))
    assert ctrl_f[ops.CTRL_GRAD_NORM].item() == _f32(64.0 / (3 * 2.0 ** 24 + 1))


# ---------------------------------------------------------------------------------------------------------------------
# 2. nothing moves inside a cycle
# ---------------------------------------------------------------------------------------------------------------------
def test_nothing_moves_inside_a_cycle(dev):
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep
    m = _model(dev)
    n = 3
    ts = TrainStep(m, accumulate=n, **_device_kw(m))
    table = torch.tensor(COSINE, dtype=torch.float64).to(torch.float32)
    start = _bits(ts)
    for cycle in range(2):
        before = _bits(ts)
        for k in range(n - 1):
            loss = ts.step(*_batch(dev, 10 * cycle + k))
            assert torch.isfinite(loss).item() and ts.micro == k + 1
            _same_bits(_bits(ts), before)                                # parameters, moments, EMA, control block: untouched
            assert ts._accum.view(torch.int32)[ops.ACCUM_MICRO].item() == k + 1
        ts.step(*_batch(dev, 10 * cycle + n - 1))
        assert ts.micro == 0 and ts.t == cycle + 1
        assert ts._ctrl[ops.CTRL_CALLS].item() == ts.applied_steps.item() == cycle + 1
        assert ts.last_lr.item() == table[cycle].item()
        assert ts.last_clip_coef.item() < 1.0                            # clipping was live, on the mean-scale gradient
        assert ts.accum_count.item() == n * 2 * 16 * 16 and torch.isfinite(ts.accum_loss).item()
        after = _bits(ts)
        for k in ("flat", "m", "v", "ema"):
            assert not torch.equal(after[k], before[k]), k
    assert not torch.equal(start["flat"], ts.arena.flat)


def test_accumulate_1_is_the_plain_step(dev):
    """No control block, no accumulation block, no new keyword in the model call, the plain step's bits."""
    from lc2is_amd.step import TrainStep
    m_a, m_b = _model(dev), _model(dev)
    ts_a, ts_b = TrainStep(m_a, lr=1e-3), TrainStep(m_b, lr=1e-3, accumulate=1)
    assert ts_b._ctrl is None and ts_b._accum is None and ts_b._accum_n is None
    seen = []
    inner = m_b.forward_loss
    m_b.forward_loss = lambda *a, **kw: (seen.append(sorted(kw)), inner(*a, **kw))[1]
    for s in range(2):
        assert torch.equal(ts_a.step(*_batch(dev, s)), ts_b.step(*_batch(dev, s)))
        assert ts_b.micro == 0
    assert seen == [[], []]
    assert torch.equal(ts_a.arena.flat, ts_b.arena.flat)
    ts_b.flush()                                                         # nothing open: nothing happens
    assert torch.equal(ts_a.arena.flat, ts_b.arena.flat) and ts_b.t == 2
    with pytest.raises(RuntimeError, match="does not accumulate"):
        ts_b.accum_loss


# ---------------------------------------------------------------------------------------------------------------------
# 3. an all-ignored micro-batch is exactly nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ignored_first", "ignored_last"])
def test_all_ignored_micro_batch_is_exactly_nothing(dev, order):
    """reduction='sum', SGD without momentum or decay: the cycle {real, all-ignored} in either order leaves every parameter equal
    to a plain N = 1 step on the real micro-batch alone: the first call overwrites, the later call adds (zeros) in every writer."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    real = _batch(dev, 3)
    dead = _batch(dev, 4, ignore_rows=16)
    assert bool((dead[1] == IGNORE).all())
    kw = dict(optimizer="sgd", lr=1e-5)
    ts_ref = TrainStep(_model(dev), criterion=N.CrossEntropyLoss(ignore_index=IGNORE, reduction="sum"), device_state=True, **kw)
    ts_acc = TrainStep(_model(dev), criterion=N.CrossEntropyLoss(ignore_index=IGNORE, reduction="sum"), accumulate=2, **kw)
    start = ts_ref.arena.flat.clone()
    loss_ref = ts_ref.step(*real)
    losses = [ts_acc.step(*b) for b in ((dead, real) if order == "ignored_first" else (real, dead))]
    loss_real, loss_dead = (losses[1], losses[0]) if order == "ignored_first" else losses
    assert torch.equal(loss_real, loss_ref) and loss_dead.item() == 0.0
    assert not torch.equal(ts_ref.arena.flat, start)
    moved = 0
    for (k, p), (_, q) in zip(ts_acc.model.named_parameters(), ts_ref.model.named_parameters()):
        assert torch.equal(p, q), k
        moved += int(not torch.equal(p.detach().flatten(), start[ts_ref.arena.ranges[id(q)][0]:ts_ref.arena.ranges[id(q)][1]]))
    assert moved > 10
    assert ts_acc.accum_loss.item() == loss_ref.item() and ts_acc.accum_count.item() == 2 * 16 * 16


# ---------------------------------------------------------------------------------------------------------------------
# 4. the exact mean
# ---------------------------------------------------------------------------------------------------------------------
def _weights(dev):
    """Class weights in {0.5, 1, 1.5, 2}: every weighted count is a multiple of 0.5 far below 2^24, exact in fp32 in any order."""
    g = torch.Generator().manual_seed(21)
    return (torch.randint(1, 5, (151,), generator=g).float() * 0.5).to(dev)


def _criterion(dev, weighted):
    import lc2is_amd.nn as N
    if not weighted:
        return N.CrossEntropyLoss(ignore_index=IGNORE)
    return N.CrossEntropyLoss(weight=_weights(dev), ignore_index=IGNORE, label_smoothing=0.1).to(dev)


def _count(labels, dev, weighted):
    valid = labels[labels != IGNORE]
    return float(_weights(dev).double()[valid].sum().item()) if weighted else float(valid.numel())


def _one_step_delta(dev, batch, weighted):
    from lc2is_amd.step import TrainStep
    ts = TrainStep(_model(dev), optimizer="sgd", lr=LR, criterion=_criterion(dev, weighted))
    before = _named(ts)
    loss = ts.step(*batch)
    after = _named(ts)
    return {k: (after[k] - before[k]).double() for k in KEYS}, loss


def _exact_mean_case(dev, n, weighted, ignore_rows, tag):
    from lc2is_amd.step import TrainStep
    micro = [_batch(dev, 40 + k, ignore_rows=ignore_rows if k == 0 else 0) for k in range(n)]
    counts = [_count(b[1], dev, weighted) for b in micro]
    # the code under test
    ts = TrainStep(_model(dev), optimizer="sgd", lr=LR, criterion=_criterion(dev, weighted), accumulate=n)
    before = _named(ts)
    for b in micro:
        ts.step(*b)
    after = _named(ts)
    got = {k: (after[k] - before[k]).double() for k in KEYS}
    # reference (a): one plain step on the concatenated batch; reference (b): the count-weighted mean of the plain single steps
    ref_a, loss_a = _one_step_delta(dev, _cat(micro), weighted)
    singles = [_one_step_delta(dev, b, weighted)[0] for b in micro]
    ctot = sum(counts)
    res = {}
    for k in KEYS:
        ref_b = sum(c * d[k] for c, d in zip(counts, singles)) / ctot
        mean_of_means = sum(d[k] for d in singles) / n
        res[k] = dict(vs_a=_rel(got[k], ref_a[k]), vs_b=_rel(got[k], ref_b), a_vs_b=_rel(ref_a[k], ref_b),
                      mean_of_means_vs_b=_rel(mean_of_means, ref_b))
    loss_err = abs(ts.accum_loss.item() - loss_a.item())
    print(f"{tag}: counts {counts} accum_count {ts.accum_count.item()} loss |accum - (a)| {loss_err:.3e}")
    for k in KEYS:
        print(f"  {k}: " + " ".join(f"{a}={b:.3e}" for a, b in res[k].items()))
    _note(tag, dict(max_vs_a=max(r["vs_a"] for r in res.values()), max_vs_b=max(r["vs_b"] for r in res.values()),
                    min_mean_of_means_vs_b=min(r["mean_of_means_vs_b"] for r in res.values()), loss_abs_err=loss_err))
    return res, loss_err, ts.accum_count.item(), ctot


@pytest.mark.parametrize("n,weighted", [(2, False), (2, True), (3, False), (3, True)],
                         ids=["n2", "n2_weights_smoothing", "n3", "n3_weights_smoothing"])
def test_exact_large_batch_mean(dev, n, weighted):
    """Micro-batch 1 has 7/8 of its label rows ignored (64 valid labels), the others none (512 each).  The accumulated update is
    within relative L2 8e-2 of (a) a plain step on the concatenated batch and of (b) (sum_k c_k D_k) / (sum_k c_k), D_k the change
    of a plain step on micro-batch k alone, c_k its (weighted) valid count.  Precondition: the mean of means (sum_k D_k) / N is at
    least 3 x 8e-2 from (b) for every compared parameter, so an implementation that averages micro-batch means cannot pass."""
    tag = f"exact_mean/n{n}" + ("_weighted" if weighted else "")
    res, loss_err, got_count, want_count = _exact_mean_case(dev, n, weighted, 14, tag)
    if min(r["mean_of_means_vs_b"] for r in res.values()) < 3 * GRAD_BOUND:   # (the issue's rule: raise the share, never the factor)
        res, loss_err, got_count, want_count = _exact_mean_case(dev, n, weighted, 15, tag + "_15of16")
    for k in KEYS:
        assert res[k]["mean_of_means_vs_b"] >= 3 * GRAD_BOUND, (k, res[k])
    for k in KEYS:
        assert res[k]["vs_a"] <= GRAD_BOUND and res[k]["vs_b"] <= GRAD_BOUND, (k, res[k])
    assert loss_err <= LOSS_BOUND, loss_err
    assert got_count == want_count, (got_count, want_count)


# ---------------------------------------------------------------------------------------------------------------------
# 5. non-finite
# ---------------------------------------------------------------------------------------------------------------------
def test_nonfinite_cycle_is_skipped_and_the_next_starts_clean(dev):
    from lc2is_amd import ops
    from lc2is_amd.step import TrainStep
    m = _model(dev)
    kw = dict(_device_kw(m), skip_nonfinite=True)
    ts = TrainStep(m, accumulate=2, **kw)
    bad = _batch(dev, 1)
    bad[0]["pixel_values"][1, 1, 20, 33] = float("nan")                  # arithmetic, not a fault: the NaN spreads through the forward
    before = _bits(ts)
    loss = ts.step(*bad)
    assert not torch.isfinite(loss).item()
    ts.step(*_batch(dev, 2))
    assert ts.skipped_steps.item() == 1 and ts.applied_steps.item() == 0 and ts._ctrl[ops.CTRL_CALLS].item() == 1
    assert not torch.isfinite(ts.last_grad_norm).item() and ts.micro == 0
    _same_bits(_bits(ts), before, skip=("_ctrl",))                       # parameters, moments, EMA
    clean = [_batch(dev, 3), _batch(dev, 4)]
    losses = [ts.step(*b).clone() for b in clean]
    # the same cycle on a fresh TrainStep whose schedule index was advanced by one
    m2 = _model(dev)
    ts2 = TrainStep(m2, accumulate=2, **dict(_device_kw(m2), skip_nonfinite=True))
    ts2._ctrl[ops.CTRL_CALLS] = 1
    losses2 = [ts2.step(*b).clone() for b in clean]
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    _same_bits(_bits(ts), _bits(ts2), skip=("_ctrl",))
    assert ts.last_lr.item() == ts2.last_lr.item() == _f32(COSINE[1]) and ts.applied_steps.item() == 1
    assert torch.equal(ts.accum_loss, ts2.accum_loss) and not torch.equal(ts.arena.flat, before["flat"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. reproducible, resumable, ragged
# ---------------------------------------------------------------------------------------------------------------------
def _fresh(dev, n=2):
    from lc2is_amd.step import TrainStep
    m = _model(dev)
    return m, TrainStep(m, accumulate=n, **_device_kw(m))


def test_reproducible_and_resumable(dev, tmp_path):
    from lc2is_amd.checkpoint import load_checkpoint, load_train_state, save_checkpoint, save_train_state
    batches = [_batch(dev, s) for s in range(6)]                          # three cycles of N = 2
    runs = []
    for _ in range(2):
        _, ts = _fresh(dev)
        losses = [ts.step(*b).clone() for b in batches]
        runs.append((losses, _bits(ts), ts.accum_loss.clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and torch.equal(runs[0][2], runs[1][2])
    _same_bits(runs[0][1], runs[1][1])
    # stop after cycle 1, save, load into fresh objects, continue
    m_b, ts_b = _fresh(dev)
    ts_b.step(*batches[0])
    with pytest.raises(RuntimeError, match="cycle is open"):
        ts_b.state_dict()
    with pytest.raises(RuntimeError, match="cycle is open"):
        save_train_state(ts_b, tmp_path, 0)
    with pytest.raises(RuntimeError, match="cycle is open"):
        ts_b.load_state_dict({})
    ts_b.step(*batches[1])
    f_model, f_train = save_checkpoint(m_b, tmp_path, 1), save_train_state(ts_b, tmp_path, 1)
    m_c, ts_c = _fresh(dev)
    load_checkpoint(m_c, f_model)
    load_train_state(ts_c, f_train)
    assert ts_c.t == 1 and ts_c.micro == 0
    losses_c = [ts_c.step(*b).clone() for b in batches[2:]]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0][2:], losses_c))
    _same_bits(_bits(ts_c), runs[0][1])
    assert ts_c.t == 3 and ts_c.applied_steps.item() == 3
    # the saved state does not depend on N: it loads into a plain device-held TrainStep
    from lc2is_amd.step import TrainStep
    m_d = _model(dev)
    TrainStep(m_d, **_device_kw(m_d)).load_state_dict(torch.load(f_train, weights_only=True))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights_smoothing"])
def test_flush_applies_the_ragged_cycle(dev, weighted):
    """flush() after 1 of 3 calls: the update of an N = 1 step on that micro-batch, within the gradient bound."""
    from lc2is_amd.step import TrainStep
    b = _batch(dev, 50, ignore_rows=5)
    ts = TrainStep(_model(dev), optimizer="sgd", lr=LR, criterion=_criterion(dev, weighted), accumulate=3)
    ts.flush()
    assert ts.t == 0 and ts.micro == 0
    before = _named(ts)
    loss = ts.step(*b)
    assert ts.micro == 1 and ts.t == 0
    ts.flush()
    assert ts.micro == 0 and ts.t == 1 and ts.applied_steps.item() == 1
    after = _named(ts)
    ref, loss_ref = _one_step_delta(dev, b, weighted)
    worst = max(_rel((after[k] - before[k]).double(), ref[k]) for k in KEYS)
    _note("flush_1_of_3" + ("_weighted" if weighted else ""), worst)
    assert worst <= GRAD_BOUND, worst
    assert torch.equal(loss, loss_ref) and abs(ts.accum_loss.item() - loss_ref.item()) <= LOSS_BOUND
    assert ts.accum_count.item() == _count(b[1], dev, weighted)
    ts.step(*_batch(dev, 51))                                            # the next cycle starts at its first call
    assert ts.micro == 1


# ---------------------------------------------------------------------------------------------------------------------
# 7. seg_metrics keeps counting every micro-batch
# ---------------------------------------------------------------------------------------------------------------------
def test_seg_metrics_count_every_micro_batch(dev):
    from lc2is_amd.step import TrainStep
    ts = TrainStep(_model(dev), optimizer="sgd", lr=1e-3, ignore_index=IGNORE, accumulate=3, seg_metrics=True)
    micro = [_batch(dev, 60, ignore_rows=3), _batch(dev, 61), _batch(dev, 62, ignore_rows=9)]
    for b in micro:
        ts.step(*b)
    valid = sum(int((b[1] != IGNORE).sum()) for b in micro)
    assert ts.seg_counts[2].sum().item() == valid == ts.accum_count.item()


def test_ohem_denominator_is_the_kept_count(dev):
    """OHEM selects per micro-batch; the cycle's denominator is the number of pixels the head saw after relabelling, over all calls."""
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    crit = N.OhemCrossEntropyLoss(thresh=0.7, min_kept=40, ignore_index=IGNORE)
    ts = TrainStep(_model(dev), optimizer="sgd", lr=1e-3, criterion=crit, accumulate=2)
    kept, losses = 0, []
    for b in (_batch(dev, 80, ignore_rows=4), _batch(dev, 81)):
        losses.append(ts.step(*b).item())
        seen = int((ts.ohem_labels != IGNORE).sum())
        assert 0 < seen <= int((b[1] != IGNORE).sum())
        kept += seen
    assert ts.accum_count.item() == kept and ts.micro == 0 and ts.applied_steps.item() == 1
    lo, hi = min(losses), max(losses)                                     # a count-weighted mean of the two lies between them
    assert lo - 1e-4 <= ts.accum_loss.item() <= hi + 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture: the whole cycle as one graph
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_cycle_equals_the_eager_cycles(dev):
    """AdamW, a warm-up-and-decay table, clipping; a captured N = 2 cycle replayed for two cycles against the eager cycles on a twin:
    losses, parameters and control block bit for bit."""
    from lc2is_amd.step import TrainStep
    rates = [2e-4, 6e-4, 1e-3, 8e-4, 6e-4, 4e-4, 2e-4]
    kw = dict(optimizer="adamw", weight_decay=0.01, lr_schedule=rates, max_grad_norm=MAX_NORM, skip_nonfinite=True, accumulate=2)
    ts_e, ts_g = TrainStep(_model(dev), **kw), TrainStep(_model(dev), **kw)
    first = [_batch(dev, 0), _batch(dev, 1)]
    ins, lbs = [b[0] for b in first], [b[1] for b in first]
    with pytest.raises(ValueError, match="sequences"):
        ts_g.capture(*first[0])
    for _ in range(2):                                                   # capture() runs 2 real warm-up cycles, then records one
        for b in first:
            ts_e.step(*b)
    run = ts_g.capture(ins, lbs)
    try:
        torch.cuda.synchronize()
        assert ts_g._ctrl[0].item() == 2 and ts_g.t == 2 and ts_g.micro == 0     # the recorded cycle did not run
        for c in range(2):
            cyc = [_batch(dev, 10 + 2 * c), _batch(dev, 11 + 2 * c, ignore_rows=6)]
            losses_e = [ts_e.step(*b).item() for b in cyc]
            losses_g = [x.item() for x in run([b[0] for b in cyc], [b[1] for b in cyc])]
            print(f"cycle {c}: eager {losses_e} captured {losses_g}")
            assert losses_e == losses_g
            assert ts_g.last_lr.item() == ts_e.last_lr.item() == _f32(rates[2 + c]) and ts_g.last_clip_coef.item() < 1.0
            assert torch.equal(ts_g.accum_loss, ts_e.accum_loss) and ts_g.accum_count.item() == 2 * 256 + 2 * 160
        assert torch.equal(ts_g._ctrl, ts_e._ctrl) and ts_g.t == ts_e.t == 4
        diff = (ts_g.arena.flat != ts_e.arena.flat).sum().item()
        assert diff == 0, f"{diff} of {ts_g.arena.flat.numel()} parameter elements differ"
        assert torch.equal(ts_g.m, ts_e.m) and torch.equal(ts_g.v, ts_e.v)
    finally:
        run.release()


# ---------------------------------------------------------------------------------------------------------------------
# 9. two gloo ranks on the one GPU
# ---------------------------------------------------------------------------------------------------------------------
def _rank_batches(dev, rank):
    """N = 2 micro-batches of 2 images per rank; rank 1's first micro-batch has 7/8 of its rows ignored: unequal counts."""
    return [_batch(dev, 70 + 10 * rank, ignore_rows=14 if rank == 1 else 0), _batch(dev, 71 + 10 * rank)]


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")                             # gloo: both ranks share the one GPU of the test box
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import lc2is_amd.nn as N
    from lc2is_amd.dp import GradReducer
    from lc2is_amd.step import TrainStep
    red = GradReducer(bucket_elems=100_000)
    ts = TrainStep(_model(dev), optimizer="sgd", lr=LR, criterion=N.CrossEntropyLoss(ignore_index=IGNORE), accumulate=2,
                   reducer=red)
    red.broadcast_params(ts.arena.flat, src=0)
    before = _named(ts)
    colls = []
    for b in _rank_batches(dev, rank):
        ts.step(*b)
        colls.append(red.collectives_last_step)
    torch.cuda.synchronize()
    after = _named(ts)
    torch.save(dict(colls=colls, flat=ts.arena.flat.cpu(), delta={k: (after[k] - before[k]).cpu() for k in KEYS},
                    count=ts.accum_count.item(), loss=ts.accum_loss.item(), micro=ts.micro, t=ts.t),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reduce_once_per_cycle_to_the_global_mean(dev, tmp_path):
    ctx = mp.get_context("spawn")
    port = 29650 + os.getpid() % 100
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    # meanwhile, the reference: a single-process plain step on all 2 * N * 2 images
    every = [b for r in range(2) for b in _rank_batches(dev, r)]
    ref, loss_ref = _one_step_delta(dev, _cat(every), False)
    want_count = sum(_count(b[1], dev, False) for b in every)
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
    for r in (r0, r1):
        assert r["colls"][0] == 0 and r["colls"][1] > 0, r["colls"]
        assert r["count"] == want_count == 512 + 512 + 64 + 512 and r["micro"] == 0 and r["t"] == 1
        assert abs(r["loss"] - loss_ref.item()) <= LOSS_BOUND
    assert torch.equal(r0["flat"], r1["flat"]), "replicas diverged"
    worst = max(_rel(r0["delta"][k].to(dev), ref[k]) for k in KEYS)
    print(f"two ranks, N = 2: update vs one plain step on all 8 images, worst rel-L2 {worst:.3e}; collectives {r0['colls']}")
    _note("two_ranks_n2_vs_global_step", worst)
    assert worst <= GRAD_BOUND, worst
