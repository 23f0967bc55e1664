"""Exact resume of a run: TrainStep.state_dict / load_state_dict and checkpoint.save_train_state / load_train_state.

The train step is bitwise reproducible (test_gpu_step_repro.py), so "stop, save, load, continue" is held to the same standard:
run A goes straight through, run B stops and saves, run C starts from fresh objects, loads and continues — and every loss,
parameter, optimizer buffer, the EMA and the control block of C equal A's bit for bit.  The tiny model and the 2-image batches
are those of test_gpu_optim_ctrl.py."""
import math
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

MAX_NORM = 0.05
COSINE = [0.5e-3 * (1.0 + math.cos(math.pi * i / 8)) for i in range(8)]


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


def _device_kw(model):
    from lc2is_amd.step import make_param_groups
    return dict(optimizer="adamw", lr_schedule=COSINE, max_grad_norm=MAX_NORM, ema_decay=0.99, ema_warmup=True,
                param_groups=make_param_groups(model, weight_decay=0.05, layer_decay=0.9))


def _buffers(ts):
    out = {"flat": ts.arena.flat}
    for k in ("mom", "m", "v", "ema", "_ctrl"):
        t = getattr(ts, k, None)
        if t is not None:
            out[k] = t
    return out


def _same_bits(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        x, y = a[k].view(torch.int32), b[k].view(torch.int32)
        assert torch.equal(x, y), f"{k}: {(x != y).sum().item()} of {x.numel()} elements differ"


def _fresh(dev, make_kw, dropout=0.0):
    """A new model from the fixed seed, the dropout stream restarted, a new TrainStep."""
    from lc2is_amd.nn.base import DropoutRng
    from lc2is_amd.step import TrainStep
    m = _model(dev, dropout)
    DropoutRng.set_state(None)
    return m, TrainStep(m, **make_kw(m))


def _resume_case(dev, tmp_path, make_kw, dropout=0.0, steps=5, stop=2):
    from lc2is_amd.checkpoint import load_checkpoint, load_train_state, save_checkpoint, save_train_state
    from lc2is_amd.nn.base import DropoutRng
    batches = [_batch(dev, s) for s in range(steps)]
    # run A: straight through
    _, ts_a = _fresh(dev, make_kw, dropout)
    losses_a = [ts_a.step(*b).clone() for b in batches]
    if dropout:
        assert any(p == pytest.approx(dropout) for _, p in DropoutRng.last.values())
    state_a = {k: v.clone() for k, v in _buffers(ts_a).items()}
    # run B: stop after `stop` steps and save
    m_b, ts_b = _fresh(dev, make_kw, dropout)
    for b in batches[:stop]:
        ts_b.step(*b)
    f_model = save_checkpoint(m_b, tmp_path, stop)
    f_train = save_train_state(ts_b, tmp_path, stop)
    assert f_train == tmp_path / "checkpoints" / f"step-{stop}.train.pt" and f_train.is_file() and f_model.is_file()
    assert (tmp_path / "checkpoints" / f"step-{stop}.ema.pt").is_file() == (ts_b.ema is not None)
    del m_b, ts_b
    # run C: fresh objects (the dropout stream back at its start: the sidecar must carry it), load, continue
    m_c, ts_c = _fresh(dev, make_kw, dropout)
    ptrs = {k: v.data_ptr() for k, v in _buffers(ts_c).items()}
    load_checkpoint(m_c, f_model)
    load_train_state(ts_c, f_train)
    assert {k: v.data_ptr() for k, v in _buffers(ts_c).items()} == ptrs      # copied in place
    assert ts_c.t == stop
    losses_c = [ts_c.step(*b).clone() for b in batches[stop:]]
    for i, (la, lc) in enumerate(zip(losses_a[stop:], losses_c)):
        assert torch.equal(la, lc), f"step {stop + i + 1}: loss {lc.item()!r}, the uninterrupted run's {la.item()!r}"
    _same_bits(_buffers(ts_c), state_a)
    assert ts_c.t == ts_a.t == steps
    return ts_a, ts_c


@pytest.mark.parametrize("dropout", [0.0, 0.1], ids=["no_dropout", "decoder_dropout"])
def test_bitwise_resume_device_path(dev, tmp_path, dropout):
    """AdamW + cosine table + clipping + parameter groups (weight decay, layer decay) + EMA with warm-up: 5 steps against 2 + save +
    load + 3.  With decoder dropout the existing sidecar carries the stream: the masks continue."""
    from lc2is_amd import ops
    ts_a, ts_c = _resume_case(dev, tmp_path, _device_kw, dropout)
    assert ts_c.applied_steps.item() == 5 and ts_c._ctrl[ops.CTRL_CALLS].item() == 5
    assert ts_c.last_lr.item() == torch.tensor(COSINE[4], dtype=torch.float64).to(torch.float32).item()
    assert ts_c.last_clip_coef.item() < 1.0 and len(ts_c.param_groups) > 2      # clipping and the groups were live
    assert not torch.equal(ts_c.ema, ts_c.arena.flat)


@pytest.mark.parametrize("kw", [dict(optimizer="sgd", lr=1e-3, momentum=0.9, weight_decay=1e-4),
                                dict(optimizer="adamw", lr=1e-3, weight_decay=0.01)], ids=["sgd_momentum", "adamw"])
def test_bitwise_resume_host_path(dev, tmp_path, kw):
    """No device-path option: t and the moments (or the momentum buffer) alone.  A resumed AdamW that restarted t would redo the
    bias correction of step 1 and miss the uninterrupted run's bits."""
    ts_a, ts_c = _resume_case(dev, tmp_path, lambda m: kw)
    assert ts_c._ctrl is None and ts_c.ema is None
    sd = ts_c.state_dict()
    assert "ctrl" not in sd and "ema" not in sd and sd["t"] == 5 and sd["meta"]["device_path"] is False
    assert ("mom" in sd) == (kw["optimizer"] == "sgd") and ("m" in sd and "v" in sd) == (kw["optimizer"] == "adamw")


def test_load_is_in_place_and_a_captured_step_stays_valid(dev, tmp_path):
    """A step captured BEFORE the load replays on the loaded state: the load copies into the buffers the graph holds pointers to.
    Run A: capture, 4 replays (and the same six steps eagerly).  Run B: capture, 2 replays, save.  Run C: capture (its own 2
    warm-up steps leave it in another state), load B's files, 2 replays: A's bits."""
    from lc2is_amd.checkpoint import load_checkpoint, load_train_state, save_checkpoint, save_train_state
    kw = dict(optimizer="sgd", momentum=0.9, weight_decay=1e-4, lr_schedule=[1e-3, 2e-3, 3e-3, 2e-3, 1e-3, 5e-4, 2e-4],
              ema_decay=0.9, ema_warmup=True)
    batches = [_batch(dev, s) for s in range(5)]
    runs = []
    try:
        _, ts_a = _fresh(dev, lambda m: kw)
        run_a = ts_a.capture(*batches[0])
        runs.append(run_a)
        losses_a = [run_a(*b).clone() for b in batches[1:]]
        torch.cuda.synchronize()
        state_a = {k: v.clone() for k, v in _buffers(ts_a).items()}
        _, ts_e = _fresh(dev, lambda m: kw)                          # ... and the same run eagerly: on this model the same bits
        for b in [batches[0]] * 2 + batches[1:]:
            ts_e.step(*b)
        _same_bits(_buffers(ts_e), state_a)
        del ts_e

        m_b, ts_b = _fresh(dev, lambda m: kw)
        run_b = ts_b.capture(*batches[0])
        runs.append(run_b)
        for b in batches[1:3]:
            run_b(*b)
        f_model, f_train = save_checkpoint(m_b, tmp_path, 4), save_train_state(ts_b, tmp_path, 4)

        m_c, ts_c = _fresh(dev, lambda m: kw)
        run_c = ts_c.capture(*batches[4])                            # another batch: C's state before the load is not B's
        runs.append(run_c)
        torch.cuda.synchronize()
        assert not torch.equal(ts_c.arena.flat, ts_b.arena.flat)
        ptrs = {k: v.data_ptr() for k, v in _buffers(ts_c).items()}
        assert set(ptrs) == {"flat", "mom", "ema", "_ctrl"}
        load_checkpoint(m_c, f_model)
        load_train_state(ts_c, f_train)
        assert {k: v.data_ptr() for k, v in _buffers(ts_c).items()} == ptrs
        assert ts_c.t == 4 and ts_c.applied_steps.item() == 4
        _same_bits(_buffers(ts_c), _buffers(ts_b))
        losses_c = [run_c(*b).clone() for b in batches[3:]]
        torch.cuda.synchronize()
        for la, lc in zip(losses_a[2:], losses_c):
            assert torch.equal(la, lc), (la.item(), lc.item())
        _same_bits(_buffers(ts_c), state_a)
        assert ts_c.t == ts_a.t == 6
    finally:
        for r in runs:
            r.release()


def test_refusals_name_the_difference_and_change_nothing(dev, tmp_path):
    from lc2is_amd.checkpoint import load_train_state, save_train_state
    from lc2is_amd.step import TrainStep, make_param_groups
    m, ts = _fresh(dev, _device_kw)
    ts.step(*_batch(dev, 0))
    f = save_train_state(ts, tmp_path, 1)
    base = _device_kw(m)

    def other(**change):
        m2 = _model(dev)
        kw = dict(_device_kw(m2), **change)
        kw = {k: v for k, v in kw.items() if v is not ...}
        return TrainStep(m2, **kw)

    cases = [
        (other(optimizer="sgd"), r"saved optimizer is 'adamw'.*'sgd'"),
        (other(param_groups=make_param_groups(m, weight_decay=0.05, layer_decay=0.8)), r"another group recipe"),
        (other(param_groups=[dict(params=["vision_encoder.enc.embeddings.class_embedding"], lr_scale=0.5)]), r"another group"),
        (other(param_groups=...), r"param_groups saved but not configured"),
        (other(lr_schedule=COSINE[:4] + [1e-6] + COSINE[5:]), r"another lr table: entry 4"),
        (other(lr_schedule=COSINE[:5]), r"another lr table: saved 8 entries"),
        (other(ema_decay=..., ema_warmup=...), r"EMA saved but not configured"),
        (other(ema_decay=0.999), r"EMA setting decay"),
        (other(max_grad_norm=1.0), r"max_grad_norm"),
    ]
    assert base["ema_decay"] == 0.99
    for ts2, match in cases:
        ts2.step(*_batch(dev, 1))                                   # live, non-zero state that a partial load would disturb
        before = {k: v.clone() for k, v in _buffers(ts2).items()}
        t_before = ts2.t
        with pytest.raises(ValueError, match=match):
            load_train_state(ts2, f)
        _same_bits(_buffers(ts2), before)
        assert ts2.t == t_before
    # a state saved WITHOUT an EMA into a step that keeps one
    m3, ts3 = _fresh(dev, lambda mm: {k: v for k, v in _device_kw(mm).items() if not k.startswith("ema_")})
    ts3.step(*_batch(dev, 0))
    with pytest.raises(ValueError, match=r"EMA configured but not in the saved state"):
        ts.load_state_dict(ts3.state_dict())
    # a model with another layout
    import lc2is_amd.nn as N
    torch.manual_seed(7)
    m4 = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 4, 128),
                             text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                             dim_feedforward=128, out_dim=64).to(dev).train()
    ts4 = TrainStep(m4, **_device_kw(m4))
    with pytest.raises(ValueError, match=r"parameter '.*' has \d+ elements, the saved state \d+"):
        load_train_state(ts4, f)
    with pytest.raises(ValueError, match="not a TrainStep.state_dict"):
        ts.load_state_dict({"state_dict": {}})
    # and the matching one loads
    ts.step(*_batch(dev, 1))
    load_train_state(ts, f)
    assert ts.t == 1 and ts.applied_steps.item() == 1


def test_file_format(dev, tmp_path):
    from lc2is_amd.checkpoint import save_train_state
    m, ts = _fresh(dev, _device_kw)
    for s in range(2):
        ts.step(*_batch(dev, s))
    assert not (tmp_path / "none").exists()
    f0 = save_train_state(ts, tmp_path / "none", 2, write=False)    # write=False: the path is returned, nothing is written
    assert not f0.exists() and not f0.with_name("step-2.ema.pt").exists()
    f = save_train_state(ts, tmp_path, 2)
    d = tmp_path / "checkpoints"
    assert sorted(p.name for p in d.iterdir()) == ["step-2.ema.pt", "step-2.train.pt"]
    sd = torch.load(f, weights_only=True)                            # tensors, numbers, strings, lists and dicts only

    def plain(x):
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, (list, tuple)):
            return all(plain(v) for v in x)
        if isinstance(x, torch.Tensor):
            return x.device.type == "cpu"
        return x is None or isinstance(x, (bool, int, float, str))

    assert plain(sd)
    assert {"meta", "t", "m", "v", "ctrl", "lr_table", "group_table", "ema"} <= set(sd) and "mom" not in sd
    assert sd["t"] == 2 and sd["ctrl"].dtype == torch.int32 and sd["ctrl"].numel() == 12
    assert torch.equal(sd["ctrl"], ts._ctrl.cpu()) and torch.equal(sd["lr_table"], ts.lr_table.cpu())
    assert torch.equal(sd["group_table"], ts._group_table.cpu())
    for k in ("m", "v", "ema"):
        assert sd[k].dtype == torch.float32 and sd[k].shape == (ts.arena.numel,)
        assert torch.equal(sd[k].view(torch.int32), getattr(ts, k).cpu().view(torch.int32))
    meta = sd["meta"]
    assert meta["optimizer"] == "adamw" and meta["ema"] == dict(decay=0.99, warmup=True, every=1)
    names = [n for n, _ in m.named_parameters()]
    assert meta["layout"]["names"] == names and meta["layout"]["total"] == ts.arena.numel
    assert meta["layout"]["offsets"] == ts.arena.offsets and meta["layout"]["numels"] == [p.numel() for p in ts.arena.params]
    assert len(meta["groups"]["ids"]) == len(names) and len(meta["groups"]["table"]) == len(ts.param_groups)
    # step-N.ema.pt: exactly model.state_dict()'s keys and shapes, loadable with strict=True, and not the parameters themselves
    ema_sd = torch.load(d / "step-2.ema.pt", weights_only=True)
    ref = m.state_dict()
    assert list(ema_sd) == list(ref) and all(ema_sd[k].shape == ref[k].shape and ema_sd[k].dtype == ref[k].dtype for k in ref)
    fresh = _model(dev)
    fresh.load_state_dict(ema_sd, strict=True)
    assert any(not torch.equal(ema_sd[k], ref[k].cpu()) for k in ref)
