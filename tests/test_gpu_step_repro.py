"""The headline train step is bitwise reproducible and does not depend on stream order.

The step has no float atomics in its reductions, so a rerun from the same state gives the same bits, and so does the text tower
on its side stream against the same launches serialised on one stream.  A missing wait, record_stream or per-stream workspace
key, or a float atomic put back into a reduction, leaves the numbers close to right: the oracle tests' tolerances do not notice,
torch.equal does.  The configuration is bench.py's: BaseModelWithText(16, 512, 128), B = 32, text length 16, bench.synth_batch.
Runs go one after another from the same state_dict.  The second half checks the kernel families the step's reductions run
through at the step's own shapes, against fp64 and run to run."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_bench import SMALL

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
B, IN, OUT, L = 32, 512, 128, 16
SEED = 4321


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------------
# bench.py --dump-outputs: two runs with the same arguments write the same bytes (run first: the module's model is not
# built yet, so the bench processes have the GPU to themselves)
# ---------------------------------------------------------------------------------------------------------------------
def _dump(out, args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args, "--dump-outputs", str(out)], capture_output=True,
                       text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    return {f.name: f.read_bytes() for f in sorted(out.iterdir())}


@pytest.mark.parametrize("args", [SMALL, ["--gpus", "1", "--batch", "32", "--steps", "2", "--warmup", "1"]], ids=["small", "b32"])
def test_bench_dump_outputs_are_bitwise_identical(dev, tmp_path, args):
    a, b = _dump(tmp_path / "a", args), _dump(tmp_path / "b", args)
    assert set(a) == {"loss.npy", "params_sample.npy", "grads_sample.npy"}
    for name in a:
        assert a[name] == b[name], f"{name} differs between two bench.py runs with the same arguments"


# ---------------------------------------------------------------------------------------------------------------------
# the composed step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def headline(dev):
    import lc2is_amd.nn as N
    from bench import synth_batch
    torch.manual_seed(1024)
    model = N.BaseModelWithText(16, IN, OUT).to(dev).train()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batches = [synth_batch(B, IN, OUT, L, seed, dev) for seed in (2, 3, 4)]
    yield model, state, batches
    del model, state, batches
    torch.cuda.empty_cache()


def _fresh_step(model, state, **opt):
    from lc2is_amd.nn.base import DropoutRng
    from lc2is_amd.step import TrainStep
    model.load_state_dict(state)
    torch.manual_seed(SEED)
    # the dropout seed stream restarts when torch's seed CHANGES; the same seed again would continue it, so restart it here
    DropoutRng.set_state(None)
    return TrainStep(model, lr=1e-5, **opt)


def _state(ts, loss):
    out = {"loss": loss, "grad": ts.arena.grad, "flat": ts.arena.flat}
    if ts.mom is not None:
        out["mom"] = ts.mom
    if ts.kind == "adamw":
        out["m"], out["v"] = ts.m, ts.v
    return out


def _check_or_keep(i, cur, ref, keep):
    """Step i: keep a copy (reference run) or compare with torch.equal."""
    if ref is None:
        keep.append({k: v.clone() for k, v in cur.items()})
        return
    assert set(cur) == set(ref[i])
    for k, v in cur.items():
        if not torch.equal(v, ref[i][k]):
            n = int((v != ref[i][k]).sum().item())
            raise AssertionError(f"step {i}: {k} differs from the reference run in {n} of {v.numel()} elements")


def _eager(model, state, batches, ref=None, **opt):
    ts = _fresh_step(model, state, **opt)
    keep = []
    for i, (inputs, labels) in enumerate(batches):
        loss = ts.step(inputs, labels)
        torch.cuda.synchronize()
        _check_or_keep(i, _state(ts, loss), ref, keep)
    return keep


@pytest.mark.parametrize("case", ["sgd_momentum", "adamw", "sgd_dropout"])
def test_eager_rerun_is_bitwise_equal(dev, headline, case):
    model, state, batches = headline
    opt = dict(optimizer="adamw", weight_decay=0.05) if case == "adamw" else dict(optimizer="sgd", momentum=0.9)
    if case == "sgd_dropout":
        import lc2is_amd.nn as N
        model = N.BaseModelWithText(16, IN, OUT, dropout=0.1).to(dev).train()
    ref = _eager(model, state, batches, **opt)
    if case == "sgd_dropout":
        from lc2is_amd.nn.base import DropoutRng
        assert any(p == pytest.approx(0.1) for _, p in DropoutRng.last.values())
    _eager(model, state, batches, ref=ref, **opt)


def test_text_overlap_matches_serial(dev, headline, monkeypatch):
    """The text tower beside the vision tower (high-priority side stream, then a normal-priority one) against the same launches
    serialised on one stream.  The side stream is created lazily, at the first overlapped forward: reset it per setting."""
    model, state, batches = headline
    opt = dict(optimizer="sgd", momentum=0.9)
    try:
        model.overlap_text = False
        ref = _eager(model, state, batches, **opt)
        model.overlap_text = True
        for prio in ("-1", "0"):
            monkeypatch.setenv("LC2IS_TEXT_STREAM_PRIO", prio)
            model._text_stream = None
            _eager(model, state, batches, ref=ref, **opt)
            prio_now = model._text_stream.priority
            assert prio_now == 0 if prio == "0" else prio_now < 0
    finally:
        model.overlap_text = True
        model._text_stream = None


def _captured(model, state, batches, ref=None):
    ts = _fresh_step(model, state, optimizer="sgd", momentum=0.9)
    replay = ts.capture(*batches[0])        # two real warm-up steps on batch 0, then the captured step
    keep = []
    try:
        for i, (inputs, labels) in enumerate(batches):
            loss = replay(inputs, labels)
            torch.cuda.synchronize()
            _check_or_keep(i, _state(ts, loss), ref, keep)
    finally:
        replay.release()
        model.overlap_text = True
    return keep


def test_captured_step_replays_are_bitwise_equal(dev, headline, monkeypatch):
    """Two captures from the same state replay the same bits; one captured stream (LC2IS_GRAPH_OVERLAP=0) against the captured
    text-tower fork / join."""
    model, state, batches = headline
    monkeypatch.delenv("LC2IS_GRAPH_OVERLAP", raising=False)
    ref = _captured(model, state, batches)
    _captured(model, state, batches, ref=ref)
    monkeypatch.setenv("LC2IS_GRAPH_OVERLAP", "0")
    _captured(model, state, batches, ref=ref)


def test_evaluation_overlap_on_equals_off(dev, headline):
    """Evaluator.evaluate over 4 batches at 512x512: eval_loss and every per-image mIoU, text tower overlapped or serialised."""
    from bench import synth_batch
    from lc2is_amd.evalloop import Evaluator
    from lc2is_amd.nn import CrossEntropyLoss
    model, state, _ = headline
    model.load_state_dict(state)
    data = []
    for seed in range(4):
        inputs, labels = synth_batch(B, IN, OUT, L, 10 + seed, dev)
        data.append(({**inputs, "label": labels}, None))
    res = []
    try:
        for overlap in (False, True):
            model.overlap_text = overlap
            ev = Evaluator(model, data, CrossEntropyLoss(), device=dev)
            rec, loop = {}, ev.eval_loop

            def recording(loop=loop, rec=rec):
                m, o = loop()
                rec.update(o)
                return m, o
            ev.eval_loop = recording
            metrics = ev.evaluate()
            res.append((metrics, rec["per_image_mIOU"].clone()))
    finally:
        model.overlap_text = True
        model.train()
    (m0, p0), (m1, p1) = res
    assert p0.shape == (4 * B,) and torch.isfinite(p0).all()
    assert m0["eval_loss"] == m1["eval_loss"], (m0, m1)
    assert torch.equal(p0, p1) and m0["eval_mIOU_label"] == m1["eval_mIOU_label"]


# ---------------------------------------------------------------------------------------------------------------------
# kernel families at the step's own shapes: fp64 and run-to-run bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grouped_calls(dev, headline):
    """The problem lists ops.gemm_tn_grouped receives during one eager B = 32 step (distinct lists once each)."""
    from lc2is_amd import ops
    model, state, batches = headline
    calls, orig = [], ops.gemm_tn_grouped

    def recording(problems):
        calls.append(tuple((tuple(dy.shape), dy.stride(), x.shape[1], x.stride(), dw.stride(), db is not None, bool(acc))
                           for dy, x, dw, db, acc in problems))
        return orig(problems)

    ops.gemm_tn_grouped = recording
    try:
        ts = _fresh_step(model, state)
        ts.step(*batches[0])
        torch.cuda.synchronize()
    finally:
        ops.gemm_tn_grouped = orig
    assert calls, "the step made no grouped weight-gradient launch"
    return list(dict.fromkeys(calls))


def _strided(shape, stride, dtype, fill, dev):
    n = (shape[0] - 1) * stride[0] + shape[1]
    return torch.full((n,), fill, dtype=dtype, device=dev).as_strided(shape, stride)


def _replay(call, seed, dev):
    """Seeded operands with the recorded shapes and strides (row padding NaN, outputs NaN unless accumulated into)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    probs, priors = [], []
    for (M, N), sdy, K, sx, sw, has_db, acc in call:
        dy = _strided((M, N), sdy, torch.bfloat16, float("nan"), dev)
        dy.copy_(torch.randn(M, N, generator=g, device=dev))
        x = _strided((M, K), sx, torch.bfloat16, float("nan"), dev)
        x.copy_(torch.randn(M, K, generator=g, device=dev))
        w0 = torch.randn(N, K, generator=g, device=dev) if acc else None
        b0 = torch.randn(N, generator=g, device=dev) if acc and has_db else None
        dw = _strided((N, K), sw, torch.float32, float("nan"), dev)
        db = torch.full((N,), float("nan"), device=dev) if has_db else None
        probs.append([dy, x, dw, db, acc])
        priors.append((w0, b0))
    return probs, priors


def _launch(probs, priors):
    from lc2is_amd import ops
    for (_, _, dw, db, acc), (w0, b0) in zip(probs, priors):
        dw.fill_(float("nan"))
        if db is not None:
            db.fill_(float("nan"))
        if acc:
            dw.copy_(w0)
            if db is not None:
                db.copy_(b0)
    ops.gemm_tn_grouped([tuple(p) for p in probs])
    torch.cuda.synchronize()
    return [(dw.clone(), None if db is None else db.clone()) for _, _, dw, db, _ in probs]


def _check_fp64(probs, priors, outs, where):
    for j, ((dy, x, _, db, acc), (w0, b0), (dw, dbo)) in enumerate(zip(probs, priors, outs)):
        M = dy.shape[0]
        bound = 3e-6 * M ** 0.5 + 1e-6
        ref = dy.double().T @ x.double() + (w0.double() if acc else 0)
        assert _rel(dw, ref) < bound, (where, j, tuple(dy.shape), x.shape[1], acc, _rel(dw, ref))
        if db is not None:
            refb = dy.double().sum(0) + (b0.double() if acc else 0)
            assert _rel(dbo, refb) < bound, (where, j, "db", _rel(dbo, refb))


def test_grouped_weight_gradient_step_problems(dev, grouped_calls):
    """Every distinct grouped launch of the step, replayed on seeded data: dW / db vs fp64, and a second launch bit for bit."""
    assert any(len(c) > 1 for c in grouped_calls)
    for i, call in enumerate(grouped_calls):
        probs, priors = _replay(call, 100 + i, dev)
        first = _launch(probs, priors)
        _check_fp64(probs, priors, first, f"call {i}")
        second = _launch(probs, priors)
        for j, ((w1, b1), (w2, b2)) in enumerate(zip(first, second)):
            assert torch.equal(w1, w2) and (b1 is None or torch.equal(b1, b2)), f"call {i} problem {j}: relaunch differs"
        del probs, priors, first, second


def test_grouped_weight_gradient_step_problems_cu_budget(dev, grouped_calls):
    """The same launches under a 200-CU budget (another tile plan): dW / db vs fp64."""
    from lc2is_amd import ops
    prev = ops.get_cu_budget()
    try:
        ops.set_cu_budget(200)
        for i, call in enumerate(grouped_calls):
            probs, priors = _replay(call, 200 + i, dev)
            _check_fp64(probs, priors, _launch(probs, priors), f"budget 200, call {i}")
            del probs, priors
    finally:
        ops.set_cu_budget(prev)


def test_fused_head_bench_shape(dev):
    """head_upsample_ce at the step's shape (B = 32, 32x32 -> 128x128 bicubic, 151 classes, a band of ignored labels): loss,
    count and dscores_lo vs fp64 torch, and three calls give the same bits."""
    from lc2is_amd import ops
    Bh, h, C, S = 32, 32, 151, 4
    g = torch.Generator().manual_seed(32)
    lo = torch.zeros(Bh * h * h, 192)
    lo[:, :C] = torch.randn(Bh * h * h, C, generator=g) * 3
    lo = lo.to(dev)
    labels = torch.randint(0, C, (Bh, h * S, h * S), generator=g)
    labels[:, 40:56] = -100
    labels = labels.to(dev)
    runs = []
    for _ in range(3):
        loss, dlo, _ = ops.head_upsample_ce(lo, labels, Bh, h, h, C, S, ops.INTERP_BICUBIC, want_grad=True, grad_scale=1.0)
        runs.append((loss.clone(), dlo.clone()))
    for loss, dlo in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(dlo, runs[0][1])
    loss, dlo = runs[0]
    lod = lo[:, :C].double().reshape(Bh, h, h, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(lod, scale_factor=S, mode="bicubic"), labels, reduction="sum")
    ref.backward()
    assert abs(loss[0].item() - ref.item()) < 1e-4 * abs(ref.item())
    assert int(loss[1].item()) == int((labels != -100).sum().item())
    assert _rel(dlo[:, :C], lod.grad.permute(0, 2, 3, 1).reshape(Bh * h * h, C)) < 2e-5
    assert dlo[:, C:].abs().sum().item() == 0


@pytest.mark.parametrize("Bt,Lt", [(32, 16), (151, 77)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_text_embed_bwd_matches_row_ordered_sum(dev, Bt, Lt, accumulate):
    """text_embed_bwd with the bench's ids (BOS, 10 tokens, then the EOS / pad id 49407 to the end: one owner block walks most
    rows).  The kernel sums each id's rows in row order in fp32 and adds the sum to dtok; dpos sums over the batch in order.
    A row-ordered cumsum restates that exactly (np.sum would add pairwise), so the result must match bit for bit."""
    from lc2is_amd import ops
    V, C = 49408, 512
    g = torch.Generator().manual_seed(Bt + Lt + accumulate)
    ids = torch.full((Bt, Lt), 49407, dtype=torch.int64)
    ids[:, 0] = 49406
    ids[:, 1:11] = torch.randint(1, 49405, (Bt, 10), generator=g)
    dx = torch.randn(Bt * Lt, C, generator=g)
    dtok0 = torch.randn(V, C, generator=g) * 0.1
    dpos0 = torch.randn(77, C, generator=g)
    wide = torch.full((Bt * Lt, C + 64), float("nan"), device=dev)
    wide[:, :C] = dx.to(dev)
    dtok, dpos = dtok0.to(dev), dpos0.to(dev)
    ops.text_embed_bwd(ids.to(dev), wide[:, :C], dtok, dpos, accumulate=accumulate)
    flat, dxn = ids.reshape(-1).numpy(), dx.numpy()
    exp_tok = dtok0.numpy().copy()
    order = np.argsort(flat, kind="stable")                   # each id's rows, in ascending row order
    uniq, starts = np.unique(flat[order], return_index=True)
    for u, s, e in zip(uniq, starts, list(starts[1:]) + [len(flat)]):
        exp_tok[u] = exp_tok[u] + np.cumsum(dxn[order[s:e]], axis=0, dtype=np.float32)[-1]
    assert (flat == 49407).sum() > len(flat) // 4
    exp_pos = dpos0.numpy().copy()
    colsum = np.cumsum(dxn.reshape(Bt, Lt, C), axis=0, dtype=np.float32)[-1]
    exp_pos[:Lt] = exp_pos[:Lt] + colsum if accumulate else colsum
    assert torch.equal(dtok.cpu(), torch.from_numpy(exp_tok))
    assert torch.equal(dpos.cpu(), torch.from_numpy(exp_pos))


@pytest.mark.parametrize("shape,opts", [((32, 151, 128, 128), False), ((32, 151, 128, 128), True), ((1, 2, 1500, 1500), False)],
                         ids=["eval", "eval_opts", "grid_capped"])
def test_ce_nchw_fwd_sums_are_ordered(dev, shape, opts):
    """CrossEntropyLoss's forward (the evaluation loss) at the evaluation shape, and past the 8192-block grid cap: the loss and
    count sums vs fp64 torch and the same bits in three calls; the workspace-less atomic entry point within the fp64 bound."""
    from lc2is_amd import ops
    Bc, C, H, W = shape
    g = torch.Generator().manual_seed(H + C + opts)
    logits = (torch.randn(shape, generator=g) * 3).to(dev)
    labels = torch.randint(0, C, (Bc, H, W), generator=g)
    labels[:, 7:19] = -100
    labels = labels.to(dev)
    kw = dict(class_weight=(torch.rand(C, generator=g) + 0.5).to(dev), label_smoothing=0.1) if opts else {}
    runs = [ops.ce_nchw_fwd(logits, labels, **kw)[0].clone() for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    ld = logits.double()
    wd = kw["class_weight"].double() if opts else None
    ref = F.cross_entropy(ld, labels, weight=wd, reduction="sum", label_smoothing=kw.get("label_smoothing", 0.0))
    kept = labels != -100
    cnt = wd[labels[kept]].sum() if opts else kept.sum().double()
    assert abs(runs[0][0].item() - ref.item()) < 1e-5 * abs(ref.item())
    assert abs(runs[0][1].item() - cnt.item()) < 1e-6 * cnt.item()
    legacy = torch.zeros(2, device=dev)
    lse = torch.empty((Bc, H, W), device=dev)
    if opts:
        rc = ops._fn("lc2is_ce_nchw_fwd_opts")(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), legacy.data_ptr(), None, Bc, C,
                                              H * W, -100, kw["class_weight"].data_ptr(), 0.1, ops._stream())
    else:
        rc = ops._fn("lc2is_ce_nchw_fwd")(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), legacy.data_ptr(), Bc, C, H * W,
                                         -100, ops._stream())
    assert rc == 0
    # one float atomic per wave into the same two words: a few ulps of 4e6 off, and different bits from run to run
    assert abs(legacy[0].item() - ref.item()) < 1e-5 * abs(ref.item())
    assert abs(legacy[1].item() - cnt.item()) < 1e-5 * cnt.item()
