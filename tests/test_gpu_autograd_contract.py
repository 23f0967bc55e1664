"""The autograd contract of the drop-in modules: which gradients exist, where they go and whether they add up, under partial
freezing, repeated ``backward()`` and every combination of input flags — against the fp64 oracle under torch autograd
(tests/autograd_cases.py) for WHICH gradients exist, and against the module's own all-trainable baseline for their values.

(a) baseline: everything trainable, one backward; every gradient vs the oracle at the bound the module's own parity test states
    (quoted per case in autograd_cases.Bounds.src).  (b)-(f) and (h) are differential: a gradient under a pattern vs the same
    gradient of the baseline run.  Freezing or a mixed state may change how weight gradients are grouped into launches and with
    that the fp32 summation order, so the bound is the one the project asserts for "same weight gradient, different plan":
    relative L2 < 1e-5 (tests/test_gpu_gemm_ln.py:730-731 `assert _rel_l2(c1, ref) < 1e-5 and ... < 1e-5`), per tensor.

Worst differential figures measured on an MI355X (printed when the module finishes; 0 = bitwise equal to the baseline):
    vision tower  patterns 0         accumulation 2.3e-8      text tower    patterns 3.4e-8   accumulation 3.7e-8
    decoder       patterns 0         accumulation 2.4e-8      hierarchical  patterns 0        accumulation 3.7e-8
    FTN           patterns 1.1e-8    accumulation 2.1e-8      Swin          patterns 1.7e-6   accumulation 3.8e-7
    whole model   patterns 3.0e-9    accumulation 3.7e-8      train step (h) 3.0e-9
    (Swin's 1.7e-6 is a key bias: a mathematically zero gradient whose value is the round-off of the summed dK rows, summed by
    the separate column-sum launch instead of the weight-gradient launch once its weight is frozen.)
"""
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import autograd_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu
DIFF = 1e-5
_CTX = {}
WORST = {}      # (family, check) -> worst measured differential figure of this run (printed when the module finishes)


class Ctx:
    """One case on the device: the module, its oracle, both inputs, and the all-trainable baseline gradients of A and B."""

    def __init__(self, cid, dev):
        self.case = c = AC.case(cid)
        self.dev = dev
        m = c.build()
        self.oracle = AC.Oracle(c, m)
        self.m = m.to(dev).train()
        self.named = dict(self.m.named_parameters())
        self.names = list(self.named)
        self.inp = {}
        for w, i in self.oracle.inputs.items():
            self.inp[w] = AC.Inputs({k: v.to(dev) for k, v in i.floats.items()},
                                    {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in i.other.items()},
                                    [d.to(dev) for d in i.douts])
        self.relu = None      # the relu patterns of the baseline forward on A, per decoder layer (cases tagged fed_relu)
        if c.tags.get("fed_relu"):
            from test_gpu_parity3 import _CaptureRelu
            with _CaptureRelu() as cap:
                self.base = {"A": self._baseline("A")}
            B, Sq = self.inp["A"].floats["tgt"].shape[:2]
            self.relu = [{"relu_mask": (a > 0).double().cpu().view(B, Sq, -1)} for a in cap.acts]
            self.base["B"] = self._baseline("B")
        else:
            self.base = {w: self._baseline(w) for w in ("A", "B")}

    def run(self, which="A", trainable=None, flags=None, clear=True, backward=True):
        """forward (+ backward from the seeded output gradients) with requires_grad set as the pattern says.  Returns (outputs,
        the float-input leaves)."""
        trainable = set(self.names) if trainable is None else trainable
        for n, p in self.named.items():
            p.requires_grad_(n in trainable)
            if clear:
                p.grad = None
        inp = self.inp[which]
        flags = {k: True for k in inp.floats} if flags is None else flags
        fl = {k: v.detach().clone().requires_grad_(bool(flags.get(k, False))) for k, v in inp.floats.items()}
        outs = self.case.call(self.m, fl, inp.other)
        live = [(o, d) for o, d in zip(outs, inp.douts) if o.requires_grad]
        if backward and live:
            torch.autograd.backward([o for o, _ in live], [d for _, d in live])
        return outs, fl

    def grads(self):
        return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in self.named.items()}

    def _baseline(self, which):
        outs, fl = self.run(which)
        return dict(outs=[o.detach().clone() for o in outs], g=self.grads(), gi={k: v.grad for k, v in fl.items()})

    def restore(self):
        for p in self.named.values():
            p.requires_grad_(True)
            p.grad = None
            if hasattr(p, "_lc2is_grad"):
                del p._lc2is_grad


def ctx(cid, dev) -> Ctx:
    if cid not in _CTX:
        _CTX[cid] = Ctx(cid, dev)
    return _CTX[cid]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _diff_figures(pairs):
    """[(label, got, want)] -> [(label, ||got - want|| / ||want||)] with one device read."""
    if not pairs:
        return []
    vals = torch.stack([(g.double() - w.double()).norm() / w.double().norm().clamp_min(1e-30) for _, g, w in pairs]).cpu().tolist()
    return [(label, v) for (label, _, _), v in zip(pairs, vals)]


def _assert_diff(c, kind, check, pairs):
    figs = _diff_figures(pairs)
    if figs:
        key = (c.case.family, kind)
        worst = max(figs, key=lambda t: t[1])
        if worst[1] > WORST.get(key, ("", -1.0))[1]:
            WORST[key] = worst
    bad = [(lbl, v) for lbl, v in figs if not v < DIFF]
    assert not bad, f"{c.case.id} ({check}): differs from the all-trainable baseline by more than {DIFF}: {bad[:6]}"


def _check_pattern(c: Ctx, kind, check, trainable, which="A", nan_fill=False):
    """One freezing pattern: frozen parameters have no .grad, the set of parameters with one is the oracle's, every gradient
    agrees with the baseline's."""
    if nan_fill:      # the buffers base.grad_buf would reuse: poisoned, so one that is installed and never written shows
        for p in c.named.values():
            p.grad = None
            p._lc2is_grad = torch.full_like(p, float("nan"))
    outs, fl = c.run(which, trainable)
    got = {n for n, p in c.named.items() if p.grad is not None}
    frozen_with_grad = sorted(got - set(trainable))
    assert not frozen_with_grad, f"{c.case.id} ({check}): frozen parameters were given a .grad: {frozen_with_grad[:6]}"
    want = c.oracle.grad_set(trainable)
    assert got == want, (f"{c.case.id} ({check}): gradients missing {sorted(want - got)[:6]}, unexpected {sorted(got - want)[:6]} "
                         f"against the fp64 oracle under torch autograd")
    base = c.base[which]
    if nan_fill:
        fin = torch.stack([torch.isfinite(c.named[n].grad).all() for n in sorted(got)]).cpu().tolist() if got else []
        bad = [n for n, ok in zip(sorted(got), fin) if not ok]
        assert not bad, f"{c.case.id} ({check}): non-finite values (an unwritten gradient buffer) in {bad[:6]}"
    _assert_diff(c, kind, check, [(n, c.named[n].grad, base["g"][n]) for n in sorted(got)])
    for k, t in fl.items():       # the inputs all require grad here: their gradients are still produced, and unchanged
        assert (t.grad is None) == (base["gi"][k] is None), (c.case.id, check, k)
    _assert_diff(c, kind + ", inputs", check, [(k, t.grad, base["gi"][k]) for k, t in fl.items() if t.grad is not None])
    return outs


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_baseline_vs_fp64_oracle(dev, cid):
    """(a) everything trainable, one backward from a seeded output gradient: outputs, every parameter gradient and every input
    gradient against the fp64 oracle, which gradients are None included.

    The decoder cases: relu is discontinuous, and a pre-activation within bf16 rounding distance of 0 fires in one of the two runs
    only (about 0.25 % of the units; tests/test_gpu_parity3.py measured this as the whole of the decoder's gradient error).  At the
    2 x 5 tokens x 128 units of these cases that is a Poisson(~3) number of flips per layer and the error it leaves on
    `linear1.weight` and on every parameter behind the feed-forward block in backward order has no bound the number formats
    imply.  With the oracle deciding its own pattern the worst parameter gradient per case measured, on input A: pre_kv64_bias
    4.3e-2, pre_kv64_nobias 4.0e-2, post_kv64_bias 9.4e-2 (layers.0.multihead_attn.k_proj_weight), post_kv64_nobias 1.24e-1
    (layers.1.linear1.weight), pre_kv128_bias 5.3e-2, pre_kv128_nobias 8.8e-2 (layers.1.norm3.weight), pre_kv64_bias_norm 5.7e-2;
    on input B pre_kv64_bias measured 9.5e-2 (layers.0.linear1.weight) — three of seven past the stated 8e-2.  The four cases
    inside it are compared with the oracle as it is.  For the other three (autograd_cases.FED_RELU) the GRADIENTS are compared
    with the oracle fed the pattern the HIP forward used (``relu_mask`` of oracle/ref_cpu.py decoder_layer, the measurement of
    test_gpu_parity3.py), at the stated bounds: what is left is the arithmetic, and the own-pattern figure is printed.  For those
    three the gradient reference is therefore NOT independent of the device forward: a relu mask that the device forward gets
    wrong would not show in their gradients here (it would in tests/test_gpu_modules.py at its d96 shape, and in the four cases
    above).  The forward OUTPUT of all seven is compared with the oracle's own pattern, and WHICH gradients exist, in every other
    test of this file, is decided by the oracle with its own pattern."""
    c = ctx(cid, dev)
    b = c.case.bounds
    for which in ("A",):      # one backward, as stated; input B only serves (e), whose expected values are formed on the device
        outs, pg, ig = c.oracle.run(which=which)
        if c.relu:
            own = pg
            _, pg, ig = c.oracle.run(which=which, extra=dict(drops=c.relu))
            figs = {n: _rel(c.base[which]["g"][n], r) for n, r in own.items() if r is not None and float(r.abs().sum()) > 0}
            n_worst = max(figs, key=figs.get)
            print(f"own relu pattern: {cid}: worst parameter-gradient rel-L2 {figs[n_worst]:.3e} ({n_worst})")
        base = c.base[which]
        for i, (o, r) in enumerate(zip(base["outs"], outs)):
            if c.case.tags.get("scalar_loss"):
                assert abs(o.item() - r.item()) < b.out, (cid, which, o.item(), r.item())
            else:
                assert o.shape == r.shape and _rel(o, r) < b.out, (cid, which, i, _rel(o, r))
        for n in c.names:
            g, r = base["g"][n], pg[n]
            assert (g is None) == (r is None), f"{cid} {which}: {n} has {'no ' if g is None else 'a '}gradient, the oracle the opposite"
            if r is None:
                continue
            if float(r.abs().sum()) < 1e-6 * r.numel():
                b.zero_ref(n, g.cpu(), pg)
                continue
            assert _rel(g, r) < b.param, (cid, which, n, _rel(g, r))
        for k, r in ig.items():
            g = base["gi"][k]
            assert (g is None) == (r is None), (cid, which, k)
            if r is not None:
                assert _rel(g, r) < b.inputs[k], (cid, which, k, _rel(g, r))


# ---- (b), (c) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_leave_one_frozen(dev, cid):
    """(b) once per parameter p: p frozen, everything else trainable."""
    c = ctx(cid, dev)
    try:
        for k in range(len(c.names)):
            _check_pattern(c, "leave-one-frozen", c.names[k], AC.pattern_leave_one(c.names, k))
            assert c.named[c.names[k]].grad is None
    finally:
        c.restore()


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_only_one_trainable(dev, cid):
    """(c) once per parameter p: only p trainable (the pattern that a save decision anchored on ONE parameter fails)."""
    c = ctx(cid, dev)
    try:
        for k in range(len(c.names)):
            _check_pattern(c, "only-one-trainable", c.names[k], AC.pattern_only_one(c.names, k))
    finally:
        c.restore()


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen_parity", [0, 1], ids=["even_frozen", "odd_frozen"])
@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_complementary_halves(dev, cid, frozen_parity):
    """(d) the parameters at even (odd) positions of named_parameters() frozen: weight and bias of one Linear or LayerNorm in
    opposite states; every reusable gradient buffer is NaN beforehand."""
    c = ctx(cid, dev)
    try:
        trainable = AC.pattern_half(c.names, frozen_parity)
        _check_pattern(c, "halves", f"parity {frozen_parity} frozen", trainable, nan_fill=True)
        lit = {n for n, g in c.oracle.run(trainable)[1].items() if g is not None}     # the oracle with the flags set, literally
        assert {n for n, p in c.named.items() if p.grad is not None} == lit
    finally:
        c.restore()


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["kept", "even_none", "zero_filled"])
@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_accumulation(dev, cid, variant):
    """(e) backward on A, then on B, without clearing.  Expected per parameter, formed in fp64 from the separately computed device
    gradients: g_A + g_B (all kept), g_B where the grad was set to None in between (g_A + g_B elsewhere), g_B after an in-place
    zero fill.  Residual norm against ||g_A|| + ||g_B||."""
    c = ctx(cid, dev)
    gA, gB = c.base["A"]["g"], c.base["B"]["g"]
    try:
        c.run("A")
        dropped = set()
        if variant == "even_none":
            dropped = set(c.names[0::2])
            for n in dropped:
                c.named[n].grad = None
        elif variant == "zero_filled":
            for p in c.named.values():
                if p.grad is not None:
                    p.grad.zero_()
        c.run("B", clear=False)
        pairs = []
        for n in c.names:
            g = c.named[n].grad
            assert (g is None) == (gB[n] is None), (cid, variant, n)
            if g is None:
                continue
            only_b = variant == "zero_filled" or n in dropped
            want = gB[n].double() if only_b else gA[n].double() + gB[n].double()
            pairs.append((n, (g.double() - want).norm() / (gA[n].double().norm() + gB[n].double().norm()).clamp_min(1e-30)))
        figs = torch.stack([v for _, v in pairs]).cpu().tolist()
        key = (c.case.family, "accumulation")
        worst = max(zip([n for n, _ in pairs], figs), key=lambda t: t[1])
        if worst[1] > WORST.get(key, ("", -1.0))[1]:
            WORST[key] = worst
        bad = [(n, v) for (n, _), v in zip(pairs, figs) if not v < DIFF]
        assert not bad, f"{cid} ({variant}): accumulated gradients off by more than {DIFF} of ||g_A|| + ||g_B||: {bad[:6]}"
    finally:
        c.restore()


# ---- (f) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [i for i in AC.CASE_IDS if i.startswith(("decoder", "hier", "block", "ftn"))])
def test_input_flags(dev, cid):
    """(f) every combination of the float inputs' requires_grad, with all parameters trainable and with all frozen."""
    c = ctx(cid, dev)
    base = c.base["A"]
    try:
        for frozen in (False, True):
            trainable = set() if frozen else set(c.names)
            for flags in AC.input_flag_sets(c.inp["A"].floats):
                tag = f"flags {flags} {'frozen' if frozen else 'trainable'}"
                outs, fl = c.run("A", trainable, flags)
                _, opg, oig = c.oracle.run(trainable, flags)
                for k, t in fl.items():
                    assert (t.grad is None) == (oig[k] is None), f"{cid} ({tag}): input {k} gradient " \
                        f"{'missing' if t.grad is None else 'unexpected'} against the fp64 oracle"
                _assert_diff(c, "input flags, inputs", tag, [(k, t.grad, base["gi"][k]) for k, t in fl.items() if t.grad is not None])
                got = {n for n, p in c.named.items() if p.grad is not None}
                assert got == {n for n, g in opg.items() if g is not None}, (cid, tag)
                _assert_diff(c, "input flags", tag, [(n, c.named[n].grad, base["g"][n]) for n in sorted(got)])
                if frozen and not any(flags.values()):
                    assert not any(o.requires_grad for o in outs), f"{cid}: output requires grad with nothing to differentiate"
    finally:
        c.restore()


# ---- (g) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_saving_forward_is_the_forward(dev, cid):
    """(g) the output under torch.no_grad(), in eval mode with grad enabled, and of the saving (training) forward are torch.equal:
    saving only adds stores (LayerNorm statistics, the attention log-sum-exp, the pre-activation of the MLP) to the same launches."""
    c = ctx(cid, dev)
    try:
        saving = [o.detach() for o in c.run("A", backward=False)[0]]
        with torch.no_grad():
            plain = c.run("A", backward=False)[0]
        c.m.eval()
        evald = [o.detach() for o in c.run("A", backward=False)[0]]
        for s, p, e in zip(saving, plain, evald):
            assert torch.equal(s, p) and torch.equal(s, e), (cid, _rel(p, s), _rel(e, s))
    finally:
        c.m.train()
        c.restore()


# ---- (h) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen_parity", [0, 1], ids=["even_frozen", "odd_frozen"])
def test_train_step_under_half_freeze(dev, frozen_parity):
    """(h) TrainStep on the tiny model, SGD with weight decay, one step, even (odd) positions frozen: frozen parameters are bitwise
    unchanged, live parameters move as in the all-trainable step.  lr = 1 and weight decay 0.1 keep an update (>= ~0.1 |p|) far
    above the fp32 spacing of the weight it is read back from (2^-24 |p|: a floor of ~1e-6 relative, below the 1e-5 bound)."""
    from lc2is_amd.step import TrainStep
    c = AC.case("base_model")
    inp = c.make_inputs("A").other
    inputs = {k: inp[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = inp["labels"].to(dev)

    def one_step(frozen):
        m = c.build().to(dev).train()
        for n, p in m.named_parameters():
            p.requires_grad_(n not in frozen)
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        TrainStep(m, optimizer="sgd", lr=1.0, weight_decay=0.1).step(inputs, labels)
        torch.cuda.synchronize()
        return before, {n: p.detach().clone() for n, p in m.named_parameters()}

    names = AC.param_names(c.build())
    frozen = set(names) - AC.pattern_half(names, frozen_parity)
    b0, a0 = one_step(set())
    b1, a1 = one_step(frozen)
    changed = [n for n in sorted(frozen) if not torch.equal(a1[n], b1[n])]
    assert not changed, f"frozen parameters moved under weight decay: {changed[:6]}"
    pairs = []
    for n in names:
        if n in frozen:
            continue
        if torch.equal(a0[n], b0[n]):          # no gradient in the all-trainable step either (the unreached post_layernorm)
            assert torch.equal(a1[n], b1[n]), n
            continue
        pairs.append((n, a1[n] - b1[n], a0[n] - b0[n]))
    assert len(pairs) > 20
    figs = _diff_figures(pairs)
    WORST[("whole model", f"train step {frozen_parity}")] = max(figs, key=lambda t: t[1])
    bad = [(n, v) for n, v in figs if not v < DIFF]
    assert not bad, f"live parameters' updates differ from the all-trainable step's by more than {DIFF}: {bad[:6]}"


def test_contrastive_head_trains_under_frozen_towers(dev):
    """ContrastiveModel's head (TextToPatch behind its own Function): with both towers frozen the two Linears still get their
    gradients, equal to those of the all-trainable run; with everything frozen the output does not require grad."""
    import lc2is_amd.nn as N
    torch.manual_seed(21)
    m = N.ContrastiveModel(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                           text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), out_dim=64)
    m = AC.seed_weights(m, 22).to(dev).train()
    g = torch.Generator().manual_seed(23)
    ids = torch.randint(1, 500, (4, 6), generator=g)
    ids[:, -1] = 511
    inputs = dict(pixel_values=torch.randn(2, 3, 64, 64, generator=g).to(dev), input_ids=ids.to(dev))
    dout = (torch.randn(2, 256, 4, generator=g) * 0.1).to(dev)
    head = [n for n, _ in m.named_parameters() if n.startswith("pixel_patch.")]
    m(inputs)[2].backward(dout)
    base = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert set(head) <= set(base)
    for n, p in m.named_parameters():
        p.grad = None
        p.requires_grad_(n in head)
    m(inputs)[2].backward(dout)
    got = {n for n, p in m.named_parameters() if p.grad is not None}
    assert got == set(head), (sorted(set(head) - got), sorted(got - set(head)))
    bad = [(n, v) for n, v in _diff_figures([(n, dict(m.named_parameters())[n].grad, base[n]) for n in head]) if not v < DIFF]
    assert not bad, bad
    for p in m.parameters():
        p.grad = None
        p.requires_grad_(False)
    assert not m(inputs)[2].requires_grad


@pytest.fixture(scope="module", autouse=True)
def _report_worst_differential_figures():
    """After the module's last test: the worst measured differential figure per family and check (pytest -s shows it)."""
    yield
    for (family, check), (label, v) in sorted(WORST.items()):
        print(f"worst differential figure: {family:14s} {check:26s} {v:.3e}  ({label})")
