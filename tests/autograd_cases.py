"""The case table of the autograd-contract tests and its fp64 side (no GPU needed to import).

Every drop-in module of ``lc2is_amd.nn`` has a hand-written backward that is orchestrated on the host: per parameter it decides
whether a gradient is computed, into which buffer it goes and whether the kernel overwrites or accumulates.  A case of this
table names a module family at the smallest architecture that still runs every kernel of its backward, makes two seeded,
independent inputs A and B, and restates the module through ``oracle/ref_cpu.py``.  The reference side is that oracle function
evaluated in fp64 on the CPU under torch autograd: the module's parameters are cast to double, ``requires_grad`` of every
parameter and float input is set exactly as on the device module, and torch decides which gradients exist.

tests/test_gpu_autograd_contract.py runs the device side; tests/test_autograd_cases_cpu.py keeps the table complete and shows
that the reference side can fail.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
if str(HERE.parent) not in sys.path:
    sys.path.insert(0, str(HERE.parent))
G = HERE / "golden"


@dataclass
class Inputs:
    """One input of a case.  ``floats``: the differentiable inputs by name (CPU fp32); ``other``: everything else the call
    takes (ids, masks, pixels — a vision tower returns no pixel gradient); ``douts``: one seeded output gradient per output."""
    floats: dict
    other: dict
    douts: list


@dataclass
class Bounds:
    """Relative-L2 bounds of the baseline (a), each taken from the existing parity test of the same module (``src`` quotes it)."""
    out: float
    param: float
    inputs: dict
    src: str
    zero_ref: Callable | None = None     # (name, device grad, oracle grads) -> None, asserts: rule for mathematically zero gradients


@dataclass
class Case:
    id: str
    family: str
    classes: tuple                       # the lc2is_amd.nn classes this case runs the backward of
    build: Callable                      # () -> module on the CPU, seeded weights
    make_inputs: Callable                # (which: "A" | "B") -> Inputs
    call: Callable                       # (module, floats, other) -> list of output tensors (device side)
    oracle: Callable                     # (sd, floats, other) -> list of output tensors (any dtype: the tensors decide)
    bounds: Bounds
    tags: dict = field(default_factory=dict)


# ---- weights and patterns -----------------------------------------------------------------------------------------------
def seed_weights(m, seed: int):
    """golden_util.make_weights under the module's parameter names: norm weights 1 + 0.1 n, biases 0.05 n, the rest n / sqrt(fan_in)
    — no bias is zero and no LayerNorm is the identity, so a gradient that is dropped or doubled shows."""
    from golden_util import make_weights
    named = dict(m.named_parameters())
    w = make_weights({k: list(v.shape) for k, v in named.items()}, seed)
    with torch.no_grad():
        for k, p in named.items():
            p.copy_(w[k])
    return m


def param_names(m) -> list:
    return [k for k, _ in m.named_parameters()]


def pattern_leave_one(names, k):          # (b)
    return set(names) - {names[k]}


def pattern_only_one(names, k):           # (c)
    return {names[k]}


def pattern_half(names, frozen_parity):   # (d): the parameters at positions of `frozen_parity` (0 even, 1 odd) are frozen
    return {n for i, n in enumerate(names) if i % 2 != frozen_parity}


def input_flag_sets(float_names):         # (f): every combination of the inputs' requires_grad
    names = list(float_names)
    for bits in range(1 << len(names)):
        yield {n: bool(bits >> i & 1) for i, n in enumerate(names)}


# ---- the fp64 side --------------------------------------------------------------------------------------------------------
class Oracle:
    """The oracle function of a case in fp64 under torch autograd, on the parameters of one built module."""

    def __init__(self, case: Case, module):
        self.case = case
        self.params = {k: v.detach().cpu().double().clone() for k, v in module.named_parameters()}
        self.inputs = {w: case.make_inputs(w) for w in ("A", "B")}
        self._reach = None

    def _leaves(self, trainable, flags, which):
        inp = self.inputs[which]
        sd = {k: v.clone().requires_grad_(k in trainable) for k, v in self.params.items()}
        fl = {k: v.double().clone().requires_grad_(bool(flags.get(k, False))) for k, v in inp.floats.items()}
        return sd, fl, inp

    @staticmethod
    def _backward(outs, douts):
        live = [(o, d.to(o.dtype)) for o, d in zip(outs, douts) if o.requires_grad]
        if live:
            torch.autograd.backward([o for o, _ in live], [d for _, d in live])

    def run(self, trainable=None, flags=None, which="A", extra=None):
        """One forward + backward with ``requires_grad`` set as the pattern says (None: everything trainable / required).
        ``extra``: further non-differentiable arguments of the oracle function (its diagnostic inputs).
        Returns (outputs, {parameter: grad or None}, {float input: grad or None})."""
        trainable = set(self.params) if trainable is None else set(trainable)
        flags = {k: True for k in self.inputs[which].floats} if flags is None else flags
        sd, fl, inp = self._leaves(trainable, flags, which)
        outs = self.case.oracle(sd, fl, {**inp.other, **(extra or {})})
        self._backward(outs, inp.douts)
        return [o.detach() for o in outs], {k: v.grad for k, v in sd.items()}, {k: v.grad for k, v in fl.items()}

    def run_accumulate(self, trainable=None, between: Callable | None = None):
        """backward on A, then on B, on the SAME leaves without clearing; ``between(sd)`` may edit the .grad fields in between."""
        trainable = set(self.params) if trainable is None else set(trainable)
        sd, fl, inp = self._leaves(trainable, {}, "A")
        self._backward(self.case.oracle(sd, fl, inp.other), inp.douts)
        if between is not None:
            between(sd)
        inp = self.inputs["B"]
        fl = {k: v.double().clone() for k, v in inp.floats.items()}
        self._backward(self.case.oracle(sd, fl, inp.other), inp.douts)
        return {k: v.grad for k, v in sd.items()}

    def reachable(self) -> set:
        """The parameters torch gives a gradient when everything is trainable: the leaves the outputs' graph reaches."""
        if self._reach is None:
            self._reach = {k for k, g in self.run()[1].items() if g is not None}
        return self._reach

    def grad_set(self, trainable) -> set:
        """The parameters that get a gradient under a freezing pattern.  Whether a leaf gets one is a property of torch's graph
        alone — it requires grad and the outputs' graph reaches it — and freezing OTHER leaves removes no path to it, so the set is
        reachable() & trainable without another fp64 pass; tests/test_autograd_cases_cpu.py checks this against run() with the
        flags set, pattern by pattern."""
        return self.reachable() & set(trainable)


# ---- families -------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _zero_rule_mean(name, g, ref):
    """tests/test_gpu_modules.py:85-88 (the same rule at test_gpu_hier.py:62-63, test_gpu_ftn.py:101-102): a gradient the
    reference has exactly zero (softmax shift invariance: key biases) is bf16 rounding noise — negligible per element."""
    assert float(g.abs().mean()) < 1e-3, name


MODULES_SRC = ("tests/test_gpu_modules.py:5-6 'relative L2 error of logits <= 2e-2, of any parameter gradient <= 8e-2'; "
               "zero gradients: :85-88")


def _vision_case(full: bool) -> Case:
    import lc2is_amd.nn as N
    from oracle import ref_cpu as O
    cls = N.ImageEncoderCLIPFull if full else N.ImageEncoderCLIP
    cfg = O.ClipCfg(128, 2, 2, patch=16)
    fn = O.image_encoder_clip_full if full else O.image_encoder_clip

    def make_inputs(which):
        g = _gen(101 if which == "A" else 202)
        pix = torch.randn(2, 3, 32, 32, generator=g)
        return Inputs({}, dict(pixel_values=pix), [torch.randn(2, 5 if full else 4, 128, generator=g) * 0.1])

    return Case(id="vision_full" if full else "vision", family="vision tower", classes=(cls.__name__,),
                build=lambda: seed_weights(cls(32, 16, arch=N.ClipArch(128, 2, 2, 256)), 11),
                make_inputs=make_inputs, call=lambda m, fl, other: [m(other["pixel_values"])],
                oracle=lambda sd, fl, other: [fn(sd, "", other["pixel_values"].to(next(iter(sd.values())).dtype), cfg)],
                bounds=Bounds(2e-2, 8e-2, {}, MODULES_SRC, _zero_rule_mean))


def _text_case(pooler: bool) -> Case:
    import lc2is_amd.nn as N
    from oracle import ref_cpu as O
    cls = N.TextEncoderCLIPPooler if pooler else N.TextEncoderCLIP
    cfg = O.ClipCfg(64, 1, 2, eos_token_id=511)
    fn = O.text_encoder_clip_pooler if pooler else O.text_encoder_clip

    def make_inputs(which):
        g = _gen(303 if which == "A" else 404)
        B, L = 3, 7
        ids = torch.full((B, L), 511, dtype=torch.int64)          # EOS padding, mask 0 on it (the reference's tokenizer layout)
        mask = torch.zeros(B, L, dtype=torch.int64)
        for b, n in enumerate((3, 5, 2)):
            ids[b, 0] = 510
            ids[b, 1:1 + n] = torch.randint(1, 500, (n,), generator=g)
            mask[b, :n + 2] = 1
        ids[1, 2] = ids[0, 1]                                      # one id repeated: two rows add into one row of the token table
        dout = torch.randn(*((B, 64) if pooler else (B, L, 64)), generator=g) * 0.1
        return Inputs({}, dict(input_ids=ids, attention_mask=mask), [dout])

    return Case(id="text_pooler" if pooler else "text", family="text tower", classes=(cls.__name__,),
                build=lambda: seed_weights(cls(16, arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511)), 12),
                make_inputs=make_inputs, call=lambda m, fl, other: [m(other["input_ids"], other["attention_mask"])],
                oracle=lambda sd, fl, other: [fn(sd, "", other["input_ids"], other["attention_mask"], cfg)],
                bounds=Bounds(2e-2, 8e-2, {}, MODULES_SRC, _zero_rule_mean))


# The decoder cases whose baseline GRADIENTS are compared with the oracle fed the HIP forward's relu pattern: with its own pattern
# they measured 9.4e-2, 1.24e-1 and 8.8e-2 against the stated 8e-2 (tests/test_gpu_autograd_contract.py test_baseline_vs_fp64_oracle
# says why); the other four decoder cases are compared with the oracle as it is.
FED_RELU = ("decoder_post_kv64_bias", "decoder_post_kv64_nobias", "decoder_pre_kv128_nobias")


def _decoder_case(norm_first: bool, d_kv: int, bias: bool, final_norm: bool = False) -> Case:
    import lc2is_amd.nn as N
    from oracle import ref_cpu as O

    def build():
        layer = N.DecoderLayer(128, d_kv, 2, dim_feedforward=128, dropout=0, batch_first=True, norm_first=norm_first, bias=bias)
        return seed_weights(N.DecoderBlock(layer, 2, norm=torch.nn.LayerNorm(128) if final_norm else None), 13)

    def make_inputs(which):
        g = _gen(505 if which == "A" else 606)
        tgt, mem = torch.randn(2, 5, 128, generator=g), torch.randn(2, 9, d_kv, generator=g)
        kpm = torch.zeros(2, 9, dtype=torch.bool)
        kpm[0, 6:] = True
        kpm[1, 8:] = True
        return Inputs(dict(tgt=tgt, memory=mem), dict(kpm=kpm), [torch.randn(2, 5, 128, generator=g) * 0.1])

    def oracle(sd, fl, other):
        x = O.decoder_block(sd, "", fl["tgt"], fl["memory"], 2, 2, norm_first, other["kpm"], drops=other.get("drops"))
        if final_norm:
            x = O.layer_norm(x, sd["norm.weight"], sd["norm.bias"])
        return [x]

    cid = f"decoder_{'pre' if norm_first else 'post'}_kv{d_kv}_{'bias' if bias else 'nobias'}{'_norm' if final_norm else ''}"
    return Case(id=cid, family="decoder", classes=("DecoderBlock", "DecoderLayer"), build=build, make_inputs=make_inputs,
                call=lambda m, fl, other: [m(tgt=fl["tgt"], memory=fl["memory"], memory_key_padding_mask=other["kpm"])],
                oracle=oracle,
                bounds=Bounds(1e-2, 8e-2, dict(tgt=3e-2, memory=3e-2),
                              "tests/test_gpu_modules.py:129 'assert r < 1e-2', :132 'dtgt ... < 3e-2 and ... dmem ... < 3e-2', "
                              ":137 'assert r < 8e-2, (k, r)'", _zero_rule_mean), tags=dict(fed_relu=cid in FED_RELU))


def _hier_inputs(which, in_dims, dim, text: bool, B=2, K=10):
    g = _gen(707 if which == "A" else 808)
    vis = [torch.randn(B, p, c, generator=g) for p, c in zip((256, 64, 16, 4), in_dims)]
    fl = dict(v0=vis[0], v3=vis[3])
    if text:
        fl["textual"] = torch.randn(B, K, dim, generator=g)
    return Inputs(fl, dict(v1=vis[1], v2=vis[2]), [torch.randn(B, 256, dim, generator=g) * 0.1])


def _hier_call(text):
    def call(m, fl, other):
        vis = [fl["v0"], other["v1"], other["v2"], fl["v3"]]
        return [m(vis, fl["textual"]) if text else m(vis)]
    return call


def _hier_oracle(text, nhead, depth, layer_key):
    from oracle import ref_cpu as O

    def oracle(sd, fl, other):
        dt = fl["v0"].dtype
        vis = [fl["v0"], other["v1"].to(dt), other["v2"].to(dt), fl["v3"]]
        return [O.hierarchical(sd, "", vis, fl["textual"] if text else None, nhead=nhead, depth=depth, layer_key=layer_key)]
    return oracle


HIER_SRC = ("tests/test_gpu_hier.py:46 'assert r < 1.5e-2', :48 'dvisual0 ... < 3e-2', :49 'dvisual3 ... < 5e-2', "
            ":52 'dtextual ... < 5e-2', :57 'assert worst < 8e-2'; zero gradients :62-63")


def _hier_case(cross: bool) -> Case:
    import lc2is_amd.nn as N
    in_dims, dim = [64, 128, 192, 256], 128
    depth = [2, 1, 1] if cross else [1, 1, 2]
    cls = N.HierarchicalCrossA if cross else N.HierarchicalSelfA
    return Case(id="hier_cross" if cross else "hier_self", family="hierarchical", classes=(cls.__name__,),
                build=lambda: seed_weights(cls(in_dims, depth, dim, nhead=2, dropout=0, batch_first=True), 14),
                make_inputs=lambda which: _hier_inputs(which, in_dims, dim, cross), call=_hier_call(cross),
                oracle=_hier_oracle(cross, 2, tuple(depth), "layers.0."),
                bounds=Bounds(1.5e-2, 8e-2, dict(v0=3e-2, v3=5e-2, textual=5e-2), HIER_SRC, _zero_rule_mean))


def _block_case(kind: str) -> Case:
    """An SR block on its own (CrossABlock / SelfABlock / FTNBlock.forward -> _SRBlock._apply_block -> _BlockFn): the pyramids
    drive their blocks' _fwd / _bwd directly, so this path and its save decision are reached only here.  The block of
    tests/test_gpu_hier.py:96-101 (d_model 128, 2 heads, the shared layer applied twice; 5 memory rows)."""
    import lc2is_amd.nn as N
    from oracle import ref_cpu as O
    text = kind != "self"
    depth = 1 if kind == "ftn" else 2
    key = "attention_block." if kind == "ftn" else "layers.0."

    def build():
        if kind == "cross":
            m = N.CrossABlock(N.SRTransformerCrossA(d_model=128, nhead=2, sr_ratio=2, dropout=0, batch_first=True), depth=2)
        elif kind == "self":
            m = N.SelfABlock(N.SRTransformerSelfA(d_model=128, nhead=2, sr_ratio=2, dropout=0, batch_first=True), depth=2)
        else:
            m = N.FTNBlock(N.SRTransformerDecoder(d_model=128, nhead=2, sr_ratio=2, dropout=0, batch_first=True))
        return seed_weights(m, 9)

    def make_inputs(which):
        g = _gen(1414 if which == "A" else 1515)
        fl = dict(x=torch.randn(2, 64, 128, generator=g))
        if text:
            fl["memory"] = torch.randn(2, 5, 128, generator=g)
        return Inputs(fl, {}, [torch.randn(2, 256, 128, generator=g) * 0.1])

    return Case(id=f"block_{kind}", family="hierarchical", classes=(dict(cross="CrossABlock", self="SelfABlock", ftn="FTNBlock")[kind],),
                build=build, make_inputs=make_inputs,
                call=lambda m, fl, other: [m(fl["x"], fl["memory"]) if text else m(fl["x"])],
                oracle=lambda sd, fl, other: [O.attn_block(sd, "", fl["x"], fl.get("memory"), nhead=2, depth=depth, layer_key=key)],
                bounds=Bounds(1.5e-2, 8e-2, dict(x=5e-2, memory=5e-2),
                              "tests/test_gpu_hier.py:105 '_rel(outb, refb) < 1.5e-2' (the block alone); its gradients at the bounds "
                              "the same layers meet inside the pyramid, :49 'dvisual3 ... < 5e-2', :52 'dtextual ... < 5e-2', :57 "
                              "'assert worst < 8e-2'; zero gradients :62-63", _zero_rule_mean))


def _ftn_decoder_case() -> Case:
    """FTNDecoder hard-codes 8 heads, hence dim 512; the constructor and the oracle call of tests/test_gpu_hier.py:73-84 (the
    pyramid is the hierarchical one with ``attention_block.`` as the layer key), at B = 1 and 5 text rows."""
    import lc2is_amd.nn as N
    in_dims, dim = [96, 192, 384, 768], 512
    return Case(id="ftn_decoder", family="FTN", classes=("FTNDecoder",),
                build=lambda: seed_weights(N.FTNDecoder(in_dims, dim, dropout=0), 5),
                make_inputs=lambda which: _hier_inputs(which, in_dims, dim, True, B=1, K=5), call=_hier_call(True),
                oracle=_hier_oracle(True, 8, (1, 1, 1), "attention_block."),
                bounds=Bounds(1.5e-2, 8e-2, dict(v0=3e-2, v3=6e-2, textual=6e-2),
                              "tests/test_gpu_hier.py:91 '_rel(out, ref) < 1.5e-2', :93 'vis[0] ... < 3e-2 and ... vis[3] ... < 6e-2', "
                              ":94 'txt ... < 6e-2'; parameters: :57 'assert worst < 8e-2'", _zero_rule_mean))


def _ftn_transformer_case(sr_ratio, repeat, upsample) -> Case:
    from lc2is_amd.nn.ftn import Transformer
    from oracle import ref_cpu as O

    def make_inputs(which):
        g = _gen(909 if which == "A" else 1010)
        B, h = 2, 8
        x = torch.randn(B, h * h, 512, generator=g)
        n = h * h * (4 ** repeat if upsample else 1)
        return Inputs(dict(x=x), dict(h=h), [torch.randn(B, n, 512, generator=g) * 0.1])

    return Case(id=f"ftn_transformer_sr{sr_ratio}", family="FTN", classes=("ftn.Transformer",),
                build=lambda: seed_weights(Transformer(repeat=repeat, upsample=upsample, sr_ratio=sr_ratio, dim=512, nhead=8,
                                                       dropout=0.0), 77),
                make_inputs=make_inputs, call=lambda m, fl, other: [m(fl["x"], other["h"])],
                oracle=lambda sd, fl, other: [O.ftn_transformer(sd, "", fl["x"], other["h"], repeat, sr_ratio, upsample, 8)],
                bounds=Bounds(1.5e-2, 8e-2, dict(x=5e-2),
                              "tests/test_gpu_ftn.py:93 '_rel(out, ref.detach()) < 1.5e-2', :95 '_rel(xd.grad, xr.grad) < 5e-2', "
                              ":104 '_rel(p.grad, gr) < 8e-2'; zero gradients :101-102", _zero_rule_mean))


def _swin_zero_rule(name, g, ref):
    """tests/test_gpu_swin.py:101-103: a key bias has a mathematically zero gradient; what is there is the bf16 round-off of the
    summed dK rows, judged against the query bias' gradient."""
    qg = ref[name.replace("k_proj", "q_proj")]
    assert float(g.abs().max()) < 0.05 * float(qg.abs().max()) + 1e-3, name


def _swin_case() -> Case:
    from lc2is_amd.nn.swin import SwinArch, SwinTransformer
    from oracle import ref_cpu as O
    cfg = O.SwinCfg(32, (2, 2, 2, 2), (1, 2, 4, 8), 5)

    def make_inputs(which):
        g = _gen(1111 if which == "A" else 1212)
        pix = torch.randn(2, 3, 176, 176, generator=g)      # grids 44 / 22 / 11 at window 5: padded stages, shifted second blocks
        douts = [torch.randn(2, n, c, generator=g) * 0.2 for n, c in ((1936, 32), (484, 64), (121, 128), (36, 256))]
        return Inputs({}, dict(pixel_values=pix), douts)

    return Case(id="swin", family="Swin", classes=("SwinTransformer",),
                build=lambda: seed_weights(SwinTransformer(SwinArch(32, (2, 2, 2, 2), (1, 2, 4, 8), 5), drop_path_rate=0.0), 15),
                make_inputs=make_inputs, call=lambda m, fl, other: list(m(other["pixel_values"])),
                oracle=lambda sd, fl, other: O.swin_hidden_states(sd, "encoder.", other["pixel_values"].to(next(iter(sd.values())).dtype), cfg),
                bounds=Bounds(1.5e-2, 8e-2, {}, "tests/test_gpu_swin.py:94 'assert _rel(o, r) < 1.5e-2', :108 'assert worst[1] < 8e-2'; "
                              "zero gradients :101-103", _swin_zero_rule))


def _model_case() -> Case:
    """BaseModelWithText at the dims and weights of tests/test_gpu_modules.py ``tiny_model`` (the golden fixture's, i.e. the
    reference's own parameters); the output is the fused mean cross-entropy, the oracle base_model_with_text + cross_entropy."""
    import lc2is_amd.nn as N
    from oracle import ref_cpu as O
    cfg = O.BaseCfg(in_size=64, out_size=16, patch=16, vision=O.ClipCfg(128, 2, 2, patch=16),
                    text=O.ClipCfg(64, 1, 2, eos_token_id=511), dec_heads=2, dec_layers=1)

    def build():
        m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                                text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2, dim_feedforward=128,
                                out_dim=64)
        m.load_state_dict(torch.load(G / "base_tiny.pt", weights_only=True)["state_dict"], strict=True)
        return m

    def make_inputs(which):
        fx = torch.load(G / "base_tiny.pt", weights_only=True)
        other = {k: fx[k].clone() for k in ("pixel_values", "input_ids", "attention_mask", "labels")}
        if which == "B":
            g = _gen(1313)
            other["pixel_values"] = torch.randn(2, 3, 64, 64, generator=g)
            other["input_ids"][:, 1:4] = torch.randint(1, 500, (2, 3), generator=g)
            other["labels"] = torch.randint(0, 151, (2, 16, 16), generator=g)
        return Inputs({}, other, [torch.ones(())])

    def call(m, fl, other):
        inputs = {k: other[k] for k in ("pixel_values", "input_ids", "attention_mask")}
        return [m.forward_loss(inputs, other["labels"])]

    def oracle(sd, fl, other):
        dt = sd["class_prototypes"].dtype
        inputs = dict(pixel_values=other["pixel_values"].to(dt), input_ids=other["input_ids"], attention_mask=other["attention_mask"])
        return [O.cross_entropy(O.base_model_with_text(sd, inputs, cfg)[2], other["labels"])]

    return Case(id="base_model", family="whole model", classes=("BaseModelWithText", "TextToPatch"), build=build, make_inputs=make_inputs,
                call=call, oracle=oracle,
                bounds=Bounds(2e-2, 8e-2, {}, MODULES_SRC + "; the loss: :73 'abs(loss.item() - fx[\"loss\"].item()) < 2e-2'",
                              _zero_rule_mean), tags=dict(scalar_loss=True))


def cases() -> list:
    out = [_vision_case(False), _vision_case(True), _text_case(False), _text_case(True)]
    for nf, dkv in ((True, 64), (False, 64), (True, 128)):     # d_kv == d_model: the packed-key load path
        for bias in (True, False):
            out.append(_decoder_case(nf, dkv, bias))
    out.append(_decoder_case(True, 64, True, final_norm=True))
    out += [_hier_case(True), _hier_case(False), _block_case("cross"), _block_case("self"), _block_case("ftn"),
            _ftn_transformer_case(2, 2, True), _ftn_transformer_case(1, 1, False),
            _ftn_decoder_case(), _swin_case(), _model_case()]
    return out


CASE_IDS = ["vision", "vision_full", "text", "text_pooler", "decoder_pre_kv64_bias", "decoder_pre_kv64_nobias", "decoder_post_kv64_bias",
            "decoder_post_kv64_nobias", "decoder_pre_kv128_bias", "decoder_pre_kv128_nobias", "decoder_pre_kv64_bias_norm", "hier_cross",
            "hier_self", "block_cross", "block_self", "block_ftn", "ftn_transformer_sr2", "ftn_transformer_sr1", "ftn_decoder", "swin", "base_model"]


def case(cid: str) -> Case:
    return {c.id: c for c in cases()}[cid]


# Classes exported by lc2is_amd.nn (``ftn.X`` for the ftn submodule) whose forward goes through a torch.autograd.Function of their
# own (or of a base class) and that no case names: each with the reason.
EXEMPT = {
    "PromptDecoder": "DecoderBlock under another name (adds no method): the decoder cases run its forward and backward",
    "ftn.Decoder": "hard-coded 128x128 / 64x64 / 32x32 / 16x16 stage grids, far above the table's shapes; its host branches are "
                   "linear_bwd_params and ftn.Transformer's, which the ftn_transformer cases and tests/test_gpu_ftn.py run",
    "ContrastiveModel": "towers and TextToPatch head of the base_model case behind another head function; its save decision is "
                        "checked by test_contrastive_head_trains_under_frozen_towers",
    "DenseClip": "a composition of ImageEncoderCLIPFull, TextEncoderCLIP, PromptDecoder and DecoderBlock (each a case of its own) "
                 "whose own Function has no parameters",
    "ScoreMapTail": "no parameters: gradients go to its two inputs only (tests/test_gpu_hier.py test_score_map_tail_vs_reference)",
    "AuxiliaryLoss": "a loss: no parameters, one input gradient (tests/test_gpu_modules.py)",
    "ContrastiveLoss": "a loss: no parameters, one input gradient (tests/test_gpu_modules.py)",
    "CrossEntropyLoss": "a loss: no parameters, one input gradient (tests/test_gpu_parity2.py)",
    "DiceCrossEntropyLoss": "a loss: no parameters, one input gradient (tests/test_gpu_dice.py)",
    "FocalLoss": "a loss: no parameters, one input gradient (tests/test_gpu_focal.py)",
    "Poly1CrossEntropyLoss": "a loss: no parameters, one input gradient (tests/test_gpu_focal.py)",
    "SigmoidFocalLoss": "a loss: no parameters, one input gradient (tests/test_gpu_sigmoid.py)",
    "SigmoidCrossEntropyLoss": "a loss: no parameters, one input gradient (tests/test_gpu_sigmoid.py)",
    "OhemCrossEntropyLoss": "a loss: no parameters, one input gradient (tests/test_gpu_ohem.py)",
    "NPairLoss": "a loss: no parameters, three input gradients (tests/test_gpu_modules.py)",
}
