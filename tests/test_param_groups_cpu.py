"""CPU-side checks of the parameter-group optimizers (lc2is_amd/csrc/optim.hip: lc2is_sgd_step_groups /
lc2is_adamw_step_groups): the C ABI is declared, exported and bound, the group-table entry is 8 bytes, and both layers refuse
bad arguments before any launch."""
import ctypes
import re

import pytest
import torch

from lc2is_amd import _lib, ops

SYMS = ("lc2is_sgd_step_groups", "lc2is_adamw_step_groups")
P = 0x10000   # 16-byte aligned stand-in: the argument checks never dereference a pointer
OK, ERR_SHAPE, ERR_NULL = 0, -1, -2


def test_header_declares_library_exports_and_ops_binds():
    syms = _lib.header_symbols()
    for s in SYMS:
        assert s in syms and s in ops._ARGTYPES
        assert isinstance(getattr(_lib.load(), s), ctypes._CFuncPtr)
    assert "lc2is_param_group" not in syms                       # a struct, not an entry point
    header = _lib._HEADER.read_text()
    body = header[header.rindex("typedef struct {", 0, header.index("} lc2is_param_group;")):header.index("} lc2is_param_group;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert fields == [("float", "lr_scale"), ("float", "weight_decay")]                # two fp32 words: 8 bytes, table row of ops
    assert 4 * len(fields) == 8
    for name, value in (("LC2IS_GROUP_GRANULE", ops.GROUP_GRANULE), ("LC2IS_MAX_PARAM_GROUPS", ops.MAX_PARAM_GROUPS),
                        ("LC2IS_GROUP_SKIP", ops.GROUP_SKIP)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (ops.GROUP_GRANULE, ops.MAX_PARAM_GROUPS, ops.GROUP_SKIP) == (64, 255, 255)
    # the control block keeps its layout: the grouped kernels read the same 12 words
    assert ops.OPTIM_CTRL_WORDS == 12


def test_the_granule_is_the_arena_alignment():
    from lc2is_amd.nn.base import ParamArena
    assert ParamArena.ALIGN == ops.GROUP_GRANULE


def test_sgd_step_groups_refuses_before_launching():
    f = ops._fn("lc2is_sgd_step_groups")
    ok = dict(params=P, grads=P, mom=None, n=1024, ctrl=P, gmap=P, groups=P, ngroups=3)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["params"], a["grads"], a["mom"], a["n"], a["ctrl"], a["gmap"], a["groups"], a["ngroups"], 0.9, 0, None)

    for k in ("params", "grads", "ctrl", "gmap", "groups"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(n=0) == ERR_SHAPE and call(n=1028) == ERR_SHAPE and call(n=96) == ERR_SHAPE      # whole 64-element granules
    assert call(ngroups=0) == ERR_SHAPE and call(ngroups=-1) == ERR_SHAPE and call(ngroups=256) == ERR_SHAPE
    assert call(params=P + 4) == ERR_SHAPE and call(grads=P + 8) == ERR_SHAPE and call(mom=P + 4) == ERR_SHAPE


def test_adamw_step_groups_refuses_before_launching():
    f = ops._fn("lc2is_adamw_step_groups")
    ok = dict(params=P, grads=P, m=P, v=P, n=1024, ctrl=P, gmap=P, groups=P, ngroups=255)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["params"], a["grads"], a["m"], a["v"], a["n"], a["ctrl"], a["gmap"], a["groups"], a["ngroups"], 0.9, 0.999,
                 1e-8, 0, None)

    for k in ("params", "grads", "m", "v", "ctrl", "gmap", "groups"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(n=0) == ERR_SHAPE and call(n=1056) == ERR_SHAPE
    assert call(ngroups=0) == ERR_SHAPE and call(ngroups=256) == ERR_SHAPE
    assert call(params=P + 4) == ERR_SHAPE and call(m=P + 4) == ERR_SHAPE and call(v=P + 12) == ERR_SHAPE


def test_python_launchers_refuse_cpu_tensors():
    g = torch.zeros(1024)
    ctrl = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32)
    gmap, table = torch.zeros(16, dtype=torch.uint8), torch.zeros(2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sgd_step_groups(g, g, None, ctrl, gmap, table)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.adamw_step_groups(g, g, g, g, ctrl, gmap, table, 0.9, 0.999, 1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# TrainStep(param_groups=...): validation before anything is built
# ---------------------------------------------------------------------------------------------------------------------
from torch import nn  # noqa: E402

from lc2is_amd.nn.base import GROUP_SKIP, granule_group_map  # noqa: E402
from lc2is_amd.step import TrainStep, make_param_groups  # noqa: E402


class _Refuse(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so a ValueError proves the guard ran before anything was built."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4, 4))
        self.b = nn.Parameter(torch.zeros(4))
        self.many = nn.ParameterList([nn.Parameter(torch.zeros(1)) for _ in range(256)])


def test_param_groups_keyword_is_keyword_only_and_defaults_to_none():
    import inspect
    prm = inspect.signature(TrainStep.__init__).parameters["param_groups"]
    assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None


def _cases():
    m = _Refuse()
    stranger = nn.Parameter(torch.zeros(3))
    singles = [dict(params=[f"many.{i}"]) for i in range(256)]
    return m, [
        ([dict(params=["w"]), dict(params=[m.w])], "two groups"),
        ([dict(params=["w", "w"])], "twice"),
        ([dict(params=["nope"])], "not a parameter"),
        ([dict(params=[stranger])], "not a parameter"),
        ([dict(params=[])], "empty params"),
        ([], "empty"),
        ([dict(params=["w"], lr=0.1)], "unknown keys"),
        ([dict(params=["w"], lr_scale=-1.0)], "lr_scale"),
        ([dict(params=["w"], lr_scale=float("nan"))], "lr_scale"),
        ([dict(params=["w"], lr_scale=float("inf"))], "lr_scale"),
        ([dict(params=["w"], weight_decay=-0.1)], "weight_decay"),
        ([dict(params=["w"], weight_decay=float("nan"))], "weight_decay"),
        (singles, "more than 255"),
        (singles[:255], "more than 255"),                    # 255 explicit groups + the implicit one for w and b
    ]


@pytest.mark.parametrize("idx", range(14))
def test_param_groups_guards_raise_before_any_allocation(idx):
    m, cases = _cases()
    groups, match = cases[idx]
    with pytest.raises(ValueError, match=match):
        TrainStep(m, param_groups=groups)


def test_valid_param_groups_reach_the_arena():
    m = _Refuse()
    every = [n for n, _ in m.named_parameters()]
    for groups in ([dict(params=["w"], lr_scale=0.1, weight_decay=0.0)], [dict(params=[m.b]), dict(params=iter(["w"]))],
                   [dict(params=every[:254]), dict(params=every[254:])], [dict(params="w", lr_scale=0.0)]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TrainStep(m, param_groups=groups)
    singles = [dict(params=[f"many.{i}"]) for i in range(254)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # 254 + the implicit group = 255: allowed
        TrainStep(m, param_groups=singles)


# ---------------------------------------------------------------------------------------------------------------------
# make_param_groups on the base_tiny architecture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    import lc2is_amd.nn as N
    return N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                               text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                               dim_feedforward=128, out_dim=64)


def _by_name(groups):
    out = {}
    for g in groups:
        assert set(g) == {"params", "lr_scale", "weight_decay"}
        for n in g["params"]:
            assert n not in out, n
            out[n] = (g["lr_scale"], g["weight_decay"])
    return out


TABLES = ("vision_encoder.enc.embeddings.position_embedding.weight", "text_encoder.enc.embeddings.position_embedding.weight",
          "text_encoder.enc.embeddings.token_embedding.weight")


def test_make_param_groups_no_decay(tiny):
    named = dict(tiny.named_parameters())
    assert len(named) == 93 and sum(p.dim() == 1 for p in named.values()) == 54
    groups = make_param_groups(tiny, weight_decay=0.05)
    got = _by_name(groups)
    assert set(got) == set(named)                                    # each of the 93 in exactly one group
    for n, p in named.items():
        want = 0.0 if (p.dim() == 1 or n in TABLES) else 0.05
        assert got[n] == (1.0, want), n
    assert got["vision_encoder.enc.embeddings.patch_embedding.weight"][1] == 0.05 and got["class_prototypes"][1] == 0.05
    assert got["vision_encoder.enc.embeddings.class_embedding"][1] == 0.0
    assert len(groups) == 2
    got = _by_name(make_param_groups(tiny, weight_decay=0.05, no_decay=("class_prototypes",)))
    assert got["class_prototypes"][1] == 0.0 and got["pixel_patch.visual.weight"][1] == 0.05 and got["pixel_patch.visual.bias"][1] == 0.0
    groups = make_param_groups(tiny, weight_decay=0.05, no_decay=False)
    assert len(groups) == 1 and set(_by_name(groups).values()) == {(1.0, 0.05)}


def test_make_param_groups_lr_scales_and_layer_decay(tiny):
    named = dict(tiny.named_parameters())
    scales = {"vision_encoder": 0.1, "text_encoder": 0}
    got = _by_name(make_param_groups(tiny, weight_decay=0.05, lr_scales=scales))
    for n in named:
        want = 0.1 if n.startswith("vision_encoder") else 0.0 if n.startswith("text_encoder") else 1.0
        assert got[n][0] == want, n
    # the longest prefix wins
    got = _by_name(make_param_groups(tiny, weight_decay=0.05, lr_scales={"vision_encoder": 0.1, "vision_encoder.enc.encoder": 0.3}))
    assert got["vision_encoder.enc.encoder.layers.0.mlp.fc1.weight"][0] == 0.3 and got["vision_encoder.enc.pre_layrnorm.weight"][0] == 0.1
    groups = make_param_groups(tiny, weight_decay=0.05, lr_scales=scales, layer_decay=0.5)
    got = _by_name(groups)
    v = "vision_encoder.enc."
    for n in named:
        if n.startswith(v + "embeddings.") or n.startswith(v + "pre_layrnorm."):
            want = 0.1 * 0.125
        elif n.startswith(v + "encoder.layers.0."):
            want = 0.1 * 0.25
        elif n.startswith(v + "encoder.layers.1."):
            want = 0.1 * 0.5
        elif n.startswith(v):
            assert "post_layernorm" in n
            want = 0.1
        elif n.startswith("text_encoder"):
            want = 0.0
        else:
            want = 1.0                                                # decoder (vision_decoder.layers.0.) and head untouched
        assert got[n][0] == want, (n, got[n], want)
    assert got["vision_decoder.layers.0.linear1.weight"][0] == 1.0
    assert len(groups) == len(set(got.values()))                     # one group per distinct (lr_scale, weight_decay)
    # a tower with its own prefix scale 1: the factors themselves
    got = _by_name(make_param_groups(tiny, weight_decay=0.0, layer_decay=0.5))
    t = "text_encoder.enc."
    L = len(tiny.text_encoder.enc.encoder.layers)
    assert got[t + "embeddings.token_embedding.weight"][0] == 0.5 ** (L + 1) and got[t + "encoder.layers.0.mlp.fc1.bias"][0] == 0.5 ** L
    assert got[t + "final_layer_norm.weight"][0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the host-side granule map
# ---------------------------------------------------------------------------------------------------------------------
def _layout(sizes, align=64):
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + align - 1) // align * align
    return offs, total


def test_granule_map_follows_the_arena_layout():
    sizes = [1, 64, 65, 4096, 127, 128 * 3 * 16 * 16, 17 * 128, 63]
    gids = [0, 1, 0, 2, 254, 1, 3, 2]
    offs, total = _layout(sizes)
    dead = {2, 6}
    m = granule_group_map(offs, sizes, gids, dead)
    assert m.dtype == torch.uint8 and m.device.type == "cpu" and m.numel() == total // 64
    for k, (o, n, g) in enumerate(zip(offs, sizes, gids)):
        end = offs[k + 1] if k + 1 < len(offs) else total
        want = GROUP_SKIP if k in dead else g
        assert bool((m[o // 64:end // 64] == want).all()), k       # every granule of the parameter, its padding included
        assert end - o >= n and (end - o) % 64 == 0
    assert torch.equal(granule_group_map(offs, sizes, gids), granule_group_map(offs, sizes, gids, ()))
    assert int((granule_group_map(offs, sizes, gids) == GROUP_SKIP).sum()) == 0
    assert bool((granule_group_map(offs, sizes, gids, range(len(sizes))) == GROUP_SKIP).all())


def test_granule_map_refuses_ids_the_kernels_would_skip_silently():
    sizes = [10, 100]
    offs, _ = _layout(sizes)
    with pytest.raises(ValueError, match="group id"):
        granule_group_map(offs, sizes, [0, 255])
    with pytest.raises(ValueError, match="group id"):
        granule_group_map(offs, sizes, [0, 7], ngroups=5)            # a stale map against a 5-entry table
    with pytest.raises(ValueError, match="group id"):
        granule_group_map(offs, sizes, [0, -1])
    with pytest.raises(ValueError, match="layout"):
        granule_group_map([0, 32], sizes, [0, 1])
    with pytest.raises(ValueError, match="one length"):
        granule_group_map(offs, sizes, [0])
    assert granule_group_map(offs, sizes, [0, 4], ngroups=5).tolist() == [0, 4, 4]
