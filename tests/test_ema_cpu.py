"""CPU-side checks of the weight EMA and of the resumable train state (lc2is_amd/csrc/optim.hip: ema_ctrl_kernel and
swap_f32_kernel; TrainStep's ema_decay / ema_warmup / ema_every, state_dict / load_state_dict): the C ABI is declared with its
`replaces:` note and bound, both entry points refuse bad arguments before any launch, TrainStep validates the new keywords before
anything is built, the host mirror of the kernel's weight is the closed form, and check_train_state names each mismatch."""
import copy
import ctypes
import inspect
import math
import re

import pytest
import torch
from torch import nn

from lc2is_amd import _lib, ops
from lc2is_amd.step import TrainStep, check_train_state, ema_weight_at

SYMS = ("lc2is_ema_update_ctrl", "lc2is_swap_f32")
P, Q = 0x10000, 0x80000   # 16-byte aligned stand-ins, 458752 bytes apart: the argument checks never dereference a pointer
OK, ERR_SHAPE, ERR_NULL = 0, -1, -2


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def test_header_declares_both_symbols_with_a_replaces_note_and_ops_binds_them():
    syms = _lib.header_symbols()
    header = _lib._HEADER.read_text()
    for s in SYMS:
        assert s in syms and s in ops._ARGTYPES
        assert isinstance(getattr(_lib.load(), s), ctypes._CFuncPtr)
        decl = header.index(f"int {s}(")
        comment = header[header.rindex("/*", 0, decl):decl]
        assert comment.rstrip().endswith("*/") and comment.count("/*") == 1          # the comment directly above the declaration
        note = comment[comment.index("replaces:"):]
        assert "nothing in the reference" in note and "torch" in note, s            # no counterpart; the torch idiom it stands for
    assert ops._ARGTYPES["lc2is_ema_update_ctrl"] == [ops._P, ops._P, ops._Z, ops._P, ops._F, ops._I, ops._I, ops._I, ops._P]
    assert ops._ARGTYPES["lc2is_swap_f32"] == [ops._P, ops._P, ops._Z, ops._P]
    # the control block is read, not changed: still 12 words
    assert ops.OPTIM_CTRL_WORDS == 12 and "int32_t reserved;\n} lc2is_optim_ctrl;" in header


def test_launcher_signatures():
    p = inspect.signature(ops.ema_update_ctrl).parameters
    assert list(p) == ["ema", "params", "ctrl", "one_minus_decay", "warmup", "every", "reverse"]
    assert (p["warmup"].default, p["every"].default, p["reverse"].default) == (False, 1, False)
    assert list(inspect.signature(ops.swap_f32).parameters) == ["a", "b"]


def test_ema_update_refuses_before_launching():
    f = ops._fn("lc2is_ema_update_ctrl")
    ok = dict(ema=P, params=Q, n=1024, ctrl=P, w=1e-4, warmup=0, every=1, reverse=0)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["ema"], a["params"], a["n"], a["ctrl"], a["w"], a["warmup"], a["every"], a["reverse"], None)

    for k in ("ema", "params", "ctrl"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(n=0) == ERR_SHAPE and call(n=1022) == ERR_SHAPE
    assert call(ema=P + 4) == ERR_SHAPE and call(params=Q + 8) == ERR_SHAPE       # one float4 per lane: 16-byte alignment
    assert call(ctrl=P + 2) == ERR_SHAPE
    for w in (0.0, -0.1, 1.0 + 1e-6, math.nan, math.inf):                         # (0, 1]: decay 0 is w = 1
        assert call(w=w) == ERR_SHAPE, w
    assert call(every=0) == ERR_SHAPE and call(every=-3) == ERR_SHAPE


def test_swap_refuses_before_launching():
    f = ops._fn("lc2is_swap_f32")
    assert f(None, Q, 1024, None) == ERR_NULL and f(P, None, 1024, None) == ERR_NULL
    assert f(P, Q, 0, None) == ERR_SHAPE and f(P, Q, 1022, None) == ERR_SHAPE
    assert f(P + 4, Q, 1024, None) == ERR_SHAPE and f(P, Q + 8, 1024, None) == ERR_SHAPE
    assert f(P, P, 1024, None) == ERR_SHAPE                                       # the same buffer
    assert f(P, P + 4096 - 16, 1024, None) == ERR_SHAPE                           # the last float4 of a is the first of b
    assert f(P + 4096 - 16, P, 1024, None) == ERR_SHAPE                           # ... in either order
    assert f(P, P + 16, 1024, None) == ERR_SHAPE


def test_python_launchers_refuse_cpu_tensors_and_unequal_lengths():
    g = torch.zeros(1024)
    ctrl = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ema_update_ctrl(g, g.clone(), ctrl, 1e-4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.swap_f32(g, g.clone())


def test_trainstep_keywords_exist_and_default_to_no_ema():
    params = inspect.signature(TrainStep.__init__).parameters
    for name, default in (("ema_decay", None), ("ema_warmup", False), ("ema_every", 1)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, name
    for name in ("ema_weights", "ema_state_dict", "reset_ema", "state_dict", "load_state_dict"):
        assert callable(getattr(TrainStep, name)), name


class _Refuse(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so a ValueError proves the guard ran before anything was built."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))


@pytest.mark.parametrize("kw,match", [
    (dict(ema_decay=1.0), "ema_decay"),
    (dict(ema_decay=-0.1), "ema_decay"),
    (dict(ema_decay=1.5), "ema_decay"),
    (dict(ema_decay=float("nan")), "ema_decay"),
    (dict(ema_decay=0.99, ema_every=0), "ema_every"),
    (dict(ema_decay=0.99, ema_every=-2), "ema_every"),
    (dict(ema_decay=0.99, ema_every=1.5), "ema_every"),
    (dict(ema_warmup=True), "need ema_decay"),
    (dict(ema_every=2), "need ema_decay"),
])
def test_trainstep_ema_argument_guards_raise_before_any_allocation(kw, match):
    with pytest.raises(ValueError, match=match):
        TrainStep(_Refuse(), **kw)


def test_valid_ema_arguments_pass_the_guards_and_then_build():
    """The guards pass and the (CPU) model is refused by the arena instead: ema_decay selects the device-held path."""
    for kw in (dict(ema_decay=0.0), dict(ema_decay=0.9999, ema_warmup=True, ema_every=4)):
        with pytest.raises(RuntimeError):
            TrainStep(_Refuse(), **kw)


def test_ema_weight_at_is_the_closed_form():
    """fp32(1 - decay) with the difference in fp64; under warm-up max of it and fp32(9 / (10 + j)), i.e. 1 - min(decay,
    (1 + j) / (10 + j)) — equal in exact arithmetic, compared here to one fp32 ulp of the weight."""
    for decay in (0.0, 0.5, 0.9, 0.999, 0.9999):
        w = _f32(1.0 - decay)
        assert ema_weight_at(1, decay) == ema_weight_at(10 ** 6, decay) == w
        for j in (1, 2, 5, 30, 91, 8_990, 89_989, 89_990, 89_991, 89_999, 10 ** 7):
            got = ema_weight_at(j, decay, warmup=True)
            assert got == max(w, _f32(9.0 / (10.0 + j))), (decay, j)
            tf = 1.0 - min(decay, (1.0 + j) / (10.0 + j))
            assert abs(got - tf) <= 2.0 ** -23 * tf + 1e-18, (decay, j, got, tf)
            assert _f32(got) == got                                                # an fp32 value
    assert ema_weight_at(1, 0.9999, True) == _f32(9.0 / 11.0)
    assert ema_weight_at(89_999, 0.9999, True) == _f32(1.0 - 0.9999)               # 9 / 90 009 < 1e-4: the weight is w itself
    # what forming 1.f - 0.9999f on the device would have given: off by ~3e-4 relative
    naive = float(torch.tensor(1.0) - torch.tensor(0.9999))
    assert abs(naive - 1e-4) / 1e-4 > 1e-4 and abs(_f32(1.0 - 0.9999) - 1e-4) / 1e-4 < 1e-7


def _meta(**over):
    m = dict(optimizer="adamw",
             hyper=dict(lr=1e-5, momentum=0.0, weight_decay=0.05, betas=[0.9, 0.999], eps=1e-8),
             device_path=True,
             layout=dict(names=["a.weight", "a.bias", "b.weight"], offsets=[0, 128, 192], numels=[100, 10, 64], total=256),
             groups=dict(table=[[1.0, 0.05], [0.5, 0.0]], ids=[0, 1, 0]),
             lr_table=[1e-3, 5e-4, 1e-4], clip=[1.0, True], ema=dict(decay=0.999, warmup=True, every=1))
    m.update(over)
    return m


def test_check_train_state_accepts_the_same_meta():
    assert check_train_state(_meta(), _meta()) is None
    assert check_train_state(copy.deepcopy(_meta()), _meta(groups=dict(table=[[1.0, 0.05], [0.5, 0.0]], ids=[0, 1, 0]))) is None


def _layout(**over):
    lay = dict(_meta()["layout"])
    lay.update(over)
    return lay


@pytest.mark.parametrize("saved,live,match", [
    (_meta(optimizer="sgd"), _meta(), r"saved optimizer is 'sgd'.*'adamw'"),
    (_meta(), _meta(hyper=dict(_meta()["hyper"], weight_decay=0.1)), r"hyper-parameter weight_decay: saved 0\.05.*0\.1"),
    (_meta(), _meta(hyper=dict(_meta()["hyper"], betas=[0.9, 0.99])), r"hyper-parameter betas"),
    (_meta(layout=_layout(names=["a.weight", "a.bias"], offsets=[0, 128], numels=[100, 10])), _meta(),
     r"parameter 'b\.weight' is missing from the saved state"),
    (_meta(layout=_layout(numels=[100, 12, 64])), _meta(), r"parameter 'a\.bias' has 10 elements, the saved state 12"),
    (_meta(layout=_layout(offsets=[0, 128, 256])), _meta(), r"parameter 'b\.weight' lies at arena offset 192.*256"),
    (_meta(layout=_layout(names=["a.weight", "a.bias", "b.weight", "c"], offsets=[0, 128, 192, 256], numels=[100, 10, 64, 1])),
     _meta(), r"parameter 'c' of the saved state is missing from the model"),
    (_meta(groups=dict(table=[[1.0, 0.05], [0.5, 0.0]], ids=[0, 1, 1])), _meta(),
     r"another group assignment: parameter 'b\.weight' was in group 1, is in group 0"),
    (_meta(groups=dict(table=[[1.0, 0.05], [0.25, 0.0]], ids=[0, 1, 0])), _meta(), r"another group recipe"),
    (_meta(groups=None), _meta(), r"param_groups configured but not in the saved state"),
    (_meta(), _meta(groups=None), r"param_groups saved but not configured"),
    (_meta(lr_table=[1e-3, 5e-4, 2e-4]), _meta(), r"another lr table: entry 2 is 0\.0001, saved 0\.0002"),
    (_meta(lr_table=[1e-3]), _meta(), r"another lr table: saved 1 entries.*3"),
    (_meta(), _meta(clip=[float("inf"), True]), r"max_grad_norm, skip_nonfinite"),
    (_meta(), _meta(ema=None), r"EMA saved but not configured"),
    (_meta(ema=None), _meta(), r"EMA configured but not in the saved state"),
    (_meta(ema=dict(decay=0.99, warmup=True, every=1)), _meta(), r"EMA setting decay: saved 0\.99.*0\.999"),
    (_meta(), _meta(ema=dict(decay=0.999, warmup=True, every=2)), r"EMA setting every: saved 1.*2"),
    (_meta(device_path=False, lr_table=None, clip=None, groups=None, ema=None), _meta(groups=None, ema=None),
     r"host-scalar path.*device-held"),
])
def test_check_train_state_names_the_difference(saved, live, match):
    with pytest.raises(ValueError, match=match):
        check_train_state(saved, live)


def test_check_train_state_is_a_pure_host_function():
    """Dicts of strings, numbers and lists in, nothing out: no tensor, no device, inputs left as they were."""
    a, b = _meta(), _meta()
    check_train_state(a, b)
    assert a == _meta() and b == _meta()
    src = inspect.getsource(check_train_state)
    assert not re.search(r"\btorch\.|\bops\.|\.cuda\b", src)


def test_checkpoint_module_has_the_train_state_functions():
    from lc2is_amd import checkpoint
    p = inspect.signature(checkpoint.save_train_state).parameters
    assert list(p) == ["ts", "out_dir", "train_step", "write"] and p["write"].default is None
    assert list(inspect.signature(checkpoint.load_train_state).parameters) == ["ts", "path"]
    assert "weights_only=True" in inspect.getsource(checkpoint.load_train_state)
