"""CPU-side checks of gradient accumulation (TrainStep(accumulate=N); lc2is_accum_add / lc2is_optim_ctrl_update_accum in
lc2is_amd/csrc/optim.hip): the C ABI is declared and bound, the accumulation block's layout in the header is what the Python
offsets index, the C entry points refuse bad arguments before any launch, and TrainStep validates the keyword before anything is
built or allocated — and passes no new keyword to the model without it."""
import ctypes
import inspect
import re

import pytest
import torch
from torch import nn

from lc2is_amd import _lib, ops
from lc2is_amd.step import TrainStep, _accepts_accum

SYMS = ("lc2is_accum_add", "lc2is_optim_ctrl_update_accum")
P = 0x10000   # aligned stand-in: the argument checks never dereference a pointer
OK, ERR_SHAPE, ERR_NULL = 0, -1, -2


def test_header_declares_and_ops_binds_the_entry_points():
    syms = _lib.header_symbols()
    for s in SYMS:
        assert s in syms and s in ops._ARGTYPES
        assert isinstance(getattr(_lib.load(), s), ctypes._CFuncPtr)
    assert "lc2is_accum_block" not in syms          # a struct, not an entry point
    # the new update takes (ctrl, block, use_denom) in front of the old one's arguments after ctrl
    old, new = ops._ARGTYPES["lc2is_optim_ctrl_update"], ops._ARGTYPES["lc2is_optim_ctrl_update_accum"]
    assert new == [old[0], ctypes.c_void_p, ctypes.c_int] + old[1:]
    assert callable(ops.accum_add) and callable(ops.optim_ctrl_update_accum)


def test_block_layout_matches_the_python_offsets():
    """32 bytes: two doubles, two int32, two floats, in the header's order — what ops.ACCUM_* index (fp64 words for the sums,
    4-byte words for the rest)."""
    header = (_lib._HEADER).read_text()
    body = header[header.index("typedef struct {\n  double loss_sum;"):header.index("} lc2is_accum_block;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, decl in re.findall(r"(double|int32_t|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert fields == [("double", "loss_sum"), ("double", "denom"), ("int32_t", "micro"), ("int32_t", "reserved"),
                      ("float", "last_loss"), ("float", "last_denom")]
    size = {"double": 8, "int32_t": 4, "float": 4}
    offset, at = {}, 0
    for t, n in fields:
        assert at % size[t] == 0                     # naturally aligned: no padding, the C layout is the packed one
        offset[n] = at
        at += size[t]
    assert at == ops.ACCUM_BLOCK_BYTES == 32
    assert offset["loss_sum"] == 8 * ops.ACCUM_LOSS_SUM and offset["denom"] == 8 * ops.ACCUM_DENOM
    assert offset["micro"] == 4 * ops.ACCUM_MICRO
    assert offset["last_loss"] == 4 * ops.ACCUM_LAST_LOSS and offset["last_denom"] == 4 * ops.ACCUM_LAST_DENOM


def test_accum_add_refuses_before_launching():
    f = ops._fn("lc2is_accum_add")
    assert f(None, P, None) == ERR_NULL and f(P, None, None) == ERR_NULL
    assert f(P + 4, P, None) == ERR_SHAPE            # the block holds doubles: 8-byte aligned
    assert f(P, P + 2, None) == ERR_SHAPE


def test_optim_ctrl_update_accum_refuses_before_launching():
    f = ops._fn("lc2is_optim_ctrl_update_accum")
    ok = dict(ctrl=P, block=P, use_denom=1, partials=P, flags=P, nparts=4096, table=P, table_len=10, grad_scale=1.0, max_norm=1.0,
              skip=1, b1=0.9, b2=0.999)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["ctrl"], a["block"], a["use_denom"], a["partials"], a["flags"], a["nparts"], a["table"], a["table_len"],
                 a["grad_scale"], a["max_norm"], a["skip"], a["b1"], a["b2"], None)

    for k in ("ctrl", "block", "partials", "flags", "table"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(nparts=0) == ERR_SHAPE and call(nparts=4097) == ERR_SHAPE
    assert call(table_len=0) == ERR_SHAPE
    assert call(use_denom=2) == ERR_SHAPE and call(use_denom=-1) == ERR_SHAPE
    assert call(block=P + 4) == ERR_SHAPE and call(ctrl=P + 2) == ERR_SHAPE
    assert call(max_norm=0.0) == ERR_SHAPE and call(grad_scale=0.0) == ERR_SHAPE and call(b1=1.0) == ERR_SHAPE


def test_python_launchers_refuse_cpu_tensors_and_wrong_blocks():
    block = torch.zeros(4, dtype=torch.float64)
    ctrl = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.accum_add(block, torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.optim_ctrl_update_accum(ctrl, block, True, torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(1))
    with pytest.raises(RuntimeError, match="required"):
        ops.accum_add(None, torch.zeros(2))


class _Refuse(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so another exception proves the guard ran before anything was built."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))
        self.calls = []


class _NoAccum(_Refuse):
    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", dice=None,
                     seg_counts=None):
        raise AssertionError("never called")


class _WithAccum(_Refuse):
    def forward_loss(self, inputs, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean", dice=None,
                     seg_counts=None, accum=None):
        raise AssertionError("never called")


def test_keyword_is_keyword_only_and_defaults_to_the_plain_step():
    prm = inspect.signature(TrainStep.__init__).parameters["accumulate"]
    assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None
    assert _accepts_accum(_WithAccum()) and not _accepts_accum(_NoAccum()) and not _accepts_accum(_Refuse())
    import lc2is_amd.nn as N
    for cls in (N.BaseModelWithText, N.PromptFTN):
        assert "accum" in inspect.signature(cls.forward_loss).parameters, cls
    assert "accum" in inspect.signature(N.ScoreMapTail.loss).parameters


@pytest.mark.parametrize("bad", [0, -3, True, False, 2.5, "2"])
def test_bad_accumulate_values_raise_before_any_allocation(bad):
    with pytest.raises(ValueError, match="accumulate"):
        TrainStep(_WithAccum(), accumulate=bad)


def test_dice_with_accumulation_raises_at_construction():
    from lc2is_amd.nn.loss import DiceCrossEntropyLoss
    for n in (2, 3):
        with pytest.raises(ValueError, match="Dice"):
            TrainStep(_WithAccum(), criterion=DiceCrossEntropyLoss(), accumulate=n)
    with pytest.raises(RuntimeError):                # N = 1 is the plain step: the guards pass, the (CPU) model is refused by the arena
        TrainStep(_WithAccum(), criterion=DiceCrossEntropyLoss(), accumulate=1)


def test_model_without_accum_keyword_is_refused_before_any_allocation():
    with pytest.raises(TypeError, match="accum="):
        TrainStep(_NoAccum(), accumulate=2)
    with pytest.raises(TypeError, match="accum="):
        TrainStep(_Refuse(), accumulate=4)
    for n in (None, 1):                              # the plain step asks nothing of the model: refused by the arena instead
        with pytest.raises(RuntimeError):
            TrainStep(_NoAccum(), accumulate=n)
    with pytest.raises(RuntimeError):                # a model that takes accum=: the guards pass
        TrainStep(_WithAccum(), accumulate=2)


def test_accum_with_dice_is_a_value_error_in_forward_loss():
    """Refused before the towers run: no tensor is touched."""
    import lc2is_amd.nn as N
    tail = N.ScoreMapTail()
    with pytest.raises(ValueError, match="accum="):
        tail.loss(torch.zeros(1, 4, 8), torch.zeros(1, 3, 8), torch.zeros(1, 8, 8, dtype=torch.long),
                  dice=(1.0, 1.0, 1.0, False), accum=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="accum="):
        N.BaseModelWithText.forward_loss(object(), {}, None, dice=(1.0, 1.0, 1.0, False), accum=torch.zeros(4, dtype=torch.float64))


class _Spy:
    """Stands in for a TrainStep whose model records the keywords of its forward_loss call and then stops the step."""

    class Stop(Exception):
        pass

    def __init__(self, accum_n):
        from types import SimpleNamespace
        self.seen = None
        spy = self

        def forward_loss(inputs, labels, ignore_index, **kw):
            spy.seen = kw
            raise _Spy.Stop

        self._ema_swapped, self._accum_n, self.micro, self.reducer = False, accum_n, 0, None
        self._accum = None if accum_n is None else torch.zeros(4, dtype=torch.float64)
        self._seg_counts, self._ohem, self._dice, self._loss_opts, self.ignore_index = None, False, False, False, -100
        self.arena = SimpleNamespace(zero_grad=lambda set_to_none=True: None)
        self.model = SimpleNamespace(forward_loss=forward_loss)


def test_accumulate_1_adds_no_keyword_to_the_model_call():
    for accumulate in (None, 1):
        with pytest.raises(RuntimeError):
            TrainStep(_WithAccum(), accumulate=accumulate)   # (builds the plain step: the arena refuses the CPU model)
    spy = _Spy(None)                                 # what accumulate=None / 1 leaves in the object: _accum_n None, no block
    with pytest.raises(_Spy.Stop):
        TrainStep.step(spy, {}, None)
    assert spy.seen == {}
    spy = _Spy(2)
    with pytest.raises(_Spy.Stop):
        TrainStep.step(spy, {}, None)
    assert list(spy.seen) == ["accum"] and spy.seen["accum"] is spy._accum
