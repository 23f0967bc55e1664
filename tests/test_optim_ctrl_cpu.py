"""CPU-side checks of the device-held optimizer path (lc2is_amd/csrc/optim.hip, TrainStep's lr_schedule / max_grad_norm /
skip_nonfinite / device_state): the C ABI is declared and bound, the workspace query is a pure host function with the stated
formula, the C entry points refuse bad arguments before any launch, TrainStep validates the new keywords before anything is
built or allocated, and lr_table_from_torch reproduces entry for entry what a torch scheduler hands its optimizer in the
reference loop's order (optimizer.step() first, lr_scheduler.step() after: engine.py:101-104)."""
import ctypes
import inspect
import math

import pytest
import torch
from torch import nn

from lc2is_amd import _lib, ops
from lc2is_amd.step import TrainStep, lr_table_from_torch

SYMS = ("lc2is_grad_sumsq_blocks", "lc2is_grad_sumsq_workspace_bytes", "lc2is_grad_sumsq", "lc2is_optim_ctrl_update",
        "lc2is_sgd_step_ctrl", "lc2is_adamw_step_ctrl")
P = 0x10000   # 16-byte aligned stand-in: the argument checks never dereference a pointer
OK, ERR_SHAPE, ERR_NULL, ERR_WORKSPACE = 0, -1, -2, -4


def test_header_declares_and_ops_binds_the_entry_points():
    syms = _lib.header_symbols()
    for s in SYMS:
        assert s in syms and s in ops._ARGTYPES
        assert isinstance(getattr(_lib.load(), s), ctypes._CFuncPtr)
    assert "lc2is_optim_ctrl" not in syms          # the control block is a struct, not an entry point
    header = (_lib._HEADER).read_text()
    assert "} lc2is_optim_ctrl;" in header
    for field in ("calls", "applied", "skipped", "finite", "grad_norm", "clip_coef", "lr", "bc1, bc2", "grad_mul", "apply"):
        assert f" {field};" in header, field


def test_control_block_layout_matches_the_python_indices():
    """12 four-byte words in the header's order: what ops.CTRL_* index."""
    header = (_lib._HEADER).read_text()
    body = header[header.index("typedef struct {\n  int32_t calls;"):header.index("} lc2is_optim_ctrl;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == ["calls", "applied", "skipped", "finite", "grad_norm", "clip_coef", "lr", "bc1", "bc2", "grad_mul", "apply",
                     "reserved"]
    assert len(names) == ops.OPTIM_CTRL_WORDS
    for name, idx in (("calls", ops.CTRL_CALLS), ("applied", ops.CTRL_APPLIED), ("skipped", ops.CTRL_SKIPPED),
                      ("finite", ops.CTRL_FINITE), ("grad_norm", ops.CTRL_GRAD_NORM), ("clip_coef", ops.CTRL_CLIP_COEF),
                      ("lr", ops.CTRL_LR), ("bc1", ops.CTRL_BC1), ("bc2", ops.CTRL_BC2), ("grad_mul", ops.CTRL_GRAD_MUL),
                      ("apply", ops.CTRL_APPLY)):
        assert names[idx] == name


def test_workspace_query_is_a_pure_host_function():
    """blocks = min(4096, ceil(n / 1024)) — a function of n alone — and 8 bytes (fp32 partial + uint32 flag) per block."""
    blocks, ws = ops._fn("lc2is_grad_sumsq_blocks"), ops._fn("lc2is_grad_sumsq_workspace_bytes")
    for n in (4, 1024, 1028, 4096 * 1024, 4096 * 1024 + 4, 157_090_048):
        want = min(4096, -(-n // 1024))
        assert blocks(n) == want and ws(n) == 8 * want, n
    assert blocks(157_090_048) == 4096
    # the summation geometry the norm tolerance of the GPU test is derived from: 38 float4s = 152 additions per lane
    assert -(-(157_090_048 // 4) // (4096 * 256)) * 4 == 152
    assert blocks(0) == 0 and ws(0) == 0 and blocks(6) == 0 and ws(1023) == 0


def test_grad_sumsq_refuses_before_launching():
    f = ops._fn("lc2is_grad_sumsq")
    assert f(None, 1024, P, 8, None) == ERR_NULL and f(P, 1024, None, 8, None) == ERR_NULL
    assert f(P, 0, P, 8, None) == ERR_SHAPE and f(P, 1022, P, 8, None) == ERR_SHAPE
    assert f(P + 4, 1024, P, 8, None) == ERR_SHAPE                 # 16 bytes per lane: the gradient must be 16-byte aligned
    assert f(P, 1024, P + 2, 8, None) == ERR_SHAPE
    assert f(P, 1024, P, 7, None) == ERR_WORKSPACE and f(P, 4096 * 1024, P, 8 * 4096 - 1, None) == ERR_WORKSPACE


def test_optim_ctrl_update_refuses_before_launching():
    f = ops._fn("lc2is_optim_ctrl_update")
    ok = dict(ctrl=P, partials=P, flags=P, nparts=4096, table=P, table_len=10, grad_scale=1.0, max_norm=1.0, skip=1, b1=0.9,
              b2=0.999)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["ctrl"], a["partials"], a["flags"], a["nparts"], a["table"], a["table_len"], a["grad_scale"], a["max_norm"],
                 a["skip"], a["b1"], a["b2"], None)

    for k in ("ctrl", "partials", "flags", "table"):
        assert call(**{k: None}) == ERR_NULL, k
    assert call(nparts=0) == ERR_SHAPE and call(nparts=4097) == ERR_SHAPE
    assert call(table_len=0) == ERR_SHAPE                                          # an empty schedule
    assert call(max_norm=0.0) == ERR_SHAPE and call(max_norm=-1.0) == ERR_SHAPE and call(max_norm=math.nan) == ERR_SHAPE
    assert call(grad_scale=0.0) == ERR_SHAPE and call(grad_scale=math.nan) == ERR_SHAPE
    assert call(b1=1.0) == ERR_SHAPE and call(b2=-0.1) == ERR_SHAPE
    assert call(ctrl=P + 2) == ERR_SHAPE


def test_ctrl_optimizers_refuse_before_launching():
    sgd, adamw = ops._fn("lc2is_sgd_step_ctrl"), ops._fn("lc2is_adamw_step_ctrl")
    assert sgd(None, P, None, 1024, P, 0.0, 0.0, 0, None) == ERR_NULL
    assert sgd(P, None, None, 1024, P, 0.0, 0.0, 0, None) == ERR_NULL
    assert sgd(P, P, None, 1024, None, 0.0, 0.0, 0, None) == ERR_NULL               # no control block
    assert sgd(P, P, None, 0, P, 0.0, 0.0, 0, None) == ERR_SHAPE and sgd(P, P, P, 1022, P, 0.9, 0.0, 0, None) == ERR_SHAPE
    for missing in range(4):
        a = [P, P, P, P]
        a[missing] = None
        assert adamw(*a, 1024, P, 0.9, 0.999, 1e-8, 0.0, 0, None) == ERR_NULL
    assert adamw(P, P, P, P, 1024, None, 0.9, 0.999, 1e-8, 0.0, 0, None) == ERR_NULL
    assert adamw(P, P, P, P, 6, P, 0.9, 0.999, 1e-8, 0.0, 0, None) == ERR_SHAPE


def test_python_launchers_refuse_cpu_tensors():
    g = torch.zeros(1024)
    ctrl = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.grad_sumsq(g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.optim_ctrl_update(ctrl, g[:4], torch.zeros(4, dtype=torch.int32), g[:1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sgd_step_ctrl(g, g, None, ctrl)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.adamw_step_ctrl(g, g, g, g, ctrl, 0.9, 0.999, 1e-8, 0.0)


def test_trainstep_keywords_exist_and_default_to_the_old_path():
    params = inspect.signature(TrainStep.__init__).parameters
    for name, default in (("lr_schedule", None), ("schedule_steps", None), ("max_grad_norm", None), ("skip_nonfinite", False),
                          ("device_state", False)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, name
    assert params["lr"].default == 1e-5 and params["optimizer"].default == "sgd"


class _Refuse(nn.Module):
    """A CPU model: ParamArena refuses it with a RuntimeError, so a ValueError proves the guard ran before anything was built."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4))


@pytest.mark.parametrize("kw,match", [
    (dict(max_grad_norm=0.0), "max_grad_norm"),
    (dict(max_grad_norm=-1.0), "max_grad_norm"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm"),
    (dict(lr_schedule=[]), "empty"),
    (dict(lr_schedule=torch.zeros(0)), "empty"),
    (dict(lr_schedule=torch.zeros(2, 2)), "1-D"),
    (dict(lr_schedule=lambda i: 1e-3), "schedule_steps"),
    (dict(lr_schedule=lambda i: 1e-3, schedule_steps=0), "schedule_steps"),
    (dict(lr_schedule=[1e-3, 1e-4], schedule_steps=2), "schedule_steps"),
    (dict(schedule_steps=5), "schedule_steps"),
    (dict(lr_schedule=[1e-3, float("nan")]), "finite"),
    (dict(lr_schedule=[1e-3, 1e-4], lr=0.05), "conflicts"),
])
def test_trainstep_argument_guards_raise_before_any_allocation(kw, match):
    with pytest.raises(ValueError, match=match):
        TrainStep(_Refuse(), **kw)


def test_trainstep_accepts_a_restated_first_rate_and_then_builds():
    """lr equal to the table's first entry is not a conflict: the guards pass and the (CPU) model is refused by the arena instead."""
    for kw in (dict(lr_schedule=[0.05, 0.01], lr=0.05), dict(lr_schedule=lambda i: 0.1 / (i + 1), schedule_steps=3),
               dict(device_state=True), dict(max_grad_norm=float("inf")), dict(skip_nonfinite=True)):
        with pytest.raises(RuntimeError):
            TrainStep(_Refuse(), **kw)


def _engine_order_rates(make_scheduler, base_lr, steps):
    """The plain torch loop in the reference's order, recording the rate optimizer.step() is called with."""
    p = nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=base_lr)
    sched = make_scheduler(opt)
    used = []
    for _ in range(steps):
        p.grad = torch.ones(3)
        used.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return used


def _warmup_decay(i, warm=5, total=50):
    return (i + 1) / warm if i < warm else max(0.0, (total - i) / (total - warm))


SCHEDULERS = {
    "lambda_warmup_decay": lambda o: torch.optim.lr_scheduler.LambdaLR(o, _warmup_decay),
    "polynomial": lambda o: torch.optim.lr_scheduler.PolynomialLR(o, total_iters=40, power=0.9),
    "one_cycle": lambda o: torch.optim.lr_scheduler.OneCycleLR(o, max_lr=3e-4, total_steps=60),
}


@pytest.mark.parametrize("name", sorted(SCHEDULERS))
def test_lr_table_from_torch_matches_the_scheduler_entry_for_entry(name):
    steps, base = 50, 6e-5
    table = lr_table_from_torch(SCHEDULERS[name], base, steps)
    assert table.dtype == torch.float32 and table.shape == (steps,) and table.device.type == "cpu"
    used = _engine_order_rates(SCHEDULERS[name], base, steps)
    want = torch.tensor(used, dtype=torch.float64).to(torch.float32)
    assert torch.equal(table, want), (table - want).abs().max()
    assert len(set(used)) > 10                               # a schedule that actually moves
    if name != "one_cycle":
        assert used[0] == pytest.approx(base * (0.2 if name == "lambda_warmup_decay" else 1.0))
