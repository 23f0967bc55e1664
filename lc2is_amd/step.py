"""The training step — this repo's counterpart of ``Engine.train_loop`` (reference engine.py:69-123).

One call to :meth:`TrainStep.step` is one iteration of the reference's hot loop:
    optimizer.zero_grad()                                   engine.py:78
    outputs_dict = model(inputs)                            engine.py:93
    loss = criterion(outputs_dict["outputs"], labels)       engine.py:94     (CE; fused with the head here)
    loss.backward()                                         engine.py:100    (+ NEW: DP gradient all-reduce)
    optimizer.step()                                        engine.py:101
and returns the loss as a DEVICE tensor (the reference's per-step ``.item()`` sync, engine.py:108, is left to
the caller's logging cadence).

MI355X layout: all parameters and gradients live in one flat fp32 arena (``ParamArena``), so the optimizer is
a single fused HIP launch and the data-parallel reduction is over one contiguous buffer, issued per module
(head, decoder, vision, text) as soon as that module's backward has run, on RCCL's own stream, overlapping
the remaining backward (``lc2is_amd.dp.GradReducer``).

``criterion``: an ``lc2is_amd.nn.CrossEntropyLoss`` (or ``torch.nn.CrossEntropyLoss``) whose ``ignore_index``, ``weight``,
``label_smoothing`` and ``reduction`` ('mean' / 'sum') configure the fused head; default: ``CrossEntropyLoss()``.  An
``lc2is_amd.nn.OhemCrossEntropyLoss`` adds its hard-pixel selection in front of the fused head (two launches and the selection's,
all on the device: eager, captured, under a reducer — each rank selects over its own batch — and with the device-held options);
``ohem_info`` is the last selection's device info block.  An ``lc2is_amd.nn.DiceCrossEntropyLoss`` trains on ce_weight * mean CE
+ dice_weight * soft Dice through the fused head (a statistics pass, a one-block launch and the gradient pass, all on the device:
eager, captured, under a reducer — each rank takes the statistics of its own batch); ``dice_stats`` are the last step's device
tensors (I, P, T, loss block).  The loss is deterministic, so the criterion's ``eval()`` mode changes nothing.  An
``lc2is_amd.nn.FocalLoss`` / ``Poly1CrossEntropyLoss`` trains on its per-pixel loss through the fused head in the launches of the
plain step (``forward_loss(focal=...)``; its ``weight`` and 'mean' / 'sum' apply): eager, captured, under ``accumulate=N``, with
``seg_metrics=True`` and under a reducer.  An ``lc2is_amd.nn.SigmoidFocalLoss`` / ``SigmoidCrossEntropyLoss`` (per-class binary
terms, no softmax; 'mean' divides by a count of elements or pixels, not a weight sum) trains the same way through
``forward_loss(sigmoid=...)``: eager, captured, under ``accumulate=N`` (``accum_count`` is then the number of counted pixels), with
``seg_metrics=True`` and under a reducer.

The device-held path (opt-in: any of ``lr_schedule``, ``max_grad_norm``, ``skip_nonfinite``, ``device_state``) adds what the
reference's loop has around ``optimizer.step()``:
    scaler.step(optimizer)    skips on inf / NaN gradients        engine.py:89-91   -> ``skip_nonfinite``
    lr_scheduler.step()       after every iteration               engine.py:103-104 -> ``lr_schedule`` (a device table)
plus global gradient-norm clipping (``torch.nn.utils.clip_grad_norm_``; the reference does not clip).  The learning rate, the
AdamW bias corrections, the clip coefficient and the skip verdict then live in a control block on the device (``ops.grad_sumsq``
-> ``ops.optim_ctrl_update`` -> ``ops.sgd_step_ctrl`` / ``ops.adamw_step_ctrl``): no host sync, and a captured step advances its
schedule — and AdamW's ``t`` — across replays.

``ema_decay`` (device-held path too) keeps an exponential moving average of the parameters in a second flat buffer, updated by one
launch after the optimizer's that follows the control block (a skipped step leaves it alone; it is captured with the step);
``ema_weights()`` evaluates with it by exchanging the two buffers in place.  ``state_dict()`` / ``load_state_dict()`` hold
everything a step reads besides the model and the batch, so a stopped run continues bit for bit (``checkpoint.save_train_state``).

``accumulate=N`` (device-held path too) makes N calls one optimizer update with the exact large-batch mean: the reference calls
``optimizer.step()`` after every batch (engine.py:89-101) and has no counterpart; the cycle's denominator lives on the device.
"""
from __future__ import annotations

import contextlib
import math
import os
import re

import torch
from torch import nn

from . import ops
from .nn.base import HipModule, ParamArena


_DEFAULT_LR = 1e-5


def _accepts(model, keyword: str) -> bool:
    """Whether ``model.forward_loss`` takes ``keyword`` (a fused-head option the criterion or the step needs)."""
    import inspect
    fl = getattr(model, "forward_loss", None)
    return fl is not None and keyword in inspect.signature(fl).parameters


def _accepts_accum(model) -> bool:
    """``_accepts(model, "accum")`` under the name tests/test_accum_cpu.py imports at module level."""
    return _accepts(model, "accum")


def _n_classes(model) -> int | None:
    """Class count of a model's fused head: the prototypes' rows, or the prompts' (known only from a batch: None)."""
    protos = getattr(model, "class_prototypes", None)
    return None if protos is None else int(protos.shape[0])


def lr_table_from_torch(make_scheduler, base_lr: float, steps: int) -> torch.Tensor:
    """Tabulate a real ``torch.optim.lr_scheduler`` for ``TrainStep(lr_schedule=...)``: ``make_scheduler(optimizer)`` is run on a
    dummy CPU optimizer whose lr is ``base_lr``, and entry i is the rate in force at iteration i in ``Engine``'s order —
    ``optimizer.step()`` first, ``lr_scheduler.step()`` after (engine.py:101-104).  Returns an fp32 [steps] CPU tensor.
    Only ``param_groups[0]`` is tabulated: with ``TrainStep(param_groups=...)`` every group follows this one table times its constant
    ``lr_scale``, so per-group schedules that are not a common factor of one another (a non-zero ``eta_min``, per-group warm-ups)
    are not representable."""
    if steps < 1:
        raise ValueError("lr_table_from_torch: steps must be >= 1")
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = make_scheduler(opt)
    rates = []
    for i in range(steps):
        rates.append(opt.param_groups[0]["lr"])
        if i + 1 < steps:   # (the rate after the last iteration is never used; OneCycleLR refuses the step past its total)
            opt.step()
            sched.step()
    return torch.tensor(rates, dtype=torch.float64).to(torch.float32)


def _lr_table(lr_schedule, schedule_steps, lr) -> torch.Tensor:
    """The host-side fp32 table of a ``lr_schedule`` argument (validated; nothing touches the device)."""
    if lr_schedule is None:
        if schedule_steps is not None:
            raise ValueError("TrainStep: schedule_steps needs a callable lr_schedule")
        return torch.tensor([lr], dtype=torch.float64).to(torch.float32)
    if callable(lr_schedule):
        if schedule_steps is None or int(schedule_steps) < 1:
            raise ValueError("TrainStep: a callable lr_schedule needs schedule_steps=N >= 1 (the table is tabulated on the host)")
        table = torch.tensor([float(lr_schedule(i)) for i in range(int(schedule_steps))], dtype=torch.float64)
    else:
        if schedule_steps is not None:
            raise ValueError("TrainStep: schedule_steps goes with a callable lr_schedule, not with a table")
        table = torch.as_tensor(lr_schedule).detach().to("cpu", torch.float64)
        if table.dim() != 1:
            raise ValueError("TrainStep: lr_schedule must be a 1-D sequence or tensor of rates")
    if table.numel() == 0:
        raise ValueError("TrainStep: lr_schedule is empty")
    if not bool(torch.isfinite(table).all()) or bool((table < 0).any()):
        raise ValueError("TrainStep: lr_schedule must hold finite, non-negative rates")
    table = table.to(torch.float32)
    if lr != _DEFAULT_LR and torch.tensor(lr, dtype=torch.float64).to(torch.float32) != table[0]:
        raise ValueError(f"TrainStep: lr={lr} conflicts with lr_schedule, which starts at {float(table[0])}; give the rates "
                         "through lr_schedule alone")
    return table


_GROUP_KEYS = {"params", "lr_scale", "weight_decay"}
_MAX_GROUPS = ops.MAX_PARAM_GROUPS


def _resolve_param_groups(model: nn.Module, param_groups, weight_decay: float):
    """Validate a ``param_groups`` argument against ``model`` (host only; nothing is built).  Returns (groups, group_of) where
    groups is a list of dict(names, numel, lr_scale, weight_decay) — an implicit last group holding the parameters named in none —
    and group_of maps id(parameter) to its group index."""
    named, seen = [], set()
    for name, prm in model.named_parameters():
        if id(prm) not in seen:
            seen.add(id(prm))
            named.append((name, prm))
    by_name, name_of = dict(named), {id(prm): name for name, prm in named}
    if isinstance(param_groups, dict) or not hasattr(param_groups, "__iter__"):
        raise ValueError("TrainStep: param_groups must be a sequence of dicts")
    param_groups = list(param_groups)
    if not param_groups:
        raise ValueError("TrainStep: param_groups is empty (use None for no groups)")
    if len(param_groups) > _MAX_GROUPS:
        raise ValueError(f"TrainStep: {len(param_groups)} param_groups; more than {_MAX_GROUPS} groups are not supported")
    groups, group_of = [], {}
    for gi, g in enumerate(param_groups):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(f"TrainStep: param_groups[{gi}] must be a dict with a 'params' entry")
        unknown = set(g) - _GROUP_KEYS
        if unknown:
            raise ValueError(f"TrainStep: param_groups[{gi}] has unknown keys {sorted(unknown)} (known: {sorted(_GROUP_KEYS)})")
        lr_scale, wd = float(g.get("lr_scale", 1.0)), float(g.get("weight_decay", weight_decay))
        for key, val in (("lr_scale", lr_scale), ("weight_decay", wd)):
            if not math.isfinite(val) or val < 0.0:
                raise ValueError(f"TrainStep: param_groups[{gi}] {key} must be finite and >= 0, got {val}")
        members = g["params"]
        members = [members] if isinstance(members, (str, torch.Tensor)) else list(members)
        if not members:
            raise ValueError(f"TrainStep: param_groups[{gi}] has empty params")
        names = []
        for m in members:
            if isinstance(m, str):
                if m not in by_name:
                    raise ValueError(f"TrainStep: param_groups[{gi}]: '{m}' is not a parameter of the model")
                prm = by_name[m]
            elif isinstance(m, torch.Tensor) and id(m) in name_of:
                prm = m
            else:
                what = f"a tensor of shape {tuple(m.shape)}" if isinstance(m, torch.Tensor) else repr(m)
                raise ValueError(f"TrainStep: param_groups[{gi}]: {what} is not a parameter of the model")
            if id(prm) in group_of:
                raise ValueError(f"TrainStep: parameter '{name_of[id(prm)]}' is in two groups (param_groups[{group_of[id(prm)]}] "
                                 f"and param_groups[{gi}])" if group_of[id(prm)] != gi else
                                 f"TrainStep: parameter '{name_of[id(prm)]}' is listed twice in param_groups[{gi}]")
            group_of[id(prm)] = gi
            names.append(name_of[id(prm)])
        groups.append(dict(names=tuple(names), numel=sum(by_name[n].numel() for n in names), lr_scale=lr_scale, weight_decay=wd))
    rest = [name for name, prm in named if id(prm) not in group_of]
    if rest:
        if len(groups) + 1 > _MAX_GROUPS:
            raise ValueError(f"TrainStep: {len(groups)} param_groups plus the implicit group of the {len(rest)} parameters named in "
                             f"none; more than {_MAX_GROUPS} groups are not supported")
        for n in rest:
            group_of[id(by_name[n])] = len(groups)
        groups.append(dict(names=tuple(rest), numel=sum(by_name[n].numel() for n in rest), lr_scale=1.0,
                           weight_decay=float(weight_decay)))
    return groups, group_of


def _f32(x: float) -> float:
    """x rounded once to fp32, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


def ema_weight_at(j: int, decay: float, warmup: bool = False) -> float:
    """The host mirror of ``ops.ema_update_ctrl``'s weight for the j-th EMA update (1-based): fp32(1 - decay) with the difference
    formed in fp64, and under warm-up the larger of that and fp32(9 / (10 + j)) — TF's decay ``min(decay, (1 + j) / (10 + j))``."""
    w = _f32(1.0 - float(decay))
    return max(w, _f32(9.0 / (10.0 + int(j)))) if warmup else w


def _check_ema_args(ema_decay, ema_warmup, ema_every) -> None:
    if isinstance(ema_every, bool) or not isinstance(ema_every, int) or ema_every < 1:
        raise ValueError(f"TrainStep: ema_every must be an integer >= 1, got {ema_every!r}")
    if ema_decay is None:
        if ema_warmup or ema_every != 1:
            raise ValueError("TrainStep: ema_warmup / ema_every need ema_decay")
        return
    if not 0.0 <= float(ema_decay) < 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"TrainStep: ema_decay must satisfy 0 <= ema_decay < 1, got {ema_decay}")


def check_train_state(saved: dict, live: dict) -> None:
    """Compare the ``meta`` of a saved ``TrainStep.state_dict()`` with that of the live object (pure host function: dicts of
    strings, numbers and lists).  Raises ``ValueError`` naming the first difference; returns None when the state fits."""
    def fail(what):
        raise ValueError(f"TrainStep.load_state_dict: {what}")

    if saved.get("optimizer") != live["optimizer"]:
        fail(f"saved optimizer is '{saved.get('optimizer')}', this TrainStep runs '{live['optimizer']}'")
    se, le = saved.get("ema"), live["ema"]
    if se is not None and le is None:
        fail("EMA saved but not configured (give the TrainStep the run's ema_decay)")
    if se is None and le is not None:
        fail("EMA configured but not in the saved state")
    sh, lh = saved.get("hyper", {}), live["hyper"]
    for k in lh:
        if sh.get(k) != lh[k]:
            fail(f"optimizer hyper-parameter {k}: saved {sh.get(k)!r}, this TrainStep has {lh[k]!r}")
    if bool(saved.get("device_path")) != bool(live["device_path"]):
        fail("saved state is from the " + ("device-held" if saved.get("device_path") else "host-scalar") + " path, this TrainStep "
             "runs the " + ("device-held" if live["device_path"] else "host-scalar") + " one (lr_schedule / max_grad_norm / "
             "skip_nonfinite / device_state / param_groups / ema_decay select it)")
    sl, ll = saved.get("layout", {}), live["layout"]
    s_at = {n: (o, c) for n, o, c in zip(sl.get("names", []), sl.get("offsets", []), sl.get("numels", []))}
    for n, o, c in zip(ll["names"], ll["offsets"], ll["numels"]):
        if n not in s_at:
            fail(f"parameter '{n}' is missing from the saved state")
        if s_at[n][1] != c:
            fail(f"parameter '{n}' has {c} elements, the saved state {s_at[n][1]}")
        if s_at[n][0] != o:
            fail(f"parameter '{n}' lies at arena offset {o}, in the saved state at {s_at[n][0]}")
    extra = [n for n in sl.get("names", []) if n not in set(ll["names"])]
    if extra:
        fail(f"parameter '{extra[0]}' of the saved state is missing from the model")
    if sl.get("total") != ll["total"]:
        fail(f"arena of {ll['total']} elements, the saved state has {sl.get('total')}")
    sg, lg = saved.get("groups"), live["groups"]
    if (sg is None) != (lg is None):
        fail("param_groups " + ("saved but not configured" if lg is None else "configured but not in the saved state"))
    if lg is not None:
        if sg["table"] != lg["table"]:
            fail(f"another group recipe: saved (lr_scale, weight_decay) table {sg['table']}, this TrainStep has {lg['table']}")
        for n, a, b in zip(ll["names"], sg["ids"], lg["ids"]):
            if a != b:
                fail(f"another group assignment: parameter '{n}' was in group {a}, is in group {b}")
    st, lt = saved.get("lr_table"), live["lr_table"]
    if st != lt:
        if st is None or lt is None or len(st) != len(lt):
            fail(f"another lr table: saved {None if st is None else len(st)} entries, this TrainStep has "
                 f"{None if lt is None else len(lt)}")
        i = next(k for k, (a, b) in enumerate(zip(st, lt)) if a != b)
        fail(f"another lr table: entry {i} is {lt[i]!r}, saved {st[i]!r}")
    if saved.get("clip") != live["clip"]:
        fail(f"(max_grad_norm, skip_nonfinite) saved as {saved.get('clip')}, this TrainStep has {live['clip']}")
    if se != le:
        k = next(k for k in le if se.get(k) != le[k])
        fail(f"EMA setting {k}: saved {se.get(k)!r}, this TrainStep has {le[k]!r}")


_TOWER_LAYER = re.compile(r"^(.*)\.encoder\.layers\.(\d+)\.")


def make_param_groups(model: nn.Module, *, weight_decay: float, no_decay=True, lr_scales=None, layer_decay=None) -> list:
    """The usual fine-tuning recipes as a ``TrainStep(param_groups=...)`` list, from parameter NAMES alone (any nn.Module, no GPU).
      no_decay=True   every 1-D parameter (biases, LayerNorm gains / biases, class_embedding) and every parameter whose name ends
                      in position_embedding.weight or token_embedding.weight gets weight_decay 0; a tuple adds name substrings
                      (("class_prototypes",)); False decays everything
      lr_scales       {name prefix: factor}; the longest matching prefix wins, default 1
      layer_decay=d   in a tower whose names match <prefix>.encoder.layers.<i>. with L layers: layer i gets d ** (L - i), what
                      precedes the layers (<prefix>.embeddings.*, <prefix>.pre_layrnorm.*) d ** (L + 1), the rest of the tower 1,
                      multiplied into the prefix factor
    Parameters with the same (lr_scale, weight_decay) share a group."""
    extra = tuple(no_decay) if isinstance(no_decay, (tuple, list)) else ()
    lr_scales = dict(lr_scales or {})
    named, seen = [], set()
    for name, prm in model.named_parameters():
        if id(prm) not in seen:
            seen.add(id(prm))
            named.append((name, prm))
    depth = {}
    for name, _ in named:
        m = _TOWER_LAYER.match(name)
        if m:
            depth[m.group(1)] = max(depth.get(m.group(1), 0), int(m.group(2)) + 1)
    merged = {}
    for name, prm in named:
        wd = float(weight_decay)
        if no_decay and (prm.dim() == 1 or name.endswith(("position_embedding.weight", "token_embedding.weight"))
                         or any(sub in name for sub in extra)):
            wd = 0.0
        scale, best = 1.0, -1
        for prefix, f in lr_scales.items():
            if name.startswith(prefix) and len(prefix) > best:
                scale, best = float(f), len(prefix)
        if layer_decay is not None:
            m = _TOWER_LAYER.match(name)
            if m:
                scale *= float(layer_decay) ** (depth[m.group(1)] - int(m.group(2)))
            else:
                for tower, L in depth.items():
                    if name.startswith((tower + ".embeddings.", tower + ".pre_layrnorm.")):
                        scale *= float(layer_decay) ** (L + 1)
        merged.setdefault((scale, wd), []).append(name)
    return [dict(params=names, lr_scale=scale, weight_decay=wd) for (scale, wd), names in merged.items()]


class TrainStep:
    """``param_groups`` (keyword-only; selects the device-held path): a sequence of dicts ``{"params": parameters or their names in
    model.named_parameters(), "lr_scale": 1.0, "weight_decay": <TrainStep's weight_decay>}``.  Group g trains at
    ``fp32(lr_table[i]) * fp32(lr_scale_g)`` with its own decay, in ONE optimizer launch per step whatever the groups are; clipping
    stays global and ``skip_nonfinite`` all-or-nothing.  Parameters named in no group form an implicit last group (lr_scale 1,
    TrainStep's weight_decay) — unlike ``torch.optim``, which would not train them: a tower that must not move is
    ``requires_grad=False``, or a group with ``lr_scale`` 0 (which, like torch at lr = 0, still advances AdamW's moments and SGD's
    momentum buffer and leaves the parameter bits unchanged).  ``make_param_groups`` writes the usual recipes.

    ``ema_decay`` (keyword-only; selects the device-held path): ``ts.ema``, a flat fp32 buffer laid out like ``arena.flat`` and
    initialised from it, takes ``ema += (1 - ema_decay) * (p - ema)`` after every APPLIED optimizer update (every ``ema_every``-th
    one; with ``ema_warmup`` the j-th EMA update uses the decay ``min(ema_decay, (1 + j) / (10 + j))``).  One launch over the arena,
    captured with the step.  ``ema_state_dict()`` is the averaged model, ``with ts.ema_weights():`` evaluates with it in place,
    ``reset_ema()`` restarts it from the current parameters (after loading weights into the model).

    ``seg_metrics=True`` (keyword-only): every step also counts, on the device, how the argmax of the head's own upsampled scores
    meets the batch's labels (``forward_loss(seg_counts=)``: one more forward pass of the fused head, the logits are never formed;
    loss, gradients and parameters keep their bits).  ``ts.seg_counts`` is the running int64 [3, K] {intersection, predicted,
    labelled} buffer, ``ts.seg_metrics(reset=False)`` its ``metrics.dataset_iou``: ``aAcc`` (mmseg's ``acc_seg`` / 100), ``mAcc``,
    ``mIoU``, ``IoU`` [K] as device float64 tensors.  Under OHEM the counts are those of the labels before relabelling.  K is the
    model's ``class_prototypes`` row count, or ``seg_classes=`` for a model that takes its classes from the batch (PromptFTN).  The
    buffer exists before ``capture``; the captured launches keep adding into it across replays, and reading or resetting happens
    outside the graph (the warm-up steps of ``capture`` are real steps and count).  The counts are this rank's own (no collective)
    and are not part of ``state_dict`` / ``save_train_state``: a resumed run starts its counters at zero.

    ``accumulate=N`` (keyword-only; ``None`` or 1 is the plain step, bit for bit; N >= 2 selects the device-held path): N calls of
    ``step()`` are one CYCLE and one optimizer update with the gradient of the concatenated batch — (sum of the pixel losses of all
    N micro-batches) / (count of all their non-ignored pixels), not the mean of the micro-batch means, which would weight the pixels
    of sparsely labelled crops more heavily.  Calls 1..N-1 run forward and backward only (every gradient writer adds into the arena;
    the head leaves the gradient of the SUM); call N also takes the norm, advances the lr table and AdamW's t, clips, decides the
    non-finite skip, updates, runs the EMA launch and invalidates the bf16 shadows — all once per update.  The denominator is held
    on the device in fp64 across the cycle (``ops.accum_add``) and folded into the gradient scale by ``ops.optim_ctrl_update_accum``:
    no host sync.  It is the weighted count under class weights / label smoothing, the kept count under OHEM (selected per
    micro-batch), absent with ``reduction='sum'``; a cycle whose every pixel is ignored applies zero gradients at scale 1 and
    reports a NaN loss.  ``step()`` returns the micro-batch's own loss; ``ts.accum_loss`` / ``ts.accum_count`` are the last
    completed cycle's mean loss and denominator (device tensors), ``ts.micro`` the calls so far in the open cycle (host int),
    ``ts.flush()`` applies the update with the micro-batches seen so far.  ``last_grad_norm`` and the clip are those of the
    mean-scale gradient.  ``state_dict()`` / ``save_train_state`` raise while a cycle is open; the saved state does not depend on N.
    A ``DiceCrossEntropyLoss`` is refused (its batch statistics do not add).  Under a ``GradReducer`` calls 1..N-1 issue no
    collective, call N reduces under its backward and also sums the two fp64 sums over the ranks: for 'mean' the scale is
    1 / (sum over ranks and micro-batches of the count) with no extra 1/world — the GLOBAL-batch mean, which differs from the
    N = 1 behaviour (the mean of the ranks' means) when the ranks' counts differ; 'sum' keeps the 1/world of N = 1.  ``capture``
    then takes sequences of N inputs and N labels and records the whole cycle as one graph.
    ``distill=(weight, temperature, region)`` (keyword-only; ``None``: today's step, no new launch, no new keyword): every step adds
    weight * the mean per-pixel T^2 KL(teacher || student) of the upsampled scores to the criterion's loss
    (``forward_loss(distill=...)``); the teacher's low-resolution scores of the batch come with each call of the step's own
    entry, ``step_distill(inputs, labels, model.head_scores(view))`` — taken inside ``ema_weights()`` for a soft mean teacher, or
    another model's — with an optional ``teacher_weight=`` per pixel (``step`` and ``capture`` keep their parameter lists).  Eager,
    captured (``capture_distill``: static buffers), with ``seg_metrics=True`` and under a reducer; not with ``accumulate >= 2``
    (``NotImplementedError``: the term has its own denominator); a model whose ``forward_loss`` has no ``distill=`` is refused at
    construction (``TypeError``), and ``step`` / ``capture`` on such a TrainStep, which bring no teacher scores, with a ``ValueError``."""

    def __init__(self, model: nn.Module, *, optimizer: str = "sgd", lr: float = _DEFAULT_LR, momentum: float = 0.0,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, reducer=None,
                 ignore_index: int | None = None, criterion: nn.Module | None = None, lr_schedule=None,
                 schedule_steps: int | None = None, max_grad_norm: float | None = None, skip_nonfinite: bool = False,
                 device_state: bool = False, param_groups=None, ema_decay: float | None = None, ema_warmup: bool = False,
                 ema_every: int = 1, seg_metrics: bool = False, seg_classes: int | None = None,
                 accumulate: int | None = None, distill=None) -> None:
        # (argument checks first: nothing is built or allocated for a step that cannot run)
        _check_ema_args(ema_decay, ema_warmup, ema_every)
        if distill is not None:
            from .nn.head_loss import check_distill_options
            try:
                d_weight, d_temp, d_region = distill
            except (TypeError, ValueError):
                raise ValueError(f"TrainStep: distill must be (weight, temperature, region), got {distill!r}") from None
            distill = check_distill_options(d_weight, d_temp, d_region)
            if accumulate not in (None, 1):
                raise NotImplementedError("TrainStep: distill cannot be combined with accumulate >= 2 (the distillation term has its "
                                          "own denominator and the accumulation block carries one)")
            if not _accepts(model, "distill"):
                raise TypeError("TrainStep: distill needs a model whose forward_loss takes distill= (BaseModelWithText, PromptFTN)")
        self._distill = distill
        if accumulate is not None and (isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1):
            raise ValueError(f"TrainStep: accumulate must be None or an integer >= 1, got {accumulate!r}")
        accum_n = None if accumulate in (None, 1) else int(accumulate)   # None: today's step, no new launch, no new keyword
        if accum_n is not None:
            from .nn.loss import DiceCrossEntropyLoss as _Dice
            if isinstance(criterion, _Dice):
                raise ValueError("TrainStep: a DiceCrossEntropyLoss cannot be trained with accumulate >= 2: its batch statistics "
                                 "do not add across micro-batches")
            if not _accepts(model, "accum"):
                raise TypeError("TrainStep: accumulate >= 2 needs a model whose forward_loss takes accum= "
                                "(BaseModelWithText, PromptFTN)")
        if not isinstance(seg_metrics, bool):
            raise TypeError(f"TrainStep: seg_metrics must be a bool, got {seg_metrics!r}")
        n_seg = None
        if seg_metrics:
            if not _accepts(model, "seg_counts"):
                raise TypeError("TrainStep: seg_metrics=True needs a model whose forward_loss takes seg_counts= "
                                "(BaseModelWithText, PromptFTN)")
            n_seg = _n_classes(model) if seg_classes is None else seg_classes
            if isinstance(n_seg, bool) or not isinstance(n_seg, int) or not 1 <= n_seg <= 1024:
                raise ValueError("TrainStep: seg_metrics=True needs the class count of the fused head, 1..1024: the model's "
                                 f"class_prototypes rows, or seg_classes= for a model without them (got {seg_classes!r})")
            if _n_classes(model) not in (None, n_seg):   # the head counts the model's own classes: a [3, K] buffer of another K is refused
                raise ValueError(f"TrainStep: seg_classes={seg_classes!r} does not match the model's {_n_classes(model)} "
                                 "class_prototypes rows")
        elif seg_classes is not None:
            raise ValueError("TrainStep: seg_classes is only meaningful with seg_metrics=True")
        device_path = bool(device_state or skip_nonfinite or lr_schedule is not None or max_grad_norm is not None
                           or param_groups is not None or ema_decay is not None or accum_n is not None)
        groups = None
        if param_groups is not None:
            groups, group_of = _resolve_param_groups(model, param_groups, weight_decay)
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"TrainStep: max_grad_norm must be > 0 (or None / inf for no clipping), got {max_grad_norm}")
        table = _lr_table(lr_schedule, schedule_steps, lr) if (device_path or schedule_steps is not None) else None
        self._loss_opts = False
        self._ohem = False
        self._dice = False
        if criterion is not None:
            from .nn.loss import (AuxiliaryLoss, CrossEntropyLoss, DiceCrossEntropyLoss, FocalLoss, OhemCrossEntropyLoss,
                                  SigmoidFocalLoss)
            if not isinstance(criterion, (CrossEntropyLoss, nn.CrossEntropyLoss)) or isinstance(criterion, AuxiliaryLoss):
                raise TypeError("TrainStep: criterion must be a CrossEntropyLoss (lc2is_amd.nn or torch.nn)")
            if ignore_index is not None and ignore_index != -100:
                raise ValueError("TrainStep: give ignore_index through the criterion, not as a TrainStep argument too")
            if criterion.reduction == "none":
                raise ValueError("TrainStep: a training step needs a scalar loss; criterion reduction='none' cannot train")
            ignore_index = criterion.ignore_index
            self._loss_opts = (criterion.weight is not None or criterion.label_smoothing != 0.0
                               or criterion.reduction != "mean")
            self._ohem = isinstance(criterion, OhemCrossEntropyLoss)
            if self._ohem and not _accepts(model, "ohem"):
                raise TypeError("TrainStep: an OhemCrossEntropyLoss needs a model whose forward_loss takes ohem= "
                                "(BaseModelWithText); the compose models do not select hard pixels")
            self._dice = isinstance(criterion, DiceCrossEntropyLoss)
            if self._dice and not _accepts(model, "dice"):
                raise TypeError("TrainStep: a DiceCrossEntropyLoss needs a model whose forward_loss takes dice= "
                                "(BaseModelWithText); the compose models have no Dice head")
            if isinstance(criterion, FocalLoss):   # rides the options call: weight=, reduction= and focal=(gamma, poly_eps)
                if not _accepts(model, "focal"):
                    raise TypeError("TrainStep: a FocalLoss / Poly1CrossEntropyLoss needs a model whose forward_loss takes focal= "
                                    "(BaseModelWithText, PromptFTN)")
                self._loss_opts = True
            if isinstance(criterion, SigmoidFocalLoss):   # rides the options call too: weight=, reduction= and sigmoid=(gamma, alpha, normalize)
                if not _accepts(model, "sigmoid"):
                    raise TypeError("TrainStep: a SigmoidFocalLoss / SigmoidCrossEntropyLoss needs a model whose forward_loss takes "
                                    "sigmoid= (BaseModelWithText, PromptFTN)")
                self._loss_opts = True
        self.criterion = criterion
        self.model = model
        self.arena = ParamArena(model)
        self.kind = optimizer.lower()
        if self.kind not in ("sgd", "adamw"):
            raise ValueError("TrainStep: optimizer must be 'sgd' or 'adamw'")
        self.lr, self.momentum, self.weight_decay, self.betas, self.eps = lr, momentum, weight_decay, betas, eps
        dev = self.arena.flat.device
        self.mom = torch.zeros_like(self.arena.flat) if (self.kind == "sgd" and momentum != 0.0) else None
        if self.kind == "adamw":
            self.m, self.v = torch.zeros_like(self.arena.flat), torch.zeros_like(self.arena.flat)
        self.t = 0
        self.reducer = reducer
        self.ignore_index = -100 if ignore_index is None else ignore_index
        self._hip_modules = [m for m in model.modules() if isinstance(m, HipModule)]
        if reducer is not None:
            reducer.attach(model, self.arena)
        self._dev = dev
        # the device-held path: control block (lc2is_optim_ctrl) + lr table on the device; None = today's path, untouched
        self._ctrl = None
        if device_path:
            self._ctrl = torch.zeros(ops.OPTIM_CTRL_WORDS, dtype=torch.int32, device=dev)
            self._ctrl_f = self._ctrl.view(torch.float32)
            self.lr_table = table.to(dev)
            self.max_grad_norm = float("inf") if max_grad_norm is None else float(max_grad_norm)
            self.skip_nonfinite = bool(skip_nonfinite)
            self.reverse_walk = False   # the _ctrl optimizer walks the arena from its end (same bits): tools/optim_ctrl_cost.py's A/B
        # parameter groups: the constants in a small device table, the granule map in the arena (rebuilt when the dead set changes)
        self._groups = groups
        if groups is not None:
            self.arena.set_groups([group_of[id(p)] for p in self.arena.params], len(groups))
            self._group_table = torch.tensor([[g["lr_scale"], g["weight_decay"]] for g in groups], dtype=torch.float32).to(dev)
        # weight EMA: a second arena-shaped buffer; None = no launch is added to the step
        self.ema, self._ema_swapped = None, False
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup, self.ema_every = bool(ema_warmup), int(ema_every)
        if ema_decay is not None:
            self._ema_w = 1.0 - self.ema_decay   # fp64 here; rounded to fp32 once, at the C boundary
            # walk the arena from its end (the same bits): the optimizer has just finished there, so the tail of p is the part
            # still cache-warm; 401 against 415 us per launch, faster in both repetitions of profiles/ema_cost.txt
            self.ema_reverse_walk = True
            self.ema = self.arena.flat.clone()
        # accuracy / IoU counts of the training batches: None = forward_loss gets no seg_counts=, no launch is added
        self._seg_counts = torch.zeros((3, n_seg), dtype=torch.int64, device=dev) if seg_metrics else None
        # gradient accumulation: the cycle's fp64 loss sum and denominator in a device block (lc2is_accum_block); None = no launch
        self._accum_n, self.micro, self._accum = accum_n, 0, None
        if accum_n is not None:
            self._accum = torch.zeros(ops.ACCUM_BLOCK_BYTES // 8, dtype=torch.float64, device=dev)
            self._accum_f = self._accum.view(torch.float32)
            reduction = "mean" if criterion is None else criterion.reduction
            self._accum_use_denom = reduction != "sum"

    # -- views of the control block: device tensors, no sync unless the caller asks (.item()) --------------------------------
    def _ctrl_view(self, word: int, as_float: bool) -> torch.Tensor:
        if self._ctrl is None:
            raise RuntimeError("TrainStep: this accessor needs the device-held path (lr_schedule / max_grad_norm / "
                               "skip_nonfinite / device_state=True)")
        return (self._ctrl_f if as_float else self._ctrl)[word]

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the last step's gradient (after the 1/world scaling, before clipping)."""
        return self._ctrl_view(ops.CTRL_GRAD_NORM, True)

    @property
    def last_clip_coef(self) -> torch.Tensor:
        return self._ctrl_view(ops.CTRL_CLIP_COEF, True)

    @property
    def last_lr(self) -> torch.Tensor:
        return self._ctrl_view(ops.CTRL_LR, True)

    @property
    def skipped_steps(self) -> torch.Tensor:
        return self._ctrl_view(ops.CTRL_SKIPPED, False)

    @property
    def applied_steps(self) -> torch.Tensor:
        return self._ctrl_view(ops.CTRL_APPLIED, False)

    @property
    def ohem_info(self):
        """The device info block (n_valid, k, L, L_eff: ``ops.ohem_info_fields``) of the last step's hard-pixel selection, None
        before the first step; ``ohem_labels`` are the labels the head saw.  After ``capture`` both are the graph's own buffers:
        a replay rewrites them in place."""
        if not self._ohem:
            raise RuntimeError("TrainStep.ohem_info: the criterion is not an OhemCrossEntropyLoss")
        return self.criterion.last_info

    @property
    def ohem_labels(self):
        if not self._ohem:
            raise RuntimeError("TrainStep.ohem_labels: the criterion is not an OhemCrossEntropyLoss")
        return self.criterion.last_labels

    @property
    def dice_stats(self):
        """The device tensors (I, P, T, loss block = [loss, CE mean, Dice, n_valid]) of the last step's Dice + CE loss, None before
        the first step.  After ``capture`` they are the graph's own buffers: a replay rewrites them in place."""
        if not self._dice:
            raise RuntimeError("TrainStep.dice_stats: the criterion is not a DiceCrossEntropyLoss")
        return self.criterion.last_stats

    @property
    def seg_counts(self) -> torch.Tensor:
        """The running int64 [3, K] {intersection, predicted, labelled} counts of the steps so far (the buffer itself: the steps,
        captured ones included, add into it in place)."""
        if self._seg_counts is None:
            raise RuntimeError("TrainStep.seg_counts: this TrainStep counts nothing (seg_metrics=False)")
        return self._seg_counts

    def seg_metrics(self, reset: bool = False) -> dict:
        """``metrics.dataset_iou`` of ``seg_counts``: ``aAcc``, ``mAcc``, ``mIoU`` and ``IoU`` [K] as float64 tensors on the device
        (nothing is read to the host).  The ignored class takes part in none of them when ``0 <= ignore_index < K`` (pixels
        predicted as it would drag the means).  ``reset=True`` zeroes the buffer in place after reading.  Call it outside a graph
        capture."""
        from .metrics import dataset_iou
        counts = self.seg_counts
        K = counts.shape[1]
        out = dataset_iou(counts, self.ignore_index if 0 <= self.ignore_index < K else None)
        if reset:
            counts.zero_()
        return out

    def _need_accum(self, what: str) -> None:
        if self._accum is None:
            raise RuntimeError(f"TrainStep.{what}: this TrainStep does not accumulate (accumulate=None or 1)")

    @property
    def accum_loss(self) -> torch.Tensor:
        """The last completed cycle's loss on the device: (sum of the pixel losses of all its micro-batches) / ``accum_count`` —
        the concatenated batch's mean, NaN when every pixel was ignored; with ``reduction='sum'`` the sum."""
        self._need_accum("accum_loss")
        return self._accum_f[ops.ACCUM_LAST_LOSS]

    @property
    def accum_count(self) -> torch.Tensor:
        """The last completed cycle's denominator (device fp32): the count of its non-ignored pixels — the weighted count under
        class weights, the kept count under OHEM, summed over the ranks under a reducer."""
        self._need_accum("accum_count")
        return self._accum_f[ops.ACCUM_LAST_DENOM]

    @property
    def param_groups(self):
        """Per group: parameter names, element count, lr_scale, weight_decay (the implicit group last); None without groups."""
        return None if self._groups is None else tuple(dict(g) for g in self._groups)

    # -- weight EMA --------------------------------------------------------------------------------------------------------
    def _need_ema(self, what: str) -> None:
        if self.ema is None:
            raise RuntimeError(f"TrainStep.{what}: this TrainStep keeps no EMA (ema_decay=None)")

    def reset_ema(self) -> None:
        """Restart the EMA from the current parameters (after weights were loaded into the model)."""
        self._need_ema("reset_ema")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.reset_ema: not inside ema_weights()")
        self.ema.copy_(self.arena.flat)

    def ema_state_dict(self) -> dict:
        """``model.state_dict()``'s keys and shapes on the CPU, parameters taken from the EMA buffer and buffers from the model:
        loads with ``strict=True`` into a fresh drop-in model, or into the reference."""
        self._need_ema("ema_state_dict")
        avg = self.arena.flat if self._ema_swapped else self.ema   # inside ema_weights() the two have changed places
        params = dict(self.model.named_parameters(remove_duplicate=False))
        out = {}
        for k, v in self.model.state_dict().items():
            r = self.arena.ranges.get(id(params[k])) if k in params else None
            out[k] = (v.detach() if r is None else avg[r[0]:r[1]].view(v.shape)).to("cpu", copy=True)
        return out

    def _exchange_ema(self) -> None:
        ops.swap_f32(self.arena.flat, self.ema)
        for m in self._hip_modules:
            m.invalidate_shadows()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model's parameters ARE the EMA: ``arena.flat`` and ``ts.ema`` exchange their contents in place (one
        launch, no host sync, nothing allocated; every parameter view and every captured pointer stays valid) and the bf16 weight
        shadows are rebuilt on the next forward.  On exit — also when the body raises — they change back.  ``step()`` and a
        captured replay raise inside the block; so does entering it twice."""
        self._need_ema("ema_weights")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.ema_weights: already inside ema_weights()")
        self._exchange_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._exchange_ema()
            self._ema_swapped = False

    # -- everything a step reads besides the model and the batch ---------------------------------------------------------------
    def _state_meta(self) -> dict:
        arena = self.arena
        name_of = {}
        for name, prm in self.model.named_parameters():
            name_of.setdefault(id(prm), name)
        hyper = dict(lr=float(self.lr), momentum=float(self.momentum), weight_decay=float(self.weight_decay),
                     betas=[float(b) for b in self.betas], eps=float(self.eps))
        meta = dict(optimizer=self.kind, hyper=hyper, device_path=self._ctrl is not None,
                    layout=dict(names=[name_of[id(p)] for p in arena.params], offsets=[int(o) for o in arena.offsets],
                                numels=[int(p.numel()) for p in arena.params], total=int(arena.numel)),
                    groups=None, lr_table=None, clip=None, ema=None)
        if self._ctrl is not None:
            meta["lr_table"] = [float(x) for x in self.lr_table.cpu().tolist()]
            meta["clip"] = [float(self.max_grad_norm), bool(self.skip_nonfinite)]
        if self._groups is not None:
            meta["groups"] = dict(table=[[_f32(g["lr_scale"]), _f32(g["weight_decay"])] for g in self._groups],
                                  ids=[int(g) for g in arena._group_ids])
        if self.ema is not None:
            meta["ema"] = dict(decay=self.ema_decay, warmup=self.ema_warmup, every=self.ema_every)
        return meta

    def _state_buffers(self) -> dict:
        bufs = {}
        if self.mom is not None:
            bufs["mom"] = self.mom
        if self.kind == "adamw":
            bufs["m"], bufs["v"] = self.m, self.v
        if self._ctrl is not None:
            bufs["ctrl"] = self._ctrl
        if self.ema is not None:
            bufs["ema"] = self.ema
        return bufs

    def state_dict(self) -> dict:
        """Optimizer kind and hyper-parameters, ``t``, the momentum buffer or AdamW's moments, the control block and lr table, the
        group table and ids, the EMA and its settings, and the arena's layout (names, offsets, sizes).  CPU tensors, numbers,
        strings, lists and dicts only: the file loads with ``torch.load(weights_only=True)``."""
        if self._ema_swapped:
            raise RuntimeError("TrainStep.state_dict: not inside ema_weights()")
        if self.micro != 0:
            raise RuntimeError(f"TrainStep.state_dict: an accumulation cycle is open ({self.micro} of {self._accum_n} micro-batches); "
                               "a checkpoint is taken at an update boundary (finish the cycle or flush())")
        sd = {"format": 1, "meta": self._state_meta(), "t": int(self.t)}
        for k, b in self._state_buffers().items():
            sd[k] = b.detach().to("cpu", copy=True)
        if self._ctrl is not None:
            sd["lr_table"] = self.lr_table.detach().to("cpu", copy=True)
        if self._groups is not None:
            sd["group_table"] = self._group_table.detach().to("cpu", copy=True)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Check ``sd`` against this object (``check_train_state``: ValueError naming the first difference, nothing changed), then
        copy IN PLACE into the existing device buffers: no pointer changes, a step captured before the load stays valid."""
        if self._ema_swapped:
            raise RuntimeError("TrainStep.load_state_dict: not inside ema_weights()")
        if self.micro != 0:
            raise RuntimeError("TrainStep.load_state_dict: an accumulation cycle is open; a state is loaded at an update boundary "
                               "(finish the cycle or flush())")
        if not isinstance(sd, dict) or "meta" not in sd or "t" not in sd:
            raise ValueError("TrainStep.load_state_dict: not a TrainStep.state_dict()")
        check_train_state(sd["meta"], self._state_meta())
        bufs = self._state_buffers()
        for k, b in bufs.items():
            src = sd.get(k)
            if not isinstance(src, torch.Tensor) or src.dtype != b.dtype or src.shape != b.shape:
                raise ValueError(f"TrainStep.load_state_dict: '{k}' must be a {b.dtype} tensor of shape {tuple(b.shape)}")
        for k, b in bufs.items():
            b.copy_(sd[k])
        self.t = int(sd["t"])

    def _check_pixel_weight(self, who: str) -> None:
        """A per-pixel loss weight needs a model that takes it and a criterion it combines with: refused before anything runs."""
        if not _accepts(self.model, "pixel_weight"):
            raise TypeError(f"TrainStep.{who}: pixel_weight needs a model whose forward_loss takes pixel_weight= "
                            "(BaseModelWithText, PromptFTN)")
        c = self.criterion
        if self._ohem or self._dice or getattr(c, "focal", None) is not None or getattr(c, "sigmoid", None) is not None:
            raise ValueError(f"TrainStep.{who}: pixel_weight weights the cross-entropy (weight, label_smoothing, reduction); it cannot "
                             "be combined with an OHEM, Dice, focal or sigmoid criterion")

    def _check_teacher(self, who: str, teacher_scores, teacher_weight) -> None:
        """The per-step tensors of the distillation term against how the TrainStep was built: refused before anything runs."""
        if getattr(self, "_distill", None) is None:
            if teacher_scores is not None or teacher_weight is not None:
                raise ValueError(f"TrainStep.{who}: teacher_scores / teacher_weight need a TrainStep built with "
                                 "distill=(weight, temperature, region)")
        elif teacher_scores is None:
            raise ValueError(f"TrainStep.{who}: this TrainStep was built with distill=: every step needs teacher_scores — "
                             "step_distill(inputs, labels, teacher_scores) / capture_distill(...), the teacher's "
                             "model.head_scores(inputs), e.g. under ema_weights()")

    def step(self, inputs: dict, labels: torch.Tensor, pixel_weight: torch.Tensor | None = None) -> torch.Tensor:
        """One training step (with ``accumulate=N``: one micro-batch of a cycle).  ``pixel_weight``: a contiguous fp32 device tensor
        of the labels' shape, finite and >= 0, that multiplies each counted pixel's cross-entropy and not its count — the mean, the
        accumulation block, a reducer's global count and the seg counts stay those of the unweighted step (``forward_loss``);
        None: no weight, the keyword is not passed.  A TrainStep built with ``distill=`` steps through ``step_distill``."""
        return TrainStep._step(self, inputs, labels, pixel_weight, None, None)   # (through the class: a stand-in object has no methods)

    def step_distill(self, inputs: dict, labels: torch.Tensor, teacher_scores: torch.Tensor, teacher_weight: torch.Tensor | None = None,
                     pixel_weight: torch.Tensor | None = None) -> torch.Tensor:
        """One training step of a ``TrainStep(distill=(weight, temperature, region))``: ``step`` with the teacher's low-resolution
        scores of this batch, fp32 [B*g*g, class_pad(K)], no grad — ``model.head_scores(inputs)`` inside ``ema_weights()`` or of
        another model.  The loss is the criterion's plus weight * the mean per-pixel T^2 KL to them (``forward_loss(distill=...)``).
        ``teacher_weight``: an optional fp32 tensor of the labels' shape on each pixel's KL."""
        return self._step(inputs, labels, pixel_weight, teacher_scores, teacher_weight)

    def _step(self, inputs, labels, pixel_weight, teacher_scores, teacher_weight):
        if self._ema_swapped:
            raise RuntimeError("TrainStep.step: inside ema_weights() the parameters are the EMA; leave the block before training")
        if pixel_weight is not None:
            TrainStep._check_pixel_weight(self, "step")
        TrainStep._check_teacher(self, "step", teacher_scores, teacher_weight)
        arena = self.arena
        # accumulate=N: N calls are one cycle.  The first overwrites the gradients, the later ones find p.grad set, so every writer
        # accumulates; only the last finalizes, reduces, updates and invalidates the shadows.
        last = self._accum_n is None or self.micro + 1 == self._accum_n
        if self.micro == 0:
            arena.zero_grad(set_to_none=True)
        if self.reducer is not None:
            if self._accum_n is None:
                self.reducer.begin_step()
            else:
                self.reducer.begin_step(sync=last)
        # the keywords of the fused head, from the criterion as it is now (its weight buffer: criterion.to(device) replaces it; no
        # host sync).  Only what is set is passed: a model's forward_loss need not know the options this step does not use.
        kw = {}
        ohem = dice = False
        if self._ohem or self._dice or self._loss_opts:
            c = self.criterion
            ohem = self._ohem and c.training   # the selection applies while the criterion is in training mode (as its forward)
            dice = self._dice and not self._ohem   # CE + soft Dice (deterministic: the training flag does not matter)
            if dice:
                kw["dice"] = c.dice
            else:
                kw.update(weight=c.weight, label_smoothing=float(c.label_smoothing), reduction=c.reduction)
                if self._ohem:
                    kw["ohem"] = c.ohem if ohem else None
                else:   # a FocalLoss / Poly1CrossEntropyLoss has .focal, a SigmoidFocalLoss / SigmoidCrossEntropyLoss .sigmoid
                    kw.update({k: getattr(c, k) for k in ("focal", "sigmoid") if getattr(c, k, None) is not None})
        if self._seg_counts is not None:
            kw["seg_counts"] = self._seg_counts
        if self._accum is not None:
            kw["accum"] = self._accum
        if pixel_weight is not None:
            kw["pixel_weight"] = pixel_weight
        if getattr(self, "_distill", None) is not None:
            from .nn.head_loss import Distill
            kw["distill"] = Distill(teacher_scores, *self._distill, teacher_weight)
        loss = self.model.forward_loss(inputs, labels, self.ignore_index, **kw)
        if ohem:
            c.last_labels, c.last_info = self.model.last_ohem
        if dice:
            c.last_stats = self.model.last_dice
        loss.backward()
        if not last:   # inside a cycle: nothing but the gradient arena, the accumulation block and the metric counts has moved
            self.micro += 1
            return loss.detach()
        self._apply_update()
        return loss.detach()

    def flush(self) -> None:
        """Apply the update with the micro-batches seen so far (a ragged end of an epoch): the denominator is that of those
        micro-batches, so the update is the exact mean over them.  Does nothing when no cycle is open (``micro == 0``).  Under a
        reducer every rank calls it at the same point: the arena is reduced here, no collective ran under a backward."""
        if self.micro == 0:
            return
        if self._ema_swapped:
            raise RuntimeError("TrainStep.flush: inside ema_weights() the parameters are the EMA; leave the block before training")
        self._apply_update()

    def _apply_update(self) -> None:
        """Everything that happens once per optimizer update: finalize, reduce, norm, control block, optimizer, EMA, shadows."""
        arena = self.arena
        live = arena.finalize_grads()
        gscale = 1.0
        if self.reducer is not None:
            if self._accum is not None:   # the two fp64 sums travel with the gradients: every rank divides by the global count
                self.reducer.reduce_block(self._accum[:2])
            self.reducer.finish_step()
            # 'mean' under accumulation: 1 / (sum over ranks and micro-batches of the count) is the whole scale, no extra 1/world
            if self._accum is None or not self._accum_use_denom:
                gscale = 1.0 / self.reducer.world_size
        self.t += 1
        self.micro = 0
        # One fused launch over the whole arena; a zero gradient leaves a parameter untouched unless weight decay is on —
        # then, like torch.optim (which skips parameters whose grad is None), only the live segments are updated so that
        # frozen / unreached parameters stay bit-identical.
        segs = [(0, arena.numel)] if (self.weight_decay == 0.0 or live == [(0, arena.numel)]) else live
        if self._ctrl is not None:
            # Pass 1 runs over the WHOLE arena: finalize_grads has zeroed the segments that got no gradient and the alignment
            # padding is never written (zero since allocation), so the sum is clip_grad_norm_'s over the parameters that have
            # a gradient.  Under a reducer every rank runs these deterministic kernels on the same all-reduced bytes with the
            # same 1/world: all ranks reach the same clip and skip decision without another collective.
            ctrl = self._ctrl
            b1, b2 = self.betas if self.kind == "adamw" else (0.0, 0.0)
            partials, flags = ops.grad_sumsq(arena.grad)
            if self._accum is None:
                ops.optim_ctrl_update(ctrl, partials, flags, self.lr_table, grad_scale=gscale, max_norm=self.max_grad_norm,
                                      skip_nonfinite=self.skip_nonfinite, beta1=b1, beta2=b2)
            else:   # the arena holds the cycle's SUM: the scale becomes gscale / (the cycle's denominator), in fp64 on the device
                ops.optim_ctrl_update_accum(ctrl, self._accum, self._accum_use_denom, partials, flags, self.lr_table,
                                            grad_scale=gscale, max_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite,
                                            beta1=b1, beta2=b2)
            if self._groups is not None:
                # one launch over the whole arena: parameters without a gradient carry the skip id in the map
                gmap = arena.group_map()
                if self.kind == "sgd":
                    ops.sgd_step_groups(arena.flat, arena.grad, self.mom, ctrl, gmap, self._group_table, self.momentum,
                                        reverse=self.reverse_walk)
                else:
                    ops.adamw_step_groups(arena.flat, arena.grad, self.m, self.v, ctrl, gmap, self._group_table, self.betas[0],
                                          self.betas[1], self.eps, reverse=self.reverse_walk)
                segs = []
            for lo, hi in segs:
                sl = slice(lo, hi)
                if self.kind == "sgd":
                    ops.sgd_step_ctrl(arena.flat[sl], arena.grad[sl], None if self.mom is None else self.mom[sl], ctrl,
                                      self.momentum, self.weight_decay, reverse=self.reverse_walk)
                else:
                    ops.adamw_step_ctrl(arena.flat[sl], arena.grad[sl], self.m[sl], self.v[sl], ctrl, self.betas[0],
                                        self.betas[1], self.eps, self.weight_decay, reverse=self.reverse_walk)
            segs = []
        for lo, hi in segs:
            sl = slice(lo, hi)
            if self.kind == "sgd":
                ops.sgd_step(arena.flat[sl], arena.grad[sl], None if self.mom is None else self.mom[sl], self.lr,
                             self.momentum, self.weight_decay, gscale)
            else:
                ops.adamw_step(arena.flat[sl], arena.grad[sl], self.m[sl], self.v[sl], self.lr, self.betas[0],
                               self.betas[1], self.eps, self.weight_decay, self.t, gscale)
        if self.ema is not None:   # after the optimizer: reads the verdict and the counter this step's optim_ctrl_update wrote
            ops.ema_update_ctrl(self.ema, arena.flat, self._ctrl, self._ema_w, warmup=self.ema_warmup, every=self.ema_every,
                                reverse=self.ema_reverse_walk)
        for m in self._hip_modules:
            m.invalidate_shadows()

    # -- HIP graph replay ------------------------------------------------------------------------------------
    def capture(self, inputs: dict, labels: torch.Tensor, warmup: int = 2, pixel_weight=None):
        """Capture one full step (shadow refresh -> forward -> CE -> backward -> optimizer) into a hipGraph over
        static copies of the batch; returns ``replay(inputs, labels) -> loss`` which copies the new batch into the
        static buffers and launches the graph (one host call per step instead of ~800 kernel launches).  ``warmup`` REAL
        steps on ``inputs`` run before the capture (lazy initialisation must not happen inside it); the captured step itself
        is only recorded.
        On the device-held path the learning-rate table index, AdamW's t and the skip counters are device state that the
        captured kernels advance: a schedule moves across replays and AdamW can be captured; so is the EMA launch.
        Single-process only (the RCCL reduction is not captured).
        With ``accumulate=N`` both arguments are sequences of N batches: the whole cycle (N forward / backward passes and the one
        update) is recorded as ONE graph over N static copies, a warm-up step is a whole cycle, and ``replay`` takes the same two
        sequences and returns the tuple of the N micro-batch losses.
        ``pixel_weight`` (with ``accumulate=N``: a sequence of N): the step is captured with a per-pixel loss weight held in a
        static buffer, and ``replay`` takes the new weight as its third argument, ``replay(inputs, labels, pixel_weight)``.
        A TrainStep built with ``distill=`` captures through ``capture_distill``."""
        return self._capture(inputs, labels, warmup, pixel_weight, None, None)

    def capture_distill(self, inputs: dict, labels: torch.Tensor, teacher_scores: torch.Tensor, teacher_weight=None, warmup: int = 2,
                        pixel_weight=None):
        """``capture`` for a TrainStep built with ``distill=``: the teacher's scores (and weight) are held in static buffers as the
        pixel weight is; ``replay(inputs, labels, teacher_scores=..., teacher_weight=...)`` copies the new ones in, and a replay that
        omits what the capture had (or gives what it had not) is refused.  ``replay.static_teacher_scores`` /
        ``static_teacher_weight``."""
        return self._capture(inputs, labels, warmup, pixel_weight, teacher_scores, teacher_weight)

    def _capture(self, inputs, labels, warmup, pixel_weight, teacher_scores, teacher_weight):
        n_micro = self._accum_n or 1
        if pixel_weight is not None:
            self._check_pixel_weight("capture")
        self._check_teacher("capture", teacher_scores, teacher_weight)
        if self._accum_n is not None:
            if isinstance(inputs, dict) or isinstance(labels, torch.Tensor) or len(inputs) != n_micro or len(labels) != n_micro:
                raise ValueError(f"TrainStep.capture: with accumulate={n_micro} give sequences of {n_micro} inputs and {n_micro} labels")
            if self.micro != 0:
                raise RuntimeError("TrainStep.capture: an accumulation cycle is open; finish it or flush() first")
            many_in, many_lb = list(inputs), list(labels)
            if pixel_weight is not None and (isinstance(pixel_weight, torch.Tensor) or len(pixel_weight) != n_micro):
                raise ValueError(f"TrainStep.capture: with accumulate={n_micro} give a sequence of {n_micro} pixel weights")
            many_pw = None if pixel_weight is None else list(pixel_weight)
        else:
            many_in, many_lb = [inputs], [labels]
            many_pw = None if pixel_weight is None else [pixel_weight]
        if self.reducer is not None:
            raise RuntimeError("TrainStep.capture: graph capture is only wired for single-GPU steps")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.capture: inside ema_weights() the parameters are the EMA; leave the block before training")
        if self.kind == "adamw" and self._ctrl is None:   # (checked BEFORE anything runs or is captured)
            raise RuntimeError("TrainStep.capture: AdamW bias correction is step-dependent; capture supports SGD")
        if hasattr(self.model, "overlap_text") and os.environ.get("LC2IS_GRAPH_OVERLAP", "1") == "0":
            self.model.overlap_text = False   # LC2IS_GRAPH_OVERLAP=0: one captured stream (default: the text-tower fork / join is captured too)
        from .nn.base import DropoutRng
        DropoutRng.last.clear()
        static_ins = [{k: v.clone() for k, v in d.items()} for d in many_in]
        static_lbs = [lb.clone() for lb in many_lb]
        static_in, static_lb = static_ins[0], static_lbs[0]
        static_pws = None if many_pw is None else [pw.clone() for pw in many_pw]
        static_ts = None if teacher_scores is None else teacher_scores.clone()   # (distill= excludes accumulate: one micro-batch)
        static_tw = None if teacher_weight is None else teacher_weight.clone()

        def cycle():
            if static_ts is not None:
                return [self._step(static_in, static_lb, None if static_pws is None else static_pws[0], static_ts, static_tw)]
            if static_pws is None:
                return [self.step(d, lb) for d, lb in zip(static_ins, static_lbs)]
            return [self.step(d, lb, pw) for d, lb, pw in zip(static_ins, static_lbs, static_pws)]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # warm-up on the capture stream: lazy inits, workspaces, attributes
            for _ in range(warmup):
                cycle()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if DropoutRng.last:   # dropout seeds are kernel ARGUMENTS drawn on the host: a replay would repeat one step's masks
            raise RuntimeError("TrainStep.capture: the model has active dropout / drop-path sites "
                               f"({len(DropoutRng.last)}); their per-step seeds cannot be captured — train eagerly or set the rates to 0")
        prev = getattr(self, "_captured", None)
        if prev is not None:          # capturing again: the previous captured step of THIS TrainStep is released first
            prev.release()
        graph = torch.cuda.CUDAGraph()
        t_before = self.t
        mark0 = ops.captured_tables_mark()
        with torch.cuda.graph(graph, stream=side):
            static_losses = cycle()
        static_loss = static_losses[0] if self._accum_n is None else tuple(static_losses)
        mark1 = ops.captured_tables_mark()   # the pinned descriptor-table images registered in between belong to this graph
        self.t = t_before   # capture records the step; nothing ran

        def replay(new_inputs, new_labels, new_pixel_weight=None, teacher_scores=None, teacher_weight=None):
            if self._ema_swapped:
                raise RuntimeError("TrainStep replay: inside ema_weights() the parameters are the EMA; leave the block before "
                                   "training")
            if (new_pixel_weight is None) != (static_pws is None):
                raise ValueError("TrainStep replay: the step was captured " + ("without a pixel weight: replay(inputs, labels)"
                                 if static_pws is None else "with a pixel weight: replay(inputs, labels, pixel_weight)"))
            for what, new, held in (("teacher_scores", teacher_scores, static_ts), ("teacher_weight", teacher_weight, static_tw)):
                if (new is None) != (held is None):
                    raise ValueError(f"TrainStep replay: the step was captured {'without' if held is None else 'with'} {what}: "
                                     f"replay(inputs, labels, ...{'' if held is None else ', ' + what + '=...'})")
            if self._accum_n is None:
                new_inputs, new_labels = [new_inputs], [new_labels]
                new_pixel_weight = None if new_pixel_weight is None else [new_pixel_weight]
            elif isinstance(new_inputs, dict) or len(new_inputs) != n_micro or len(new_labels) != n_micro:
                raise ValueError(f"TrainStep replay: the captured cycle takes sequences of {n_micro} inputs and {n_micro} labels")
            elif self.micro != 0:
                raise RuntimeError("TrainStep replay: an eager accumulation cycle is open; finish it or flush() first")
            for dst, src in zip(static_ins, new_inputs):
                for k, v in src.items():
                    if v is not dst[k]:
                        dst[k].copy_(v, non_blocking=True)
            for dst, src in zip(static_lbs, new_labels):
                if src is not dst:
                    dst.copy_(src, non_blocking=True)
            if static_pws is not None:
                if len(new_pixel_weight) != n_micro:
                    raise ValueError(f"TrainStep replay: the captured cycle takes a sequence of {n_micro} pixel weights")
                for dst, src in zip(static_pws, new_pixel_weight):
                    if src is not dst:
                        dst.copy_(src, non_blocking=True)
            for dst, src in ((static_ts, teacher_scores), (static_tw, teacher_weight)):
                if dst is not None and src is not dst:
                    if src.shape != dst.shape or src.dtype != dst.dtype:
                        raise ValueError(f"TrainStep replay: the captured teacher tensor is {dst.dtype} {list(dst.shape)}, got "
                                         f"{src.dtype} {list(src.shape)}")
                    dst.copy_(src, non_blocking=True)
            graph.replay()
            self.t += 1
            return static_loss

        state = {"live": True}

        def release() -> None:
            """Destroy the captured graph and the pinned descriptor tables ITS grouped launches own (other captured steps of the
            process keep theirs).  The replay function must not be called afterwards; releasing twice is a no-op."""
            if not state["live"]:
                return
            state["live"] = False
            torch.cuda.synchronize()
            graph.reset()
            ops.release_captured_tables_range(mark0, mark1)
            if getattr(self, "_captured", None) is replay:
                self._captured = None

        replay.static_inputs = static_in if self._accum_n is None else static_ins
        replay.static_labels = static_lb if self._accum_n is None else static_lbs
        if static_pws is not None:
            replay.static_pixel_weight = static_pws[0] if self._accum_n is None else static_pws
        if static_ts is not None:
            replay.static_teacher_scores, replay.static_teacher_weight = static_ts, static_tw
        replay.graph, replay.release = graph, release
        self._captured = replay
        return replay
