#!/usr/bin/env python3
"""What parameter groups cost on the headline step (config 2: B = 32, 512x512), taken in one call:
  ctrl       TrainStep(device_state=True, weight_decay=0.05): the _ctrl optimizer, one decay, one rate
  groups     TrainStep(param_groups=make_param_groups(weight_decay=0.05, lr_scales={"vision_encoder": 0.1}, layer_decay=0.9)):
             sgd_groups_kernel / adamw_groups_kernel, one launch over the arena
for SGD and AdamW (a fresh process each), alternating round by round inside the process; once per kind, for scale, the same
recipe emulated with the existing _ctrl kernels range by range (the launches the single launch replaces); then ONE
`rocprofv3 --kernel-trace --stats` run of its own (a fresh child process) in which both variants run twice each, so the _ctrl
kernels' own spread between two traces of one call is the margin the grouped kernels are read against.
usage: python tools/param_groups_cost.py [--steps N] [--rounds R] [--no-trace] [--out FILE]"""
import argparse
import csv
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

LR, WD = 1e-5, 0.05
RECIPE = dict(weight_decay=WD, lr_scales={"vision_encoder": 0.1}, layer_decay=0.9)
KERNELS = ("sgd_ctrl_kernel", "sgd_groups_kernel", "adamw_ctrl_kernel", "adamw_groups_kernel")
BYTES = {"sgd_ctrl_kernel": 12, "sgd_groups_kernel": 12, "adamw_ctrl_kernel": 28, "adamw_groups_kernel": 28}


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def make(dev, kind, variant):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep, make_param_groups
    torch.manual_seed(1024)
    m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
    if variant == "ctrl":
        return TrainStep(m, optimizer=kind, lr=LR, weight_decay=WD, device_state=True)
    return TrainStep(m, optimizer=kind, lr=LR, weight_decay=WD, param_groups=make_param_groups(m, **RECIPE))


def batch(dev):
    import bench
    return bench.synth_batch(32, 512, 128, 16, 2, dev)


def ranges_of(ts):
    """Maximal runs of arena granules with one group id (dead parameters left out): what an emulation with the existing kernels
    launches one by one."""
    gmap = ts.arena.group_map().cpu()
    change = torch.nonzero(gmap[1:] != gmap[:-1]).flatten() + 1
    bounds = [0] + change.tolist() + [gmap.numel()]
    return [(lo * 64, hi * 64, int(gmap[lo])) for lo, hi in zip(bounds[:-1], bounds[1:]) if int(gmap[lo]) != 255]


def emulated_step(ts, inputs, labels, runs, ctrl_copy):
    """The grouped step with the optimizer launch replaced by the existing _ctrl kernels, range by range."""
    from lc2is_amd import ops
    arena = ts.arena
    arena.zero_grad(set_to_none=True)
    loss = ts.model.forward_loss(inputs, labels, ts.ignore_index)
    loss.backward()
    arena.finalize_grads()
    partials, flags = ops.grad_sumsq(arena.grad)
    b1, b2 = ts.betas if ts.kind == "adamw" else (0.0, 0.0)
    ops.optim_ctrl_update(ts._ctrl, partials, flags, ts.lr_table, max_norm=ts.max_grad_norm, beta1=b1, beta2=b2)
    lr_word = ts._ctrl_f[ops.CTRL_LR]
    cf = ctrl_copy.view(torch.float32)
    for lo, hi, gid in runs:
        g = ts.param_groups[gid]
        ctrl_copy.copy_(ts._ctrl)
        cf[ops.CTRL_LR] = lr_word * g["lr_scale"]
        sl = slice(lo, hi)
        if ts.kind == "sgd":
            ops.sgd_step_ctrl(arena.flat[sl], arena.grad[sl], None, ctrl_copy, 0.0, g["weight_decay"])
        else:
            ops.adamw_step_ctrl(arena.flat[sl], arena.grad[sl], ts.m[sl], ts.v[sl], ctrl_copy, b1, b2, ts.eps, g["weight_decay"])
    for m in ts._hip_modules:
        m.invalidate_shadows()
    return loss.detach()


def child(steps):
    """Under rocprofv3: ctrl, groups, ctrl, groups per optimizer kind (two traces of each in one run), nothing else."""
    dev = torch.device("cuda", 0)
    inputs, labels = batch(dev)
    for kind in ("sgd", "adamw"):
        for rep in range(2):
            for v in ("ctrl", "groups"):
                ts = make(dev, kind, v)
                for _ in range(steps):
                    ts.step(inputs, labels)
                torch.cuda.synchronize()
                print(f"child: {kind} {v} rep {rep} arena {ts.arena.numel}", flush=True)
                del ts
                torch.cuda.empty_cache()


def trace(steps, lines):
    print("(rocprofv3 run)", flush=True)
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable,
               str(Path(__file__).resolve()), "--child", "all", "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=d)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        arena = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("child")).split()[-1])
        traces = sorted(Path(d).rglob("*kernel_trace.csv"))
        if not traces:
            raise RuntimeError("rocprofv3 wrote no kernel_trace.csv")
        rows = list(csv.DictReader(open(traces[0])))
    lines.append(f"rocprofv3 --kernel-trace --stats, one run: per kind ctrl, groups, ctrl, groups ({steps} steps each), arena {arena} "
                 f"fp32 = {4 * arena / 1e6:.1f} MB")
    out = {}
    for k in KERNELS:
        durs = [(int(r_["End_Timestamp"]) - int(r_["Start_Timestamp"])) / 1e3 for r_ in rows if re.search(rf"\b{k}\b", r_["Kernel_Name"])]
        if not durs:
            lines.append(f"  {k:22s} not launched")
            continue
        halves = [durs[:len(durs) // 2], durs[len(durs) // 2:]]      # the two repetitions of the variant, in launch order
        means = [statistics.mean(h) for h in halves]
        out[k] = (statistics.mean(durs), means)
        lines.append(f"  {k:22s} x{len(durs):3d}  avg {out[k][0]:8.1f} us  {BYTES[k] * arena / out[k][0] / 1e6:5.2f} TB/s ({BYTES[k]} B/element)"
                     f"  first / second repetition {means[0]:8.1f} / {means[1]:8.1f} us")
    for kind in ("sgd", "adamw"):
        c, g = out.get(f"{kind}_ctrl_kernel"), out.get(f"{kind}_groups_kernel")
        if c and g:
            spread = abs(c[1][0] - c[1][1]) / min(c[1])
            diff = (g[0] - c[0]) / c[0]
            lines.append(f"  {kind}: groups - ctrl = {g[0] - c[0]:+.1f} us ({diff:+.1%}); the _ctrl kernel's own spread between its two repetitions "
                         f"in this run: {spread:.1%} -> {'within it' if diff <= spread else 'SLOWER than that margin'}")


def ab(kind, steps, rounds):
    """One optimizer kind in THIS process: ctrl and groups alternated round by round, then the range-by-range emulation once."""
    dev = torch.device("cuda", 0)
    lines = Lines()
    inputs, labels = batch(dev)
    variants = {v: make(dev, kind, v) for v in ("ctrl", "groups")}
    for ts in variants.values():
        for _ in range(3):
            ts.step(inputs, labels)
    torch.cuda.synchronize()
    res = {v: [] for v in variants}
    for _ in range(rounds):
        for v, ts in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ts.step(inputs, labels)
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t0) / steps * 1e3)
    ts = variants["groups"]
    lines.append(f"{kind} on {torch.cuda.get_device_name(0)}: {len(ts.param_groups)} groups, arena {ts.arena.numel}, "
                 f"{len(ts.arena.dead)} parameters without a gradient (skip id)")
    for v in variants:
        r = res[v]
        lines.append(f"  {v:9s} median {statistics.median(r):7.3f} ms/step  (min {min(r):7.3f}, max {max(r):7.3f}; {32e3 / statistics.median(r):7.1f} img/s)")
    d = [x - y for x, y in zip(res["groups"], res["ctrl"])]
    lines.append(f"  groups    - ctrl, round by round: median {statistics.median(d) * 1e3:+7.1f} us  (min {min(d) * 1e3:+7.1f}, max {max(d) * 1e3:+7.1f})")
    runs = ranges_of(ts)
    ctrl_copy = ts._ctrl.clone()
    for _ in range(2):
        emulated_step(ts, inputs, labels, runs, ctrl_copy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        emulated_step(ts, inputs, labels, runs, ctrl_copy)
    torch.cuda.synchronize()
    lines.append(f"  emulated with the existing _ctrl kernels range by range: {len(runs)} optimizer launches per step, "
                 f"{(time.perf_counter() - t0) / steps * 1e3:7.3f} ms/step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--kind", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    if a.kind:
        return ab(a.kind, a.steps, a.rounds)
    lines = Lines()
    lines.append(f"command: python tools/param_groups_cost.py --steps {a.steps} --rounds {a.rounds}")
    lines.append(f"headline step (config 2, B = 32, 512x512), lr {LR}; ctrl = device_state, weight_decay {WD}; groups = make_param_groups("
                 f"weight_decay={WD}, lr_scales={{'vision_encoder': 0.1}}, layer_decay=0.9); {a.rounds} alternating rounds of {a.steps} "
                 "steps after 3 warm-up steps each; one process per optimizer kind")
    for kind in ("sgd", "adamw"):
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--kind", kind, "--steps", str(a.steps), "--rounds",
                            str(a.rounds)], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"--kind {kind} failed ({r.returncode}): {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            lines.append(ln)
    if not a.no_trace:
        trace(4, lines)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
