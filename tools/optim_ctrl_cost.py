#!/usr/bin/env python3
"""What the device-held optimizer path costs on the headline step (config 2: B = 32, 512x512), taken in one call:
  default    TrainStep as bench.py builds it (lr a kernel argument, no norm pass)
  ctrl       TrainStep(lr_schedule=[lr], max_grad_norm=1.0, skip_nonfinite=True): grad_sumsq + optim_ctrl_update + the _ctrl optimizer
  ctrl-rev   the SAME TrainStep object (same buffers) with the _ctrl optimizer walking the arena from its END (the tail of the 628 MB
             that grad_sumsq read last may still sit in the 256 MiB Infinity Cache)
for SGD and AdamW (a fresh process each), alternating round by round inside the process; then two `rocprofv3 --kernel-trace --stats` runs of their own (fresh child processes)
for the per-kernel times: one of default steps only (it must show no grad_sumsq / _ctrl kernel) and one of all variants (grad_sumsq
next to sgd_kernel from the same trace).
usage: python tools/optim_ctrl_cost.py [--steps N] [--rounds R] [--no-trace] [--out FILE]"""
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

LR = 1e-5
NEW_KERNELS = ("grad_sumsq_kernel", "optim_ctrl_update_kernel", "sgd_ctrl_kernel", "adamw_ctrl_kernel")


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def make(dev, kind, variant):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    torch.manual_seed(1024)
    m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
    if variant == "default":
        return TrainStep(m, optimizer=kind, lr=LR)
    return TrainStep(m, optimizer=kind, lr_schedule=[LR], max_grad_norm=1.0, skip_nonfinite=True)


def batch(dev):
    import bench
    return bench.synth_batch(32, 512, 128, 16, 2, dev)


def child(which, steps):
    """Under rocprofv3: `steps` steps of each requested variant, nothing else."""
    dev = torch.device("cuda", 0)
    inputs, labels = batch(dev)
    variants = ["default"] if which == "default" else ["default", "ctrl"]
    for kind in ("sgd", "adamw"):
        for v in variants:
            ts = make(dev, kind, v)
            for _ in range(steps):
                ts.step(inputs, labels)
            torch.cuda.synchronize()
            print(f"child {which}: {kind} {v} arena {ts.arena.numel}", flush=True)
            del ts
            torch.cuda.empty_cache()


def trace(which, steps, lines):
    print(f"(rocprofv3 run: {which})", flush=True)
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable,
               str(Path(__file__).resolve()), "--child", which, "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=360, cwd=d)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        arena = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("child")).split()[-1])
        stats = sorted(Path(d).rglob("*kernel_stats.csv"))
        if not stats:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(stats[0])))
    by = {}
    for k in ("sgd_kernel", "adamw_kernel") + NEW_KERNELS:
        for r_ in rows:
            if re.search(rf"\b{k}\b", r_["Name"]):
                by[k] = (int(r_["Calls"]), float(r_["AverageNs"]) / 1e3, float(r_["TotalDurationNs"]) / 1e3)
    lines.append(f"rocprofv3 --kernel-trace --stats, {which} steps only ({steps} per variant), arena {arena} fp32 = {4 * arena / 1e6:.1f} MB:")
    bytes_per = {"grad_sumsq_kernel": 4, "sgd_kernel": 12, "sgd_ctrl_kernel": 12, "adamw_kernel": 28, "adamw_ctrl_kernel": 28}
    for k in ("sgd_kernel", "adamw_kernel") + NEW_KERNELS:
        if k in by:
            calls, avg, _ = by[k]
            bw = f"  {bytes_per[k] * arena / avg / 1e6:6.2f} TB/s ({bytes_per[k]} B/element)" if k in bytes_per else ""
            lines.append(f"  {k:26s} x{calls:4d}  avg {avg:8.1f} us{bw}")
        else:
            lines.append(f"  {k:26s} not launched")
    return by, arena


def ab(kind, steps, rounds):
    """One optimizer kind in THIS process: a default and a device-held TrainStep, alternated round by round."""
    dev = torch.device("cuda", 0)
    lines = Lines()
    inputs, labels = batch(dev)
    variants = {v: make(dev, kind, v) for v in ("default", "ctrl")}
    variants["ctrl-rev"] = variants["ctrl"]
    for ts in variants.values():
        for _ in range(3):
            ts.step(inputs, labels)
    torch.cuda.synchronize()
    res = {v: [] for v in variants}
    for _ in range(rounds):
        for v, ts in variants.items():
            if v != "default":
                ts.reverse_walk = v == "ctrl-rev"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ts.step(inputs, labels)
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t0) / steps * 1e3)
    ts = variants["ctrl"]
    lines.append(f"{kind} on {torch.cuda.get_device_name(0)}: (grad norm of the last ctrl step {ts.last_grad_norm.item():.4f}, clip coefficient "
                 f"{ts.last_clip_coef.item():.4f}, applied {ts.applied_steps.item()}, skipped {ts.skipped_steps.item()})")
    for v in variants:
        r = res[v]
        lines.append(f"  {v:9s} median {statistics.median(r):7.3f} ms/step  (min {min(r):7.3f}, max {max(r):7.3f}; {32e3 / statistics.median(r):7.1f} img/s)")
    for v in ("ctrl", "ctrl-rev"):
        d = [x - y for x, y in zip(res[v], res["default"])]     # same round: the pair ran back to back
        lines.append(f"  {v:9s} - default, round by round: median {statistics.median(d) * 1e3:+7.1f} us  (min {min(d) * 1e3:+7.1f}, max {max(d) * 1e3:+7.1f})")
    d = [x - y for x, y in zip(res["ctrl-rev"], res["ctrl"])]
    lines.append(f"  ctrl-rev  - ctrl,    round by round: median {statistics.median(d) * 1e3:+7.1f} us  (min {min(d) * 1e3:+7.1f}, max {max(d) * 1e3:+7.1f})")


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
        return child(a.child, a.steps)
    if a.kind:
        return ab(a.kind, a.steps, a.rounds)
    lines = Lines()
    lines.append(f"command: python tools/optim_ctrl_cost.py --steps {a.steps} --rounds {a.rounds}")
    lines.append(f"headline step (config 2, B = 32, 512x512), lr {LR}; ctrl = constant table, max_grad_norm 1.0, skip on; {a.rounds} "
                 f"alternating rounds of {a.steps} steps after 3 warm-up steps each; one process per optimizer kind, default and ctrl "
                 "alternating inside it")
    for kind in ("sgd", "adamw"):
        # a fresh process per kind: a second pair of 157 M-parameter models built after the first pair was freed ran 8 ms/step
        # slower whichever variant it was (buffer placement), which drowns a 0.1 ms difference
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--kind", kind, "--steps", str(a.steps), "--rounds",
                            str(a.rounds)], capture_output=True, text=True, timeout=360)
        if r.returncode != 0:
            raise RuntimeError(f"--kind {kind} failed ({r.returncode}): {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            lines.append(ln)
    if not a.no_trace:
        by_d, _ = trace("default", 6, lines)
        leaked = [k for k in NEW_KERNELS if k in by_d]
        lines.append(f"  default steps launch none of {', '.join(NEW_KERNELS)}: {'TRUE' if not leaked else 'FALSE ' + str(leaked)}")
        by, arena = trace("all", 6, lines)
        t_sgd, t_sq = by["sgd_kernel"][1], by["grad_sumsq_kernel"][1]
        est = t_sgd / 3.0
        lines.append(f"  grad_sumsq {4 * arena / t_sq / 1e6:.2f} TB/s vs sgd_kernel {12 * arena / t_sgd / 1e6:.2f} TB/s in the same trace: "
                     f"{'at least as fast' if 4 * arena / t_sq >= 12 * arena / t_sgd else 'SLOWER'}")
        lines.append(f"  byte-derived estimate of pass 1 at sgd_kernel's rate: {est:.1f} us; twice that: {2 * est:.1f} us; "
                     f"kernels added per step in the trace: {t_sq + by['optim_ctrl_update_kernel'][1]:.1f} us "
                     f"(grad_sumsq {t_sq:.1f} + optim_ctrl_update {by['optim_ctrl_update_kernel'][1]:.1f}); "
                     f"sgd_ctrl - sgd {by['sgd_ctrl_kernel'][1] - t_sgd:+.1f} us, adamw_ctrl - adamw "
                     f"{by['adamw_ctrl_kernel'][1] - by['adamw_kernel'][1]:+.1f} us")
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
