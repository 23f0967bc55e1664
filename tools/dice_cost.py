#!/usr/bin/env python3
"""What the Dice + cross-entropy criterion costs on the headline step (config 2: B = 32, 512x512), taken in one call:
  plain      TrainStep(optimizer="sgd")                                          the bench-shape step, CrossEntropyLoss()
  dice       the same with criterion=DiceCrossEntropyLoss(dice_weight=3.0)
alternating round by round in one process (the step-time difference: the comparison is this commit's own plain step, which is the
parent commit's — no existing kernel changed; no threshold is fixed in advance), then ONE `rocprofv3 --kernel-trace --stats` run of
its own (a fresh child process) that records the per-launch times of the kernels of the Dice step's head: head_dice_stats_grp_kernel
(the forward-only statistics pass), dice_coef_kernel (one block: the fixed-order fp64 sums and the coefficients),
head_ce_dice_grp_kernel (forward + gradient; it stands where head_ce_grp_kernel stands in the plain step) and head_finish_kernel.
The batch is synthetic and the model untrained; the passes cost the same whatever the labels are.
usage: python tools/dice_cost.py [--steps N] [--rounds R] [--no-trace] [--out FILE]"""
import argparse
import csv
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

LR, DICE_WEIGHT = 1e-5, 3.0
KERNELS = ("head_dice_stats_grp_kernel", "dice_coef_kernel", "head_ce_dice_grp_kernel", "head_finish_kernel")


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def make(dev, dice):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    torch.manual_seed(1024)
    m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
    crit = N.DiceCrossEntropyLoss(dice_weight=DICE_WEIGHT).to(dev) if dice else None
    return TrainStep(m, optimizer="sgd", lr=LR, criterion=crit)


def batch(dev):
    import bench
    return bench.synth_batch(32, 512, 128, 16, 2, dev)


def child(steps):
    """Under rocprofv3: the Dice step alone."""
    dev = torch.device("cuda", 0)
    inputs, labels = batch(dev)
    ts = make(dev, True)
    for _ in range(steps):
        ts.step(inputs, labels)
    torch.cuda.synchronize()
    print(f"child: pixels {labels.numel()}", flush=True)


def trace(steps, lines):
    print("(rocprofv3 run)", flush=True)
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--output-format", "csv",
               "--", sys.executable, str(Path(__file__).resolve()), "--child", "all", "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        n = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("child")).split()[-1])
        traces = sorted(Path(d).rglob("*kernel_trace.csv"))
        if not traces:
            raise RuntimeError("rocprofv3 wrote no kernel_trace.csv")
        rows = list(csv.DictReader(open(traces[0])))
    lines.append(f"rocprofv3 --kernel-trace --stats, one run of a fresh process: {steps} Dice + CE steps, {n} label pixels per step")
    total = 0.0
    for k in KERNELS:
        v = [(int(r_["End_Timestamp"]) - int(r_["Start_Timestamp"])) / 1e3 for r_ in rows if k in r_["Kernel_Name"]]
        if not v:
            raise RuntimeError(f"no launch of {k} in the trace")
        per_step = len(v) / steps
        total += statistics.median(v) * per_step
        lines.append(f"  {k:26s} x{len(v):3d} ({per_step:.0f} per step)  median {statistics.median(v):7.1f} us  (min {min(v):7.1f}, max {max(v):7.1f})")
    lines.append(f"  the head of the Dice step, medians summed per step: {total:.1f} us (the plain step's head: head_ce_grp_kernel + head_finish_kernel)")


def ab(steps, rounds, lines):
    """Plain and Dice + CE criterion in THIS process, alternated round by round."""
    dev = torch.device("cuda", 0)
    inputs, labels = batch(dev)
    variants = {"plain": make(dev, False), "dice": make(dev, True)}
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
    I, P, T, block = variants["dice"].dice_stats
    tot, ce, dice, n = block.tolist()
    lines.append(f"sgd on {torch.cuda.get_device_name(0)}: {labels.numel()} label pixels per step; last Dice step: loss {tot:.4f} = CE {ce:.4f} "
                 f"+ {DICE_WEIGHT} x Dice {dice:.4f}, n_valid {int(n)}, classes present {int((T > 0).sum())}")
    for v in variants:
        r = res[v]
        lines.append(f"  {v:5s} median {statistics.median(r):7.3f} ms/step  (min {min(r):7.3f}, max {max(r):7.3f}; {32e3 / statistics.median(r):7.1f} img/s)")
    d = [x - y for x, y in zip(res["dice"], res["plain"])]
    lines.append(f"  dice - plain, round by round: median {statistics.median(d) * 1e3:+7.1f} us  (min {min(d) * 1e3:+7.1f}, max {max(d) * 1e3:+7.1f})"
                 f" = {statistics.median(d) / statistics.median(res['plain']):+.2%} of the step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    lines = Lines()
    if a.ab:
        return ab(a.steps, a.rounds, lines)
    lines.append(f"command: python tools/dice_cost.py --steps {a.steps} --rounds {a.rounds}")
    lines.append(f"headline step (config 2, B = 32, 512x512), SGD (lr {LR}); criterion CrossEntropyLoss() / DiceCrossEntropyLoss(dice_weight={DICE_WEIGHT}); "
                 f"{a.rounds} alternating rounds of {a.steps} steps after 3 warm-up steps each, one process")
    # every GPU step under its own time limit, in a fresh process
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(Path(__file__).resolve()), "--ab", "--steps", str(a.steps),
                        "--rounds", str(a.rounds)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"--ab failed ({r.returncode}): {r.stderr[-1500:]}")
    for ln in r.stdout.splitlines():
        lines.append(ln)
    if not a.no_trace:
        trace(4, lines)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
