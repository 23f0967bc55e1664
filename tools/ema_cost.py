#!/usr/bin/env python3
"""What the weight EMA costs on the headline step (config 2: B = 32, 512x512), taken in one call:
  off        TrainStep(optimizer="adamw", weight_decay=0.05, device_state=True)
  on         the same plus ema_decay=0.9999: one ema_ctrl_kernel launch over the arena after the optimizer's
alternating round by round in one process (the step-time difference), then ONE `rocprofv3 --kernel-trace --stats` run of its own
(a fresh child process) that records per-launch times of ema_ctrl_kernel — forward and reverse walk — and, as the yardstick, of
sgd_ctrl_kernel without momentum from the same trace: that kernel moves the same 12 bytes per element (read p, read g, write p).
ema_ctrl_kernel should take no longer than sgd_ctrl_kernel plus 10 %.
usage: python tools/ema_cost.py [--steps N] [--rounds R] [--no-trace] [--out FILE]"""
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

LR, WD, DECAY = 1e-5, 0.05, 0.9999
MARGIN = 0.10
BYTES = 12   # per element, both kernels: two fp32 reads and one fp32 write


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def make(dev, kind="adamw", **kw):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    torch.manual_seed(1024)
    m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
    return TrainStep(m, optimizer=kind, lr=LR, weight_decay=WD, device_state=True, **kw)


def batch(dev):
    import bench
    return bench.synth_batch(32, 512, 128, 16, 2, dev)


def child(steps):
    """Under rocprofv3: AdamW + EMA walking forward, AdamW + EMA walking in reverse, then plain SGD (no momentum, no decay: one
    sgd_ctrl_kernel launch over the whole arena per step), twice each; nothing else."""
    dev = torch.device("cuda", 0)
    inputs, labels = batch(dev)
    for rep in range(2):
        for name in ("ema_forward", "ema_reverse", "sgd"):
            if name == "sgd":
                import lc2is_amd.nn as N
                from lc2is_amd.step import TrainStep
                torch.manual_seed(1024)
                m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
                ts = TrainStep(m, optimizer="sgd", lr=LR, device_state=True)
            else:
                ts = make(dev, ema_decay=DECAY)
                ts.ema_reverse_walk = name == "ema_reverse"
            for _ in range(steps):
                ts.step(inputs, labels)
            torch.cuda.synchronize()
            print(f"child: {name} rep {rep} arena {ts.arena.numel}", flush=True)
            del ts
            torch.cuda.empty_cache()


def trace(steps, lines):
    print("(rocprofv3 run)", flush=True)
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--output-format", "csv",
               "--", sys.executable, str(Path(__file__).resolve()), "--child", "all", "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        arena = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("child")).split()[-1])
        traces = sorted(Path(d).rglob("*kernel_trace.csv"))
        if not traces:
            raise RuntimeError("rocprofv3 wrote no kernel_trace.csv")
        rows = list(csv.DictReader(open(traces[0])))
    rows.sort(key=lambda r_: int(r_["Start_Timestamp"]))
    lines.append(f"rocprofv3 --kernel-trace --stats, one run of a fresh process: ema forward, ema reverse, sgd, twice ({steps} steps "
                 f"each), arena {arena} fp32 = {4 * arena / 1e6:.1f} MB; {BYTES} B/element for both kernels")

    def durs(kernel):
        return [(int(r_["End_Timestamp"]) - int(r_["Start_Timestamp"])) / 1e3 for r_ in rows if re.search(rf"\b{kernel}\b", r_["Kernel_Name"])]

    ema, sgd = durs("ema_ctrl_kernel"), durs("sgd_ctrl_kernel")
    if len(ema) != 4 * steps or len(sgd) != 2 * steps:
        raise RuntimeError(f"expected {4 * steps} ema_ctrl_kernel and {2 * steps} sgd_ctrl_kernel launches, found {len(ema)} and {len(sgd)}")
    # launch order: rep 0 forward, rep 0 reverse, rep 1 forward, rep 1 reverse
    parts = {"ema_ctrl_kernel forward": ema[:steps] + ema[2 * steps:3 * steps], "ema_ctrl_kernel reverse": ema[steps:2 * steps] + ema[3 * steps:],
             "sgd_ctrl_kernel (no momentum)": sgd}
    med = {}
    for k, v in parts.items():
        halves = [statistics.median(v[:len(v) // 2]), statistics.median(v[len(v) // 2:])]
        med[k] = statistics.median(v)
        lines.append(f"  {k:30s} x{len(v):3d}  median {med[k]:7.1f} us  (min {min(v):7.1f}, max {max(v):7.1f})  {BYTES * arena / med[k] / 1e6:5.2f} TB/s"
                     f"  first / second repetition {halves[0]:7.1f} / {halves[1]:7.1f} us")
    yard = med["sgd_ctrl_kernel (no momentum)"]
    for k in ("ema_ctrl_kernel forward", "ema_ctrl_kernel reverse"):
        diff = (med[k] - yard) / yard
        lines.append(f"  {k} - sgd_ctrl_kernel = {med[k] - yard:+.1f} us ({diff:+.1%}): "
                     f"{'within' if diff <= MARGIN else 'SLOWER than'} the yardstick + {MARGIN:.0%}")
    f, r_ = med["ema_ctrl_kernel forward"], med["ema_ctrl_kernel reverse"]
    lines.append(f"  reverse - forward = {r_ - f:+.1f} us ({(r_ - f) / f:+.1%}); the default walk is the faster one, forward if the two are "
                 "within the +-2 % box spread")


def ab(steps, rounds, lines):
    """EMA off and on in THIS process, alternated round by round."""
    dev = torch.device("cuda", 0)
    inputs, labels = batch(dev)
    variants = {"off": make(dev), "on": make(dev, ema_decay=DECAY)}
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
    ts = variants["on"]
    lines.append(f"adamw on {torch.cuda.get_device_name(0)}: arena {ts.arena.numel} fp32 = {4 * ts.arena.numel / 1e6:.1f} MB, the EMA buffer "
                 f"as much again; bytes alone: {BYTES * ts.arena.numel / 1e9:.2f} GB per step")
    lines.append(f"  EMA walk in the step: {'reverse' if ts.ema_reverse_walk else 'forward'} (TrainStep's default)")
    for v in variants:
        r = res[v]
        lines.append(f"  ema {v:4s} median {statistics.median(r):7.3f} ms/step  (min {min(r):7.3f}, max {max(r):7.3f}; {32e3 / statistics.median(r):7.1f} img/s)")
    d = [x - y for x, y in zip(res["on"], res["off"])]
    lines.append(f"  on - off, round by round: median {statistics.median(d) * 1e3:+7.1f} us  (min {min(d) * 1e3:+7.1f}, max {max(d) * 1e3:+7.1f})"
                 f" = {statistics.median(d) / statistics.median(res['off']):+.2%} of the step")


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
    lines.append(f"command: python tools/ema_cost.py --steps {a.steps} --rounds {a.rounds}")
    lines.append(f"headline step (config 2, B = 32, 512x512), AdamW on the device path (device_state, lr {LR}, weight_decay {WD}); EMA off / on "
                 f"(ema_decay {DECAY}); {a.rounds} alternating rounds of {a.steps} steps after 3 warm-up steps each, one process")
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
