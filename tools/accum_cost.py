#!/usr/bin/env python3
"""What gradient accumulation costs per optimizer UPDATE at a fixed effective batch of 32 images (config 2, 512x512):
  (N, micro-batch) = (1, 32)   TrainStep(optimizer="adamw", weight_decay=0.05, device_state=True): the plain device-held step
                     (2, 16)   the same with accumulate=2: two forward / backward passes of 16 images, one update
                     (4, 8)    accumulate=4: four passes of 8 images, one update
The three variants alternate round by round in one process; a round times a train of whole cycles between two device events
(hipEventRecord on the step's stream: no host sync inside the train), after warm-up cycles.  Reported: milliseconds per update
(median, min, max over the rounds) and the difference to N = 1.  What accumulation adds per cycle: N - 1 more rounds of the
per-launch overheads and of the GEMMs at a smaller M, N accum_add launches; what it removes: nothing at one GPU (the optimizer,
the norm, the EMA and the shadow refresh already ran once per 32 images).
usage: python tools/accum_cost.py [--cycles C] [--rounds R] [--out FILE]"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

LR, WD = 1e-5, 0.05
VARIANTS = ((1, 32), (2, 16), (4, 8))


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def make(dev, n):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    torch.manual_seed(1024)
    m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
    return TrainStep(m, optimizer="adamw", lr=LR, weight_decay=WD, device_state=True, accumulate=n)


def measure(cycles, rounds):
    """In THIS process (started by main() under a time limit): the three variants, alternated round by round."""
    import bench
    dev = torch.device("cuda", 0)
    runs = {}
    for n, b in VARIANTS:
        runs[(n, b)] = (make(dev, n), [bench.synth_batch(b, 512, 128, 16, 2 + k, dev) for k in range(n)])
    for ts, micro in runs.values():
        for _ in range(3):
            for inputs, labels in micro:
                ts.step(inputs, labels)
    torch.cuda.synchronize()
    res = {v: [] for v in runs}
    for _ in range(rounds):
        for v, (ts, micro) in runs.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(cycles):
                for inputs, labels in micro:
                    ts.step(inputs, labels)
            stop.record()
            stop.synchronize()
            res[v].append(start.elapsed_time(stop) / cycles)
    lines = Lines()
    lines.append(f"adamw on {torch.cuda.get_device_name(0)}: arena {ts.arena.numel} fp32; {rounds} alternating rounds of {cycles} "
                 "cycles between two device events, after 3 warm-up cycles each")
    base = statistics.median(res[VARIANTS[0]])
    for n, b in VARIANTS:
        r = res[(n, b)]
        med = statistics.median(r)
        d = [x - y for x, y in zip(r, res[VARIANTS[0]])]
        lines.append(f"  N = {n}, micro-batch {b:2d}: median {med:8.3f} ms/update  (min {min(r):8.3f}, max {max(r):8.3f}; "
                     f"{32e3 / med:7.1f} img/s)  vs N = 1, round by round: median {statistics.median(d):+7.3f} ms "
                     f"= {statistics.median(d) / base:+.2%}")
        ts_n = runs[(n, b)][0]
        assert ts_n.micro == 0 and ts_n.applied_steps.item() == 3 + rounds * cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.measure:
        return measure(a.cycles, a.rounds)
    lines = Lines()
    lines.append(f"command: python tools/accum_cost.py --cycles {a.cycles} --rounds {a.rounds}")
    lines.append(f"config 2 at 512x512, 32 images per update, AdamW on the device path (device_state, lr {LR}, weight_decay {WD}); "
                 "(N, micro-batch) = (1, 32), (2, 16), (4, 8)")
    # the GPU work under its own time limit, in a fresh process
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, str(Path(__file__).resolve()), "--measure", "--cycles",
                        str(a.cycles), "--rounds", str(a.rounds)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"--measure failed ({r.returncode}): {r.stderr[-1500:]}")
    for ln in r.stdout.splitlines():
        lines.append(ln)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
