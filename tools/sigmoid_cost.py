#!/usr/bin/env python3
"""What the sigmoid focal / sigmoid cross-entropy loss costs on the fused head, taken in one call and written to
profiles/sigmoid_cost.txt:
  launch pair   ops.head_upsample_sigmoid(gamma=2, alpha=0.25, class_weight=w) and its gamma = 0 form against
                ops.head_upsample_ce(class_weight=w) — the OPT pair that moves the same bytes — on the same warm buffers at the
                headline head shape (B = 32, h = w = 32, S = 4 bicubic, K = 151): device events around trains of back-to-back
                calls, the variants alternated round by round; each call is the forward + backward launch and the fixed-order
                finish launch;
  step          TrainStep(optimizer="sgd") at the bench shape (config 2: B = 32, 512x512) with criterion=SigmoidFocalLoss(2.0, 0.25)
                against the plain criterion, alternated round by round in one process (device events around trains of steps).
No ratio is a gate: the figures are this commit's own, measured against its own plain paths.
usage: python tools/sigmoid_cost.py [--calls N] [--steps N] [--rounds R] [--out FILE]"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

LR, GAMMA, ALPHA = 1e-5, 2.0, 0.25
B, H, S, K, LD = 32, 32, 4, 151, 192


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def timed(fn, n):
    """Milliseconds per call of ``fn`` over a train of n back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def report(lines, res, unit, scale):
    names = list(res)
    for v in names:
        r = res[v]
        lines.append(f"  {v:14s} median {statistics.median(r) * scale:9.2f} {unit}  (min {min(r) * scale:9.2f}, max {max(r) * scale:9.2f})")
    for v in names[1:]:
        d = [x - y for x, y in zip(res[v], res[names[0]])]
        lines.append(f"  {v} - {names[0]}, round by round: median {statistics.median(d) * scale:+9.2f} {unit}  (min {min(d) * scale:+9.2f}, "
                     f"max {max(d) * scale:+9.2f}) = {statistics.median(d) / statistics.median(res[names[0]]):+.2%}")


def launches(calls, rounds, lines):
    from lc2is_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    lo = torch.zeros(B * H * H, LD)
    lo[:, :K] = torch.randn(B * H * H, K, generator=g) * 3
    labels = torch.randint(0, K, (B, H * S, H * S), generator=g)
    labels[:, 1::9] = -100
    lo, labels = lo.to(dev), labels.to(dev)
    w = (torch.rand(K, generator=g) * 1.5 + 0.25).to(dev)
    variants = {
        "ce (OPT)": lambda: ops.head_upsample_ce(lo, labels, B, H, H, K, S, ops.INTERP_BICUBIC, want_grad=True, class_weight=w),
        "sigmoid focal": lambda: ops.head_upsample_sigmoid(lo, labels, B, H, H, K, S, ops.INTERP_BICUBIC, want_grad=True,
                                                           class_weight=w, gamma=GAMMA, alpha=ALPHA, class_scale=1.0 / K),
        "sigmoid CE": lambda: ops.head_upsample_sigmoid(lo, labels, B, H, H, K, S, ops.INTERP_BICUBIC, want_grad=True,
                                                        class_weight=w, gamma=0.0, alpha=None, class_scale=1.0 / K),
    }
    for fn in variants.values():
        timed(fn, calls)
    res = {v: [] for v in variants}
    for _ in range(rounds):
        for v, fn in variants.items():
            res[v].append(timed(fn, calls))
    lines.append(f"launch pair on {torch.cuda.get_device_name(0)}: B = {B}, h = w = {H}, S = {S} bicubic, K = {K} (ld {LD}), class weights, "
                 f"gradient; {rounds} alternating rounds of {calls} back-to-back calls after one warm-up train each")
    report(lines, res, "us/call", 1e3)


def steps(nsteps, rounds, lines):
    import bench
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    dev = torch.device("cuda", 0)
    inputs, labels = bench.synth_batch(32, 512, 128, 16, 2, dev)

    def make(crit):
        torch.manual_seed(1024)
        m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
        return TrainStep(m, optimizer="sgd", lr=LR, criterion=crit)

    variants = {"plain": make(None), "sigmoid focal": make(N.SigmoidFocalLoss(GAMMA, ALPHA))}
    for ts in variants.values():
        timed(lambda: ts.step(inputs, labels), 3)
    res = {v: [] for v in variants}
    for _ in range(rounds):
        for v, ts in variants.items():
            res[v].append(timed(lambda: ts.step(inputs, labels), nsteps))
    lines.append(f"step: config 2 (B = 32, 512x512), SGD (lr {LR}); criterion CrossEntropyLoss() / SigmoidFocalLoss({GAMMA}, {ALPHA}); {rounds} alternating "
                 f"rounds of {nsteps} steps after 3 warm-up steps each, one process")
    report(lines, res, "ms/step", 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", default=None, choices=["launches", "steps"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sigmoid_cost.txt"))
    a = ap.parse_args()
    lines = Lines()
    if a.part == "launches":
        return launches(a.calls, a.rounds, lines)
    if a.part == "steps":
        return steps(a.steps, a.rounds, lines)
    lines.append(f"command: python tools/sigmoid_cost.py --calls {a.calls} --steps {a.steps} --rounds {a.rounds}")
    # every GPU part under its own time limit, in a fresh process; a part that fails ends the run
    for part, limit in (("launches", 120), ("steps", 400)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--part", part, "--calls",
                            str(a.calls), "--steps", str(a.steps), "--rounds", str(a.rounds)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"--part {part} failed ({r.returncode}): {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            lines.append(ln)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
