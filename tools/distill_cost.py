#!/usr/bin/env python3
"""What distillation on the fused head costs, taken in one call and written to profiles/distill_cost.txt: device events around
trains of back-to-back calls on warm buffers, the sides of a comparison alternated round by round.
  launches  ops.head_upsample_kd(labels, pixel_weight, want_grad=True) — the forward + backward launch and the fixed-order finish
            launch — against the weighted-CE pair ops.head_upsample_ce(class_weight=w, want_grad=True) on the same buffers, at the
            headline head shape (B = 32, 32 x 32 -> 128 x 128 bicubic) for K = 151 (ld 192: TN = 10, one block per CU), K = 64
            (ld 64: TN = 4, two blocks per CU) and K = 192 (TN = 12);
  glue      the elementwise device ops that combine the two low-resolution gradients (nn/head_loss.py), on [B h w, 192] fp32;
  step      the headline train step (bench.py's model and batch) with and without distill on precomputed teacher scores, and the
            teacher's model.head_scores(inputs) forward on its own.
The register / LDS figures of the kernel (tools/check_kernel_resources.py's compile, no GPU needed) head the file.
No ratio is a gate: the figures are this commit's own, measured against its own existing paths.
usage: python tools/distill_cost.py [--calls N] [--rounds R] [--steps N] [--out FILE]"""
import argparse
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

from selftrain_cost import Lines, report, timed  # noqa: E402

B, H, S, TEMP = 32, 32, 4, 2.0


def resources(lines):
    """VGPRs / occupancy / scratch of every head_kd_grp_kernel instantiation and the LDS its launch asks for."""
    import check_kernel_resources as ck
    rows = ck.one(ck.CSRC / "head_distill.hip")
    names = [re.sub(r"\(.*", "", n).replace("void ", "") for n in ck.demangle([r["name"] for r in rows])]
    lines.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): <MODE 0 bicubic / 1 bilinear, TN, S>")
    for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
        if n.startswith("head_kd"):
            lines.append(f"  {n:40s} VGPR {r.get('vgpr', 0):4d}  waves/SIMD {r.get('occ', 0):2d}  scratch {r.get('scratch', 0)}")
    for ld in (64, 128, 192):
        lines.append(f"  dynamic LDS at ld = {ld}, bicubic S = 4 (7 x 7 footprint): {(3 * 49 * (ld + 4) + 512) * 4} bytes (student "
                     "footprint, teacher footprint, mirror, labels, pixel weights) + 64 static")


def launches(calls, rounds, lines):
    from lc2is_amd import ops
    dev = torch.device("cuda", 0)
    lines.append(f"launches on {torch.cuda.get_device_name(0)}: B = {B}, h = w = {H}, S = {S} bicubic; {rounds} alternating rounds of "
                 f"{calls} back-to-back calls after one warm-up train each")
    for K in (151, 64, 192):
        ld = (K + 63) // 64 * 64
        g = torch.Generator().manual_seed(7)
        lo, t = torch.zeros(B * H * H, ld), torch.zeros(B * H * H, ld)
        lo[:, :K] = torch.randn(B * H * H, K, generator=g) * 3
        t[:, :K] = torch.randn(B * H * H, K, generator=g) * 3
        labels = torch.randint(0, K, (B, H * S, H * S), generator=g)
        labels[:, 1::9] = -100
        pw = 2.0 * torch.rand(B, H * S, H * S, generator=g)
        lo, t, labels, pw = lo.to(dev), t.to(dev), labels.to(dev), pw.to(dev)
        w = (torch.rand(K, generator=g) * 1.5 + 0.25).to(dev)
        geom = (B, H, H, K, S, ops.INTERP_BICUBIC)
        variants = {"ce (OPT)": lambda: ops.head_upsample_ce(lo, labels, *geom, want_grad=True, class_weight=w),
                    "kd": lambda: ops.head_upsample_kd(lo, t, *geom, temperature=TEMP, labels=labels, pixel_weight=pw, want_grad=True),
                    "kd (all, no pw)": lambda: ops.head_upsample_kd(lo, t, *geom, temperature=TEMP, want_grad=True)}
        for fn in variants.values():
            timed(fn, calls)
        res = {v: [] for v in variants}
        for _ in range(rounds):
            for v, fn in variants.items():
                res[v].append(timed(fn, calls))
        lines.append(f" K = {K} (ld {ld}, TN = {(lambda n: 4 if n <= 4 else 8 if n <= 8 else 10 if n <= 10 else 12)((K + 15) // 16)}):")
        report(lines, res, "us/call", 1e3)
        if K == 151:   # the glue of nn/head_loss.py on this shape's gradients
            _, dlo, _ = ops.head_upsample_ce(lo, labels, *geom, want_grad=True)
            loss2, dkd = ops.head_upsample_kd(lo, t, *geom, temperature=TEMP, want_grad=True)
            one = torch.ones((), device=dev)   # multipliers of 1: the buffers keep their magnitudes over a train of calls

            def glue():
                dlo.mul_(one)
                dlo.add_(dkd.mul_(one.masked_fill(one == 0, 1.0).reciprocal().mul_(1.0)))
            timed(glue, calls)
            r = [timed(glue, calls) for _ in range(rounds)]
            lines.append(f" glue (dlo * mul + dkd * weight / count, [{B * H * H}, {ld}] fp32, {dlo.numel() * 4 / 1e6:.1f} MB each): median "
                         f"{statistics.median(r) * 1e3:.2f} us/call (min {min(r) * 1e3:.2f}, max {max(r) * 1e3:.2f})")


def step(steps, rounds, lines):
    import lc2is_amd.nn as N
    from bench import synth_batch
    from lc2is_amd.step import TrainStep
    dev = torch.device("cuda", 0)
    models = [N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train() for _ in range(2)]
    inputs, labels = synth_batch(B, 512, 128, 16, 2, dev)
    plain = TrainStep(models[0], optimizer="sgd", lr=1e-5)
    kd = TrainStep(models[1], optimizer="sgd", lr=1e-5, distill=(1.0, TEMP, "all"))
    noisy = {**inputs, "pixel_values": inputs["pixel_values"] + 0.5 * torch.randn_like(inputs["pixel_values"])}
    ts = models[0].head_scores(noisy)   # precomputed: the teacher's forward is timed on its own
    variants = {"step": lambda: plain.step(inputs, labels),
                "step + distill": lambda: kd.step_distill(inputs, labels, ts),
                "head_scores": lambda: models[0].head_scores(noisy)}
    for fn in variants.values():
        timed(fn, 3)
    res = {v: [] for v in variants}
    for _ in range(rounds):
        for v, fn in variants.items():
            res[v].append(timed(fn, steps))
    lines.append(f"headline step on {torch.cuda.get_device_name(0)} (ViT-B/16, B = {B}, 512 x 512, K = 151, SGD, eager): {rounds} "
                 f"alternating rounds of {steps} steps; teacher scores precomputed; head_scores = the teacher's forward alone")
    report(lines, res, "ms", 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--part", default=None, choices=["launches", "step"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "distill_cost.txt"))
    a = ap.parse_args()
    lines = Lines()
    if a.part == "launches":
        return launches(a.calls, a.rounds, lines)
    if a.part == "step":
        return step(a.steps, a.rounds, lines)
    lines.append(f"command: python tools/distill_cost.py --calls {a.calls} --rounds {a.rounds} --steps {a.steps}")
    resources(lines)
    # each GPU part under its own time limit, in a fresh process; a part that fails ends the run
    for part, limit in (("launches", 180), ("step", 300)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--part", part, "--calls",
                            str(a.calls), "--rounds", str(a.rounds), "--steps", str(a.steps)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"--part {part} failed ({r.returncode}): {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            lines.append(ln)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
