#!/usr/bin/env python3
"""What the training accuracy / mIoU counts cost (ops.head_upsample_argmax, TrainStep(seg_metrics=True)), taken in one call:
  launches   lc2is_head_upsample_argmax (head_argmax_grp_kernel + head_argmax_finish_kernel) alone, counts only (what the step adds),
             pred only and both, against lc2is_head_upsample_px on the SAME buffers as the yardstick: device events around trains of
             calls on preallocated buffers, the variants alternated round by round.  Two shapes, both B = 32, K = 151, bicubic x4:
             the headline step's 32 x 32 -> 128 x 128 (512 x 512 images at patch 16) and 128 x 128 -> 512 x 512 outputs;
  step       the headline step (config 2: B = 32, 512 x 512) with seg_metrics on and off, alternated round by round in one process.
The bytes each pass must move are computed from the shapes and printed beside the times.  No threshold is fixed here.
usage: python tools/seg_metrics_cost.py [--calls N] [--steps N] [--rounds R] [--out FILE]"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

LR, K, B, S = 1e-5, 151, 32, 4


class Lines(list):
    """The report: every line is printed as it is made and kept for --out."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def launches(calls, rounds, lines):
    from lc2is_amd import _lib, ops
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    px, am = ops._fn("lc2is_head_upsample_px"), ops._fn("lc2is_head_upsample_argmax")
    for h in (32, 128):
        H = h * S
        g = torch.Generator().manual_seed(0)
        lo = torch.zeros(B * h * h, 192)
        lo[:, :K] = torch.randn(B * h * h, K, generator=g)
        lo = lo.to(dev)
        # piecewise-constant labels (16 x 16 blocks), as label maps are: the histogram loop runs once or twice per wave
        labels = torch.randint(0, K, (B, H // 16, H // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().to(dev)
        lpx = torch.empty(B, H, H, dtype=torch.float32, device=dev)
        pred = torch.empty(B, H, H, dtype=torch.uint8, device=dev)
        counts = torch.empty(B, 3, K, dtype=torch.int32, device=dev)
        nws = ops._fn("lc2is_head_upsample_argmax_workspace_bytes")(B, h, h, K, S, ops.INTERP_BICUBIC)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        a = (lo.data_ptr(), 192, labels.data_ptr())
        t = (B, h, h, K, S, ops.INTERP_BICUBIC, -100)
        variants = {
            "px (yardstick)": lambda: px(*a, lpx.data_ptr(), *t, stream),
            "argmax counts": lambda: am(*a, None, counts.data_ptr(), *t, ws.data_ptr(), nws, stream),
            "argmax pred": lambda: am(a[0], a[1], None, pred.data_ptr(), None, *t, None, 0, stream),
            "argmax both": lambda: am(*a, pred.data_ptr(), counts.data_ptr(), *t, ws.data_ptr(), nws, stream),
        }
        for name, f in variants.items():
            for _ in range(5):
                _lib.check(f(), name)
        torch.cuda.synchronize()
        res = {v: [] for v in variants}
        for _ in range(rounds):
            for name, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    f()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) / calls * 1e3)
        # the counts of the timed buffers against torch on the kernel's own class map (the run measures what the tests check)
        am(*a, pred.data_ptr(), counts.data_ptr(), *t, ws.data_ptr(), nws, stream)
        p, c = pred.long().reshape(B, -1), counts.long()
        ok = all(torch.equal(c[b, 1], torch.bincount(p[b], minlength=K)) and torch.equal(c[b, 2], torch.bincount(labels[b].reshape(-1), minlength=K))
                 for b in range(B))
        px_b = lo.numel() * 4 + labels.numel() * 8 + lpx.numel() * 4
        cnt_b = lo.numel() * 4 + labels.numel() * 8 + 2 * nws + counts.numel() * 4
        lines.append(f"B = {B}, {h} x {h} -> {H} x {H}, K = {K}, bicubic x{S} on {torch.cuda.get_device_name(0)}: {rounds} alternating rounds of "
                     f"{calls} calls, device events; counts equal torch.bincount of the kernel's pred: {ok}")
        lines.append(f"  bytes a pass must move: px {px_b / 1e6:.1f} MB (scores {lo.numel() * 4 / 1e6:.1f}, labels {labels.numel() * 8 / 1e6:.1f}, "
                     f"losses {lpx.numel() * 4 / 1e6:.1f}); argmax counts {cnt_b / 1e6:.1f} MB (slabs {nws / 1e6:.1f} MB written, then read by the finish launch)")
        base = statistics.median(res["px (yardstick)"])
        for name in variants:
            r = res[name]
            lines.append(f"  {name:15s} median {statistics.median(r):8.1f} us/call  (min {min(r):8.1f}, max {max(r):8.1f})  = {statistics.median(r) / base:5.2f} x px")


def make(dev, seg):
    import lc2is_amd.nn as N
    from lc2is_amd.step import TrainStep
    torch.manual_seed(1024)
    m = N.BaseModelWithText(patch_size=16, in_size=512, out_size=128).to(dev).train()
    return TrainStep(m, optimizer="sgd", lr=LR, seg_metrics=seg)


def step_ab(steps, rounds, lines):
    import bench
    dev = torch.device("cuda", 0)
    inputs, labels = bench.synth_batch(32, 512, 128, 16, 2, dev)
    variants = {"off": make(dev, False), "on": make(dev, True)}
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
    met = ts.seg_metrics()
    same = torch.equal(variants["on"].arena.flat, variants["off"].arena.flat)
    lines.append(f"headline step (config 2, B = 32, 512x512), SGD (lr {LR}), seg_metrics off / on: {rounds} alternating rounds of {steps} steps "
                 f"after 3 warm-up steps each, one process; parameters bitwise equal after all steps: {same}")
    lines.append(f"  counted pixels {int(ts.seg_counts[2].sum())} over {3 + steps * rounds} steps; aAcc {met['aAcc'].item():.4f}, mIoU {met['mIoU'].item():.4f} "
                 "(synthetic batch, untrained model)")
    for v in variants:
        r = res[v]
        lines.append(f"  {v:3s} median {statistics.median(r):7.3f} ms/step  (min {min(r):7.3f}, max {max(r):7.3f}; {32e3 / statistics.median(r):7.1f} img/s)")
    d = [x - y for x, y in zip(res["on"], res["off"])]
    lines.append(f"  on - off, round by round: median {statistics.median(d) * 1e3:+7.1f} us  (min {min(d) * 1e3:+7.1f}, max {max(d) * 1e3:+7.1f})"
                 f" = {statistics.median(d) / statistics.median(res['off']):+.2%} of the step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", default=None, choices=("launches", "step"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = Lines()
    if a.part == "launches":
        return launches(a.calls, a.rounds, lines)
    if a.part == "step":
        return step_ab(a.steps, a.rounds, lines)
    lines.append(f"command: python tools/seg_metrics_cost.py --calls {a.calls} --steps {a.steps} --rounds {a.rounds}")
    for part, limit in (("launches", 300), ("step", 400)):   # every GPU part under its own time limit, in a fresh process
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--part", part, "--calls",
                            str(a.calls), "--steps", str(a.steps), "--rounds", str(a.rounds)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"--part {part} failed ({r.returncode}): {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            lines.append(ln)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
