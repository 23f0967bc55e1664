#!/usr/bin/env python3
"""What the two self-training kernels cost on the fused head, taken in one call and written to profiles/selftrain_cost.txt, both at
the headline head shape (B = 32, h = w = 32, S = 4 bicubic, K = 151) on the same warm buffers, device events around trains of
back-to-back calls, the two sides alternated round by round:
  conf     ops.head_upsample_conf(thresh, want_counts=True) — pred + conf + pseudo + counts, the kernel and its finish launch —
           against ops.head_upsample_argmax pred-only (one launch); two rows in between (pred only; pred + conf) split the
           difference into the softmax denominator, the stores and the counts' finish launch;
  ce_pw    ops.head_upsample_ce_pw(class_weight=w, want_grad=True) against ops.head_upsample_ce(class_weight=w, want_grad=True) —
           the OPT pair that moves the same bytes but the pixel weights; each call is the forward + backward launch and the
           fixed-order finish launch.
The register / LDS figures of the new kernels (tools/check_kernel_resources.py's compile, no GPU needed) head the file.
No ratio is a gate: the figures are this commit's own, measured against its own existing paths.
usage: python tools/selftrain_cost.py [--calls N] [--rounds R] [--out FILE]"""
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

B, H, S, K, LD, THRESH = 32, 32, 4, 151, 192, 0.968


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
        lines.append(f"  {v:16s} median {statistics.median(r) * scale:9.2f} {unit}  (min {min(r) * scale:9.2f}, max {max(r) * scale:9.2f})")
    for other in names[1:]:   # every later row against the first, round by round
        d = [x - y for x, y in zip(res[other], res[names[0]])]
        lines.append(f"  {other} - {names[0]}, round by round: median {statistics.median(d) * scale:+9.2f} {unit}  (min "
                     f"{min(d) * scale:+9.2f}, max {max(d) * scale:+9.2f}); {other} / {names[0]} = "
                     f"{statistics.median(res[other]) / statistics.median(res[names[0]]):.3f}")


def resources(lines):
    """VGPRs / occupancy / scratch of the kernels of head_selftrain.hip and the LDS their launches ask for at ld = 192."""
    import check_kernel_resources as ck
    rows = ck.one(ck.CSRC / "head_selftrain.hip")
    names = [re.sub(r"\(.*", "", n).replace("void ", "") for n in ck.demangle([r["name"] for r in rows])]
    lines.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): <MODE 0 bicubic / 1 bilinear, TN, S>")
    for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
        if n.startswith("head_c"):
            lines.append(f"  {n:40s} VGPR {r.get('vgpr', 0):4d}  waves/SIMD {r.get('occ', 0):2d}  scratch {r.get('scratch', 0)}")
    cs = LD + 4
    lines.append(f"  dynamic LDS at ld = {LD}, bicubic S = 4 (7 x 7 footprint): head_conf_grp_kernel {(49 * cs + 3 * 256) * 4} bytes "
                 f"(footprint, inside tile, class tile, confidence tile); head_ce_pw_grp_kernel {(2 * 49 * cs + 256 + 192 + 256) * 4} "
                 "bytes (footprint, mirror, labels, class weights, pixel weights) + 64 static: two blocks per CU inside 160 KB")


def launches(calls, rounds, lines):
    from lc2is_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    lo = torch.zeros(B * H * H, LD)
    lo[:, :K] = torch.randn(B * H * H, K, generator=g) * 3
    labels = torch.randint(0, K, (B, H * S, H * S), generator=g)
    labels[:, 1::9] = -100
    pw = 2.0 * torch.rand(B, H * S, H * S, generator=g)
    lo, labels, pw = lo.to(dev), labels.to(dev), pw.to(dev)
    w = (torch.rand(K, generator=g) * 1.5 + 0.25).to(dev)
    geom = (B, H, H, K, S, ops.INTERP_BICUBIC)
    pairs = {
        # the two rows between the ends say where the time goes: the softmax denominator alone (pred only: the bytes of the argmax
        # launch), then the stores (conf fp32: + 4 bytes per pixel; pseudo int64: + 8), then the counts and their finish launch
        "conf": {"argmax (pred)": lambda: ops.head_upsample_argmax(lo, None, *geom, want_counts=False),
                 "conf (pred)": lambda: ops.head_upsample_conf(lo, *geom, want_conf=False),
                 "conf (pred+conf)": lambda: ops.head_upsample_conf(lo, *geom),
                 "conf (all 4)": lambda: ops.head_upsample_conf(lo, *geom, thresh=THRESH, want_counts=True)},
        "ce_pw": {"ce (OPT)": lambda: ops.head_upsample_ce(lo, labels, *geom, want_grad=True, class_weight=w),
                  "ce_pw": lambda: ops.head_upsample_ce_pw(lo, labels, pw, *geom, want_grad=True, class_weight=w)},
    }
    lines.append(f"launches on {torch.cuda.get_device_name(0)}: B = {B}, h = w = {H}, S = {S} bicubic, K = {K} (ld {LD}); {rounds} "
                 f"alternating rounds of {calls} back-to-back calls after one warm-up train each")
    for name, variants in pairs.items():
        for fn in variants.values():
            timed(fn, calls)
        res = {v: [] for v in variants}
        for _ in range(rounds):
            for v, fn in variants.items():
                res[v].append(timed(fn, calls))
        lines.append(f" {name}:")
        report(lines, res, "us/call", 1e3)
        med = {v: statistics.median(r) * 1e3 for v, r in res.items()}
        if name == "conf":
            a, p, pc, al = (med[v] for v in variants)
            lines.append(f"  where the time goes (all 4 / argmax = {al / a:.3f}; head_px's pair stands at 1.28 x, profiles/seg_metrics_cost.txt): "
                         f"the softmax denominator, which the argmax walk does not have — one fma, one exp2 and one add per (pixel, "
                         f"class) element on the VALU, 16 x TN of them per pixel — {p - a:+.1f} us; the fp32 confidence store (4 bytes "
                         f"per pixel) {pc - p:+.1f} us; the int64 pseudo-label store (8 bytes per pixel), the ballots and the counts' "
                         f"finish launch {al - pc:+.1f} us")
        else:
            c, w_ = (med[v] for v in variants)
            lines.append(f"  ce_pw / weighted CE = {w_ / c:.3f} (the focal kernel's pair stands at +4 %, profiles/focal_cost.txt): the pixel "
                         "weights add one 1 KB LDS tile, 4 bytes per pixel of reads and four multiplies per pixel quad; the kernel is "
                         "written on head_grp.h's shared staging and operand helpers, which head_ce_grp_kernel keeps as own lines")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", default=None, choices=["launches"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "selftrain_cost.txt"))
    a = ap.parse_args()
    lines = Lines()
    if a.part == "launches":
        return launches(a.calls, a.rounds, lines)
    lines.append(f"command: python tools/selftrain_cost.py --calls {a.calls} --rounds {a.rounds}")
    resources(lines)
    # the GPU part under its own time limit, in a fresh process; a part that fails ends the run
    r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, str(Path(__file__).resolve()), "--part", "launches", "--calls",
                        str(a.calls), "--rounds", str(a.rounds)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"--part launches failed ({r.returncode}): {r.stderr[-1500:]}")
    for ln in r.stdout.splitlines():
        lines.append(ln)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
