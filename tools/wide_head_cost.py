#!/usr/bin/env python3
"""What the fused head costs past 192 classes, taken in one call and written to profiles/wide_head_cost.txt:
  resources     registers, scratch and occupancy of the kernels of head_wide.hip as hipcc reports them (no GPU needed), and the
                dynamic LDS the launchers ask for;
  launch pairs  at the headline head shape (B = 32, h = w = 32, S = 4 bicubic) on warm buffers, device events around trains of
                back-to-back calls, the variants alternated round by round:
                  K = 192       ops.head_upsample_ce(class_weight=w) against ops.head_upsample_ce_wide(class_weight=w), loss +
                                gradient, and ops.head_upsample_argmax against ops.head_upsample_argmax_wide, on the same buffers:
                                what the second sweep and the restaging cost at equal work;
                  K = 256, 512, 847, 1024   the wide pairs alone, with the time per class and the workspace bytes beside each;
  accuracy      the worst figures of the wide cross-entropy against fp64 over the cases of tests/wide_head_ref.py.
No number is a gate: the figures are this commit's own.
usage: python tools/wide_head_cost.py [--calls N] [--rounds R] [--out FILE]"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402

B, H, S = 32, 32, 4
WIDE_K = (256, 512, 847, 1024)


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


def resources(lines):
    import check_kernel_resources as ckr
    rows = ckr.one(ckr.CSRC / "head_wide.hip")
    names = ckr.demangle([r["name"] for r in rows])
    lines.append("resources of head_wide.hip (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; 512 threads = 2 waves per SIMD per "
                 "block, so 4 waves / SIMD = two blocks per CU; MODE 0 bicubic, 1 bilinear):")
    for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
        n = n.split("(")[0].replace("void ", "")
        if "wide" in n:
            lines.append(f"  {n:40s} VGPR {r.get('vgpr', 0):4d}  AGPR {r.get('agpr', 0):3d}  scratch {r.get('scratch', 0):3d}  "
                         f"occupancy by registers {r.get('occ', 0)} waves/SIMD  static LDS {r.get('lds', 0)} B")
    ce = {m: 2 * f * f * 196 * 4 + 4 * 1024 for m, f in (("bicubic", 7), ("bilinear", 5))}
    am = {m: max(f * f * 196, 4 * 3 * 1024) * 4 + 3 * 1024 for m, f in (("bicubic", 7), ("bilinear", 5))}
    lines.append(f"  dynamic LDS per block: head_ce_wide_grp_kernel {ce['bicubic']} B bicubic / {ce['bilinear']} B bilinear (chunk "
                 "footprint + mirror + four [16][16] tiles), any C;")
    lines.append(f"    head_argmax_wide_grp_kernel at most {am['bicubic']} B (count rows [4][3][1024] in the footprint's place + three tiles); "
                 "both inside 80 KB: two blocks per CU by LDS and by registers (<= 128 VGPRs), no scratch")


def launches(calls, rounds, lines):
    from lc2is_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    labels_all = torch.randint(0, 1 << 30, (B, H * S, H * S), generator=g)
    lines.append(f"launch pairs on {torch.cuda.get_device_name(0)}: B = {B}, h = w = {H}, S = {S} bicubic, class weights, loss + gradient "
                 f"(the launch and its finish launch) and class map + counts; {rounds} alternating rounds of {calls} back-to-back calls "
                 "after one warm-up train each; median us/call (min, max)")

    def bufs(K):
        ld = ops.class_pad(K)
        lo = torch.zeros(B * H * H, ld)
        lo[:, :K] = torch.randn(B * H * H, K, generator=g) * 3
        labels = labels_all % K
        labels[:, 1::9] = -100
        return lo.to(dev), labels.to(dev), (torch.rand(K, generator=g) * 1.5 + 0.25).to(dev), ld

    def run(variants):
        for fn in variants.values():
            timed(fn, calls)
        res = {v: [] for v in variants}
        for _ in range(rounds):
            for v, fn in variants.items():
                res[v].append(timed(fn, calls))
        return res

    def fmt(r):
        return f"{statistics.median(r) * 1e3:9.1f} ({min(r) * 1e3:8.1f}, {max(r) * 1e3:8.1f})"

    K = 192
    lo, labels, w, ld = bufs(K)
    m = ops.INTERP_BICUBIC
    res = run({
        "ce narrow": lambda: ops.head_upsample_ce(lo, labels, B, H, H, K, S, m, want_grad=True, class_weight=w),
        "ce wide": lambda: ops.head_upsample_ce_wide(lo, labels, B, H, H, K, S, m, want_grad=True, class_weight=w),
        "argmax narrow": lambda: ops.head_upsample_argmax(lo, labels, B, H, H, K, S, m),
        "argmax wide": lambda: ops.head_upsample_argmax_wide(lo, labels, B, H, H, K, S, m),
    })
    lines.append(f"  K = {K} (ld {ld}), narrow against wide on the same buffers:")
    for v, r in res.items():
        lines.append(f"    {v:14s} {fmt(r)}")
    for a, b in (("ce narrow", "ce wide"), ("argmax narrow", "argmax wide")):
        lines.append(f"    {b} / {a}: {statistics.median(res[b]) / statistics.median(res[a]):.2f}x")
    ce192, am192 = statistics.median(res["ce wide"]), statistics.median(res["argmax wide"])
    lines.append("  wide kernels alone:    K     ld  chunks   ce us/call (min, max)            us/class  x K=192    ce workspace   "
                 "argmax us/call (min, max)        us/class   argmax workspace")
    for K in WIDE_K:
        del lo, labels, w
        torch.cuda.empty_cache()
        lo, labels, w, ld = bufs(K)
        res = run({
            "ce": lambda: ops.head_upsample_ce_wide(lo, labels, B, H, H, K, S, m, want_grad=True, class_weight=w),
            "argmax": lambda: ops.head_upsample_argmax_wide(lo, labels, B, H, H, K, S, m),
        })
        wce = ops._fn("lc2is_head_upsample_ce_wide_workspace_bytes")(B, H, H, K, ld, S, m, 1)
        wam = ops._fn("lc2is_head_upsample_argmax_wide_workspace_bytes")(B, H, H, K, S, m)
        ce, am = statistics.median(res["ce"]), statistics.median(res["argmax"])
        lines.append(f"                      {K:5d}  {ld:5d}  {(K + 191) // 192:6d}   {fmt(res['ce'])}  {ce * 1e3 / K:8.2f}  {ce / ce192:6.2f}x  "
                     f"{wce / 2 ** 20:9.1f} MiB   {fmt(res['argmax'])}  {am * 1e3 / K:8.2f}  {wam / 2 ** 20:9.1f} MiB")
    lines.append(f"  (K = 192 wide: ce {ce192 * 1e3 / 192:.2f} us/class, argmax {am192 * 1e3 / 192:.2f} us/class; the [B, K, 128, 128] fp32 map these "
                 f"calls never form would be {B * 128 * 128 * 4 / 2 ** 20:.0f} MiB per class)")


def accuracy(lines):
    import wide_head_ref as R
    from lc2is_amd import ops
    dev = torch.device("cuda", 0)
    worst = dict(loss=0.0, wsum=0.0, grad=0.0, pad=0.0)
    for case, (Bc, h, w, mode, C) in enumerate(R.CASES):
        for weighted in (False, True):
            lo, labels, w64, (rl, rw, rg) = R.case_ref(case, weighted)
            cw = w64.float().to(dev) if weighted else None
            m = ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR
            loss, dlo = ops.head_upsample_ce_wide(lo.to(dev), labels.to(dev), Bc, h, w, C, 4, m, want_grad=True, class_weight=cw)
            d = dlo.cpu().double()
            fig = dict(loss=abs(loss[0].item() - rl) / abs(rl), wsum=abs(loss[1].item() - rw) / rw,
                       grad=((d[:, :C] - rg).norm() / rg.norm()).item(), pad=d[:, C:].abs().max().item() if d.shape[1] > C else 0.0)
            worst = {k: max(worst[k], fig[k]) for k in worst}
    lines.append(f"accuracy of ops.head_upsample_ce_wide against fp64 (F.interpolate + F.cross_entropy), worst over the {len(R.CASES)} cases of "
                 "tests/wide_head_ref.py (C = 193 .. 1024, bicubic and bilinear), with and without class weights:")
    lines.append(f"  relative loss error {worst['loss']:.2e} (bound 1e-4 x ld / 192), weight-sum error {worst['wsum']:.2e} (1e-5), gradient relative "
                 f"L2 {worst['grad']:.2e} (2e-5 x ld / 192), largest |gradient| in the pad channels {worst['pad']:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", default=None, choices=["launches", "accuracy"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wide_head_cost.txt"))
    a = ap.parse_args()
    lines = Lines()
    if a.part == "launches":
        return launches(a.calls, a.rounds, lines)
    if a.part == "accuracy":
        return accuracy(lines)
    lines.append(f"command: python tools/wide_head_cost.py --calls {a.calls} --rounds {a.rounds}")
    resources(lines)
    # every GPU part under its own time limit, in a fresh process; a part that fails ends the run
    for part, limit in (("launches", 300), ("accuracy", 120)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--part", part, "--calls",
                            str(a.calls), "--rounds", str(a.rounds)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"--part {part} failed ({r.returncode}): {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            lines.append(ln)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
