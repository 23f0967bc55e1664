"""Cost of the cross-entropy options in the fused upsample + CE head (ops.head_upsample_ce, gradient on): the default kernel
against the class-weighted one and the class-weighted + label-smoothed one, at the bench head shape (32 x 32x32 -> 128x128,
151 classes, bicubic x4) and at the AuxiliaryLoss shape (32 -> 512, bilinear x16).  The variants alternate in one process
after a warm-up; each sample is one call (tile kernel + fixed-order finish), timed with HIP events.  The register / scratch
report of the head kernels (tools/check_kernel_resources.py) is printed after the timings.
  python tools/ce_opts_cost.py [--iters 50] [--out profiles/ce_opts_cost.txt]"""
import argparse
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from lc2is_amd import ops  # noqa: E402

SHAPES = (("bench head: bicubic x4, 151 classes, 32 x 32x32 -> 128x128", 32, 32, 151, ops.INTERP_BICUBIC, 4),
          ("AuxiliaryLoss: bilinear x16, 151 classes, 32 x 32x32 -> 512x512", 32, 32, 151, ops.INTERP_BILINEAR, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ce_opts_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(dev)}; {a.iters} alternating samples per variant after 5 warm-up rounds"]
    for name, B, h, C, mode, S in SHAPES:
        g = torch.Generator().manual_seed(1)
        lo = torch.zeros(B * h * h, 192)
        lo[:, :C] = torch.randn(B * h * h, C, generator=g) * 3
        lo = lo.to(dev)
        labels = torch.randint(0, C, (B, S * h, S * h), generator=g).to(dev)
        w = (torch.rand(C, generator=g) + 0.5).to(dev)
        variants = (("default", {}), ("weighted", dict(class_weight=w)),
                    ("weighted + smoothed 0.1", dict(class_weight=w, label_smoothing=0.1)))
        run = lambda kw: ops.head_upsample_ce(lo, labels, B, h, h, C, S, mode, want_grad=True,
                                              grad_scale=1.0 / labels.numel(), **kw)
        for _ in range(5):
            for _, kw in variants:
                run(kw)
        torch.cuda.synchronize()
        ts = {v: [] for v, _ in variants}
        for _ in range(a.iters):
            for v, kw in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(kw)
                e1.record()
                torch.cuda.synchronize()
                ts[v].append(e0.elapsed_time(e1) * 1e3)
        lines.append(name)
        base = sorted(ts["default"])[len(ts["default"]) // 2]
        for v, _ in variants:
            t = sorted(ts[v])
            med = t[len(t) // 2]
            lines.append(f"  {v:26s} median {med:8.1f} us  best {t[0]:8.1f} us  ({100.0 * (med / base - 1.0):+.1f} % vs default)")
    print("\n".join(lines), flush=True)
    res = subprocess.run([sys.executable, str(ROOT / "tools" / "check_kernel_resources.py"), "-j", "8"], capture_output=True,
                         text=True)
    head = [ln for ln in res.stdout.splitlines() if re.match(r"(void )?(head_ce_grp_kernel|head_finish_kernel|ce_nchw_)", ln)
            or ln.startswith("kernel ")]
    lines += ["", "tools/check_kernel_resources.py (head.hip and loss_nchw.hip rows; exit status %d):" % res.returncode] + head
    lines.append(res.stdout.strip().splitlines()[-1] if res.stdout.strip() else "(no output)")
    print("\n".join(lines[-len(head) - 3:]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
