"""Cost of the original-size mIoU (metrics.compute_gt_mIOU, reference metrics.py:61-79): the fused resize + argmax + counts kernel
(ops.resize_argmax, one call per batch) against the literal torch path the reference runs (per image: F.interpolate(size=) to the
original size, argmax, bincount of the confusion counts; on the GPU, in this tool only), K = 151 classes on a 128 x 128 score grid,
batches of 32 images and of 1 image at 683 x 512 and at 2048 x 1536.  The fused call holds the whole batch at once (channels-last
copy of the scores, 10 MB per image, packed gt, per-tile counts); the literal loop one image's [K, H, W] map at a time.  The two
alternate in one process after a warm-up; each sample is one batch ended by a device synchronise; the peak is the allocator's peak
growth over the memory held before the call.  The predictions of the two paths are compared (they may differ at near-tie pixels:
fp32 sums in another order).
  python tools/gt_miou_cost.py [--rounds 5] [--batch 32] [--commit ID] [--out profiles/gt_miou_cost.txt]"""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lc2is_amd import ops  # noqa: E402

K, h = 151, 128
SIZES = ((683, 512), (2048, 1536))


def literal(x, sizes, gt):
    """The reference's loop, on the GPU: full [K, H, W] score map per image, argmax, counts."""
    counts, preds = [], []
    for i, s in enumerate(sizes):
        y = F.interpolate(x[i:i + 1], size=s, mode="bicubic", align_corners=False)[0]
        p = y.argmax(0).reshape(-1)
        g = gt[i].reshape(-1).long()
        lab = (g >= 0) & (g < K)
        counts.append(torch.stack([torch.bincount(p[lab & (p == g)], minlength=K), torch.bincount(p, minlength=K),
                                   torch.bincount(g[lab], minlength=K)]))
        preds.append(p)
    return preds, torch.stack(counts)


def fused(x, sizes, gt):
    preds, counts = ops.resize_argmax(x, sizes, gt=gt)
    return [p.reshape(-1) for p in preds], counts


def sample(fn, x, sizes, gt, dev):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    out = fn(x, sizes, gt)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, torch.cuda.max_memory_allocated(dev) - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_miou_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() or "unknown"
    lines = [f"device: {torch.cuda.get_device_name(dev)}; commit: {commit}",
             "command: python tools/gt_miou_cost.py" + "".join(f" --{k} {v}" for k, v in (("rounds", a.rounds), ("batch", a.batch))),
             f"K = {K}, scores {h} x {h}; {a.rounds} alternating rounds after 1 warm-up; times are medians"]
    for (H, W), B in [(s, b) for s in SIZES for b in (a.batch, 1)]:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, K, h, h, generator=g).to(dev)
        gt = torch.randint(0, K, (B, H, W), generator=g).to(dev)
        gt_list = list(gt)
        sizes = [(H, W)] * B
        arms = (("fused (ops.resize_argmax)", fused), ("literal (F.interpolate + argmax + bincount)", literal))
        ts = {n: [] for n, _ in arms}
        peak = {n: 0 for n, _ in arms}
        outs = {}
        for r in range(a.rounds + 1):
            for n, fn in arms:
                dt, pk, out = sample(fn, x, sizes, gt_list, dev)
                if r:
                    ts[n].append(dt)
                peak[n] = max(peak[n], pk)
                outs[n] = out
                del out
        lines.append(f"{H} x {W}, batch {B}:")
        for n, _ in arms:
            t = sorted(ts[n])[len(ts[n]) // 2]
            lines.append(f"  {n:46s} {t * 1e6 / B:10.1f} us/image  peak +{peak[n] / 2**20:9.1f} MiB")
        (pf, cf), (pl, cl) = outs[arms[0][0]], outs[arms[1][0]]
        diff = sum(int((p1.long() != p2).sum()) for p1, p2 in zip(pf, pl))
        lines.append(f"  pixels whose prediction differs: {diff} of {B * H * W}; counts equal: {torch.equal(cf, cl.int())}")
        tf, tl = sorted(ts[arms[0][0]])[a.rounds // 2], sorted(ts[arms[1][0]])[a.rounds // 2]
        lines.append(f"  literal / fused: {tl / tf:.1f}x time, {peak[arms[1][0]] / max(peak[arms[0][0]], 1):.1f}x peak memory")
        del x, gt, gt_list, outs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
