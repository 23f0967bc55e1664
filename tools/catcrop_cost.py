"""Cost of the class-ratio crop re-draw (TrainAugment(cat_max_ratio=0.75), lc2is_aug_crop_select) at the headline shapes: B = 32,
S = 512, L = 128 on a pool of ADE20K-like images (683 x 512 and 512 x 683 mixed).
  1. One batch through params + apply against params + select + apply (device events around trains of calls, alternating), on
     label maps of large rectangular regions, where some samples are taken at once and some are drawn again.
  2. The select launch alone on label maps where every sample is accepted at once (8 x 8 blocks of random classes) and on constant
     maps, where every sample exhausts its tries (ten candidates counted, the worst case).
  3. DeviceImagePool.class_counts over the pool (lc2is_label_histogram).
  python tools/catcrop_cost.py [--rounds 5] [--reps 200] [--out profiles/catcrop_cost.txt]"""
import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from lc2is_amd import ops  # noqa: E402
from lc2is_amd.data import DeviceImagePool, TrainAugment  # noqa: E402

B, S, L = 32, 512, 128


def event_time(fn, reps):
    """Mean device time of `reps` back-to-back calls (events around the train), seconds."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def median(v):
    return sorted(v)[len(v) // 2]


def region_map(h, w, g, dev):
    """Large rectangular regions: a 4 x 4 grid of random classes 1..149 over a background class, the top eighth unlabelled (0)."""
    grid = torch.randint(1, 150, (4, 4), device=dev, generator=g)
    grid[torch.rand(4, 4, device=dev, generator=g) < 0.6] = 7
    lab = grid.repeat_interleave(-(-h // 4), 0).repeat_interleave(-(-w // 4), 1)[:h, :w].to(torch.uint8).contiguous()
    lab[:h // 8] = 0
    return lab


def block_map(h, w, g, dev):
    grid = torch.randint(1, 150, (-(-h // 8), -(-w // 8)), device=dev, generator=g)
    return grid.repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w].to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pool", type=int, default=64, help="images in each pool")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("catcrop_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip()
    lines = [f"device: {torch.cuda.get_device_name(dev)}" + (f"; commit: {commit}" if commit else ""),
             f"command: python tools/catcrop_cost.py --rounds {a.rounds} --reps {a.reps} --pool {a.pool}",
             f"B = {B}, S = {S}, L = {L}, cat_max_ratio = 0.75, ignore label 0, 10 tries; pools of {a.pool} images, 683 x 512 and "
             "512 x 683 alternating; device events around trains of back-to-back calls (launch gaps included), medians of "
             f"{a.rounds} rounds after one warm-up round, the arms of a table alternating inside every round"]
    g = torch.Generator(device=dev).manual_seed(1)
    shapes = [(683, 512) if k % 2 == 0 else (512, 683) for k in range(a.pool)]
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g) for h, w in shapes]
    pools = {"regions": DeviceImagePool.from_arrays(imgs, [region_map(h, w, g, dev) for h, w in shapes], device=dev),
             "blocks": DeviceImagePool.from_arrays(imgs, [block_map(h, w, g, dev) for h, w in shapes], device=dev),
             "constant": DeviceImagePool.from_arrays(imgs, [torch.full((h, w), 9, dtype=torch.uint8, device=dev) for h, w in shapes],
                                                     device=dev)}
    off = TrainAugment(crop_size=S, label_size=L, seed=1)
    on = TrainAugment(crop_size=S, label_size=L, seed=1, cat_max_ratio=0.75)
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {"pixel_values": torch.empty(B, 3, S, S, device=dev), "label": torch.empty(B, L, L, dtype=torch.int64, device=dev)}

    def spread(info):
        t = info[:, 0].cpu().tolist()
        return ", ".join(f"t*={v}: {t.count(v)}" for v in sorted(set(t)))

    # ---- 1. the batch with and without the rule
    pool = pools["regions"]
    arms = (("params + apply (cat_max_ratio=None)", lambda: off(pool, idx, epoch, out=out)),
            ("params + select + apply", lambda: on(pool, idx, epoch, out=out)))
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = event_time(fn, a.reps)
            if r:
                ts[n].append(dt)
    lines.append(f"1. one batch, label maps of large regions ({spread(on.last_crop_info)}):")
    for n, _ in arms:
        lines.append(f"  {n:40s} {median(ts[n]) * 1e6:8.1f} us per batch")
    lines.append(f"  the rule adds {(median(ts[arms[1][0]]) - median(ts[arms[0][0]])) * 1e6:.1f} us per batch "
                 f"({median(ts[arms[1][0]]) / median(ts[arms[0][0]]):.3f}x)")

    # ---- 2. the select launch alone
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    raws = {k: off.params(p, idx, epoch) for k, p in pools.items()}
    rows = torch.empty_like(raws["regions"])

    def select(k):
        rows.copy_(raws[k])       # the launch rewrites top / left: start every call from the raw draw (a 2.5 KB copy, in every arm)
        ops.aug_crop_select(pools[k].labels, pools[k].desc, idx, epoch, on.config, rows, L, ratio1024=on.cat_ratio1024,
                            ignore_label=on.cat_ignore_label, tries=on.cat_tries, info=info)

    ts = {k: [] for k in pools}
    ts["copy"] = []
    spreads = {}
    for r in range(a.rounds + 1):
        for k in pools:
            dt = event_time(lambda: select(k), a.reps)
            spreads[k] = spread(info)
            if r:
                ts[k].append(dt)
        dt = event_time(lambda: rows.copy_(raws["regions"]), a.reps)
        if r:
            ts["copy"].append(dt)
    cells = B * L * L
    lines.append(f"2. aug_crop_select_kernel alone ({B} blocks of 1024 lanes; {cells} one-byte gathers per candidate and batch); every "
                 f"call includes the {median(ts['copy']) * 1e6:.1f} us copy of the raw rows:")
    for k, what in (("blocks", "every sample accepted at once"), ("regions", "mixed"), ("constant", "every sample exhausts 10 tries")):
        lines.append(f"  {k:9s} {median(ts[k]) * 1e6:8.1f} us per launch + copy  ({what}; {spreads[k]})")

    # ---- 3. class counts of the pool
    t = []
    for r in range(a.rounds + 1):
        dt = event_time(lambda: pools["regions"].class_counts(), 20)
        if r:
            t.append(dt)
    px = sum(h * w for h, w in shapes)
    lines.append(f"3. DeviceImagePool.class_counts over {a.pool} images ({px / 1e6:.1f} M labels, one block per image): "
                 f"{median(t) * 1e6:.1f} us = {px / median(t) / 1e9:.1f} G labels/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
