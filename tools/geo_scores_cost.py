"""Cost of warping a teacher's score map under a geometric view (lc2is_geo_scores, ops.geo_scores) at B = 32, g = 32, ld = 192,
L = 128: the scores of a 512 x 512 batch at patch 16 and 151 classes, the weight map at the labels' size.
  1. geo_scores on hand-written tables - all copy rows, flip only, scale 0.25 (zoomed out: most cells select the border) - and on the
     table of the class defaults (rotation within 20 degrees, scale 0.8 .. 1.25), each with the in-frame mask; time and TB/s over
     the ideal traffic, one read and one write of the scores plus the mask's write.
  2. (a) A copy_ of the score tensor [32*32*32, 192] fp32.
     (b) The torch composition of the same result from the same device table: permute to NCHW, affine_grid, grid_sample bilinear
         with border padding, permute back and contiguous; grid_sample nearest of ones and where for the mask and the copy rows.
  No target is set: the figures are what they are.  Where geo_scores does not beat (b), it says so.
  python tools/geo_scores_cost.py [--rounds 5] [--reps 50] [--out profiles/geo_scores_cost.txt]"""
import argparse
import math
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lc2is_amd import ops  # noqa: E402
from lc2is_amd.data import GeometricAugment  # noqa: E402

B, G, LD, L = 32, 32, 192, 128


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


def table(flags, deg=0.0, s=1.0, flip=False):
    """[B, 16] int32 rows of one map (host-made, as lc2is_geo_params would write it)."""
    cs, sn = math.cos(math.radians(deg)) / s, math.sin(math.radians(deg)) / s
    m = [round(cs * 65536), round(-sn * 65536), round(sn * 65536), round(cs * 65536)]
    if flip:
        m[0], m[2] = -m[0], -m[2]
    row = torch.zeros(ops.GEO_PARAM_WORDS, dtype=torch.int32)
    row[ops.GEO_FLAGS] = flags
    row[ops.GEO_M:ops.GEO_M + 4] = torch.tensor(m, dtype=torch.int32)
    return row.repeat(B, 1).contiguous()


def torch_scores(sc, tab):
    """The composition (b) from a device table; every tensor stays on the device, nothing is read back."""
    w = tab[:, ops.GEO_M:ops.GEO_M + 6].to(torch.float32) * (1.0 / 65536.0)
    theta = torch.stack([w[:, 0], w[:, 1], 2.0 * w[:, 4], w[:, 2], w[:, 3], 2.0 * w[:, 5]], dim=1).view(B, 2, 3)
    mapped = tab[:, ops.GEO_FLAGS] != 0
    x = sc.view(B, G, G, LD).permute(0, 3, 1, 2)
    y = F.grid_sample(x, F.affine_grid(theta, (B, LD, G, G), align_corners=False), "bilinear", "border", align_corners=False)
    out = torch.where(mapped[:, None, None, None], y, x).permute(0, 2, 3, 1).contiguous().view(B * G * G, LD)
    ones = torch.ones(B, 1, L, L, device=sc.device)
    m = F.grid_sample(ones, F.affine_grid(theta, (B, 1, L, L), align_corners=False), "nearest", "zeros", align_corners=False)[:, 0]
    return out, torch.where(mapped[:, None, None], m, ones[:, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geo_scores_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip()
    lines = [f"device: {torch.cuda.get_device_name(dev)}" + (f"; commit: {commit}" if commit else ""),
             f"command: python tools/geo_scores_cost.py --rounds {a.rounds} --reps {a.reps}",
             f"B = {B}, g = {G}, ld = {LD}, L = {L}; device events around trains of back-to-back calls on warm buffers (launch gaps "
             f"included), median (min .. max) of {a.rounds} rounds after one warm-up round, the arms alternating inside every round"]
    gen = torch.Generator(device=dev).manual_seed(1)
    sc = torch.randn(B * G * G, LD, device=dev, generator=gen)
    out = (torch.empty_like(sc), torch.empty(B, L, L, device=dev))
    keys = torch.arange(B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    geo = GeometricAugment(seed=1)
    tables = {"all copy rows": table(0), "flip only": table(ops.GEO_FLIP, flip=True), "scale 0.25": table(ops.GEO_WARP, 0.0, 0.25)}
    tables = {n: t.to(dev) for n, t in tables.items()}
    tables["class defaults"] = ops.geo_params(keys, epoch, geo.config)

    arms = [(f"geo_scores + mask, {n}", (lambda n=n: ops.geo_scores(sc, tables[n], B, G, label_size=L, out=out))) for n in tables]
    arms += [(f"geo_scores alone, {n}", (lambda n=n: ops.geo_scores(sc, tables[n], B, G, out=(out[0], None)))) for n in tables]
    arms += [(f"(a) copy_ of [{B * G * G},{LD}] fp32", lambda: out[0].copy_(sc))]
    arms += [(f"(b) torch composition, {n}", (lambda n=n: torch_scores(sc, tables[n]))) for n in tables]
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = event_time(fn, a.reps if "(b)" not in n else max(a.reps // 5, 2))
            if r:
                ts[n].append(dt)
    t = {n: median(v) for n, v in ts.items()}
    fl = tables["class defaults"].cpu()[:, ops.GEO_FLAGS]
    lines.append(f"class defaults: warp on {int((fl & 1).bool().sum())}, flip {int((fl & 2).bool().sum())} of {B} samples")
    for n in tables:
        got, ref = ops.geo_scores(sc, tables[n], B, G, label_size=L), torch_scores(sc, tables[n])
        lines.append(f"{n}: max |geo_scores - torch composition| = {float((got[0] - ref[0]).abs().max()):.2e} (the torch grid is fp32); mask "
                     f"cells that differ {float((got[1] != ref[1]).float().mean()) * 100:.3f} % (cell edges)")
    sc_bytes = 2 * sc.numel() * 4
    ideal = sc_bytes + out[1].numel() * 4
    copy_name = f"(a) copy_ of [{B * G * G},{LD}] fp32"
    for n, _ in arms:
        extra = ""
        if n.startswith("geo_scores + mask"):
            extra = f"   {ideal / t[n] / 1e12:6.2f} TB/s over {ideal / 1e6:.1f} MB (one read + one write of the scores, the mask's write)"
        elif n.startswith("geo_scores alone") or n.startswith("(a)"):
            extra = f"   {sc_bytes / t[n] / 1e12:6.2f} TB/s over {sc_bytes / 1e6:.1f} MB (one read + one write)"
        lines.append(f"  {n:44s} {t[n] * 1e6:9.1f} us ({min(ts[n]) * 1e6:.1f} .. {max(ts[n]) * 1e6:.1f}){extra}")
    for n in tables:
        mine, comp = t[f"geo_scores + mask, {n}"], t[f"(b) torch composition, {n}"]
        lines.append(f"  {n}: geo_scores with the mask takes {mine / comp:.3f}x the time of the torch composition ({comp / mine:.1f}x faster), "
                     f"{mine / t[copy_name]:.2f}x the copy" + ("" if mine < comp else "   <-- does NOT beat it"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
