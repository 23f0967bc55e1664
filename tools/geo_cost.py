"""Cost of the geometric views (data.GeometricAugment, lc2is_geo_params + lc2is_geo_apply) at B = 32, S = 512, L = 128.
  1. geo_apply alone on hand-written tables - all copy rows, flip only, 10 degrees at scale 1, 45 degrees at scale 0.8, 90 degrees,
     scale 0.25 (zoomed out: the largest source footprint) - and the params + apply launch pair at the class defaults; time and TB/s
     over the ideal traffic, one read and one write of pixels, labels and weights.
  2. (a) A copy_ of one [32,3,512,512] fp32 tensor.
     (b) strong_apply with no blur and mix_apply on the same buffers: the copy-row case moves the same bytes the same way.
     (c) The torch composition of the same result from the same device table: affine_grid, grid_sample bilinear on the pixels,
         grid_sample nearest on labels and weights, where for the ignore label and for the rows that are copies.
  The one claim: geo_apply takes less time than (c) in every case.  Where a case does not, it says so.
  The direct form against the staged form of the mapped path: tools/probes/geo_staged (a stand-alone program).
  python tools/geo_cost.py [--rounds 5] [--reps 50] [--out profiles/geo_cost.txt]"""
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
from lc2is_amd.data import GeometricAugment, SampleMix, StrongAugment  # noqa: E402

B, S, L = 32, 512, 128
IGNORE = -100


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


def torch_geo(x, lab, pw, tab):
    """The composition (c) from a device table; every tensor stays on the device, nothing is read back."""
    w = tab[:, ops.GEO_M:ops.GEO_M + 6].to(torch.float32) * (1.0 / 65536.0)
    theta = torch.stack([w[:, 0], w[:, 1], 2.0 * w[:, 4], w[:, 2], w[:, 3], 2.0 * w[:, 5]], dim=1).view(B, 2, 3)
    mapped = tab[:, ops.GEO_FLAGS] != 0
    px = F.grid_sample(x, F.affine_grid(theta, (B, 3, S, S), align_corners=False), "bilinear", "zeros", align_corners=False)
    both = torch.stack([lab.to(torch.float32) + 1.0, pw], dim=1)
    o = F.grid_sample(both, F.affine_grid(theta, (B, 2, L, L), align_corners=False), "nearest", "zeros", align_corners=False)
    lab2 = torch.where(o[:, 0] == 0, IGNORE, o[:, 0].to(torch.int64) - 1)
    return (torch.where(mapped[:, None, None, None], px, x), torch.where(mapped[:, None, None], lab2, lab),
            torch.where(mapped[:, None, None], o[:, 1], pw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geo_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip()
    lines = [f"device: {torch.cuda.get_device_name(dev)}" + (f"; commit: {commit}" if commit else ""),
             f"command: python tools/geo_cost.py --rounds {a.rounds} --reps {a.reps}",
             f"B = {B}, S = {S}, L = {L}; device events around trains of back-to-back calls on warm buffers (launch gaps included), "
             f"median (min .. max) of {a.rounds} rounds after one warm-up round, the arms alternating inside every round"]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    lab = torch.randint(0, 150, (B, L, L), device=dev, generator=g)
    pw = torch.rand(B, L, L, device=dev, generator=g)
    out = (torch.empty_like(x), torch.empty_like(lab), torch.empty_like(pw))
    keys = torch.arange(B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    geo = GeometricAugment(seed=1)
    cfg = geo.config
    tables = {"all copy rows": table(0), "flip only": table(ops.GEO_FLIP, flip=True), "10 degrees, scale 1": table(ops.GEO_WARP, 10.0),
              "45 degrees, scale 0.8": table(ops.GEO_WARP, 45.0, 0.8), "90 degrees": table(ops.GEO_WARP, 90.0),
              "scale 0.25": table(ops.GEO_WARP, 0.0, 0.25)}
    tables = {n: t.to(dev) for n, t in tables.items()}
    tables["class defaults"] = ops.geo_params(keys, epoch, cfg)
    params = torch.empty(B, ops.GEO_PARAM_WORDS, dtype=torch.int32, device=dev)
    # (b) on the same pixel buffers: strong_apply without blur (jitter on), mix_apply with a classmix plan of half the cells
    strong = StrongAugment(blur_prob=0.0, seed=1)
    stab = ops.strong_params(keys, epoch, strong.config)
    lab4 = torch.randint(1, 150, (B, 4, 4), device=dev, generator=g).repeat_interleave(L // 4, 1).repeat_interleave(L // 4, 2).contiguous()
    x2 = torch.randn(B, 3, S, S, device=dev, generator=g)
    mix = SampleMix("classmix", n_classes=151, exclude_label=0, seed=1)
    plan, _ = ops.mix_select(lab4, keys, epoch, mix.config)

    arms = [(f"geo_apply, {n}", (lambda n=n: ops.geo_apply((x, lab, pw), tables[n], cfg, out=out))) for n in tables]
    arms += [("params + apply, class defaults", lambda: geo((x, lab, pw), keys, epoch, out=out)),
             ("geo_params alone", lambda: ops.geo_params(keys, epoch, cfg, out=params)),
             ("(a) copy_ of [32,3,512,512] fp32", lambda: out[0].copy_(x)),
             ("(b) strong_apply, no blur", lambda: ops.strong_apply(x, stab, strong.config, out=out[0])),
             ("(b) mix_apply on the same buffers", lambda: ops.mix_apply((x, lab4, pw), (x2, lab4, pw), plan, out=out))]
    arms += [(f"(c) torch composition, {n}", (lambda n=n: torch_geo(x, lab, pw, tables[n]))) for n in tables]
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = event_time(fn, a.reps if "(c)" not in n else max(a.reps // 5, 2))
            if r:
                ts[n].append(dt)
    t = {n: median(v) for n, v in ts.items()}
    tab = tables["class defaults"].cpu()
    fl = tab[:, ops.GEO_FLAGS]
    lines.append(f"class defaults: warp on {int((fl & 1).bool().sum())}, flip {int((fl & 2).bool().sum())} of {B} samples")
    for n in tables:
        got, ref = ops.geo_apply((x, lab, pw), tables[n], cfg), torch_geo(x, lab, pw, tables[n])
        lines.append(f"{n}: max |geo_apply - torch composition| = {float((got[0] - ref[0]).abs().max()):.2e} (normalised units; the torch "
                     f"grid is fp32); label cells that differ {float((got[1] != ref[1]).float().mean()) * 100:.3f} %, weights "
                     f"{float((got[2] != ref[2]).float().mean()) * 100:.3f} % (cell edges)")
    px_bytes = 2 * x.numel() * 4
    ideal = px_bytes + 2 * lab.numel() * 12
    for n, _ in arms:
        extra = ""
        if n.startswith("geo_apply") or n.startswith("(b) mix"):
            extra = f"   {ideal / t[n] / 1e12:6.2f} TB/s over {ideal / 1e6:.1f} MB (one read + one write, maps included)"
        elif n.startswith("(a)") or n.startswith("(b) strong"):
            extra = f"   {px_bytes / t[n] / 1e12:6.2f} TB/s over {px_bytes / 1e6:.1f} MB (one read + one write)"
        lines.append(f"  {n:44s} {t[n] * 1e6:9.1f} us ({min(ts[n]) * 1e6:.1f} .. {max(ts[n]) * 1e6:.1f}){extra}")
    ok = True
    for n in tables:
        mine, comp = t[f"geo_apply, {n}"], t[f"(c) torch composition, {n}"]
        ok = ok and mine < comp
        lines.append(f"  {n}: geo_apply takes {mine / comp:.3f}x the time of the torch composition ({comp / mine:.1f}x faster), "
                     f"{mine / t['(a) copy_ of [32,3,512,512] fp32']:.2f}x the copy, {mine / t['(b) strong_apply, no blur']:.2f}x strong_apply, "
                     f"{mine / t['(b) mix_apply on the same buffers']:.2f}x mix_apply" + ("" if mine < comp else "   <-- does NOT beat it"))
    lines.append("claim (geo_apply takes less time than the torch composition of the same result, in every case): " + ("MET" if ok else "NOT MET"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
