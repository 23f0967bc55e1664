"""Cost of the mixed-sample step (data.SampleMix, lc2is_mix_select + lc2is_mix_apply) at the headline shapes: B = 32, S = 512,
L = 128, classmix on label maps of large regions.
  1. The select + apply launch pair, and each launch alone; the apply kernel's GB/s over its ideal bytes (one read and one write of
     [B,3,S,S] fp32 plus the label and weight maps).
  2. A copy_ of one [32,3,512,512] fp32 tensor: the same ideal bytes.
  3. The torch composition of the same result on the device, without the host-side unique: presence by one-hot amax, a random
     half of the present classes, the per-image isin as a gather of the chosen table, a repeat-interleaved mask and three wheres
     that read both batches.  Also with the presence as one scatter_ (no [B, L*L, K] one-hot), the leanest form we know.
  The one condition: the fused pair takes less time than the composition.
  python tools/mix_cost.py [--rounds 5] [--reps 50] [--out profiles/mix_cost.txt]"""
import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lc2is_amd import ops  # noqa: E402
from lc2is_amd.data import SampleMix  # noqa: E402

B, S, L, K = 32, 512, 128, 151


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


def region_maps(n, g, dev):
    """Large rectangular regions: a 4 x 4 grid of random classes 1..149 over a background class, the top eighth unlabelled (0)."""
    grid = torch.randint(1, 150, (n, 4, 4), device=dev, generator=g)
    grid[torch.rand(n, 4, 4, device=dev, generator=g) < 0.6] = 7
    lab = grid.repeat_interleave(L // 4, 1).repeat_interleave(L // 4, 2).contiguous()
    lab[:, :L // 8] = 0
    return lab


def torch_mix(dst, src, presence):
    """The composition; every tensor stays on the device.  (torch.isin has no per-image form: with the chosen classes as a [B, K]
    table the per-image membership test is one gather.)"""
    (dpx, dlab, dpw), (spx, slab, spw) = dst, src
    flat = slab.view(B, -1)
    if presence == "one_hot":
        present = F.one_hot(flat, K).amax(dim=1).bool()
    else:
        present = torch.zeros(B, K, dtype=torch.bool, device=flat.device).scatter_(1, flat, True)
    present[:, 0] = False                                                        # exclude_label = 0
    score = torch.rand(B, K, device=flat.device).masked_fill(~present, 2.0)
    k = (present.sum(dim=1) + 1) // 2
    thr = score.sort(dim=1).values.gather(1, (k - 1).clamp(min=0)[:, None])
    chosen = (score <= thr) & present
    mask = chosen.gather(1, flat).view(B, L, L)
    r = S // L
    big = mask.repeat_interleave(r, 1).repeat_interleave(r, 2)[:, None]
    return torch.where(big, spx, dpx), torch.where(mask, slab, dlab), torch.where(mask, spw, dpw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip()
    lines = [f"device: {torch.cuda.get_device_name(dev)}" + (f"; commit: {commit}" if commit else ""),
             f"command: python tools/mix_cost.py --rounds {a.rounds} --reps {a.reps}",
             f"B = {B}, S = {S}, L = {L}, classmix, {K} classes, exclude_label 0, label maps of large regions; device events around "
             f"trains of back-to-back calls on warm buffers (launch gaps included), medians of {a.rounds} rounds after one warm-up "
             "round, the arms alternating inside every round"]
    g = torch.Generator(device=dev).manual_seed(1)
    mk = lambda: (torch.randn(B, 3, S, S, device=dev, generator=g), region_maps(B, g, dev), torch.rand(B, L, L, device=dev, generator=g))
    dst, src = mk(), mk()
    out = (torch.empty_like(dst[0]), torch.empty_like(dst[1]), torch.empty_like(dst[2]))
    keys = torch.arange(B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    mix = SampleMix("classmix", n_classes=K, exclude_label=0, seed=1)
    plan = torch.empty(B, ops.MIX_PLAN_WORDS, dtype=torch.int32, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    copy_dst = torch.empty_like(dst[0])

    arms = (("select + apply (SampleMix)", lambda: mix(dst, src, keys, epoch, out=out)),
            ("mix_select alone", lambda: ops.mix_select(src[1], keys, epoch, mix.config, plan=plan, info=info)),
            ("mix_apply alone", lambda: ops.mix_apply(dst, src, plan, out=out)),
            ("copy_ of [32,3,512,512] fp32", lambda: copy_dst.copy_(dst[0])),
            ("torch composition, one-hot amax", lambda: torch_mix(dst, src, "one_hot")),
            ("torch composition, scatter_", lambda: torch_mix(dst, src, "scatter")))
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = event_time(fn, a.reps if "one-hot" not in n else max(a.reps // 10, 2))
            if r:
                ts[n].append(dt)
    t = {n: median(v) for n, v in ts.items()}
    i = mix.last_info.cpu()
    lines.append(f"classes present per sample {int(i[:, 0].min())}..{int(i[:, 0].max())}, chosen {int(i[:, 1].min())}..{int(i[:, 1].max())}, "
                 f"masked cells {float(i[:, 2].sum()) / float(i[:, 3].sum()):.3f} of the batch")
    px_bytes = 2 * dst[0].numel() * 4
    ideal = px_bytes + B * L * L * (2 * 8 + 2 * 4)
    for n, _ in arms:
        extra = ""
        if n == "mix_apply alone":
            extra = f"   {ideal / t[n] / 1e9:7.0f} GB/s over its {ideal / 1e6:.1f} MB of ideal traffic"
        if n.startswith("copy_"):
            extra = f"   {px_bytes / t[n] / 1e9:7.0f} GB/s over {px_bytes / 1e6:.1f} MB"
        lines.append(f"  {n:36s} {t[n] * 1e6:9.1f} us{extra}")
    pair = t[arms[0][0]]
    for n in (arms[4][0], arms[5][0]):
        lines.append(f"  the fused pair takes {pair / t[n]:.3f}x the time of the {n} ({t[n] / pair:.1f}x faster)")
    ok = pair < t[arms[4][0]]
    lines.append("condition (the fused pair takes less time than the torch composition of the same result): " + ("MET" if ok else "NOT MET"))
    if not ok or pair >= t[arms[5][0]]:
        lines.append(f"  where the pair's time goes: select {t[arms[1][0]] * 1e6:.1f} us (one block per sample, {B} blocks: latency-bound), "
                     f"apply {t[arms[2][0]] * 1e6:.1f} us, against {t[arms[3][0]] * 1e6:.1f} us for the copy of the same bytes")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
