"""Cost of the strong photometric views (data.StrongAugment, lc2is_strong_params + lc2is_strong_apply) at B = 32, S = 512.
  1. The params + apply launch pair with blur off for every sample (jitter and grey at their defaults), with blur on for every
     sample at sigma = 2.0 (R = 8), and at the default mix (jitter 0.8, grey 0.2, blur 0.5, sigma in [0.1, 2.0]); each launch alone;
     the apply kernel's TB/s over its ideal traffic, one read and one write of [B,3,S,S] fp32.
  2. (a) A copy_ of one [32,3,512,512] fp32 tensor: the same ideal bytes.
     (b) mix_apply on the same buffers.
     (c) The torch composition of the same result on the device, given per-sample parameters that are already there (its host-side
         draws are not charged): de-normalise, a batched 3x3 einsum, clamp, reflect pad, a grouped conv2d with per-sample kernels
         (rows, then columns, at the largest radius), re-normalise, and a where each for the samples without colour / blur.
  The one claim: the launch pair takes less time than (c), with no host draw.  Where the all-blur case does not, it says so.
  python tools/strong_cost.py [--rounds 5] [--reps 50] [--out profiles/strong_cost.txt]"""
import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lc2is_amd import ops  # noqa: E402
from lc2is_amd.data import SampleMix, StrongAugment  # noqa: E402

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


def torch_strong(x, table, cfg):
    """The composition (c) from a device parameter table; every tensor stays on the device, nothing is read back."""
    f = table.view(torch.float32)
    flags = table[:, ops.STRONG_FLAGS]
    M, o = f[:, ops.STRONG_M:ops.STRONG_M + 9].view(B, 3, 3), f[:, ops.STRONG_O:ops.STRONG_O + 3]
    w = f[:, ops.STRONG_W:ops.STRONG_W + 9]
    mean = torch.tensor(list(cfg.mean), device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(list(cfg.std), device=x.device).view(1, 3, 1, 1)
    v = 255.0 * (x * std + mean)
    v = torch.where((flags & ops.STRONG_COLOUR).bool()[:, None, None, None],
                    (torch.einsum("bij,bjyx->biyx", M, v) + o[:, :, None, None]).clamp_(0.0, 255.0), v)
    R = ops.STRONG_MAX_RADIUS
    k = torch.cat([w[:, 1:].flip(1), w], dim=1)                                  # [B, 17]: w_8 .. w_1 w_0 w_1 .. w_8, zeros past R
    k = k[:, None, :].expand(B, 3, 2 * R + 1).reshape(B * 3, 1, 1, 2 * R + 1)
    t = F.conv2d(F.pad(v.view(1, B * 3, S, S), (R, R, 0, 0), mode="reflect"), k, groups=B * 3)
    t = F.conv2d(F.pad(t, (0, 0, R, R), mode="reflect"), k.transpose(2, 3), groups=B * 3).view(B, 3, S, S)
    v = torch.where((flags & ops.STRONG_BLUR).bool()[:, None, None, None], t, v)
    return (v * (1.0 / 255.0) - mean) / std


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("strong_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip()
    lines = [f"device: {torch.cuda.get_device_name(dev)}" + (f"; commit: {commit}" if commit else ""),
             f"command: python tools/strong_cost.py --rounds {a.rounds} --reps {a.reps}",
             f"B = {B}, S = {S}; device events around trains of back-to-back calls on warm buffers (launch gaps included), medians of "
             f"{a.rounds} rounds after one warm-up round, the arms alternating inside every round"]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    out = torch.empty_like(x)
    keys = torch.arange(B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    cases = (("blur off", StrongAugment(blur_prob=0.0, seed=1)),
             ("blur on, sigma 2.0", StrongAugment(blur_prob=1.0, sigma_range=(2.0, 2.0), seed=1)),
             ("default mix", StrongAugment(seed=1)))
    tables = {n: ops.strong_params(keys, epoch, s.config) for n, s in cases}
    params = torch.empty(B, ops.STRONG_PARAM_WORDS, dtype=torch.int32, device=dev)
    # (b): mix_apply on the same pixel buffers, classmix plan of half the cells
    lab = torch.randint(1, 150, (B, 4, 4), device=dev, generator=g).repeat_interleave(L // 4, 1).repeat_interleave(L // 4, 2).contiguous()
    pw = torch.rand(B, L, L, device=dev, generator=g)
    x2 = torch.randn(B, 3, S, S, device=dev, generator=g)
    mix = SampleMix("classmix", n_classes=151, exclude_label=0, seed=1)
    plan, _ = ops.mix_select(lab, keys, epoch, mix.config)
    mix_out = (out, torch.empty_like(lab), torch.empty_like(pw))

    arms = [(f"params + apply, {n}", (lambda s=s: s(x, keys, epoch, out=out))) for n, s in cases]
    arms += [(f"strong_apply alone, {n}", (lambda n=n, s=s: ops.strong_apply(x, tables[n], s.config, out=out))) for n, s in cases]
    arms += [("strong_params alone", lambda: ops.strong_params(keys, epoch, cases[2][1].config, out=params)),
             ("(a) copy_ of [32,3,512,512] fp32", lambda: out.copy_(x)),
             ("(b) mix_apply on the same buffers", lambda: ops.mix_apply((x, lab, pw), (x2, lab, pw), plan, out=mix_out))]
    arms += [(f"(c) torch composition, {n}", (lambda n=n, s=s: torch_strong(x, tables[n], s.config))) for n, s in cases]
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = event_time(fn, a.reps if "(c)" not in n else max(a.reps // 5, 2))
            if r:
                ts[n].append(dt)
    t = {n: median(v) for n, v in ts.items()}
    for n, _ in cases:
        tab = tables[n].cpu()
        fl = tab[:, ops.STRONG_FLAGS]
        lines.append(f"{n}: colour on {int((fl & 1).bool().sum())}, grey {int((fl & 2).bool().sum())}, blur {int((fl & 4).bool().sum())} of {B} "
                     f"samples; radius of the blurred {sorted(tab[(fl & 4).bool(), ops.STRONG_R].tolist())}")
    for n, s in cases:
        diff = (s(x, keys, epoch, out=out) - torch_strong(x, tables[n], s.config)).abs().max()
        lines.append(f"{n}: max |launch pair - torch composition| = {float(diff):.2e} (normalised units)")
    ideal = 2 * x.numel() * 4
    for n, _ in arms:
        extra = ""
        if n.startswith("strong_apply alone") or n.startswith("(a)"):
            extra = f"   {ideal / t[n] / 1e12:6.2f} TB/s over {ideal / 1e6:.1f} MB (one read + one write)"
        lines.append(f"  {n:44s} {t[n] * 1e6:9.1f} us{extra}")
    ok = True
    for n, _ in cases:
        pair, comp = t[f"params + apply, {n}"], t[f"(c) torch composition, {n}"]
        ok = ok and pair < comp
        lines.append(f"  {n}: the launch pair takes {pair / comp:.3f}x the time of the torch composition ({comp / pair:.1f}x faster), "
                     f"{pair / t[arms[7][0]]:.2f}x the copy, {pair / t[arms[8][0]]:.2f}x mix_apply")
    lines.append("claim (the launch pair takes less time than the torch composition of the same result, in all three cases): " +
                 ("MET" if ok else "NOT MET"))
    if t["params + apply, blur on, sigma 2.0"] >= t["(c) torch composition, blur on, sigma 2.0"]:
        lines.append("  the all-blur case does NOT beat the torch composition")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
