"""Cost of the device augmentation (lc2is_amd/data/augment.py) at the headline shapes: B = 32, S = 512, L = 128 on ADE20K-like
images (683 x 512 and 512 x 683 mixed, uniform noise).
  1. aug_params_kernel and aug_apply_kernel: device-event time of a train of launches, and GB/s against the bytes the launch must
     move (written: B * (3 * S * S * 4 + L * L * 8); read: at most the source pixels and labels of the B images).
  2. The same 32 resident images through the deterministic evaluation transform, ClipImagePreprocessor + ClipLabelPreprocessor
     (the only input path there was before), alternating with the augmentation in one process.
  3. Images/s of the headline train step (BaseModelWithText(16, 512, 128), B = 32, text length 16, SGD, eager) on one resident
     batch against the same step fed by AugmentedBatches, alternating blocks of steps.
  python tools/augment_cost.py [--rounds 5] [--steps 20] [--out profiles/augment_cost.txt]"""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from lc2is_amd import ops  # noqa: E402
from lc2is_amd.data import (AugmentedBatches, ClipImagePreprocessor, ClipLabelPreprocessor, DeviceImagePool,  # noqa: E402
                            TrainAugment)

B, S, L, TEXT = 32, 512, 128, 16


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


def host_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pool", type=int, default=256, help="images in the pool")
    ap.add_argument("--skip-step", action="store_true", help="kernels and preprocessors only")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() or "unknown"
    lines = [f"device: {torch.cuda.get_device_name(dev)}; commit: {commit}",
             f"command: python tools/augment_cost.py --rounds {a.rounds} --steps {a.steps} --pool {a.pool}",
             f"B = {B}, S = {S}, L = {L}; pool of {a.pool} uniform-noise images, 683 x 512 and 512 x 683 alternating"]
    g = torch.Generator(device=dev).manual_seed(1)
    shapes = [(683, 512) if k % 2 == 0 else (512, 683) for k in range(a.pool)]
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g) for h, w in shapes]
    labs = [torch.randint(0, 151, (h, w), dtype=torch.uint8, device=dev, generator=g) for h, w in shapes]
    pool = DeviceImagePool.from_arrays(imgs, labs, device=dev)
    aug = TrainAugment(crop_size=S, label_size=L, seed=1)
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {"pixel_values": torch.empty(B, 3, S, S, device=dev), "label": torch.empty(B, L, L, dtype=torch.int64, device=dev)}
    params = aug.params(pool, idx, epoch)

    # ---- 1. the two kernels
    written = B * (3 * S * S * 4 + L * L * 8)
    source = sum(4 * h * w for h, w in shapes[:B])
    t_par, t_app = [], []
    for r in range(a.rounds + 1):
        tp = event_time(lambda: ops.aug_params(idx, epoch, pool.desc, aug.config, out=params), 200)
        ta = event_time(lambda: aug.apply(pool, idx, params, out), 200)
        if r:
            t_par.append(tp); t_app.append(ta)
    tp, ta = median(t_par), median(t_app)
    lines += ["1. kernels (device events around 200 back-to-back launches, launch gaps included; medians of "
              f"{a.rounds} rounds after one warm-up round):",
              f"  aug_params_kernel  {tp * 1e6:8.1f} us per launch ({B} samples; launch-bound)",
              f"  aug_apply_kernel   {ta * 1e6:8.1f} us per launch; writes {written / 1e6:.1f} MB, reads at most {source / 1e6:.1f} MB "
              f"(the {B} source images and label maps): {written / ta / 1e9:.0f} GB/s of stores, "
              f"at most {(written + source) / ta / 1e9:.0f} GB/s in all",
              f"  byte floor at 5 TB/s: {(written + source) / 5e12 * 1e6:.1f} us; the launch takes {ta / ((written + source) / 5e12):.2f}x that"]

    # ---- 2. against the evaluation transform on the same resident images
    pre_i, pre_l = ClipImagePreprocessor(size=S, crop_size=S, device=dev), ClipLabelPreprocessor(size=L, crop_size=L, device=dev)
    arms = (("TrainAugment (params + apply, 2 launches)", lambda: aug(pool, idx, epoch)),
            ("ClipImagePreprocessor + ClipLabelPreprocessor", lambda: (pre_i(imgs[:B]), pre_l(labs[:B]))))
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = host_time(fn)
            if r:
                ts[n].append(dt)
    lines.append(f"2. one batch of {B} resident images, host clock around the call + synchronise, alternating, medians of {a.rounds}:")
    for n, _ in arms:
        lines.append(f"  {n:48s} {median(ts[n]) * 1e6:10.1f} us per batch = {B / median(ts[n]):10.0f} images/s")
    lines.append(f"  evaluation transform / augmentation: {median(ts[arms[1][0]]) / median(ts[arms[0][0]]):.1f}x time")

    # ---- 3. the headline step, resident batch against AugmentedBatches
    if not a.skip_step:
        import lc2is_amd.nn as N
        from bench import synth_batch
        from lc2is_amd.step import TrainStep
        torch.manual_seed(1024)
        model = N.BaseModelWithText(16, S, L).to(dev).train()
        step = TrainStep(model, optimizer="sgd", lr=1e-5)
        inputs, labels = synth_batch(B, S, L, TEXT, 2, dev)
        extra = {k: v for k, v in inputs.items() if k != "pixel_values"}
        loader = AugmentedBatches(pool, aug, B, shuffle_seed=0, extra_inputs=extra)
        state = {"epoch": 0, "it": None}

        def resident():
            for _ in range(a.steps):
                step.step(inputs, labels)

        def fed():
            done = 0
            while done < a.steps:
                if state["it"] is None:
                    loader.set_epoch(state["epoch"])
                    state["it"] = iter(loader)
                    state["epoch"] += 1
                batch = next(state["it"], None)
                if batch is None:
                    state["it"] = None
                    continue
                x = batch[0]
                step.step(x, x.pop("label"))
                done += 1

        arms = (("resident batch", resident), ("fed by AugmentedBatches", fed))
        ts = {n: [] for n, _ in arms}
        for r in range(a.rounds + 1):
            for n, fn in arms:
                dt = host_time(fn)
                if r:
                    ts[n].append(dt)
        lines.append(f"3. headline step (BaseModelWithText(16, {S}, {L}), B = {B}, SGD, eager), blocks of {a.steps} steps, alternating, "
                     f"medians of {a.rounds} after one warm-up block each:")
        for n, _ in arms:
            t = median(ts[n])
            lines.append(f"  {n:28s} {t / a.steps * 1e3:8.2f} ms per step = {B * a.steps / t:8.1f} images/s "
                         f"(blocks: {', '.join(f'{B * a.steps / v:.0f}' for v in ts[n])})")
        lines.append(f"  fed / resident: {median(ts[arms[1][0]]) / median(ts[arms[0][0]]):.4f}x time")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
