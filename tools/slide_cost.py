"""Cost of sliding-window evaluation at one 683 x 512 ADE20K image, K = 151, 128 x 128 score grids (512 x 512 windows, cells of 4
pixels, canvas 128 x 171 cells, windows at columns 0 and 43):
  * the fused launch (ops.resize_argmax_windows) with 2 views (no flip) and 4 views (flip),
  * ops.resize_argmax of ONE score grid to the same output size, in the same process, as the yardstick: the same arithmetic, the
    windowed kernel adds one staged read per covering view and a division,
  * the whole SlidingWindowInference.predict per image (resize, window cuts, model forwards of a randomly initialised
    BaseModelWithText(16, 512, 128), fused launch), flip off and on.
The arms alternate in one process after a warm-up; each sample is one call ended by a device synchronise; times are medians.
The ops calls include their channels-last copy of the scores and their descriptor uploads; the "launch alone" arms call the C entry
points on prepared buffers (pred only), 20 launches between two device events.  Numbers are recorded, not gated.
  python tools/slide_cost.py [--rounds 7] [--commit ID] [--out profiles/slide_cost.txt]"""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lc2is_amd import ops, slide  # noqa: E402

K, h = 151, 128
H, W = 512, 683


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launch_alone(views, windows, canvas, size, dev):
    """A closure timing 20 back-to-back launches of the C entry point on prepared buffers (device events): seconds per launch.
    windows None: lc2is_resize_argmax of views[0]."""
    V, k, hh, ww = views.shape
    ld = (k + 3) // 4 * 4
    lo = torch.zeros(V, hh, ww, ld, dtype=torch.float32, device=dev)
    lo[..., :k] = views.permute(0, 2, 3, 1)
    Hh, Ww = size
    tiles = -(-Hh // 16) * -(-Ww // 16)
    pred = torch.empty(Hh * Ww, dtype=torch.uint8, device=dev)
    if windows is None:
        desc = torch.tensor([[Hh, Ww, 0, 0]], dtype=torch.int64).to(dev)
        call = lambda: ops._fn("lc2is_resize_argmax")(lo.data_ptr(), ld, 1, hh, ww, k, desc.data_ptr(), tiles, Hh * Ww, None, 0,
                                                      pred.data_ptr(), None, None, 0, torch.cuda.current_stream().cuda_stream)
    else:
        desc = torch.tensor([[Hh, Ww, 0, 0, canvas[0], canvas[1], 0, len(windows)]], dtype=torch.int64).to(dev)
        win = torch.tensor([[v, oy, ox, int(m)] for v, oy, ox, m in windows], dtype=torch.int32).to(dev)
        call = lambda: ops._fn("lc2is_resize_argmax_windows")(lo.data_ptr(), ld, V, hh, ww, k, desc.data_ptr(), 1, win.data_ptr(),
                                                              len(windows), tiles, Hh * Ww, None, 0, -1, pred.data_ptr(), None, None,
                                                              0, torch.cuda.current_stream().cuda_stream)

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            if call() != 0:
                raise RuntimeError("launch refused")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / 20
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slide_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() or "unknown"
    g = torch.Generator().manual_seed(1)
    views = torch.randn(4, K, h, h, generator=g).to(dev)
    Hc, Wc = (n // 4 for n in slide.eval_size(H, W, 512, 4))
    xs = slide.plan_windows(Wc, h, 340 // 4)
    w2 = [(i, 0, ox, False) for i, ox in enumerate(xs)]
    w4 = w2 + [(2 + i, 0, ox, True) for i, ox in enumerate(xs)]
    arms = [("ops.resize_argmax, one grid (yardstick)", lambda: ops.resize_argmax(views[:1], [(H, W)])),
            ("ops.resize_argmax_windows, 2 views", lambda: ops.resize_argmax_windows(views[:2], [w2], [(Hc, Wc)], [(H, W)])),
            ("ops.resize_argmax_windows, 4 views (flip)", lambda: ops.resize_argmax_windows(views, [w4], [(Hc, Wc)], [(H, W)]))]

    import lc2is_amd.nn as N
    from bench import synth_batch
    model = N.BaseModelWithText(16, 512, 128).to(dev).eval()
    image = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for flip in (False, True):
        B = 4 if flip else 2
        inputs, _ = synth_batch(B, 512, 128, 16, 3, dev)
        text = {k: inputs[k] for k in ("input_ids", "attention_mask")}
        inf = slide.SlidingWindowInference(model, text, flip=flip, window_batch=B, device=dev)
        arms.append((f"SlidingWindowInference.predict, flip={flip} ({B} forwards in one batch)", lambda inf=inf: inf.predict([image])))

    alone = {"launch alone: ra_kernel, one grid (yardstick)": launch_alone(views[:1], None, None, (H, W), dev),
             "launch alone: ra_win_kernel, 2 views": launch_alone(views[:2], w2, (Hc, Wc), (H, W), dev),
             "launch alone: ra_win_kernel, 4 views (flip)": launch_alone(views, w4, (Hc, Wc), (H, W), dev)}
    arms += [(n, f) for n, f in alone.items()]
    ts = {n: [] for n, _ in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms:
            dt = fn() if n in alone else timed(fn)
            if r:
                ts[n].append(dt)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; commit: {commit}",
             f"command: python tools/slide_cost.py --rounds {a.rounds}" + (f" --out {a.out}" if a.out else ""),
             f"one {W} x {H} image, K = {K}, score grids {h} x {h}, canvas {Hc} x {Wc} cells, windows at columns {xs}; "
             f"{a.rounds} alternating rounds after 1 warm-up; medians (min - max)"]
    for n, _ in arms:
        t = sorted(ts[n])
        lines.append(f"  {n:72s} {t[len(t) // 2] * 1e6:10.1f} us  ({t[0] * 1e6:.1f} - {t[-1] * 1e6:.1f})")
    med = lambda n: sorted(ts[n])[len(ts[n]) // 2]
    lines.append(f"  whole ops call: windows (2 views) / yardstick: {med(arms[1][0]) / med(arms[0][0]):.2f}x; "
                 f"windows (4 views) / yardstick: {med(arms[2][0]) / med(arms[0][0]):.2f}x")
    a0, a2, a4 = (med(n) for n in alone)
    lines.append("  launch alone = 20 back-to-back launches on the same prepared buffers between two device events: the views are warm "
                 "in cache, pred only, no counts")
    lines.append(f"  launch alone: windows (2 views) / yardstick: {a2 / a0:.2f}x; windows (4 views) / yardstick: {a4 / a0:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
