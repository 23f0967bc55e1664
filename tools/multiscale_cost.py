"""Cost of multi-scale + flip evaluation at one 683 x 512 ADE20K image, K = 151, 128 x 128 score grids (512 x 512 windows, cells of 4
pixels), the six standard scales 0.5 .. 1.75 with a mirrored copy of every window:
  * the fused launch alone (lc2is_resize_argmax_multiscale on prepared buffers, pred only) in both modes, with 6 canvases (one per
    scale, plain and mirrored windows together) and 12 (one per scale and flip), random views,
  * lc2is_resize_argmax_windows at scale 1.0 (2 views, no flip) in the same process as the yardstick: one canvas, the same
    arithmetic per canvas and chunk.  The logit mode walks every canvas once and the prob mode twice; the staging loop of a walk
    tests every window of its canvas, so the cost grows with the windows per canvas (2 to 24 here) as well as with the canvases,
  * the whole MultiScaleInference.predict per image (resizes, window cuts, 52 model forwards of a randomly initialised
    BaseModelWithText(16, 512, 128), fused launch), both averages.
The launch arms alternate in one process after a warm-up, 20 back-to-back launches on the same warm buffers between two device
events; predict is one call ended by a device synchronise; times are medians.  Numbers are recorded, not gated.
  python tools/multiscale_cost.py [--rounds 7] [--predict-rounds 3] [--commit ID] [--out profiles/multiscale_cost.txt]"""
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
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def prepared(V, dev):
    lo = torch.zeros(V, h, h, (K + 3) // 4 * 4, dtype=torch.float32, device=dev)
    lo[..., :K] = torch.randn(V, h, h, K, generator=torch.Generator().manual_seed(1)).to(dev)
    return lo


def events(call):
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


def launch_multiscale(lo, canvases, mode, dev):
    """Seconds per launch of the C entry point for one H x W image over ``canvases`` (as ops.resize_argmax_multiscale takes them)."""
    V = lo.shape[0]
    tiles = -(-H // 16) * -(-W // 16)
    pred = torch.empty(H * W, dtype=torch.uint8, device=dev)
    win, canv = [], []
    for (Hc, Wc), wl in canvases:
        canv.append([Hc, Wc, len(win), len(wl)])
        win += [[v, oy, ox, int(m)] for v, oy, ox, m in wl]
    desc = torch.tensor([[H, W, 0, 0, 0, len(canv)]], dtype=torch.int64).to(dev)
    canv_t, win_t = torch.tensor(canv, dtype=torch.int64).to(dev), torch.tensor(win, dtype=torch.int32).to(dev)
    fn = ops._fn("lc2is_resize_argmax_multiscale")
    return events(lambda: fn(lo.data_ptr(), lo.shape[-1], V, h, h, K, desc.data_ptr(), 1, canv_t.data_ptr(), len(canv), win_t.data_ptr(),
                             len(win), tiles, H * W, None, 0, -1, ops._MS_MODES[mode], pred.data_ptr(), None, None, 0,
                             torch.cuda.current_stream().cuda_stream))


def launch_windows(lo, canvas, wl, dev):
    V = lo.shape[0]
    tiles = -(-H // 16) * -(-W // 16)
    pred = torch.empty(H * W, dtype=torch.uint8, device=dev)
    desc = torch.tensor([[H, W, 0, 0, canvas[0], canvas[1], 0, len(wl)]], dtype=torch.int64).to(dev)
    win = torch.tensor([[v, oy, ox, int(m)] for v, oy, ox, m in wl], dtype=torch.int32).to(dev)
    fn = ops._fn("lc2is_resize_argmax_windows")
    return events(lambda: fn(lo.data_ptr(), lo.shape[-1], V, h, h, K, desc.data_ptr(), 1, win.data_ptr(), len(wl), tiles, H * W, None, 0,
                             -1, pred.data_ptr(), None, None, 0, torch.cuda.current_stream().cuda_stream))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--predict-rounds", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiscale_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() or "unknown"
    plan = slide.plan_multiscale(H, W, SCALES, 512, 512, 340, 4)
    c6, V = slide.multiscale_canvases(plan, 0, True, "logit")
    c12, V12 = slide.multiscale_canvases(plan, 0, True, "prob")
    assert V == V12 and (len(c6), len(c12)) == (6, 12)
    one = slide.multiscale_canvases(slide.plan_multiscale(H, W, (1.0,), 512, 512, 340, 4), 0, False, "logit")[0][0]
    yard = "launch alone: ra_win_kernel, scale 1.0, 2 views (yardstick)"
    lo = prepared(V, dev)                                       # one view tensor for every arm; the yardstick reads its first two
    alone = {yard: launch_windows(lo, one[0], one[1], dev)}
    for mode in ("logit", "prob"):
        for cl in (c6, c12):
            alone[f"launch alone: ra_ms_kernel, {mode}, {len(cl)} canvases, {V} views"] = launch_multiscale(lo, cl, mode, dev)
    ts = {n: [] for n in alone}
    for r in range(a.rounds + 1):
        for n, fn in alone.items():
            dt = fn()
            if r:
                ts[n].append(dt)

    import lc2is_amd.nn as N
    from bench import synth_batch
    model = N.BaseModelWithText(16, 512, 128).to(dev).eval()
    image = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    inputs, _ = synth_batch(8, 512, 128, 16, 3, dev)
    text = {k: inputs[k] for k in ("input_ids", "attention_mask")}
    for average in ("logit", "prob"):
        inf = slide.MultiScaleInference(model, text, scales=SCALES, flip=True, average=average, window_batch=8, device=dev)
        n = f"MultiScaleInference.predict, average={average} ({V} forwards in batches of 8)"
        ts[n] = [timed(lambda: inf.predict([image])) for _ in range(a.predict_rounds + 1)][1:]

    med = lambda n: sorted(ts[n])[len(ts[n]) // 2]
    lines = [f"device: {torch.cuda.get_device_name(dev)}; commit: {commit}",
             f"command: python tools/multiscale_cost.py --rounds {a.rounds} --predict-rounds {a.predict_rounds}" + (f" --out {a.out}" if a.out else ""),
             f"one {W} x {H} image, K = {K}, score grids {h} x {h}, scales {SCALES} with flip: canvases "
             f"{[c for _, c, _ in plan]} cells, {[len(o) for _, _, o in plan]} windows each (x 2 mirrored), {V} views; "
             f"{a.rounds} alternating rounds after 1 warm-up; medians (min - max)"]
    for n in ts:
        t = sorted(ts[n])
        lines.append(f"  {n:80s} {t[len(t) // 2] * 1e6:12.1f} us  ({t[0] * 1e6:.1f} - {t[-1] * 1e6:.1f})")
    lines.append("  launch alone = 20 back-to-back launches on the same prepared buffers between two device events: the views are warm in "
                 "cache, pred only, no counts")
    lines.append("  launch alone / yardstick: " + "; ".join(f"{n.split('ra_ms_kernel, ')[1].split(' canvases')[0]} canvases: "
                                                            f"{med(n) / med(yard):.1f}x" for n in alone if n != yard))
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
