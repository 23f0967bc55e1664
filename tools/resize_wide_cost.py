"""Cost of the resize + argmax kernels past 192 classes (lc2is_resize_argmax_wide, _windows_wide, _multiscale_wide) at one
683 x 512 image and 128 x 128 score grids:
  * K = 192: the wide launch against the narrow one on the same buffers, for each of the three kernels (multiscale in both modes),
    pred only and with counts: what the int16 store and the one-row-at-a-time count epilogue cost where both forms exist,
  * K = 256 / 512 / 847 / 1024: the wide launches, pred only and with counts, so that the epilogue's share is visible; us per class
    and the bytes of the per-tile count workspace.
The grid kernel reads one score grid; the window kernel the two windows of scale 1.0 (no flip); the multiscale kernel scales
0.75, 1.0 and 1.25 with a mirrored copy of every window: 3 canvases summed as logits, 6 as probabilities, 14 views.  Views are
random; the gt map holds one random class per 32 x 32 block (label maps are piecewise constant), while the predictions of random
views change every few pixels, which is the expensive case for the per-wave histograms.
The arms alternate in one process after a warm-up, 20 back-to-back launches on the same warm buffers between two device events;
times are medians.  Numbers are recorded, not gated.
  python tools/resize_wide_cost.py [--rounds 5] [--commit ID] [--out profiles/resize_wide_cost.txt]"""
import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from lc2is_amd import ops, slide  # noqa: E402

h = 128
H, W = 512, 683
TILES = -(-H // 16) * -(-W // 16)
SCALES = (0.75, 1.0, 1.25)
KERNELS = ("grid", "windows", "multiscale logit", "multiscale prob")


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


class Buffers:
    """Everything the launches of one class count share: views, descriptors, gt, pred in both widths, counts, workspace."""

    def __init__(self, K, dev):
        self.K, self.dev = K, dev
        plan = slide.plan_multiscale(H, W, SCALES, 512, 512, 340, 4)
        self.canvases = {"logit": slide.multiscale_canvases(plan, 0, True, "logit")[0],
                         "prob": slide.multiscale_canvases(plan, 0, True, "prob")[0]}
        self.V = slide.multiscale_canvases(plan, 0, True, "logit")[1]
        one = slide.multiscale_canvases(slide.plan_multiscale(H, W, (1.0,), 512, 512, 340, 4), 0, False, "logit")[0][0]
        self.one_canvas, self.one_windows = one
        ld = (K + 3) // 4 * 4
        torch.manual_seed(1)
        self.lo = torch.zeros(self.V, h, h, ld, dtype=torch.float32, device=dev)
        self.lo[..., :K] = torch.randn(self.V, h, h, K, device=dev)
        blocks = torch.randint(0, K, (H // 32 + 1, W // 32 + 1), device=dev, dtype=torch.int32)
        self.gt = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].contiguous().reshape(-1)
        self.pred8 = torch.empty(H * W, dtype=torch.uint8, device=dev)
        self.pred16 = torch.empty(H * W, dtype=torch.int16, device=dev)
        self.counts = torch.empty(1, 3, K, dtype=torch.int32, device=dev)
        self.ws_bytes = ops._fn("lc2is_resize_argmax_wide_workspace_bytes")(TILES, K)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.keep = []

    def _t(self, rows, dtype):
        t = torch.tensor(rows, dtype=dtype).to(self.dev)
        self.keep.append(t)
        return t

    def arm(self, kernel, wide, with_counts):
        """Seconds per launch of one C entry point on these buffers."""
        K, lo, s = self.K, self.lo, torch.cuda.current_stream().cuda_stream
        suffix = "_wide" if wide else ""
        pred = (self.pred16 if wide else self.pred8).data_ptr()
        tail = (self.gt.data_ptr(), 4) if with_counts else (None, 0)
        out = (pred, self.counts.data_ptr(), self.ws.data_ptr(), self.ws_bytes) if with_counts else (pred, None, None, 0)
        if kernel == "grid":
            desc = self._t([[H, W, 0, 0]], torch.int64)
            fn = ops._fn("lc2is_resize_argmax" + suffix)
            return events(lambda: fn(lo.data_ptr(), lo.shape[-1], 1, h, h, K, desc.data_ptr(), TILES, H * W, *tail, *out, s))
        if kernel == "windows":
            (Hc, Wc), wl = self.one_canvas, self.one_windows
            desc = self._t([[H, W, 0, 0, Hc, Wc, 0, len(wl)]], torch.int64)
            win = self._t([[v, oy, ox, int(m)] for v, oy, ox, m in wl], torch.int32)
            fn = ops._fn("lc2is_resize_argmax_windows" + suffix)
            return events(lambda: fn(lo.data_ptr(), lo.shape[-1], self.V, h, h, K, desc.data_ptr(), 1, win.data_ptr(), len(wl), TILES,
                                     H * W, *tail, -1, *out, s))
        mode = kernel.split()[1]
        win, canv = [], []
        for (Hc, Wc), wl in self.canvases[mode]:
            canv.append([Hc, Wc, len(win), len(wl)])
            win += [[v, oy, ox, int(m)] for v, oy, ox, m in wl]
        desc = self._t([[H, W, 0, 0, 0, len(canv)]], torch.int64)
        canv_t, win_t = self._t(canv, torch.int64), self._t(win, torch.int32)
        fn = ops._fn("lc2is_resize_argmax_multiscale" + suffix)
        return events(lambda: fn(lo.data_ptr(), lo.shape[-1], self.V, h, h, K, desc.data_ptr(), 1, canv_t.data_ptr(), len(canv),
                                 win_t.data_ptr(), len(win), TILES, H * W, *tail, -1, ops._MS_MODES[mode], *out, s))


def measure(arms, rounds):
    ts = {n: [] for n in arms}
    for r in range(rounds + 1):
        for n, fn in arms.items():
            dt = fn()
            if r:
                ts[n].append(dt)
    return {n: sorted(t) for n, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_wide_cost.py: needs a GPU")
    dev = torch.device("cuda:0")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() or "unknown"
    med = lambda t: t[len(t) // 2]
    lines = [f"device: {torch.cuda.get_device_name(dev)}; commit: {commit}",
             f"command: python tools/resize_wide_cost.py --rounds {a.rounds}" + (f" --out {a.out}" if a.out else ""),
             f"one {W} x {H} image ({TILES} tiles), score grids {h} x {h}; windows: scale 1.0, 2 views; multiscale: scales {SCALES} "
             f"with flip, 3 canvases (logit) / 6 (prob), 14 views; {a.rounds} alternating rounds after 1 warm-up, 20 back-to-back "
             f"launches per timing on warm buffers; medians (min - max); counts = main launch + the per-image sum of the slabs"]

    b = Buffers(192, dev)
    arms = {(k, w, c): b.arm(k, w, c) for k in KERNELS for c in (False, True) for w in (False, True)}
    ts = measure(arms, a.rounds)
    lines.append(f"K = 192, narrow against wide on the same buffers (workspace {b.ws_bytes} bytes either way):")
    for k in KERNELS:
        for c in (False, True):
            n, w = ts[(k, False, c)], ts[(k, True, c)]
            lines.append(f"  {k:17s} {'with counts' if c else 'pred only':11s}  narrow {med(n) * 1e6:9.1f} us ({n[0] * 1e6:.1f} - {n[-1] * 1e6:.1f})"
                         f"   wide {med(w) * 1e6:9.1f} us ({w[0] * 1e6:.1f} - {w[-1] * 1e6:.1f})   wide / narrow {med(w) / med(n):.3f}")
    del b, arms
    torch.cuda.empty_cache()

    for K in (256, 512, 847, 1024):
        b = Buffers(K, dev)
        arms = {(k, c): b.arm(k, True, c) for k in KERNELS for c in (False, True)}
        ts = measure(arms, a.rounds)
        lines.append(f"K = {K}, wide (workspace {b.ws_bytes} bytes = {b.ws_bytes / 1e6:.1f} MB):")
        for k in KERNELS:
            p, c = ts[(k, False)], ts[(k, True)]
            lines.append(f"  {k:17s} pred only {med(p) * 1e6:9.1f} us ({p[0] * 1e6:.1f} - {p[-1] * 1e6:.1f}) = {med(p) * 1e6 / K:6.3f} us/class"
                         f"   with counts {med(c) * 1e6:9.1f} us ({c[0] * 1e6:.1f} - {c[-1] * 1e6:.1f}) = {med(c) * 1e6 / K:6.3f} us/class"
                         f"   counts' share {(med(c) - med(p)) / med(c) * 100:5.1f} %")
        del b, arms
        torch.cuda.empty_cache()

    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
