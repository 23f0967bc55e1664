"""Torch restatements for the sliding-window resize + argmax (lc2is_resize_argmax_windows): the canvas mean with the kernel's
summation order, torch's own bicubic + argmax in fp64 with the top-2 margin, and the synthetic cases both test files use."""
import functools

import torch
import torch.nn.functional as F

from lc2is_amd.slide import plan_windows

MARGIN = 5e-5        # near-tie margin relative to max|views|, and the cap on the share of pixels inside it: the figures of
UNSURE_CAP = 5e-3    # tests/test_gpu_resize_argmax.py

# (make_case arguments, output sizes) of the fp64 comparison; the last one is the real grid (683 x 512 image, 128-cell windows)
FP64_CASES = [
    ((37, 8, 8, 14, 4, True), [(50, 90), (5, 9), (33, 17), (1, 1)]),
    ((37, 8, 12, 14, 4, False), [(50, 90), (7, 9), (100, 131)]),
    ((151, 32, 32, 44, 20, True), [(512, 683), (97, 131)]),
    ((151, 128, 128, 172, 85, True), [(512, 683)]),
]


def canvas_mean(views, windows, Hc, Wc, dtype=torch.float32):
    """[K, Hc, Wc]: per cell the sum of the covering views in list order, starting from the first one, divided by their number
    (0 where nothing covers).  views [V, K, h, w]; windows: (view, oy, ox, mirrored), a mirrored view is stored flipped along x."""
    _, K, h, w = views.shape
    acc = torch.zeros(K, Hc, Wc, dtype=dtype)
    cnt = torch.zeros(Hc, Wc, dtype=torch.int64)
    for view, oy, ox, mirrored in windows:
        x = views[view].to(dtype)
        if mirrored:
            x = x.flip(-1)
        a, c = acc[:, oy:oy + h, ox:ox + w], cnt[oy:oy + h, ox:ox + w]
        a.copy_(torch.where(c == 0, x, a + x))
        c += 1
    return acc / cnt.clamp_min(1).to(dtype)


def cover_counts(windows, h, w, Hc, Wc):
    cnt = torch.zeros(Hc, Wc, dtype=torch.int64)
    for _, oy, ox, _ in windows:
        cnt[oy:oy + h, ox:ox + w] += 1
    return cnt


def ref_argmax(canvas, size, chunk=16):
    """fp64 CPU F.interpolate(canvas [K,Hc,Wc], size, bicubic, align_corners=False): (argmax [H,W] (first maximum), top-1 minus
    top-2 margin [H,W]), over channel chunks with a running top-2."""
    x = canvas[None]
    v1 = v2 = i1 = None
    for c0 in range(0, x.shape[1], chunk):
        y = F.interpolate(x[:, c0:c0 + chunk].double(), size=size, mode="bicubic", align_corners=False)[0]
        if y.shape[0] == 1:
            top = torch.stack([y[0], torch.full_like(y[0], -float("inf"))])
        else:
            top = y.topk(2, dim=0).values
        m, s, a = top[0], top[1], y.argmax(0) + c0
        if v1 is None:
            v1, v2, i1 = m, s, a
        else:
            up = m > v1
            v2 = torch.where(up, torch.maximum(v1, s), torch.maximum(v2, m))
            i1 = torch.where(up, a, i1)
            v1 = torch.where(up, m, v1)
    return i1, v1 - v2


def fp32_argmax(canvas32, size, chunk=16):
    """argmax of torch's fp32 bicubic resize of an fp32 canvas (first maximum), chunked over channels."""
    best = arg = None
    for c0 in range(0, canvas32.shape[0], chunk):
        y = F.interpolate(canvas32[None, c0:c0 + chunk], size=size, mode="bicubic", align_corners=False)[0]
        m, a = y.max(0).values, y.argmax(0) + c0
        if best is None:
            best, arg = m, a
        else:
            up = m > best
            arg = torch.where(up, a, arg)
            best = torch.where(up, m, best)
    return arg


@functools.lru_cache(maxsize=None)
def make_case(K, h, Hc, Wc, stride, flip, noise=0.3, seed=0):
    """(views [V, K, h, h], windows): a base canvas randn[K, Hc, Wc]; every view is its window's crop plus noise * randn, stored
    mirrored when flagged; windows from plan_windows on both axes, rows first, with ``flip`` a mirrored copy after each window."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(K, Hc, Wc, generator=g)
    views, windows = [], []
    for oy in plan_windows(Hc, h, stride):
        for ox in plan_windows(Wc, h, stride):
            for mirrored in ((False, True) if flip else (False,)):
                v = base[:, oy:oy + h, ox:ox + h] + noise * torch.randn(K, h, h, generator=g)
                windows.append((len(views), oy, ox, mirrored))
                views.append(v.flip(-1) if mirrored else v)
    return torch.stack(views).contiguous(), tuple(windows)


@functools.lru_cache(maxsize=None)
def fp64_reference(args, size):
    """(argmax, sure mask, unsure share) of one make_case at one output size: computed once, shared, never modified."""
    views, windows = make_case(*args)
    _, _, Hc, Wc = args[:4]
    ref, margin = ref_argmax(canvas_mean(views, windows, Hc, Wc, torch.float64), size)
    sure = margin > MARGIN * views.abs().max().item()
    return ref, sure, (~sure).float().mean().item()
