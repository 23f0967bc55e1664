"""Torch restatements for the multi-scale resize + argmax (lc2is_resize_argmax_multiscale): the canvas mean of slide_ref with
windows that overhang the canvas, torch's own fp64 bicubic per canvas followed by an fp64 softmax-sum or a plain sum, the argmax
with the top-2 of the sum, the near-tie rule derived from slide_ref.MARGIN, and the synthetic cases both test files use."""
import functools

import torch
import torch.nn.functional as F

import slide_ref as R
from lc2is_amd.slide import plan_windows

POISON = 99.0        # what a view holds outside its on-canvas part: a kernel that reads the overhang cannot agree with the reference

# K, view edge h, canvases as (Hc, Wc, stride, mirrored copy of every window inside the canvas), output sizes.  "small": canvas 2
# is smaller than a view in both axes, canvas 3 overhangs along x only and holds mirrored views, (5, 9) takes the downscale band
# path.  "real_k": K = 151 is five channel chunks, the last one partial; canvas 3 is smaller than a view.
CASES = {
    "small": (37, 8, ((8, 12, 4, False), (12, 18, 4, True), (5, 7, 4, False), (14, 6, 4, True)), ((50, 90), (5, 9), (33, 17), (1, 1))),
    "real_k": (151, 32, ((32, 44, 20, False), (32, 44, 20, True), (48, 64, 20, False), (20, 28, 20, False)), ((97, 131), (256, 341))),
}


def canvas_mean(views, windows, Hc, Wc, dtype=torch.float32):
    """slide_ref.canvas_mean with windows that may overhang the canvas at the bottom / right: only the view's top-left
    min(h, Hc - oy) x min(w, Wc - ox) part is used, and a mirrored view is mirrored over that part."""
    _, K, h, w = views.shape
    acc = torch.zeros(K, Hc, Wc, dtype=dtype)
    cnt = torch.zeros(Hc, Wc, dtype=torch.int64)
    for view, oy, ox, mirrored in windows:
        vh, vw = min(h, Hc - oy), min(w, Wc - ox)
        x = views[view][:, :vh, :vw].to(dtype)
        if mirrored:
            x = x.flip(-1)
        a, c = acc[:, oy:oy + vh, ox:ox + vw], cnt[oy:oy + vh, ox:ox + vw]
        a.copy_(torch.where(c == 0, x, a + x))
        c += 1
    return acc / cnt.clamp_min(1).to(dtype)


def make_canvas(K, h, Hc, Wc, stride, flip, gen, first_view=0, noise=0.3):
    """(views [n, K, h, h], windows, max |value| on the canvas parts) of one canvas: a base randn[K, Hc, Wc]; every view holds its
    window's on-canvas crop plus noise * randn in its top-left corner, stored mirrored over that part when flagged, and POISON
    elsewhere; windows from plan_windows on both axes, rows first, with ``flip`` a mirrored copy after each window."""
    base = torch.randn(K, Hc, Wc, generator=gen)
    views, windows, amax = [], [], 0.0
    for oy in plan_windows(Hc, h, stride):
        for ox in plan_windows(Wc, h, stride):
            vh, vw = min(h, Hc - oy), min(h, Wc - ox)
            for mirrored in ((False, True) if flip else (False,)):
                part = base[:, oy:oy + vh, ox:ox + vw] + noise * torch.randn(K, vh, vw, generator=gen)
                amax = max(amax, part.abs().max().item())
                v = torch.full((K, h, h), POISON)
                v[:, :vh, :vw] = part.flip(-1) if mirrored else part
                windows.append((first_view + len(views), oy, ox, mirrored))
                views.append(v)
    return torch.stack(views), windows, amax


@functools.lru_cache(maxsize=None)
def make_case(name, seed=0):
    """(views [V, K, h, h], canvases as ops.resize_argmax_multiscale takes them for one image, max |value| the canvases hold)."""
    K, h, specs, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    views, canvases, amax, v0 = [], [], 0.0, 0
    for Hc, Wc, stride, flip in specs:
        v, wl, m = make_canvas(K, h, Hc, Wc, stride, flip, g, v0)
        views.append(v); canvases.append(((Hc, Wc), tuple(wl))); amax = max(amax, m); v0 += len(v)
    return torch.cat(views).contiguous(), tuple(canvases), amax


def ref_sum(views, canvases, size, mode):
    """fp64 [K, H, W]: per canvas the fp64 canvas mean resized by F.interpolate(bicubic, align_corners=False), then the sum over
    the canvases of the softmax over the classes (mode "prob") or of the resized logits ("logit")."""
    s = None
    for (Hc, Wc), windows in canvases:
        y = F.interpolate(canvas_mean(views, windows, Hc, Wc, torch.float64)[None], size=size, mode="bicubic", align_corners=False)[0]
        if mode == "prob":
            y = torch.softmax(y, dim=0)
        s = y if s is None else s + y
    return s


def ref_argmax(views, canvases, size, mode, amax):
    """(argmax [H, W] (first maximum), sure mask, unsure share).  A resized logit is within MARGIN * amax / 2 of fp64 (the margin
    tests/test_gpu_slide.py establishes), so a softmax term has relative error up to about MARGIN * amax: a "prob" pixel is sure
    when P1 - P2 > MARGIN * amax * (P1 + P2), and a "logit" pixel with A canvases when s1 - s2 > A * MARGIN * amax."""
    s = ref_sum(views, canvases, size, mode)
    if s.shape[0] == 1:
        top = torch.stack([s[0], torch.full_like(s[0], -float("inf"))])
    else:
        top = s.topk(2, dim=0).values
    if mode == "prob":
        sure = top[0] - top[1] > R.MARGIN * amax * (top[0] + top[1])
    else:
        sure = top[0] - top[1] > len(canvases) * R.MARGIN * amax
    return s.argmax(0), sure, (~sure).float().mean().item()


def fp32_argmax(views, canvases, size, mode):
    """The same computation in torch's fp32: fp32 canvas means, fp32 bicubic, fp32 softmax, summed in canvas order."""
    s = None
    for (Hc, Wc), windows in canvases:
        y = F.interpolate(canvas_mean(views, windows, Hc, Wc, torch.float32)[None], size=size, mode="bicubic", align_corners=False)[0]
        if mode == "prob":
            y = torch.softmax(y, dim=0)
        s = y if s is None else s + y
    return s.argmax(0)


@functools.lru_cache(maxsize=None)
def fp64_reference(name, size, mode):
    """ref_argmax of one case at one output size: computed once, shared, never modified."""
    views, canvases, amax = make_case(name)
    return ref_argmax(views, canvases, size, mode, amax)
