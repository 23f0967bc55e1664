"""Shared helper of the self-training tests (no GPU): the case list, the fp64 torch reference of the confidence / pseudo-labels
with its comparison masks, and the fp64 reference of the cross-entropy with a per-pixel weight (loss, weight sum, gradient).

Bounds (each from the project's own figures for this head, none from what the kernels give):
  * class map: compared outside head_argmax_ref's near-tie margin (top-2 gap > 5e-5 max|score|);
  * confidence: |log conf - log conf64| <= 1e-4, the bound of this head's loss — -log conf is the same log-sum-exp;
  * pseudo-labels: compared where |log conf64 - log thresh| > 1e-4 (a kernel inside its confidence bound cannot fall on the other
    side of the threshold there) and outside the tie margin; at most MAX_EXCLUDED (1 %) of a case's pixels are excluded;
  * pixel-weighted CE: loss 1e-4 relative, sum of w_y 1e-5 relative, gradient 2e-5 relative L2 (tests/wide_head_ref.py's figures
    for the narrow head)."""
import math
from functools import lru_cache

import torch
import torch.nn.functional as F

import head_argmax_ref as A

IGN = A.IGN
MAX_EXCLUDED = A.MAX_EXCLUDED
CONF_TOL = 1e-4                       # on log conf
LOSS_TOL, WSUM_TOL, GRAD_TOL = 1e-4, 1e-5, 2e-5
CLASSES = (5, 65, 151, 192)           # TN = 4, 8, 10, 12; partial last tiles; C == ld
EXTRA = [(5, 7, 4, "bilinear"), (5, 4, 8, "bicubic"), (3, 4, 16, "bicubic")]   # the (mode, S) head_argmax_ref.SHAPES does not reach
CASES = [(B, h, w, S, mode, C) for (B, h, w, S, mode) in A.SHAPES for C in CLASSES]
CASES += [(2, h, w, S, mode, C) for (h, w, S, mode) in EXTRA for C in CLASSES]
CE_VARIANTS = ("plain", "weighted", "smooth")   # no options; class weights; label smoothing 0.1 (with class weights)


def case_id(case):
    return "-".join(str(v) for v in case)


@lru_cache(maxsize=None)
def case_inputs(B, h, w, S, mode, C):
    """(scores_lo fp32 [B*h*w, ld], labels int64 [B, H, W], pixel_weight fp32 [B, H, W]): head_argmax_ref's scores (randn in the
    first C channels, PAD_SCORE past them) and labels (some negative, some >= C, every fifth row IGN); pixel weights uniform in
    [0, 2] with a fifth of the pixels exactly 0."""
    lo, labels = A.case_inputs(B, h, w, S, mode, C)
    g = torch.Generator().manual_seed(1)
    pw = 2.0 * torch.rand(labels.shape, generator=g)
    pw[torch.rand(labels.shape, generator=g) < 0.2] = 0.0
    return lo, labels, pw


def upsample64(lo, B, h, w, C, S, mode):
    x = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2)
    return F.interpolate(x, scale_factor=S, mode=mode, align_corners=False)


# ---- confidence and pseudo-labels ----
@lru_cache(maxsize=None)
def conf_ref(B, h, w, S, mode, C):
    """dict of the case's fp64 reference: arg (class map), conf, thresh (the fp64 median confidence rounded to fp32, as the kernel
    receives it: both sides of it are populated), pseudo, sure (outside the tie margin), sure_t (sure and outside the threshold
    band), kept (conf >= thresh)."""
    lo, _, _ = case_inputs(B, h, w, S, mode, C)
    hi = upsample64(lo, B, h, w, C, S, mode)
    conf, arg = hi.softmax(1).max(1)
    top2 = hi.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > A.MARGIN * lo[:, :C].abs().max().item()
    thresh = float(conf.flatten().median().float())
    kept = conf >= thresh
    pseudo = torch.where(kept, arg, torch.full_like(arg, IGN))
    sure_t = sure & ((conf.log() - math.log(thresh)).abs() > CONF_TOL)
    return dict(arg=arg, conf=conf, thresh=thresh, pseudo=pseudo, sure=sure, sure_t=sure_t, kept=kept)


def excluded_share(mask):
    return 1.0 - mask.double().mean().item()


# ---- cross-entropy with a per-pixel weight ----
def class_weights(C, seed=7, dyadic=False):
    """fp64 class weights in [0.5, 1.5] with one class at exactly 0.  dyadic: multiples of 1/8, whose sums over any set of pixels
    are exact in fp32 (the identity tests compare weight sums for equality)."""
    w = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if dyadic:
        w = (8.0 * w).round() / 8.0
    w[C // 2] = 0.0
    return w


def variant_options(variant, C):
    """(class weights fp64 [C] or None, label smoothing) of a CE variant."""
    return {"plain": (None, 0.0), "weighted": (class_weights(C), 0.0), "smooth": (class_weights(C), 0.1)}[variant]


def counted(labels, C, ignore_index=IGN):
    return A.counted(labels, C, ignore_index)


def ce_pw_ref(lo, labels, pw, B, h, w, C, S, mode, weight=None, eps=0.0, ignore_index=IGN, want_grad=True):
    """fp64: (sum_i pw_i l_i, sum_i w_y, d(sum)/d lo[:, :C] or None) over the counted pixels (label != ignore_index and 0 <= label
    < C), l_i = (1 - eps) w_y (lse - z_y) + (eps / C) (W lse - sum_c w_c z_c).  The gradient is formed analytically at the output
    resolution — dz_k = pw_i [((1 - eps) w_y + eps W / C) p_k - (1 - eps) w_y [k == y] - (eps / C) w_k] — and pulled back through
    the (linear) upsample."""
    x = lo[:, :C].double().clone().requires_grad_(want_grad)
    hi = F.interpolate(x.reshape(B, h, w, C).permute(0, 3, 1, 2), scale_factor=S, mode=mode, align_corners=False)
    z = hi.detach()
    wc = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    ok = counted(labels, C, ignore_index)
    y = labels.clamp(0, C - 1)
    lse = z.logsumexp(1)
    zy = z.gather(1, y[:, None]).squeeze(1)
    wy = wc[y]
    a1, ac, W = 1.0 - eps, eps / C, wc.sum()
    wz = (z * wc.view(1, C, 1, 1)).sum(1)
    li = a1 * wy * (lse - zy) + ac * (W * lse - wz)
    pwd = pw.double()
    loss = (pwd * li)[ok].sum()
    wsum = wy[ok].sum()
    if not want_grad:
        return loss, wsum, None
    p = z.softmax(1)
    onehot = F.one_hot(y, C).permute(0, 3, 1, 2).double()
    dz = (a1 * wy + ac * W)[:, None] * p - (a1 * wy)[:, None] * onehot - ac * wc.view(1, C, 1, 1)
    dz = dz * (pwd * ok)[:, None]
    (grad,) = torch.autograd.grad(hi, x, grad_outputs=dz)
    return loss, wsum, grad


def ce_pw_autograd(lo, labels, pw, B, h, w, C, S, mode, weight=None, eps=0.0, ignore_index=IGN):
    """The same three values from F.cross_entropy(reduction='none') * pw and autograd (labels that are not counted become
    ignore_index first: torch refuses them)."""
    x = lo[:, :C].double().clone().requires_grad_(True)
    hi = F.interpolate(x.reshape(B, h, w, C).permute(0, 3, 1, 2), scale_factor=S, mode=mode, align_corners=False)
    ok = counted(labels, C, ignore_index)
    lab = torch.where(ok, labels, torch.full_like(labels, -100))
    wd = None if weight is None else weight.double()
    li = F.cross_entropy(hi, lab, weight=wd, ignore_index=-100, reduction="none", label_smoothing=eps)
    loss = (li * pw.double()).sum()
    wsum = (torch.ones(C, dtype=torch.float64) if wd is None else wd)[labels.clamp(0, C - 1)][ok].sum()
    (grad,) = torch.autograd.grad(loss, x)
    return loss.detach(), wsum, grad


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
