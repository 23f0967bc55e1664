"""Shared helper of the head-argmax tests (no GPU): the case list, the fp64 torch reference of the class map with its top-2 gap,
and the counting rule by ``torch.bincount``."""
from functools import lru_cache

import torch
import torch.nn.functional as F

IGN = -100
MARGIN = 5e-5          # a pixel is compared iff its fp64 top-2 gap exceeds MARGIN * max|score| (tests/test_gpu_resize_argmax.py's margin)
MAX_EXCLUDED = 0.01    # at most this share of a case's pixels may be excluded

# (B, h, w, S, mode): 3 x 3 tiles starting at -2 with a ragged last tile; non-square; bilinear x8; bilinear x16
SHAPES = [(2, 9, 9, 4, "bicubic"), (1, 5, 9, 4, "bicubic"), (2, 5, 5, 8, "bilinear"), (1, 3, 3, 16, "bilinear")]
CLASSES = [5, 64, 65, 129, 151, 161, 192]   # TN = 4, 4, 8, 10, 10, 12, 12; partial last tiles; C == ld
CASES = [(B, h, w, S, mode, C) for (B, h, w, S, mode) in SHAPES for C in CLASSES]
# behind the product (indices into it are used by name): the (mode, S) it does not reach, at each TN = 4 / 8 / 10 / 12
CASES += [(2, h, w, S, mode, C) for (h, w, S, mode) in [(5, 7, 4, "bilinear"), (5, 4, 8, "bicubic"), (3, 4, 16, "bicubic")]
          for C in (10, 100, 151, 192)]
PAD_SCORE = 50.0       # what the channels past C hold: above every real score, so a kernel that does not mask them picks one


def ld_of(C: int) -> int:
    return (C + 63) // 64 * 64


@lru_cache(maxsize=None)
def case_inputs(B, h, w, S, mode, C):
    """(scores_lo fp32 [B*h*w, ld], labels int64 [B, H, W]): randn scores (seed 0) in the first C channels and PAD_SCORE past them;
    labels in [-2, C + 2] (negative and >= C values are not counted), every fifth row IGN."""
    g = torch.Generator().manual_seed(0)
    lo = torch.full((B * h * w, ld_of(C)), PAD_SCORE)
    lo[:, :C] = torch.randn(B * h * w, C, generator=g)
    labels = torch.randint(-2, C + 3, (B, h * S, w * S), generator=g)
    labels[:, 1::5] = IGN
    return lo, labels


def ref_argmax(lo, B, h, w, C, S, mode):
    """fp64: (class map int64 [B, H, W] with exact ties to the lowest class, top-2 gap [B, H, W])."""
    x = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2)
    hi = F.interpolate(x, scale_factor=S, mode=mode, align_corners=False)
    arg = hi.argmax(1)
    if C == 1:
        return arg, torch.full(arg.shape, float("inf"), dtype=torch.float64)
    top2 = hi.topk(2, dim=1).values
    return arg, top2[:, 0] - top2[:, 1]


@lru_cache(maxsize=None)
def case_ref(B, h, w, S, mode, C):
    """The reference of a case, computed once and shared: (arg, sure) with sure = the pixels outside the near-tie margin."""
    lo, _ = case_inputs(B, h, w, S, mode, C)
    arg, gap = ref_argmax(lo, B, h, w, C, S, mode)
    return arg, gap > MARGIN * lo[:, :C].abs().max().item(), gap


def counted(labels, C, ignore_index):
    return (labels != ignore_index) & (labels >= 0) & (labels < C)


def counts(pred, labels, C, ignore_index):
    """int64 [B, 3, C] {intersection, predicted, labelled}: a pixel counts iff label != ignore_index and 0 <= label < C; a counted
    pixel adds to predicted[pred] and labelled[label], and to intersection[pred] when pred == label; no other pixel adds anything."""
    pred, labels = pred.long().cpu(), labels.long().cpu()
    out = torch.zeros(pred.shape[0], 3, C, dtype=torch.int64)
    for b in range(pred.shape[0]):
        p, l = pred[b].reshape(-1), labels[b].reshape(-1)
        v = counted(l, C, ignore_index)
        out[b, 0] = torch.bincount(p[v & (p == l)], minlength=C)
        out[b, 1] = torch.bincount(p[v], minlength=C)
        out[b, 2] = torch.bincount(l[v], minlength=C)
    return out
