"""Shared helper of the wide-head tests (no GPU): the case list past 192 classes on the generator of tests/head_argmax_ref.py, the
fp64 torch reference of the upsampled cross-entropy (loss sum, weight sum, gradient wrt the low-resolution scores), the bounds, and
the online-softmax edge cases."""
import sys
from functools import lru_cache
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_argmax_ref as A  # noqa: E402

IGN = A.IGN
S = 4
CHUNK = 192
# (B, h, w, mode): 3 x 3 tiles starting at -2 with a ragged last tile; non-square; bilinear
SHAPES = [(2, 9, 9, "bicubic"), (1, 5, 9, "bicubic"), (2, 5, 5, "bilinear")]
# a second chunk of one channel; C == ld; a one-channel tile past a 64 multiple; two exact chunks; A-847's ragged fifth chunk; the cap
CLASSES = [193, 256, 257, 384, 847, 1024]
CASES = [(B, h, w, mode, C) for (B, h, w, mode) in SHAPES for C in CLASSES]
IDS = ["-".join(map(str, c)) for c in CASES]

# The project's bounds for this head at C <= 192 (tests/test_gpu_ce_options.py, tests/test_gpu_focal.py): loss 1e-4 relative, weight
# sum 1e-5 relative, gradient relative L2 2e-5.  The softmax sums of an ld-channel head have ld / 192 times as many fp32 terms, and
# linear growth of the rounding error with the number of terms is the worst case: the loss and gradient bounds scale by ld / 192.
LOSS_TOL, WSUM_TOL, GRAD_TOL = 1e-4, 1e-5, 2e-5


def bounds(ld: int):
    return LOSS_TOL * ld / CHUNK, WSUM_TOL, GRAD_TOL * ld / CHUNK


def ld_of(C: int) -> int:
    return A.ld_of(C)


def weights(C: int, seed: int) -> torch.Tensor:
    """fp64 class weights in [0.5, 1.5) with a few exact zeros (a zero-weight class is counted with weight 0)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    w[torch.randperm(C, generator=g)[:max(2, C // 50)]] = 0.0
    return w


@lru_cache(maxsize=None)
def case_inputs(B, h, w, mode, C):
    """head_argmax_ref's inputs (randn scores, PAD_SCORE past C, labels in [-2, C + 2], every fifth row IGN) with a few label pixels
    set to the chunk boundaries 0, 191, 192 and C - 1."""
    lo, labels = A.case_inputs(B, h, w, S, mode, C)
    labels = labels.clone()
    for i, v in enumerate((0, CHUNK - 1, CHUNK, C - 1)):
        labels[:, 0, i] = v          # (row 0 is not an ignored row)
        labels[:, 7, 4 * i + 1] = v
    return lo, labels


def ce_ref(lo, labels, B, h, w, C, mode, w64=None):
    """fp64: (sum_i w_y (lse - z_y), sum_i w_y, d loss / d scores_lo [B*h*w, C]) of F.interpolate(align_corners=False) +
    F.cross_entropy(reduction='sum') over the counted pixels (label != IGN and 0 <= label < C)."""
    x = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    hi = F.interpolate(x, scale_factor=S, mode=mode, align_corners=False)
    valid = A.counted(labels, C, IGN)
    lab = torch.where(valid, labels, torch.full_like(labels, IGN))
    loss = F.cross_entropy(hi, lab, weight=w64, ignore_index=IGN, reduction="sum")
    loss.backward()
    wsum = float(valid.sum()) if w64 is None else w64[labels[valid]].sum().item()
    return loss.item(), wsum, x.grad.permute(0, 2, 3, 1).reshape(B * h * w, C)


@lru_cache(maxsize=None)
def case_ref(case: int, weighted: bool):
    B, h, w, mode, C = CASES[case]
    lo, labels = case_inputs(B, h, w, mode, C)
    w64 = weights(C, 100 + case) if weighted else None
    return lo, labels, w64, ce_ref(lo, labels, B, h, w, C, mode, w64)


# ---- online-softmax edge cases: C = 847 (chunks 0..191, ..., 768..846), one bicubic shape ----
EDGE = dict(B=1, h=5, w=9, mode="bicubic", C=847)
EDGE_NAMES = ("max_last_label_first", "max_first_label_last", "huge_scores")


@lru_cache(maxsize=None)
def edge_case(name: str):
    """(scores_lo, labels): the running maximum moves in the last chunk while the label's logit was picked up in the first; the
    reverse; scores of +-1e4 in different chunks."""
    e = EDGE
    g = torch.Generator().manual_seed(11)
    C, n = e["C"], e["B"] * e["h"] * e["w"]
    lo = torch.full((n, ld_of(C)), A.PAD_SCORE)
    lo[:, :C] = torch.randn(n, C, generator=g)
    H, W = e["h"] * S, e["w"] * S
    if name == "max_last_label_first":
        lo[:, C - 1] += 8.0
        labels = torch.randint(0, CHUNK, (e["B"], H, W), generator=g)
    elif name == "max_first_label_last":
        lo[:, 3] += 8.0
        labels = torch.randint(4 * CHUNK, C, (e["B"], H, W), generator=g)
    elif name == "huge_scores":
        lo[0::3, 100] = 1e4
        lo[1::3, 800] = -1e4
        lo[2::3, 500] = 1e4
        labels = torch.randint(0, C, (e["B"], H, W), generator=g)
    else:
        raise KeyError(name)
    labels[:, 1::5] = IGN
    return lo, labels


@lru_cache(maxsize=None)
def edge_ref(name: str):
    e = EDGE
    lo, labels = edge_case(name)
    w64 = weights(e["C"], 7)
    return lo, labels, w64, ce_ref(lo, labels, e["B"], e["h"], e["w"], e["C"], e["mode"], w64)
