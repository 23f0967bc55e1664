"""Inputs and case lists that the tests of the fused head's group kernels share (no GPU).

A group kernel is instantiated per (mode, S, TN): two interpolation modes, S = 4 / 8 / 16, TN = 4 / 8 / 10 / 12 channel tiles of 16
(the smallest that covers C): C = 10 / 100 / 151 / 192 reach the four TN.  The lists name every one of the 24 combinations; those
added for that alone run at the smallest grids with an interior tile, a tile that straddles the image edge and a non-square shape
(5 x 7 at S = 4, 5 x 4 at S = 8, 3 x 4 at S = 16)."""
import torch

IGN = -100

# (mode, S, C, h, w).  C covers the four channel-tile counts of the group kernel: TN = 4 (10, 37, 64), 8 (100), 10 (150, 151), 12 (192)
HEAD_CASES = [("bicubic", 4, 151, 5, 5), ("bicubic", 4, 192, 7, 7), ("bilinear", 4, 10, 12, 12), ("bilinear", 4, 151, 12, 7),
              ("bicubic", 8, 37, 7, 5), ("bilinear", 8, 100, 5, 7), ("bicubic", 16, 150, 3, 5), ("bilinear", 16, 64, 5, 5),
              ("bicubic", 16, 100, 4, 4), ("bilinear", 8, 192, 4, 6)]
# behind them (indices 0-9 are used by name), the (mode, S, TN) the ten do not reach
HEAD_CASES_ALL = HEAD_CASES + [
    ("bicubic", 4, 10, 5, 7), ("bicubic", 4, 100, 5, 7), ("bicubic", 8, 100, 5, 4), ("bicubic", 8, 151, 5, 4),
    ("bicubic", 8, 192, 5, 4), ("bicubic", 16, 10, 3, 4), ("bicubic", 16, 192, 3, 4), ("bilinear", 4, 100, 5, 7),
    ("bilinear", 4, 192, 5, 7), ("bilinear", 8, 10, 5, 4), ("bilinear", 8, 151, 5, 4), ("bilinear", 16, 100, 3, 4),
    ("bilinear", 16, 151, 3, 4), ("bilinear", 16, 192, 3, 4)]


def head_case(B, h, w, C, S, seed):
    """Scores [B*h*w, ld] (zeros past C), labels with some >= C (skipped by the kernel) and every fifth row ignored, and the labels
    the reference sees (>= C mapped to IGN: torch raises on them)."""
    g = torch.Generator().manual_seed(seed)
    ld = 64 if C <= 64 else (128 if C <= 128 else 192)
    lo = torch.zeros(B * h * w, ld)
    lo[:, :C] = torch.randn(B * h * w, C, generator=g) * 3
    labels = torch.randint(0, C + 3, (B, h * S, w * S), generator=g)
    labels[:, 1::5] = IGN
    ref_labels = torch.where(labels >= C, torch.full_like(labels, IGN), labels)
    return lo, labels, ref_labels
