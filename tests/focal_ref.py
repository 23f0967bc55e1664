"""fp64 reference of the focal / poly-1 cross-entropy, shared by test_focal_cpu.py and test_gpu_focal.py.

Per counted pixel (label != ignore_index and 0 <= label < C) with label y, p = softmax, q = 1 - p_y, ce = -log p_y:
    l = w_y (q^gamma ce + eps1 q)
composed from ``log_softmax`` with gradients by autograd, and the closed form of the gradient
    dl/dz_j = w_y c (p_j - [j == y]),   c = q^gamma + gamma p_y q^(gamma-1) ce + eps1 p_y.
q is exp(logsumexp of the OTHER classes' log-probabilities): 1 - exp(log p_y) is exactly 0 in fp64 once the label leads by about
37, and autograd through 0^gamma is NaN for gamma < 1.  The head cases reuse head_cases.head_case's inputs."""
from functools import lru_cache

import torch
import torch.nn.functional as F

from head_cases import IGN, head_case  # noqa: F401  (head_case re-exported)

PARAMS = [(2, 0), (0.5, 0), (0, 1), (1.5, 2), (0, 0)]      # (gamma, poly_eps)
# (mode, S, C, h, w): the four channel-tile counts (TN = 4: C = 10, 37, 64; 8: 100; 10: 150, 151; 12: 192), the three scales,
# non-square grids, 16 x 16 tiles that straddle the image edge
CASES = [("bicubic", 4, 151, 5, 5), ("bicubic", 4, 192, 7, 7), ("bilinear", 4, 10, 12, 12), ("bicubic", 8, 37, 7, 5),
         ("bilinear", 8, 100, 5, 7), ("bicubic", 16, 150, 3, 5), ("bilinear", 16, 64, 5, 5)]
# behind them, the (mode, S, TN) instantiations of head_focal_grp_kernel / head_sigmoid_grp_kernel that the seven do not reach
CASES += [
    ("bicubic", 4, 10, 5, 7), ("bicubic", 4, 100, 5, 7), ("bicubic", 8, 100, 5, 4), ("bicubic", 8, 151, 5, 4),
    ("bicubic", 8, 192, 5, 4), ("bicubic", 16, 10, 3, 4), ("bicubic", 16, 100, 3, 4), ("bicubic", 16, 192, 3, 4),
    ("bilinear", 4, 100, 5, 7), ("bilinear", 4, 151, 5, 7), ("bilinear", 4, 192, 5, 7), ("bilinear", 8, 10, 5, 4),
    ("bilinear", 8, 151, 5, 4), ("bilinear", 8, 192, 5, 4), ("bilinear", 16, 100, 3, 4), ("bilinear", 16, 151, 3, 4),
    ("bilinear", 16, 192, 3, 4)]


def weights(C, seed):
    """Class weights in [0.25, 1.75], fp64."""
    return torch.rand(C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 1.5 + 0.25


def _terms(logits, labels, ignore_index):
    C = logits.shape[1]
    valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    logp = F.log_softmax(logits, 1)
    onehot = F.one_hot(safe, C).permute(0, 3, 1, 2).bool()
    lp = logp.gather(1, safe[:, None])[:, 0]
    logq = torch.logsumexp(logp.masked_fill(onehot, -float("inf")), 1)
    return valid, safe, onehot, lp, logq


def loss_px(logits, labels, gamma, poly_eps, weight=None, ignore_index=IGN):
    """Per-pixel losses [B,H,W] (0 where not counted) and the per-pixel weights w_y (0 where not counted) of fp64 NCHW logits."""
    valid, safe, _, lp, logq = _terms(logits, labels, ignore_index)
    wy = (torch.ones_like(lp) if weight is None else weight[safe]) * valid
    l = wy * (torch.exp(gamma * logq) * (-lp) + poly_eps * torch.exp(logq))
    return torch.where(valid, l, torch.zeros_like(l)), wy


def reduce(lpx, wy, reduction):
    if reduction == "none":
        return lpx
    return lpx.sum() / wy.sum() if reduction == "mean" else lpx.sum()


def closed_form_c(logits, labels, gamma, poly_eps, ignore_index=IGN):
    """The per-pixel scalar c of the closed-form gradient (0 where not counted)."""
    valid, _, _, lp, logq = _terms(logits, labels, ignore_index)
    p, ce = torch.exp(lp), -lp
    c = torch.exp(gamma * logq) + gamma * p * torch.exp((gamma - 1.0) * logq) * ce + poly_eps * p
    return torch.where(valid, c, torch.zeros_like(c))


def closed_form_grad(logits, labels, gamma, poly_eps, weight=None, ignore_index=IGN):
    """d(sum of the per-pixel losses)/d logits from the closed form."""
    valid, safe, onehot, _, _ = _terms(logits, labels, ignore_index)
    wy = (torch.ones(labels.shape, dtype=logits.dtype) if weight is None else weight[safe]) * valid
    c = closed_form_c(logits, labels, gamma, poly_eps, ignore_index)
    return (wy * c)[:, None] * (F.softmax(logits, 1) - onehot.to(logits.dtype))


def head_loss(lo, ref_labels, B, h, w, C, S, mode, gamma, poly_eps, weight=None):
    """The fused head's outputs in fp64: (sum of losses, sum of w_y, d sum / d lo as [B*h*w, C])."""
    lod = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = F.interpolate(lod, scale_factor=S, mode=mode)
    lpx, wy = loss_px(up, ref_labels, gamma, poly_eps, weight)
    total = lpx.sum()
    total.backward()
    return total.item(), wy.sum().item(), lod.grad.permute(0, 2, 3, 1).reshape(B * h * w, C)


@lru_cache(maxsize=None)
def case_ref(i, gamma, poly_eps, B=2):
    """(lo, labels, class weights, (loss sum, weighted count, gradient)) of CASES[i] at (gamma, poly_eps), computed once."""
    mode, S, C, h, w = CASES[i]
    lo, labels, ref_labels = head_case(B, h, w, C, S, 31 * C + S)
    w64 = weights(C, C)
    return lo, labels, w64, head_loss(lo, ref_labels, B, h, w, C, S, mode, gamma, poly_eps, w64)


SAT = dict(B=1, h=8, w=8, C=151, S=4, mode="bicubic", A=7, Bc=100)


def saturated_case():
    """One image of uniform (zero) scores.  On the upper half of the grid class A is 120 above the rest and is the label: q = 1 - p
    underflows to exactly 0 in fp32.  On the lower half class Bc is 120 BELOW the rest and is the label: p is 0 in fp32.  The two
    rows of pixels around the seam interpolate between the two; every seventh column is ignored."""
    s = SAT
    lo = torch.zeros(s["B"], s["h"], s["w"], 192)
    lo[:, :s["h"] // 2, :, s["A"]] = 120.0
    lo[:, s["h"] // 2:, :, s["Bc"]] = -120.0
    H = s["h"] * s["S"]
    labels = torch.full((s["B"], H, s["w"] * s["S"]), s["A"], dtype=torch.long)
    labels[:, H // 2:] = s["Bc"]
    labels[:, :, 3::7] = IGN
    return lo.reshape(-1, 192).contiguous(), labels
