"""fp64 reference of the sigmoid cross-entropy / sigmoid focal loss, shared by test_sigmoid_cpu.py and test_gpu_sigmoid.py.

Per counted pixel (label != ignore_index and 0 <= label < C) with label y and a class c < C: z the score, t = [c == y],
p = sigmoid(z), p_t = t ? p : 1 - p:
    bce  = softplus(z) - t z = -ln p_t
    l_c  = w_c a_t (1 - p_t)^gamma bce,    a_t = alpha given ? (t ? alpha : 1 - alpha) : 1
    l    = class_scale sum_c l_c
built from ``F.softplus`` with gradients by autograd, and the closed form of the gradient
    dl_c/dz = w_c a_t ( t ? (1-p)^gamma (gamma p ln p - (1-p)) : p^gamma (p - gamma (1-p) ln(1-p)) ).
softplus(z) - t z is taken as softplus(t ? -z : z) (the same value without the cancellation at a confident label), and
ln(1 - p_t) as -softplus of the opposite sign, so nothing is the logarithm of a rounded probability and gamma = 0 forms no 0^0.
The head cases are focal_ref's (test_gpu_ce_options._head_case's inputs)."""
from functools import lru_cache

import torch
import torch.nn.functional as F

from focal_ref import CASES, IGN, head_case, weights  # noqa: F401  (re-exported)

PARAMS = [(2, 0.25), (0, None), (0.5, 0.75), (1.5, None), (0, 0.25)]      # (gamma, alpha)


def _valid(labels, C, ignore_index):
    valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    return valid, F.one_hot(safe, C).permute(0, 3, 1, 2).bool()


def _alpha_t(onehot, alpha, dtype):
    if alpha is None:
        return torch.ones((), dtype=dtype, device=onehot.device)
    kw = dict(dtype=dtype, device=onehot.device)
    return torch.where(onehot, torch.tensor(float(alpha), **kw), torch.tensor(1.0 - float(alpha), **kw))


def elem_loss(logits, onehot, gamma, alpha, weight=None):
    """The [B,C,H,W] map of l_c (every pixel treated as counted)."""
    s = torch.where(onehot, -logits, logits)
    l = F.softplus(s)                                         # bce = softplus(z) - t z
    if gamma != 0:
        l = torch.exp(-gamma * F.softplus(-s)) * l            # (1 - p_t)^gamma, ln(1 - p_t) = -softplus(-s)
    l = _alpha_t(onehot, alpha, logits.dtype) * l
    return l if weight is None else l * weight.to(logits.dtype)[None, :, None, None]


def loss_px(logits, labels, gamma, alpha, weight=None, ignore_index=IGN, class_scale=1.0):
    """Per-pixel losses [B,H,W] (the sum over the classes times class_scale, 0 where not counted) and the counted mask."""
    valid, onehot = _valid(labels, logits.shape[1], ignore_index)
    l = class_scale * elem_loss(logits, onehot, gamma, alpha, weight).sum(1)
    return torch.where(valid, l, torch.zeros_like(l)), valid


def reduce(lpx, valid, reduction, normalize="elements", C=1):
    """SigmoidFocalLoss's reductions of the class-summed per-pixel losses (class_scale = 1)."""
    if reduction == "none":
        return lpx
    if reduction == "sum":
        return lpx.sum()
    return lpx.sum() / (valid.sum() * (C if normalize == "elements" else 1))


def closed_form_grad(logits, labels, gamma, alpha, weight=None, ignore_index=IGN):
    """d(sum of the per-pixel losses)/d logits from the closed form."""
    valid, onehot = _valid(labels, logits.shape[1], ignore_index)
    z = logits
    p, q = torch.sigmoid(z), torch.sigmoid(-z)                 # p, 1 - p
    lnp, lnq = -F.softplus(-z), -F.softplus(z)                 # ln p, ln(1 - p)
    pos = torch.exp(gamma * lnq) * (gamma * p * lnp - q)
    neg = torch.exp(gamma * lnp) * (p - gamma * q * lnq)
    g = _alpha_t(onehot, alpha, z.dtype) * torch.where(onehot, pos, neg)
    if weight is not None:
        g = g * weight.to(z.dtype)[None, :, None, None]
    return g * valid[:, None].to(z.dtype)


def head_loss(lo, ref_labels, B, h, w, C, S, mode, gamma, alpha, weight=None, class_scale=1.0):
    """The fused head's outputs in fp64: (sum of losses, number of counted pixels, d sum / d lo as [B*h*w, C])."""
    lod = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = F.interpolate(lod, scale_factor=S, mode=mode)
    lpx, valid = loss_px(up, ref_labels, gamma, alpha, weight, class_scale=class_scale)
    total = lpx.sum()
    total.backward()
    return total.item(), int(valid.sum()), lod.grad.permute(0, 2, 3, 1).reshape(B * h * w, C)


def upsampled(lo, B, h, w, C, S, mode):
    """(the fp64 low-res scores [B,C,h,w] as a leaf that requires grad, their upsampled map [B,C,H,W])."""
    lod = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    return lod, F.interpolate(lod, scale_factor=S, mode=mode)


@lru_cache(maxsize=None)
def case_ref(i, gamma, alpha, B=2):
    """(lo, labels, class weights, (loss sum, count, gradient)) of CASES[i] at (gamma, alpha), computed once."""
    mode, S, C, h, w = CASES[i]
    lo, labels, ref_labels = head_case(B, h, w, C, S, 31 * C + S)
    w64 = weights(C, C)
    return lo, labels, w64, head_loss(lo, ref_labels, B, h, w, C, S, mode, gamma, alpha, w64)


SAT = dict(B=1, h=8, w=8, C=151, S=4, mode="bicubic", A=7, Bc=100, Wr=42)


def saturated_case():
    """One image whose class scores are all -120 but: on the upper half of the grid (region A) class A is +120 and is the label —
    every term underflows in fp32; on the lower half (region B) the label Bc stays at -120 and class Wr is +120 — confidently
    wrong.  The rows of pixels around the seam interpolate between the two; every seventh column is ignored."""
    s = SAT
    lo = torch.zeros(s["B"], s["h"], s["w"], 192)
    lo[..., :s["C"]] = -120.0
    lo[:, :s["h"] // 2, :, s["A"]] = 120.0
    lo[:, s["h"] // 2:, :, s["Wr"]] = 120.0
    H = s["h"] * s["S"]
    labels = torch.full((s["B"], H, s["w"] * s["S"]), s["A"], dtype=torch.long)
    labels[:, H // 2:] = s["Bc"]
    labels[:, :, 3::7] = IGN
    return lo.reshape(-1, 192).contiguous(), labels


def region_a_only(labels):
    """The saturated case's labels with everything but region A's interior ignored (the last cell row of region A interpolates
    towards region B)."""
    top = labels.clone()
    top[:, SAT["h"] * SAT["S"] // 2 - 4:] = IGN
    return top
