"""fp64 torch reference of the Dice + cross-entropy loss (lc2is_amd.nn.DiceCrossEntropyLoss, ops.head_upsample_ce_dice):
the definition with autograd, the closed-form gradient the kernels evaluate, and the head form (F.interpolate in front)."""
import torch
import torch.nn.functional as F


def valid_mask(labels, C, ignore_index):
    return (labels != ignore_index) & (labels >= 0) & (labels < C)


def stats(z, labels, C, ignore_index):
    """z fp64 [B,C,H,W] -> softmax p, the counted mask v [B,1,H,W], the masked one-hot, and I, P, T per class."""
    valid = valid_mask(labels, C, ignore_index)
    p = torch.softmax(z, dim=1)
    v = valid.unsqueeze(1).to(z.dtype)
    onehot = F.one_hot(labels.clamp(0, C - 1), C).permute(0, 3, 1, 2).to(z.dtype) * v
    return p, v, onehot, (p * onehot).sum((0, 2, 3)), (p * v).sum((0, 2, 3)), onehot.sum((0, 2, 3))


def dice_ce(z, labels, ignore_index=-100, ce_weight=1.0, dice_weight=1.0, smooth=1.0, present_only=True):
    """The loss of the definition: dict(total, ce, dice, n_valid, I, P, T); differentiable in z."""
    C = z.shape[1]
    p, v, onehot, I, P, T = stats(z, labels, C, ignore_index)
    U = P + T + smooth
    m = (T > 0).to(z.dtype) if present_only else torch.ones_like(T)
    safe = torch.where(U > 0, U, torch.ones_like(U))
    dice = (m * torch.where(U > 0, 1.0 - (2.0 * I + smooth) / safe, torch.zeros_like(U))).sum() / C
    n = int(v.sum().item())
    if n > 0:
        ref_labels = torch.where(valid_mask(labels, C, ignore_index), labels, torch.full_like(labels, -100))
        ce = F.cross_entropy(z, ref_labels, ignore_index=-100, reduction="sum") / n
    else:
        ce = z.sum() * 0.0
        dice = dice * 0.0
    return dict(total=ce_weight * ce + dice_weight * dice, ce=ce, dice=dice, n_valid=n, I=I, P=P, T=T)


def closed_form_grad(z, labels, ignore_index=-100, ce_weight=1.0, dice_weight=1.0, smooth=1.0, present_only=True):
    """d total / d z by the formula of the kernels: p_c (ces + beta_c - q) - [c = y] (ces + alpha_y p_y) on the counted pixels."""
    C = z.shape[1]
    p, v, onehot, I, P, T = stats(z, labels, C, ignore_index)
    n = v.sum()
    if n == 0:
        return torch.zeros_like(z)
    U = P + T + smooth
    m = (T > 0).to(z.dtype) if present_only else torch.ones_like(T)
    ok = U > 0
    safe = torch.where(ok, U, torch.ones_like(U))
    alpha = dice_weight * torch.where(ok, 2.0 * m / (C * safe), torch.zeros_like(U)).view(1, C, 1, 1)
    beta = dice_weight * torch.where(ok, m * (2.0 * I + smooth) / (C * safe * safe), torch.zeros_like(U)).view(1, C, 1, 1)
    ces = ce_weight / n
    apy = ((alpha * p) * onehot).sum(1, keepdim=True)             # alpha_y p_y
    q = (p * beta).sum(1, keepdim=True) - apy
    return (p * (ces + beta - q) - onehot * (ces + apy)) * v


def head(lo, labels, B, h, w, C, S, mode, **kw):
    """lo [B*h*w, ld] (any float dtype) -> (dice_ce dict on the xS upsampled scores, d total / d lo[:, :C] fp64 [B*h*w, C])."""
    lod = lo[:, :C].double().reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = F.interpolate(lod, scale_factor=S, mode=mode)
    out = dice_ce(up, labels, **kw)
    out["total"].backward()
    grad = lod.grad.permute(0, 2, 3, 1).reshape(B * h * w, C)
    return {k: (t.detach() if isinstance(t, torch.Tensor) else t) for k, t in out.items()}, grad


def nchw(x, labels, **kw):
    """x [B,C,H,W] -> (dice_ce dict, d total / d x fp64)."""
    x64 = x.double().clone().requires_grad_(True)
    out = dice_ce(x64, labels, **kw)
    out["total"].backward()
    return {k: (t.detach() if isinstance(t, torch.Tensor) else t) for k, t in out.items()}, x64.grad
