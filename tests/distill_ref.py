"""Shared helper of the distillation tests (no GPU): the case list (selftrain_ref.CASES), the teacher's scores, and the fp64
torch reference of the per-pixel KL(teacher || student) of the upsampled scores at a temperature T — loss sum, count, gradient.

Per counted pixel i (labels None: every pixel; else label != ignore_index and 0 <= label < C), u = z / T, p = softmax(u):
    loss_i = pw_i T^2 sum_c p_t,c (log p_t,c - log p_s,c)      count_i = 1      dz_s,c = pw_i T (p_s,c - p_t,c)

Bounds (each from the project's figures for this head, selftrain_ref: loss 1e-4 relative, gradient 2e-5 relative L2; none from
what the kernel gives):
  * loss: KL_i = H(p_t, p_s)_i - H(p_t)_i is a difference of two quantities the head forms to 1e-4 relative each, so
    |sum - sum64| <= LOSS_TOL * sum_i pw_i T^2 (H(p_t, p_s) + H(p_t))_i, the right side in fp64 (``scale``);
  * gradient: GRAD_TOL = 2e-5 relative L2;
  * count: exact."""
from functools import lru_cache

import torch
import torch.nn.functional as F

import head_argmax_ref as A
import selftrain_ref as S

IGN = S.IGN
CASES = S.CASES
case_id = S.case_id
LOSS_TOL, GRAD_TOL = S.LOSS_TOL, S.GRAD_TOL
TEMPS = (1.0, 4.0)


@lru_cache(maxsize=None)
def case_inputs(B, h, w, S_, mode, C):
    """(student fp32 [B*h*w, ld], teacher fp32 [B*h*w, ld], labels, pixel_weight): the case's scores (PAD_SCORE past C), an
    independent randn teacher (seed 5) with -PAD_SCORE past C — a kernel that fails to mask EITHER map is caught — and the case's
    own labels and pixel weights."""
    lo, labels, pw = S.case_inputs(B, h, w, S_, mode, C)
    t = torch.full(lo.shape, -A.PAD_SCORE)
    t[:, :C] = torch.randn(lo.shape[0], C, generator=torch.Generator().manual_seed(5))
    return lo, t, labels, pw


def kd_ref(lo, tlo, labels, pw, B, h, w, C, S_, mode, temp, ignore_index=IGN, want_grad=True):
    """fp64: dict(loss = sum_i loss_i, count, grad = d loss / d lo[:, :C] or None, scale = sum_i pw_i T^2 (H(p_t, p_s) + H(p_t))_i).
    ``labels`` / ``pw`` may be None (every pixel counted / weight 1).  The gradient is formed analytically at the output resolution
    and pulled back through the (linear) upsample, as selftrain_ref.ce_pw_ref does."""
    x = lo[:, :C].double().clone().requires_grad_(want_grad)
    hi = F.interpolate(x.reshape(B, h, w, C).permute(0, 3, 1, 2), scale_factor=S_, mode=mode, align_corners=False)
    zt = S.upsample64(tlo, B, h, w, C, S_, mode)
    zs = hi.detach()
    ok = torch.ones(zs.shape[0], zs.shape[2], zs.shape[3], dtype=torch.bool) if labels is None else S.counted(labels, C, ignore_index)
    pwd = torch.ones(ok.shape, dtype=torch.float64) if pw is None else pw.double()
    ls, lt = (zs / temp).log_softmax(1), (zt / temp).log_softmax(1)
    pt = lt.exp()
    cross = -(pt * ls).sum(1)                           # H(p_t, p_s)
    ent = -torch.where(pt > 0, pt * lt, torch.zeros_like(pt)).sum(1)   # H(p_t): 0 log 0 = 0
    t2 = temp * temp
    loss = (pwd * t2 * (cross - ent))[ok].sum()
    scale = (pwd * t2 * (cross + ent))[ok].sum()
    out = dict(loss=loss, count=int(ok.sum()), scale=scale, grad=None)
    if want_grad:
        dz = temp * (ls.exp() - pt) * (pwd * ok)[:, None]
        (out["grad"],) = torch.autograd.grad(hi, x, grad_outputs=dz)
    return out


def kd_autograd(lo, tlo, labels, pw, B, h, w, C, S_, mode, temp, ignore_index=IGN):
    """(loss, grad) from T^2 F.kl_div(log_softmax(s / T), softmax(t / T), reduction='none').sum(1) * pw over the counted pixels, by
    autograd."""
    x = lo[:, :C].double().clone().requires_grad_(True)
    hi = F.interpolate(x.reshape(B, h, w, C).permute(0, 3, 1, 2), scale_factor=S_, mode=mode, align_corners=False)
    zt = S.upsample64(tlo, B, h, w, C, S_, mode)
    ok = torch.ones(hi.shape[0], hi.shape[2], hi.shape[3], dtype=torch.bool) if labels is None else S.counted(labels, C, ignore_index)
    pwd = torch.ones(ok.shape, dtype=torch.float64) if pw is None else pw.double()
    kl = temp * temp * F.kl_div((hi / temp).log_softmax(1), (zt / temp).softmax(1), reduction="none").sum(1) * pwd
    loss = kl[ok].sum()
    (grad,) = torch.autograd.grad(loss, x)
    return loss.detach(), grad


@lru_cache(maxsize=None)
def case_ref(case, temp, weighted):
    """The reference of (case, T, with labels + pixel weight or with neither), computed once and shared."""
    B, h, w, S_, mode, C = case
    lo, t, labels, pw = case_inputs(*case)
    return kd_ref(lo, t, labels if weighted else None, pw if weighted else None, B, h, w, C, S_, mode, temp)


rel = S.rel
