"""Losses of the hot path on MI355X — drop-ins for ``nn.CrossEntropyLoss()`` as used by the reference
(evaluate.py:68, engine.py:82,94,150) and for ``model/loss.py``'s ``AuxiliaryLoss``.

Both take NCHW fp32 logits and int64 labels like the reference, and nn.CrossEntropyLoss's class weights, label smoothing and
reductions ('mean' = sum of the per-pixel losses over the sum of the counted pixels' class weights, as torch).
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn.modules.loss import _Reduction

from .. import ops
from .base import require_cuda


class _PixelLossFn(torch.autograd.Function):
    """A per-pixel criterion on NCHW logits with 'mean' / 'sum' / 'none': ``fwd`` / ``bwd`` are its pair of ops, ``kw`` their
    keywords.  ``has_lse``: ``fwd`` returns (loss2, lse[, per-pixel]) and ``bwd`` takes the lse after the labels (the softmax
    losses); otherwise loss2 or (loss2, per-pixel) and no lse (the sigmoid losses).  The default cross-entropy goes through here
    too: with no weight and no smoothing the C side launches the plain kernels."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, reduction, fwd, bwd, has_lse, kw):
        lg = logits.float().contiguous()
        lb = labels.contiguous()
        out = fwd(lg, lb, ignore_index, per_pixel=reduction == "none", **kw)
        loss2, *rest = out if (has_lse or reduction == "none") else (out,)
        ctx.saved = (lg, lb, rest[:1] if has_lse else [], loss2, ignore_index, kw, reduction, bwd)
        if reduction == "none":
            return rest[-1]
        return loss2[0] / loss2[1] if reduction == "mean" else loss2[0]

    @staticmethod
    def backward(ctx, g):
        lg, lb, lse, loss2, ignore_index, kw, reduction, bwd = ctx.saved
        if reduction == "none":
            d = bwd(lg, lb, *lse, None, 1.0, ignore_index, grad_px=g.float().contiguous(), **kw)
        else:   # device scalar: upstream gradient (over the weighted count / the number of counted pixels for 'mean')
            scale = (g / loss2[1] if reduction == "mean" else g).reshape(1).float().contiguous()
            d = bwd(lg, lb, *lse, scale, 1.0, ignore_index, **kw)
        return (d,) + (None,) * 7


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss for [B,C,H,W] logits / [B,H,W] labels on the HIP path: class weights (registered as the buffer
    ``weight`` like torch's), ``reduction`` 'mean' / 'sum' / 'none', ``label_smoothing``, legacy ``size_average`` / ``reduce``."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0.0) -> None:
        super().__init__()
        if size_average is not None or reduce is not None:
            reduction = _Reduction.legacy_get_string(size_average, reduce)
        if reduction not in ("mean", "sum", "none"):   # (torch raises at the first forward)
            raise ValueError(f"{reduction} is not a valid value for reduction")
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
        self.register_buffer("weight", weight)
        self.weight: torch.Tensor | None
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing

    def _check_nchw(self, input: torch.Tensor, target: torch.Tensor, name: str) -> None:
        """The guard of every ``forward`` of this family; ``name``: the class whose forward it is."""
        require_cuda(input, "logits")
        if input.dim() != 4 or target.dim() != 3:
            raise ValueError(f"lc2is_amd {name} expects [B,C,H,W] logits and [B,H,W] labels")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self._check_nchw(input, target, "CrossEntropyLoss")
        return _PixelLossFn.apply(input, target, self.ignore_index, self.reduction, ops.ce_nchw_fwd, ops.ce_nchw_bwd, True,
                                  dict(class_weight=self.weight, label_smoothing=self.label_smoothing))


def check_ohem(thresh, min_kept) -> tuple[float, int]:
    """(thresh, min_kept per image) of an OHEM selection, validated: thresh in (0, 1], min_kept an integer >= 0."""
    if not ops.finite_ge(thresh) or not 0.0 < thresh <= 1.0:
        raise ValueError(f"OHEM thresh must be a number in (0, 1] (thresh=None, pure top-k, is not implemented), got {thresh!r}")
    if isinstance(min_kept, bool) or not isinstance(min_kept, int) or min_kept < 0:
        raise ValueError(f"OHEM min_kept must be an integer >= 0 (pixels per image), got {min_kept!r}")
    return float(thresh), int(min_kept)


class OhemCrossEntropyLoss(CrossEntropyLoss):
    """Cross-entropy over the hard pixels only (mmseg's OHEMPixelSampler with a threshold, HRNet's OhemCrossEntropy), selected on
    the device.  With l_i the plain per-pixel CE (weights and smoothing never enter the selection), K = min_kept * batch size,
    k = min(K, n_valid - 1) and L the valid loss of rank k (descending): a valid pixel is kept iff l_i > min(L, -log(thresh)) —
    the pixels whose probability of the right class is below ``thresh``, and at least about ``min_kept`` per image when fewer are.
    The loss is this module's CrossEntropyLoss (weight, label_smoothing, 'mean' over the kept weighted count / 'sum') with every
    other pixel's label set to ``ignore_index``.  The selection applies while ``self.training``; in ``eval()`` this is the plain
    criterion.  ``last_info``: the device block (n_valid, k, L, L_eff) of the last selection (``ops.ohem_info_fields`` reads it; nothing
    here syncs), ``last_labels``: the labels the criterion was then applied to.
    Under data parallelism each rank selects over its own batch."""

    def __init__(self, thresh: float = 0.7, min_kept: int = 100_000, weight=None, ignore_index: int = -100,
                 reduction: str = "mean", label_smoothing: float = 0.0) -> None:
        super().__init__(weight=weight, ignore_index=ignore_index, reduction=reduction, label_smoothing=label_smoothing)
        if self.reduction == "none":
            raise ValueError("OhemCrossEntropyLoss: reduction='none' has no meaning for a selection that drops pixels "
                             "(use 'mean' or 'sum')")
        self.thresh, self.min_kept = check_ohem(thresh, min_kept)
        self.last_labels = self.last_info = None

    @property
    def ohem(self) -> tuple[float, int]:
        return self.thresh, self.min_kept

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not self.training:
            return super().forward(input, target)
        self._check_nchw(input, target, "OhemCrossEntropyLoss")
        lg = input.detach().float().contiguous()
        lb = target.contiguous()
        _, _, lpx = ops.ce_nchw_fwd(lg, lb, self.ignore_index, per_pixel=True)   # plain CE per pixel: no weights, no smoothing
        self.last_labels, self.last_info = ops.ohem_select(lpx, lb, input.shape[1], self.thresh, self.min_kept * input.shape[0],
                                                           self.ignore_index)
        return super().forward(input, self.last_labels)


def check_dice(ce_weight, dice_weight, smooth, present_only) -> tuple[float, float, float, bool]:
    """(ce_weight, dice_weight, smooth, present_only) of a Dice + CE loss, validated: finite numbers >= 0, the weights not both 0,
    present_only a bool."""
    return ops.dice_options(ce_weight, dice_weight, smooth, present_only)


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, dice, owner):
        lg = logits.float().contiguous()
        lb = labels.contiguous()
        ce_weight, dice_weight, smooth, present_only = dice
        loss4, stats, lse, coef = ops.ce_dice_nchw_fwd(lg, lb, ignore_index, ce_weight=ce_weight, dice_weight=dice_weight,
                                                       smooth=smooth, present_only=present_only)
        owner.last_stats = (stats[0], stats[1], stats[2], loss4)
        ctx.saved = (lg, lb, lse, coef, ignore_index)
        return loss4[0]

    @staticmethod
    def backward(ctx, g):
        lg, lb, lse, coef, ignore_index = ctx.saved
        scale = g.reshape(1).float().contiguous()   # device scalar: the upstream gradient of the scalar loss
        return ops.ce_dice_nchw_bwd(lg, lb, lse, coef, scale, 1.0, ignore_index), None, None, None, None


class DiceCrossEntropyLoss(CrossEntropyLoss):
    """``ce_weight`` * mean cross-entropy + ``dice_weight`` * soft Dice, the region loss beside the per-pixel ones.  With p the
    softmax, V the counted pixels (label != ignore_index, 0 <= label < C) of the whole batch, I_c = sum_{i in V, y_i = c} p_ic,
    P_c = sum_{i in V} p_ic, T_c = #{i in V: y_i = c}:  Dice = (1/C) sum_c m_c (1 - (2 I_c + smooth) / (P_c + T_c + smooth)) with
    m_c = [T_c > 0] for ``present_only=True`` (segmentation_models_pytorch's multiclass DiceLoss) and 1 otherwise (MONAI's
    DiceLoss(softmax=True, batch=True)); the divisor is always C.  The statistics are summed on the device in a fixed order: the
    loss and its gradient are the same bytes every run, and nothing syncs.  The loss is deterministic: ``eval()`` changes nothing.
    ``last_stats``: the device tensors (I, P, T, loss block = [loss, CE mean, Dice, n_valid]) of the last call.
    Class weights, label smoothing and reductions other than 'mean' are not part of this criterion (ValueError).
    Under data parallelism each rank takes the statistics of its own batch."""

    def __init__(self, ce_weight: float = 1.0, dice_weight: float = 1.0, smooth: float = 1.0, present_only: bool = True,
                 ignore_index: int = -100, *, weight=None, reduction: str = "mean", label_smoothing: float = 0.0) -> None:
        if weight is not None or label_smoothing != 0.0 or reduction != "mean":
            raise ValueError("DiceCrossEntropyLoss: class weights, label smoothing and reductions other than 'mean' are not "
                             "supported together with the Dice term")
        super().__init__(ignore_index=ignore_index)
        self.ce_weight, self.dice_weight, self.smooth, self.present_only = check_dice(ce_weight, dice_weight, smooth, present_only)
        self.last_stats = None

    @property
    def dice(self) -> tuple[float, float, float, bool]:
        return self.ce_weight, self.dice_weight, self.smooth, self.present_only

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self._check_nchw(input, target, "DiceCrossEntropyLoss")
        return _DiceFn.apply(input, target, self.ignore_index, check_dice(*self.dice), self)


def check_focal(gamma, poly_eps) -> tuple[float, float]:
    """(gamma, poly_eps) of a focal / poly-1 loss, validated: gamma a finite number >= 0, poly_eps a finite number >= -1."""
    return ops.focal_options(gamma, poly_eps)


class FocalLoss(CrossEntropyLoss):
    """Focal loss (Lin et al. 2017) with an optional poly-1 term (Leng et al. 2022) on softmax logits.  Per counted pixel (label !=
    ignore_index, 0 <= label < C) with label y, p the softmax probability of y and q = 1 - p:
    l = weight[y] * (q^gamma * (-log p) + poly_eps * q).  ``weight`` is the per-class alpha; gamma = 0 and poly_eps = 0 is this
    module's CrossEntropyLoss.  'mean' divides the sum by the sum of weight[y] over the counted pixels — this project's
    cross-entropy rule, exact under ``ignore_index``; kornia and MONAI divide by the number of pixels, which is the same value when
    no pixel is ignored and ``weight`` is None.  q comes from the other classes' exponentials, so a saturated pixel (p = 1 or p = 0 in
    fp32) gives a finite loss and gradient for every gamma >= 0.  ``label_smoothing`` has no agreed definition here (ValueError).
    ``TrainStep(criterion=FocalLoss(...))`` trains through the fused head (``forward_loss(focal=...)``)."""

    def __init__(self, gamma: float = 2.0, poly_eps: float = 0.0, weight=None, ignore_index: int = -100, reduction: str = "mean",
                 label_smoothing: float = 0.0) -> None:
        if label_smoothing != 0.0:
            raise ValueError("FocalLoss: label_smoothing has no agreed definition for a focal / poly-1 loss")
        super().__init__(weight=weight, ignore_index=ignore_index, reduction=reduction)
        self.gamma, self.poly_eps = check_focal(gamma, poly_eps)

    @property
    def focal(self) -> tuple[float, float]:
        return self.gamma, self.poly_eps

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self._check_nchw(input, target, "FocalLoss")
        if self.label_smoothing != 0.0:
            raise ValueError("FocalLoss: label_smoothing has no agreed definition for a focal / poly-1 loss")
        gamma, poly_eps = check_focal(*self.focal)
        return _PixelLossFn.apply(input, target, self.ignore_index, self.reduction, ops.focal_nchw_fwd, ops.focal_nchw_bwd, True,
                                  dict(class_weight=self.weight, gamma=gamma, poly_eps=poly_eps))


class Poly1CrossEntropyLoss(FocalLoss):
    """Poly-1 cross-entropy (PolyLoss, Leng et al. 2022): l = weight[y] * (-log p + epsilon * (1 - p)), i.e.
    ``FocalLoss(gamma=0, poly_eps=epsilon)`` with its reductions and its 'mean' denominator."""

    def __init__(self, epsilon: float = 1.0, weight=None, ignore_index: int = -100, reduction: str = "mean",
                 label_smoothing: float = 0.0) -> None:
        super().__init__(gamma=0.0, poly_eps=epsilon, weight=weight, ignore_index=ignore_index, reduction=reduction,
                         label_smoothing=label_smoothing)

    @property
    def epsilon(self) -> float:
        return self.poly_eps


def check_sigmoid(gamma, alpha, normalize="elements"):
    """(gamma, alpha, normalize) of a sigmoid focal / sigmoid cross-entropy loss, validated: gamma a finite number >= 0, alpha None
    or a number in [0, 1], normalize 'elements' or 'pixels'."""
    return ops.sigmoid_options(gamma, alpha, normalize)


class SigmoidFocalLoss(CrossEntropyLoss):
    """Sigmoid focal loss (Lin et al. 2017, RetinaNet): ``torchvision.ops.sigmoid_focal_loss`` / mmseg's ``FocalLoss`` on one-hot
    targets.  Per counted pixel (label != ignore_index, 0 <= label < C) and class c, with t = [c == label], p = sigmoid(z_c) and
    p_t = t ? p : 1 - p:  l_c = weight[c] * a_t * (1 - p_t)^gamma * (-log p_t), a_t = alpha for the label's class and 1 - alpha for
    the others (1 when ``alpha`` is None).  No softmax: the classes of a pixel do not compete.  ``weight`` scales class c's binary
    term (mmseg's ``class_weight``).  'none' is the [B,H,W] map of the sums over the classes; 'sum' adds them up; 'mean' divides by
    a COUNT of elements, torch's and mmseg's rule for binary losses — counted pixels x C with ``normalize='elements'`` (torch's
    elementwise mean), counted pixels with ``normalize='pixels'`` — never by a weight sum: this deliberately differs from the
    softmax ``CrossEntropyLoss`` / ``FocalLoss`` of this package, whose 'mean' divides by the summed class weights.  log p and
    log(1 - p) are formed as -softplus(-z) and -softplus(z), so saturated scores give finite losses and gradients for every
    gamma >= 0.  ``label_smoothing`` must be 0 (ValueError).  ``TrainStep(criterion=SigmoidFocalLoss(...))`` trains through the fused
    head (``forward_loss(sigmoid=...)``)."""

    def __init__(self, gamma: float = 2.0, alpha=0.25, weight=None, ignore_index: int = -100, reduction: str = "mean",
                 normalize: str = "elements", label_smoothing: float = 0.0) -> None:
        if label_smoothing != 0.0:
            raise ValueError("SigmoidFocalLoss: label_smoothing is not defined for the sigmoid losses")
        super().__init__(weight=weight, ignore_index=ignore_index, reduction=reduction)
        self.gamma, self.alpha, self.normalize = check_sigmoid(gamma, alpha, normalize)

    @property
    def sigmoid(self):
        return self.gamma, self.alpha, self.normalize

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self._check_nchw(input, target, "SigmoidFocalLoss")
        if self.label_smoothing != 0.0:
            raise ValueError("SigmoidFocalLoss: label_smoothing is not defined for the sigmoid losses")
        gamma, alpha, normalize = check_sigmoid(*self.sigmoid)
        return _PixelLossFn.apply(input, target, self.ignore_index, self.reduction, ops.sigmoid_focal_nchw_fwd,
                                  ops.sigmoid_focal_nchw_bwd, False,
                                  dict(class_weight=self.weight, gamma=gamma, alpha=alpha,
                                       class_scale=ops.sigmoid_class_scale(normalize, self.reduction, input.shape[1])))


class SigmoidCrossEntropyLoss(SigmoidFocalLoss):
    """Binary cross-entropy with logits on one-hot targets (``torch.nn.BCEWithLogitsLoss``, mmseg's
    ``CrossEntropyLoss(use_sigmoid=True)``): ``SigmoidFocalLoss(gamma=0, alpha=None)`` with its reductions and its 'mean'
    denominator (a count of elements, not a weight sum)."""

    def __init__(self, weight=None, ignore_index: int = -100, reduction: str = "mean", normalize: str = "elements",
                 label_smoothing: float = 0.0) -> None:
        super().__init__(gamma=0.0, alpha=None, weight=weight, ignore_index=ignore_index, reduction=reduction, normalize=normalize,
                         label_smoothing=label_smoothing)


class _AuxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, target, ignore_index, S, weight, label_smoothing, reduction):
        B, K, h, w = inp.shape
        ld = (K + 63) // 64 * 64
        lo = torch.zeros(B * h * w, ld, dtype=torch.float32, device=inp.device)
        lo[:, :K] = inp.float().permute(0, 2, 3, 1).reshape(B * h * w, K)
        n = float(B * h * S * w * S)
        loss2, dlo, _ = ops.head_upsample_ce(lo, target.contiguous(), B, h, w, K, S, ops.INTERP_BILINEAR,
                                             want_grad=True, ignore_index=ignore_index, grad_scale=1.0 / n,
                                             class_weight=weight, label_smoothing=label_smoothing)
        ctx.saved = (dlo, loss2, n, (B, K, h, w), reduction)
        return loss2[0] / loss2[1] if reduction == "mean" else loss2[0]

    @staticmethod
    def backward(ctx, g):
        dlo, loss2, n, (B, K, h, w), reduction = ctx.saved
        d = dlo[:, :K].reshape(B, h, w, K).permute(0, 3, 1, 2) * (g * n / loss2[1] if reduction == "mean" else g * n)
        return d.contiguous(), None, None, None, None, None, None


class AuxiliaryLoss(CrossEntropyLoss):
    """Drop-in for model/loss.py:12-21: bilinear-resize the low-resolution score map to the label size, then
    cross-entropy — one fused HIP pass (the resized map is never materialised).  Class weights, label smoothing and the
    'mean' / 'sum' reductions; 'none' would materialise the per-pixel map the fusion exists to avoid."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0.0) -> None:
        super().__init__(weight, size_average, ignore_index, reduce, reduction, label_smoothing)
        if self.reduction == "none":
            raise NotImplementedError("lc2is_amd AuxiliaryLoss: reduction='none' is not implemented on the fused "
                                      "resize + cross-entropy path (use 'mean' or 'sum')")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        require_cuda(input, "input")
        B, H, W = target.shape
        h = input.shape[-1]
        if input.shape[-2] != h or H != W or H % h or (H // h) not in (4, 8, 16) or input.shape[1] > 192:
            raise NotImplementedError("lc2is_amd AuxiliaryLoss: square maps, integer scale 4/8/16, <= 192 classes")
        return _AuxFn.apply(input, target, self.ignore_index, H // h, self.weight, self.label_smoothing, self.reduction)


class _ContrastiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, labels, H):
        B, HW, K = outputs.shape
        W = HW // H
        x = outputs.reshape(B * HW, K).float().contiguous()
        lab = labels.reshape(B * HW).contiguous()
        sums = torch.zeros(2, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        ops.rows_ce(x, lab, loss_sum=sums[0:1], dx=dx, grad_scale=0.5 / (B * HW))
        ops.cols_ce(x, lab, B, H, W, K, sums[1:2], dx=dx, grad_scale=0.5 / (B * W * K))
        loss_visual = sums[0] / (B * HW)
        loss_textual = sums[1] / (B * W * K)
        ctx.dx, ctx.shape = dx, outputs.shape
        ctx.mark_non_differentiable(loss_visual, loss_textual)
        return (loss_textual + loss_visual) / 2, loss_visual, loss_textual

    @staticmethod
    def backward(ctx, g, _gv, _gt):
        return (ctx.dx * g).view(ctx.shape), None, None


class ContrastiveLoss(nn.Module):
    """Drop-in for model/loss.py:39-64.  outputs [B,HW,K], labels [B,H,W] -> (mean, loss_visual, loss_textual);
    the textual term reproduces nn.CrossEntropyLoss on a [B,H,W,K] input with one-hot float targets (class axis =
    dim 1, i.e. a softmax over image rows), exactly what the reference computes."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0) -> None:
        super().__init__()
        if weight is not None or reduction != "mean" or label_smoothing != 0:
            raise NotImplementedError("lc2is_amd ContrastiveLoss: default CrossEntropyLoss configuration only")

    def forward(self, outputs: torch.Tensor, labels: torch.Tensor):
        require_cuda(outputs, "outputs")
        HW = outputs.shape[1]
        H = math.isqrt(HW)
        if H * H != HW:
            raise ValueError(f"ContrastiveLoss: {HW} pixels do not form a square map (the reference's rearrange raises)")
        if outputs.shape[2] != 151:
            raise ValueError("ContrastiveLoss: the reference hard-codes num_classes=151 (model/loss.py:55)")
        # F.one_hot(labels, 151) in the reference raises for any label outside [0, 151); one host sync, as there
        if labels.dtype != torch.int64 or ((labels < 0) | (labels >= 151)).any().item():
            raise RuntimeError("ContrastiveLoss: labels must be int64 class indices in [0, 151)")
        return _ContrastiveFn.apply(outputs, labels, H)


class _NPairFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_pos, x_neg):
        xs = [t.float().contiguous() for t in (x, x_pos, x_neg)]
        ctx.save_for_backward(*xs)
        return ops.npair(*xs)

    @staticmethod
    def backward(ctx, dres):
        x, xp, xn = ctx.saved_tensors
        return ops.npair_bwd(x, xp, xn, dres.float().contiguous())


class NPairLoss(nn.Module):
    """Drop-in for model/loss.py:23-37 (forward and backward on the HIP path; unused by every composition)."""

    def __init__(self, reduction=torch.mean) -> None:
        super().__init__()
        self.reduction = reduction

    def forward(self, x: torch.Tensor, x_pos: torch.Tensor, x_neg: torch.Tensor):
        require_cuda(x, "x")
        res = _NPairFn.apply(x, x_pos, x_neg)
        return self.reduction(res) if self.reduction else res
