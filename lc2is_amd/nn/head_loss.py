"""The criterion of the fused head as one value: validated in one place (``head_criterion``) and dispatched in one place
(``fused_head_loss``) for every site that owns low-resolution class scores — ``BaseModelWithText.forward_loss`` (bicubic x4),
``ScoreMapTail.loss`` (bilinear) and, through the tail, ``PromptFTN.forward_loss``.  A new criterion or option is added here and
to the keyword lists of those three methods; nothing else threads it through.  ``pixel_weight=`` (self-training, boundary maps) is such an option: the last field of the criterion.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import ops
from .loss import check_dice, check_focal, check_ohem, check_sigmoid


class HeadCriterion(NamedTuple):
    """What the fused head computes; the default is the plain mean cross-entropy.  ``ohem`` = (thresh, min_kept per image),
    ``dice`` = (ce_weight, dice_weight, smooth, present_only), ``focal`` = (gamma, poly_eps), ``sigmoid`` = (gamma, alpha, normalize):
    validated tuples or None.  ``pixel_weight``: a contiguous fp32 device tensor of the labels' shape (finite, >= 0, no grad) that
    multiplies each counted pixel's cross-entropy — not its count: the mean still divides by the sum of w_y — or None."""
    weight: torch.Tensor | None = None
    label_smoothing: float = 0.0
    reduction: str = "mean"
    ohem: tuple | None = None
    dice: tuple | None = None
    focal: tuple | None = None
    sigmoid: tuple | None = None
    pixel_weight: torch.Tensor | None = None

    @property
    def plain_ce(self) -> bool:
        """No class weights, no smoothing, 'mean': the cross-entropy entry without options (ohem= only relabels in front of it)."""
        return (self.weight is None and self.label_smoothing == 0.0 and self.reduction == "mean" and self.dice is None
                and self.focal is None and self.sigmoid is None and self.pixel_weight is None)


def fused_loss_options(weight, label_smoothing: float, reduction: str):
    """(weight, label_smoothing, reduction) for a fused CE head, or None for the default configuration."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{reduction} is not a valid value for reduction")
    if reduction == "none":
        raise NotImplementedError("lc2is_amd: the fused cross-entropy heads reduce to a scalar ('mean' or 'sum'); "
                                  "reduction='none' needs the materialised logits (forward + CrossEntropyLoss)")
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
    if weight is None and label_smoothing == 0.0 and reduction == "mean":
        return None
    return weight, float(label_smoothing), reduction


def fused_dice_options(dice, opts, ohem):
    """``dice`` = (ce_weight, dice_weight, smooth, present_only) validated, or None; the Dice term does not combine with class
    weights, label smoothing, a non-mean reduction (``opts`` of fused_loss_options) or a hard-pixel selection."""
    if dice is None:
        return None
    if opts is not None or ohem is not None:
        raise ValueError("lc2is_amd: dice= cannot be combined with weight=, label_smoothing, a reduction other than 'mean' "
                         "or ohem=")
    return check_dice(*dice)


def fused_focal_options(focal, label_smoothing: float, dice):
    """``focal`` = (gamma, poly_eps) validated, or None; the focal / poly-1 loss keeps weight=, reduction=, ohem=, seg_counts= and
    accum=, and does not combine with a Dice term or label smoothing."""
    if focal is None:
        return None
    if dice is not None or label_smoothing != 0.0:
        raise ValueError("lc2is_amd: focal= cannot be combined with dice= or label_smoothing")
    return check_focal(*focal)


def fused_sigmoid_options(sigmoid, label_smoothing: float, dice, focal):
    """``sigmoid`` = (gamma, alpha, normalize) validated, or None; the sigmoid focal / sigmoid cross-entropy loss keeps weight=,
    reduction=, ohem=, seg_counts= and accum=, and does not combine with a Dice term, the softmax focal loss or label smoothing."""
    if sigmoid is None:
        return None
    if dice is not None or focal is not None or label_smoothing != 0.0:
        raise ValueError("lc2is_amd: sigmoid= cannot be combined with dice=, focal= or label_smoothing")
    return check_sigmoid(*sigmoid)


def fused_pixel_weight(who: str, pixel_weight, ohem, dice, focal, sigmoid, K):
    """``pixel_weight`` validated, or None: the per-pixel weight rides the cross-entropy (weight=, label_smoothing, reduction=,
    seg_counts=, accum=) and is refused with a hard-pixel selection, a Dice term, the focal and the sigmoid losses, and past 192
    classes (the chunked head has no such kernel yet)."""
    if pixel_weight is None:
        return None
    for name, on in (("ohem=", ohem is not None), ("dice=", dice is not None), ("focal=", focal is not None),
                     ("sigmoid=", sigmoid is not None)):
        if on:
            raise ValueError(f"lc2is_amd {who}: pixel_weight= cannot be combined with {name} (it weights the cross-entropy with "
                             "weight=, label_smoothing and reduction= only)")
    ops.check_pixel_weight(who, pixel_weight, None)
    if K is not None and K > ops.HEAD_CMAX:
        raise NotImplementedError(f"lc2is_amd {who}: pixel_weight= is limited to {ops.HEAD_CMAX} classes (its fused kernel keeps every "
                                  f"class of a pixel in registers), got {K}; the chunked head past them takes no pixel weight yet")
    return pixel_weight


def wide_refuse(who: str, K: int, scale: int, label_smoothing: float, ohem, dice, focal, sigmoid) -> None:
    """Past 192 classes the fused head is the chunked cross-entropy (``ops.head_upsample_ce_wide``): plain CE with ``weight=``,
    'mean' / 'sum', ``ignore_index``, ``seg_counts=`` and ``accum=`` at scale 4.  Every other criterion keeps its kernel's 192-class
    limit and is refused here, before anything is allocated or launched."""
    if K <= ops.HEAD_CMAX:
        return
    if K > ops.HEAD_WIDE_CMAX:
        raise NotImplementedError(f"lc2is_amd {who}: at most {ops.HEAD_WIDE_CMAX} classes are supported by the fused head, got {K}")
    for name, on in (("label_smoothing", label_smoothing != 0.0), ("ohem=", ohem is not None), ("dice=", dice is not None),
                     ("focal=", focal is not None), ("sigmoid=", sigmoid is not None)):
        if on:
            raise NotImplementedError(f"lc2is_amd {who}: {name} is limited to {ops.HEAD_CMAX} classes (its fused kernel keeps every "
                                      f"class of a pixel in registers); {K} classes train with the plain cross-entropy "
                                      "(weight=, reduction=, ignore_index, seg_counts=, accum=)")
    if scale != 4:
        raise NotImplementedError(f"lc2is_amd {who}: past {ops.HEAD_CMAX} classes the fused head upsamples by 4 only, got {scale}")


def head_criterion(who: str, *, weight=None, label_smoothing: float = 0.0, reduction: str = "mean", ohem=None, dice=None,
                   focal=None, sigmoid=None, seg_counts=None, accum=None, n_classes=None, scale=None,
                   pixel_weight=None) -> HeadCriterion:
    """The validated criterion of a ``forward_loss`` / ``ScoreMapTail.loss`` call: every refusal of the fused head, in one order,
    before a tower runs or anything is allocated.  ``n_classes``: the head's class count, or a callable that returns it (read only
    after the combination checks), or None where it is not known yet — the wide refusal then waits for the call that knows it."""
    if accum is not None and dice is not None:
        raise ValueError("lc2is_amd: accum= cannot be combined with dice= (the Dice statistics of micro-batches do not add)")
    sigmoid = fused_sigmoid_options(sigmoid, label_smoothing, dice, focal)
    focal = fused_focal_options(focal, label_smoothing, dice)
    opts = fused_loss_options(weight, label_smoothing, reduction)
    if ohem is not None:
        ohem = check_ohem(*ohem)
    dice = fused_dice_options(dice, opts, ohem)
    K = n_classes() if callable(n_classes) else n_classes
    if seg_counts is not None:
        ops.check_seg_counts(seg_counts, K)
    pixel_weight = fused_pixel_weight(who, pixel_weight, ohem, dice, focal, sigmoid, K)
    if K is not None:
        wide_refuse(who, K, scale, label_smoothing, ohem, dice, focal, sigmoid)
    return HeadCriterion(*(opts or (None, 0.0, "mean")), ohem, dice, focal, sigmoid, pixel_weight)


def _reduce(loss2, reduction: str, save: bool):
    """(loss, gradient multiplier or None) from the head's [sum of losses, weighted count]; a zero count (every pixel ignored)
    gives torch's NaN mean and a zero gradient, with no host sync."""
    if reduction == "sum":
        return loss2[0], None
    inv = loss2[1].masked_fill(loss2[1] == 0, 1.0).reciprocal() if save else None
    return loss2[0] / loss2[1], inv


def fused_head_loss(scores, labels, B: int, h: int, w: int, K: int, S: int, mode: int, ignore_index: int, crit: HeadCriterion,
                    save: bool, seg_counts=None, accum=None, plain_n: float = 1.0):
    """The loss of the upsampled low-resolution ``scores`` [B*h*w, class_pad(K)] against ``labels`` [B, S h, S w] under ``crit``.
    Returns (loss, dlo, mul, dice_stats, ohem_sel): ``dlo`` (None without ``save``) is the gradient of the SUM of the pixel losses
    wrt ``scores`` — of the scalar loss for dice= — and ``mul`` what the owner multiplies into it for the gradient of ``loss``
    (the 1/count of a mean; None: nothing, as for 'sum', dice= and under ``accum``, where the update that closes the cycle
    divides).  ``dice_stats`` = (I, P, T, loss block) and ``ohem_sel`` = (the labels the head saw, the device info block) are what
    the owner publishes as ``last_dice`` / ``last_ohem``, or None.
    ``plain_n``: the plain-CE launch writes its gradient scaled by 1 / plain_n and ``mul`` carries the plain_n back (also under
    ``accum``) — the score-map tail's scaling of that one path, kept so that its gradients stay the bytes they were."""
    labels = labels.contiguous()
    geom = (B, h, w, K, S, mode)
    kw = dict(want_grad=save, ignore_index=ignore_index)
    if seg_counts is not None:   # accuracy / IoU counts of the batch: the ORIGINAL labels (before OHEM relabels), the loss's scores
        ops.seg_counts_add(seg_counts, scores, labels, *geom, ignore_index)
    dice_stats = ohem_sel = sum_mul = None
    if crit.pixel_weight is not None:   # cross-entropy with a per-pixel weight: [sum of pw_i l_i, sum of w_y] (the count ignores pw)
        if K > ops.HEAD_CMAX:   # (head_criterion refuses it where it knows K; a caller that did not say is refused here)
            raise NotImplementedError(f"lc2is_amd: pixel_weight= is limited to {ops.HEAD_CMAX} classes, got {K}")
        loss2, dlo = ops.head_upsample_ce_pw(scores, labels, crit.pixel_weight, *geom, grad_scale=1.0, class_weight=crit.weight,
                                             label_smoothing=crit.label_smoothing, **kw)
        loss, mul = _reduce(loss2, crit.reduction, save)
    elif K > ops.HEAD_CMAX:   # the chunked cross-entropy (head_criterion refused every other criterion)
        loss2, dlo = ops.head_upsample_ce_wide(scores, labels, *geom, grad_scale=1.0, class_weight=crit.weight, **kw)
        loss, mul = _reduce(loss2, crit.reduction, save)
    elif crit.dice is not None:   # CE + soft Dice: statistics pass, coefficients, gradient pass — dlo is the gradient of the scalar loss
        ce_weight, dice_weight, smooth, present_only = crit.dice
        loss4, stats, dlo = ops.head_upsample_ce_dice(scores, labels, *geom, ce_weight=ce_weight, dice_weight=dice_weight,
                                                      smooth=smooth, present_only=present_only, **kw)
        return loss4[0], dlo, None, (stats[0], stats[1], stats[2], loss4), None
    else:
        if crit.ohem is not None:   # hard-pixel selection: per-pixel loss pass, selection, then the same fused call on the new labels
            labels, info = ohem_sel = ops.ohem_labels(scores, labels, *geom, ignore_index, crit.ohem)
        # every kernel writes the gradient of the SUM of the per-pixel losses and counts the pixels it kept (labels that are
        # negative, == ignore_index or >= K are skipped, head.hip); the 1/count of the mean comes from that device-side count
        # (no host sync, no label pass)
        if crit.plain_ce:
            loss2, dlo, _ = ops.head_upsample_ce(scores, labels, *geom, grad_scale=1.0 / plain_n, **kw)
            loss = loss2[0] / loss2[1]
            mul = plain_n / loss2[1].clamp_min(1.0) if save else None
            sum_mul = plain_n if save and plain_n != 1.0 else None
        else:
            if crit.sigmoid is not None:   # sigmoid focal / sigmoid CE: per-class binary terms, [sum, NUMBER of counted pixels]
                gamma, alpha, normalize = crit.sigmoid
                loss2, dlo = ops.head_upsample_sigmoid(scores, labels, *geom, grad_scale=1.0, class_weight=crit.weight, gamma=gamma,
                                                       alpha=alpha, class_scale=ops.sigmoid_class_scale(normalize, crit.reduction, K),
                                                       **kw)
            elif crit.focal is not None:   # focal / poly-1: the CE gradient times one scalar per pixel, the same [sum, weighted count]
                loss2, dlo = ops.head_upsample_focal(scores, labels, *geom, grad_scale=1.0, class_weight=crit.weight,
                                                     gamma=crit.focal[0], poly_eps=crit.focal[1], **kw)
            else:   # class weights / label smoothing: loss2[1] is the weighted count sum_i w_{y_i}; 'sum' drops the division
                loss2, dlo, _ = ops.head_upsample_ce(scores, labels, *geom, grad_scale=1.0, class_weight=crit.weight,
                                                     label_smoothing=crit.label_smoothing, **kw)
            loss, mul = _reduce(loss2, crit.reduction, save)
    if accum is not None:   # a micro-batch of an accumulation cycle: its sums join the cycle's on the device, and the gradient
        ops.accum_add(accum, loss2)   # stays that of the SUM; the update divides
        mul = sum_mul
    return loss, dlo, mul, None, ohem_sel
