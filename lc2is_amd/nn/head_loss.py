"""The criterion of the fused head as one value: validated in one place (``head_criterion``) and dispatched in one place
(``fused_head_loss``) for every site that owns low-resolution class scores — ``BaseModelWithText.forward_loss`` (bicubic x4),
``ScoreMapTail.loss`` (bilinear) and, through the tail, ``PromptFTN.forward_loss``.  A new criterion or option is added here and
to the keyword lists of those three methods; nothing else threads it through.  ``pixel_weight=`` (self-training, boundary maps) is such an option: the last field of the criterion.
``distill=`` (a ``Distill``: per-pixel KL to a teacher's low-resolution scores) is another: a term ADDED to whatever criterion is
chosen, with its own denominator.  It is not one more field — the criterion's eight fields and their order are what callers and
positional constructions rely on — but the ``distill`` attribute of a ``DistilledCriterion``, the same tuple with the term beside it.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import ops
from .loss import check_dice, check_focal, check_ohem, check_sigmoid


class Distill(NamedTuple):
    """The distillation term of a fused-head loss: ``weight`` * mean over the counted pixels of pw_i T^2 KL(softmax(teacher / T) ||
    softmax(student / T)) on the upsampled scores (``ops.head_upsample_kd``).  ``scores``: the teacher's low-resolution scores, fp32
    [B*h*w, class_pad(K)] contiguous, no grad — what ``BaseModelWithText.head_scores`` / ``ScoreMapTail.scores_lo`` return, from the
    same model under ``TrainStep.ema_weights()`` or another one with the same classes and patch grid.  ``region``: 'all' = every
    pixel, 'labelled' = the pixels the call's labels count (before OHEM relabels; crop padding stays out).  ``pixel_weight``: fp32
    of the labels' shape (finite, >= 0, no grad) on the pixel's KL — not on its count — or None."""
    scores: torch.Tensor
    weight: float = 1.0
    temperature: float = 1.0
    region: str = "all"
    pixel_weight: torch.Tensor | None = None


DISTILL_REGIONS = ("all", "labelled")


def check_distill_options(weight, temperature, region) -> tuple[float, float, str]:
    """(weight, temperature, region) of a distillation term, validated: weight finite and >= 0, temperature finite and > 0."""
    if not ops.finite_ge(weight):
        raise ValueError(f"lc2is_amd: the distillation weight must be a finite number >= 0, got {weight!r}")
    temperature = ops.kd_temperature(temperature)
    if region not in DISTILL_REGIONS:
        raise ValueError(f"lc2is_amd: the distillation region must be 'all' or 'labelled', got {region!r}")
    return float(weight), temperature, region


def check_distill(who: str, distill, accum=None, K=None, rows=None, dev=None):
    """``distill`` validated into a ``Distill``, or None.  ``rows`` / ``dev``: the student's B*h*w and device where the caller knows
    them before its towers run (with K: the teacher's scores must be [rows, class_pad(K)] on ``dev``)."""
    if distill is None:
        return None
    if accum is not None:
        raise NotImplementedError(f"lc2is_amd {who}: distill= cannot be combined with accum= (the term has its own denominator, the "
                                  "number of pixels it counts, and the accumulation block carries one)")
    try:
        distill = Distill(*distill)
    except TypeError:
        raise ValueError(f"lc2is_amd {who}: distill= must be a Distill(scores, weight, temperature, region, pixel_weight), got "
                         f"{type(distill).__name__}") from None
    weight, temperature, region = check_distill_options(distill.weight, distill.temperature, distill.region)
    if K is not None and K > ops.HEAD_CMAX:
        raise NotImplementedError(f"lc2is_amd {who}: distill= is limited to {ops.HEAD_CMAX} classes (its fused kernel keeps every "
                                  f"class of a pixel of both maps in registers), got {K}")
    shape = (rows, ops.class_pad(K)) if rows is not None and K is not None else None
    ops.check_teacher_scores(who, distill.scores, shape, dev)
    if distill.pixel_weight is not None:
        ops.check_pixel_weight(who, distill.pixel_weight, None, dev)
    return Distill(distill.scores, weight, temperature, region, distill.pixel_weight)


class HeadCriterion(NamedTuple):
    """What the fused head computes; the default is the plain mean cross-entropy.  ``ohem`` = (thresh, min_kept per image),
    ``dice`` = (ce_weight, dice_weight, smooth, present_only), ``focal`` = (gamma, poly_eps), ``sigmoid`` = (gamma, alpha, normalize):
    validated tuples or None.  ``pixel_weight``: a contiguous fp32 device tensor of the labels' shape (finite, >= 0, no grad) that
    multiplies each counted pixel's cross-entropy — not its count: the mean still divides by the sum of w_y — or None.
    ``distill`` (an attribute, not a field): None here; a ``DistilledCriterion`` carries a validated ``Distill`` — weight * mean KL
    to a teacher's scores, added to the criterion's loss."""
    weight: torch.Tensor | None = None
    label_smoothing: float = 0.0
    reduction: str = "mean"
    ohem: tuple | None = None
    dice: tuple | None = None
    focal: tuple | None = None
    sigmoid: tuple | None = None
    pixel_weight: torch.Tensor | None = None
    distill = None

    @property
    def plain_ce(self) -> bool:
        """No class weights, no smoothing, 'mean': the cross-entropy entry without options (ohem= only relabels in front of it)."""
        return (self.weight is None and self.label_smoothing == 0.0 and self.reduction == "mean" and self.dice is None
                and self.focal is None and self.sigmoid is None and self.pixel_weight is None)


class DistilledCriterion(HeadCriterion):
    """A ``HeadCriterion`` — the same eight fields, the same tuple — with a distillation term beside it: ``distill`` is a validated
    ``Distill``, ``base`` the criterion without the term."""

    def __new__(cls, base: HeadCriterion, distill: Distill):
        self = super().__new__(cls, *base)
        self.distill = distill
        return self

    @property
    def base(self) -> HeadCriterion:
        return HeadCriterion(*self)


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
                   pixel_weight=None, distill=None, rows=None, device=None) -> HeadCriterion:
    """The validated criterion of a ``forward_loss`` / ``ScoreMapTail.loss`` call: every refusal of the fused head, in one order,
    before a tower runs or anything is allocated.  ``n_classes``: the head's class count, or a callable that returns it (read only
    after the combination checks), or None where it is not known yet — the wide refusal then waits for the call that knows it.
    ``rows`` / ``device``: the student's B*h*w and device where the site knows them before its towers run (``distill=``'s shape)."""
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
    distill = check_distill(who, distill, accum, K, rows, device)
    if K is not None:
        wide_refuse(who, K, scale, label_smoothing, ohem, dice, focal, sigmoid)
    crit = HeadCriterion(*(opts or (None, 0.0, "mean")), ohem, dice, focal, sigmoid, pixel_weight)
    return crit if distill is None else DistilledCriterion(crit, distill)


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
    ``accum``) — the score-map tail's scaling of that one path, kept so that its gradients stay the bytes they were.
    ``crit.distill``: loss += weight * loss2_kd[0] / loss2_kd[1] on the call's ORIGINAL labels (region 'labelled') or every pixel,
    and the two gradients are combined here, on the device, each with its own multiplier: ``dlo`` is then the gradient of ``loss``
    and ``mul`` None."""
    labels = labels.contiguous()
    if crit.distill is not None:
        return _with_distill(scores, labels, B, h, w, K, S, mode, ignore_index, crit, save, seg_counts, accum, plain_n)
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


def _with_distill(scores, labels, B, h, w, K, S, mode, ignore_index, crit, save, seg_counts, accum, plain_n):
    """``fused_head_loss`` with the distillation term: the base criterion's call as it is without ``distill``, the KL launch pair on
    the same scores, and the glue — a handful of elementwise device ops on the low-resolution gradient, no host sync.  A zero count
    of the term gives ``_reduce``'s convention: a NaN mean and a zero gradient."""
    d = crit.distill
    if accum is not None:   # (head_criterion refuses it; a caller that built the criterion by hand is refused here)
        raise NotImplementedError("lc2is_amd: distill= cannot be combined with accum=")
    if K > ops.HEAD_CMAX:
        raise NotImplementedError(f"lc2is_amd: distill= is limited to {ops.HEAD_CMAX} classes, got {K}")
    ops.check_teacher_scores("distill=", d.scores, scores.shape, scores.device)
    loss, dlo, mul, dice_stats, ohem_sel = fused_head_loss(scores, labels, B, h, w, K, S, mode, ignore_index,
                                                           crit.base, save, seg_counts, None, plain_n)
    loss2, dkd = ops.head_upsample_kd(scores, d.scores, B, h, w, K, S, mode, temperature=d.temperature,
                                      labels=labels if d.region == "labelled" else None, pixel_weight=d.pixel_weight,
                                      want_grad=save, ignore_index=ignore_index, grad_scale=1.0)
    loss = loss + d.weight * (loss2[0] / loss2[1])
    if save:
        if mul is not None:   # (the plain path's plain_n rides in mul: dlo * mul is the gradient of the base loss in every case)
            dlo = dlo.mul_(mul)
        dlo = dlo.add_(dkd.mul_(loss2[1].masked_fill(loss2[1] == 0, 1.0).reciprocal().mul_(d.weight)))
    return loss, dlo, None, dice_stats, ohem_sel
