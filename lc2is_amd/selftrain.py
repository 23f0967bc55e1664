"""Self-training (mean teacher / pseudo-labelling) on the fused head: confident pseudo-labels and their per-pixel loss weights,
held on the device.

The teacher is the EMA of ``TrainStep(ema_decay=...)``, the weak view is ``TrainAugment``'s and the strong view ``StrongAugment``'s
(``lc2is_amd.data``); this module adds the two pieces between them: ``PseudoLabeler`` turns the teacher's prediction on the weak view into labels (the class where the max softmax probability
passes a threshold, ``ignore_index`` elsewhere: FixMatch, ST++, DAFormer) and a per-pixel weight, and ``combine`` forms the
``(inputs, labels, pixel_weight)`` of one ``TrainStep.step`` from a labelled and a pseudo-labelled batch.  The [B, K, H, W] logits
are never formed (``model.predict_confidence`` -> ``ops.head_upsample_conf``) and nothing reads the device: the labeler captures
into a graph.

Recipe (one iteration)::

    step = TrainStep(model, ema_decay=0.999, ...)
    labeler = PseudoLabeler(model, threshold=0.968, weight="quality")
    strong = StrongAugment(seed=1234)                          # colour jitter, greyscale, Gaussian blur: two launches
    batch_u = TrainAugment(photometric=False, seed=1234)(pool_u, keys, epoch)             # geometry only
    weak = {**prompts, "pixel_values": batch_u["pixel_values"]}
    with step.ema_weights():                                   # the teacher's weights
        labels_u, pw_u, _ = labeler(weak)
    strong_view = strong.view(weak, keys, epoch)               # the same geometry, another and stronger colour
    step.step(*labeler.combine(labelled=(inputs, labels), pseudo=(strong_view, labels_u, pw_u)))

The soft-teacher iteration beside it (soft mean teacher, the soft variants of FixMatch / UniMatch): the teacher hands over its
low-resolution scores instead of hard labels and the step adds the per-pixel KL to them (``forward_loss(distill=...)`` ->
``ops.head_upsample_kd``; no [B, K, H, W] map of either model)::

    step = TrainStep(model, ema_decay=0.999, distill=(1.0, 1.0, "all"), ...)   # (weight, temperature, region)
    with step.ema_weights():
        scores_t = model.head_scores(weak_view)                # fp32 [B*g*g, class_pad(K)], no grad
    step.step_distill(strong_view, labels, scores_t)          # CE(labels) + weight * mean T^2 KL(teacher || student)

(``labels`` all ``ignore_index`` for an unlabelled batch: the cross-entropy's mean is then NaN by torch's rule, so mix labelled
images in, as ``combine`` does for the hard recipe; ``teacher_weight=`` takes a per-pixel weight on the KL, e.g. the teacher's
confidence from ``predict_confidence``.)

The mixed-sample step of DACS / DAFormer (ClassMix) and of CPS / UniMatch (CutMix) goes between the two: the labelled batch is the
source, ``(strong_view, labels_u, pw_u)`` the destination, and the mixed batch is the step's (``lc2is_amd.data.SampleMix``, two
launches, no host read; ``mixed`` is the helper)::

    mix = SampleMix("classmix", n_classes=151, exclude_label=0, seed=1234)
    px, labels_m, pw_m, _ = mix((strong_view["pixel_values"], labels_u, pw_u), (inputs["pixel_values"], labels, None), keys, epoch)
    step.step({**strong_view, "pixel_values": px}, labels_m, pw_m)          # = step.step(*labeler.mixed(...))

``strong.view`` goes before the mix, as above (CPS, UniMatch), or after it on the mixed batch, as DACS and DAFormer do: mix
``(weak, labels_u, pw_u)`` first and call ``strong.view(mixed_inputs, keys, epoch)`` on the result - it takes any normalised fp32
``pixel_values``.

The geometric step (RandAugment-style rotate / scale / shear / translate of FixMatch, PseudoSeg, AEL) comes after the teacher has
labelled the weak view: the student's pixels, the pseudo-labels and their weights are warped under ONE per-sample affine map
(``lc2is_amd.data.GeometricAugment``, two launches, no host read); what the warp brings in from outside the frame is the mean
colour, ``ignore_index`` and weight 0, so it costs no loss::

    geo = GeometricAugment(rotate_deg=20.0, scale_range=(0.8, 1.25), seed=1234)
    strong_view, labels_u, pw_u = geo.view(strong_view, labels_u, pw_u, keys, epoch)      # then combine / mix / step as above

The soft teacher under the same step: the teacher sees the weak view, the student the warped one, and the teacher's low-resolution
scores follow the student (``geo.view_distill``: params, apply and ``ops.geo_scores``, three launches, no host read; the scores are
sampled bilinearly with border padding, every column alike).  The fifth result is the in-frame mask at the labels' size (or the
warped ``teacher_weight`` when one is given): passed on as ``teacher_weight=`` it takes the cells the warp brought in from outside
the frame out of the KL, as ``ignore_index`` takes them out of the cross-entropy::

    with step.ema_weights():
        scores_t = model.head_scores(weak_view)                # of the UNWARPED view
    view, labels_g, _, scores_g, mask = geo.view_distill(strong_view, labels, scores_t, keys, epoch)
    step.step_distill(view, labels_g, scores_g, teacher_weight=mask)

(``geo.warp_scores(scores_t, label_size=L)`` alone warps under the table of the last ``geo.view``.)

Out of scope here: the inverse map of a score field (for a teacher that sees the warped image: its shift can pass the table's limit), pooling the confident-pixel counts across ranks, and models
without ``predict_confidence`` (``AuxiliaryLoss``, ``DenseClip``, ``ContrastiveModel``, more than 192 classes).
"""
from __future__ import annotations

import torch

from . import ops

_WEIGHTS = ("quality", "confidence", None)


class PseudoLabeler:
    """``labeler(inputs) -> (labels int64 [B, H, W], pixel_weight fp32 [B, H, W] or None, counts int32 [B, 2])`` from
    ``model.predict_confidence(inputs, threshold, ignore_index)``: the class where conf >= threshold, ``ignore_index`` elsewhere;
    ``counts[b]`` = {confident pixels, pixels} of image b.

    ``weight``: "quality" — every pixel of image b weighs ``counts[b, 0] / counts[b, 1]``, the share of its confident pixels
    (DAFormer); "confidence" — each kept pixel weighs its confidence, the others 0; None — no weight.  The weights multiply the
    pixel losses and not the pixel counts (``forward_loss(pixel_weight=)``): an image with few confident pixels pulls less.
    Runs under ``no_grad`` with the weights the model holds when called (inside ``TrainStep.ema_weights()``: the teacher's);
    torch ops on device tensors after the head's launch pair, no host read."""

    def __init__(self, model, threshold: float = 0.968, weight="quality", ignore_index: int = -100) -> None:
        if not callable(getattr(model, "predict_confidence", None)):
            raise TypeError("PseudoLabeler: the model has no predict_confidence (BaseModelWithText has; AuxiliaryLoss, DenseClip and "
                            "ContrastiveModel are not supported)")
        if weight not in _WEIGHTS:
            raise ValueError(f"PseudoLabeler: weight must be 'quality', 'confidence' or None, got {weight!r}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
            raise TypeError(f"PseudoLabeler: ignore_index must be an int, got {ignore_index!r}")
        self.model, self.threshold, self.weight, self.ignore_index = model, ops.conf_thresh(threshold), weight, ignore_index

    @torch.no_grad()
    def __call__(self, inputs):
        _, conf, labels, counts = self.model.predict_confidence(inputs, self.threshold, self.ignore_index)
        if self.weight is None:
            return labels, None, counts
        if self.weight == "quality":
            share = counts[:, 0].to(torch.float32) / counts[:, 1].to(torch.float32)
            return labels, share.view(-1, 1, 1).expand_as(conf).contiguous(), counts
        return labels, torch.where(conf >= self.threshold, conf, torch.zeros_like(conf)), counts

    @staticmethod
    def combine(labelled, pseudo):
        """``labelled = (inputs, labels)`` and ``pseudo = (inputs_u, labels_u, pixel_weight_u or None)`` -> the ``(inputs, labels,
        pixel_weight)`` of one ``TrainStep.step``: the two batches concatenated along the batch axis, weight 1 on the labelled
        images (and on the pseudo-labelled ones when they carry none).  ``inputs`` are dicts of tensors with the same keys; a tensor
        that both hold as the same object (shared prompts) is kept once."""
        (inputs, labels), (inputs_u, labels_u, pw_u) = labelled, pseudo
        if set(inputs) != set(inputs_u):
            raise ValueError(f"PseudoLabeler.combine: the two batches hold different inputs: {sorted(inputs)} and {sorted(inputs_u)}")
        if labels.shape[1:] != labels_u.shape[1:]:
            raise ValueError(f"PseudoLabeler.combine: label maps of {tuple(labels.shape[1:])} and {tuple(labels_u.shape[1:])}")
        both = {k: v if v is inputs_u[k] else torch.cat([v, inputs_u[k]], dim=0) for k, v in inputs.items()}
        ones = torch.ones(labels.shape, dtype=torch.float32, device=labels.device)
        pw_u = torch.ones(labels_u.shape, dtype=torch.float32, device=labels.device) if pw_u is None else pw_u
        return both, torch.cat([labels, labels_u], dim=0), torch.cat([ones, pw_u], dim=0)

    @staticmethod
    def mixed(labelled, pseudo, mix, keys, epoch, src_index=None):
        """``labelled = (inputs, labels)`` as the source and ``pseudo = (inputs_u, labels_u, pixel_weight_u or None)`` as the
        destination of ``mix`` (a ``lc2is_amd.data.SampleMix``) -> the ``(inputs, labels, pixel_weight)`` of one ``TrainStep.step``:
        ``inputs_u`` with the mixed ``pixel_values``, the mixed labels and weights (weight 1 on what comes from the labelled
        images).  ``keys`` / ``epoch`` / ``src_index`` as ``SampleMix`` takes them; ``mix.last_info`` holds the call's statistics."""
        (inputs, labels), (inputs_u, labels_u, pw_u) = labelled, pseudo
        px, labels_m, pw_m, _ = mix((inputs_u["pixel_values"], labels_u, pw_u), (inputs["pixel_values"], labels, None), keys, epoch,
                                    src_index=src_index)
        return {**inputs_u, "pixel_values": px}, labels_m, pw_m
