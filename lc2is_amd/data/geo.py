"""Geometric views on the MI355X: a per-sample random affine warp (rotation, isotropic scale, shear, translation, horizontal flip) of
a batch in two launches, the labels and the per-pixel loss weights following the pixels - RandAugment-style rotate / shear / translate
/ scale views for the student in self-training (FixMatch, PseudoSeg, AEL), mmseg's ``RandomRotate`` on a labelled batch, or any
consistency term under a spatial transform.

    weak = TrainAugment(photometric=False, seed=1234)(pool, keys, epoch)      # the view the teacher labels
    labels_u, pw_u, _ = labeler(weak_inputs)                                  # pseudo-labels of the weak view
    geo = GeometricAugment(rotate_deg=20.0, scale_range=(0.8, 1.25), seed=1234)
    inputs_g, labels_g, pw_g = geo.view(strong_view, labels_u, pw_u, keys, epoch)      # ONE map for all three

Pixels are fp32 ``pixel_values`` [B, 3, S, S] (normalised with ``image_mean`` / ``image_std``) and are sampled bilinearly; labels int64
[B, L, L] and weights fp32 [B, L, L] take the nearest cell.  Per sample, with probability ``prob``: a rotation by theta in
[-rotate_deg, rotate_deg] (the content turns counter-clockwise for positive theta), a zoom by s in ``scale_range`` (s > 1 magnifies), a
shear by phi in [-shear_deg, shear_deg] and a shift by up to ``translate`` of the side on each axis; independently, with probability
``flip_prob``, a horizontal flip.  What the warp brings in from outside the frame is ``fill`` (an RGB triple on the 0..255 scale; None:
the mean colour, exactly 0.0 after normalisation) for pixels, ``ignore_index`` for labels and weight 0 for weights.

The map goes from the output to the source and is held as Q16 integers, so indices and bilinear fractions are exact: a sample for
which nothing is drawn is copied bit for bit, a flip, a quarter turn or a whole-pixel shift moves bits, and everywhere else the
result is ``F.grid_sample(x, F.affine_grid(theta, align_corners=False), align_corners=False)`` of the recorded matrix.  Every random
number is a pure function of (seed, epoch, key, draw number) on the counter RNG of ``TrainAugment``, with a stream constant of its
own: a ``GeometricAugment``, a ``StrongAugment``, a ``SampleMix`` and a ``TrainAugment`` with one seed share no draw, a sample's map
does not depend on the batch, and nothing is read back, so the launch pair captures into a graph whose replays draw again from the
device epoch / key tensors.  The exact definition is in include/lc2is_hip.h (lc2is_geo_params / lc2is_geo_apply); tests/geo_ref.py
restates it in numpy.  There is no CPU path.

For the soft teacher (``TrainStep.step_distill``) the teacher's low-resolution scores follow the student under the same table, in
one more launch (lc2is_geo_scores; tests/geo_scores_ref.py): bilinear with border padding, with an in-frame mask at the labels' size
that takes the cells from outside the frame out of the KL::

    view, labels_g, pw_g, scores_g, mask = geo.view_distill(strong_view, labels, scores_t, keys, epoch)
    step.step_distill(view, labels_g, scores_g, teacher_weight=mask)
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ._shared import (_epoch, _int, _keys_for, _mean_std, _number, _pair, _pixel_shape, _require_device, _seed_words, _tensor_type,
                      _threshold)
from .preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD


class GeometricAugment:
    """``geo(batch, keys, epoch, out=None) -> (pixel_values', labels', pixel_weight')``; see the module docstring for the definition.

    ``batch``: ``(pixel_values, labels or None, pixel_weight or None)`` on the device, contiguous: fp32 [B, 3, S, S], int64 [B, L, L],
    fp32 [B, L, L]; S % 4 == 0, S % L == 0, 8 <= S <= 4096.  An entry that is None stays None.  ``keys``: int64 [B], the dataset
    indices of the samples (a list or a device tensor); ``epoch``: an int or a device int32 scalar; ``out``: a triple of tensors to
    write into, none of which may overlap its input.  ``view(inputs, labels, pixel_weight, keys, epoch)`` returns
    ``({**inputs, "pixel_values": warped}, labels', pixel_weight')``.  ``rotate_deg`` (at most 180) and ``shear_deg`` (at most 45) are
    in degrees, ``scale_range`` lies inside [0.25, 4], ``translate`` (at most 0.5) is a share of the side.  ``last_params``: the
    device table int32 [B, 16] of the last call (ops.geo_params), never read back here.  ``warp_scores`` / ``view_distill``: a
    teacher's low-resolution score map under the same table."""

    def __init__(self, prob: float = 1.0, rotate_deg: float = 20.0, scale_range=(0.8, 1.25), shear_deg: float = 0.0,
                 translate: float = 0.0, flip_prob: float = 0.0, fill=None, ignore_index: int = -100,
                 image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD, seed: int = 0):
        warp_thr, flip_thr = _threshold(_number(prob, "prob"), "prob"), _threshold(_number(flip_prob, "flip_prob"), "flip_prob")
        rotate, shear = _number(rotate_deg, "rotate_deg"), _number(shear_deg, "shear_deg")
        shift = _number(translate, "translate")
        scale = _pair(scale_range, "scale_range")
        if not 0.0 <= rotate <= 180.0 or not 0.0 <= shear <= 45.0 or not 0.0 <= shift <= ops.GEO_MAX_TRANSLATE:
            raise ValueError(f"lc2is_amd.data: rotate_deg {rotate_deg} must be 0..180, shear_deg {shear_deg} 0..45 and translate "
                             f"{translate} 0..{ops.GEO_MAX_TRANSLATE}")
        if not ops.GEO_MIN_SCALE <= scale[0] <= scale[1] <= ops.GEO_MAX_SCALE:
            raise ValueError(f"lc2is_amd.data: scale_range must be ordered inside [{ops.GEO_MIN_SCALE}, {ops.GEO_MAX_SCALE}], got {scale}")
        _mean_std(image_mean, image_std)
        if fill is not None:
            if not isinstance(fill, (tuple, list)) or len(fill) != 3:
                raise TypeError(f"lc2is_amd.data: fill must be None or an (r, g, b) triple on the 0..255 scale, got {fill!r}")
            fill = [_number(v, "fill") for v in fill]
            if min(fill) < 0.0 or max(fill) > 255.0:
                raise ValueError(f"lc2is_amd.data: fill must lie in 0..255, got {fill}")
        _int(ignore_index, "ignore_index"), _int(seed, "seed")
        if not -2 ** 63 <= ignore_index < 2 ** 63:
            raise ValueError(f"lc2is_amd.data: ignore_index must fit int64, got {ignore_index}")
        c = self.config = ops.GeoConfig()
        self.seed, c.seed_lo, c.seed_hi = _seed_words(seed)
        c.warp_thr, c.flip_thr = warp_thr, flip_thr
        c.rotate, c.shear, c.translate = math.radians(rotate), math.radians(shear), shift
        c.scale_lo, c.scale_hi = scale
        for i in range(3):
            c.fill[i] = 0.0 if fill is None else (fill[i] / 255.0 - float(image_mean[i])) / float(image_std[i])
        c.ignore_index = ignore_index
        self.ignore_index = ignore_index
        self.last_params = None

    def __call__(self, batch, keys, epoch, out=None):
        if not isinstance(batch, (tuple, list)) or len(batch) != 3:
            raise TypeError("lc2is_amd.data: GeometricAugment batch must be (pixel_values, labels or None, pixel_weight or None)")
        x, lab, pw = batch
        for t, dtype, what in ((x, torch.float32, "pixel_values"), (lab, torch.int64, "labels"), (pw, torch.float32, "pixel_weight")):
            _tensor_type("GeometricAugment", t, dtype, what, optional=what != "pixel_values")
        B, S = _pixel_shape("GeometricAugment", x, ops.GEO_MIN_SIDE, ops.AUG_MAX_SIDE)
        for t, what in ((lab, "labels"), (pw, "pixel_weight")):
            if t is not None and (t.dim() != 3 or t.shape[0] != B or t.shape[1] != t.shape[2] or t.shape[1] < 1 or S % t.shape[1]):
                raise ValueError(f"lc2is_amd.data: GeometricAugment {what} must be [{B}, L, L] with L dividing {S}, got {tuple(t.shape)}")
        if lab is not None and pw is not None and lab.shape != pw.shape:
            raise ValueError(f"lc2is_amd.data: GeometricAugment labels {tuple(lab.shape)} and pixel_weight {tuple(pw.shape)} differ")
        dev = _require_device("GeometricAugment", "tests/geo_ref.py restates it in numpy", x)
        _, _, _, out = ops._geo_batch(batch, out)               # layout, alignment and overlap, before the first launch
        keys = _keys_for("GeometricAugment", keys, dev, B)
        params = ops.geo_params(keys, _epoch(epoch, dev), self.config)
        out = ops.geo_apply(batch, params, self.config, out=out)
        self.last_params = params
        return out

    def view(self, inputs: dict, labels, pixel_weight, keys, epoch, out=None):
        """``inputs`` with its ``pixel_values`` warped, and ``labels`` / ``pixel_weight`` (each may be None) under the same map;
        every other entry of ``inputs`` is passed on as it is."""
        px, labels, pixel_weight = self((inputs["pixel_values"], labels, pixel_weight), keys, epoch, out=out)
        return {**inputs, "pixel_values": px}, labels, pixel_weight

    @staticmethod
    def _scores_grid(scores, B: int, teacher_weight, label_size, who: str) -> int:
        """g of a score tensor fp32 [B*g*g, ld] for B samples, after the type and shape checks that need no device."""
        _tensor_type(who, scores, torch.float32, "teacher scores")
        _tensor_type(who, teacher_weight, torch.float32, "teacher_weight", optional=True)
        if label_size is not None:
            _int(label_size, f"{who} label_size")
        if scores.dim() != 2 or scores.shape[0] < B or scores.shape[0] % B:
            raise ValueError(f"lc2is_amd.data: {who} scores must be [B*g*g, ld] for B = {B} samples, got {tuple(scores.shape)}")
        cells = scores.shape[0] // B
        g = math.isqrt(cells)
        if g * g != cells or g > ops.GEO_SCORES_MAX_G:
            raise ValueError(f"lc2is_amd.data: {who} takes a square grid of at most {ops.GEO_SCORES_MAX_G} cells a side; {scores.shape[0]} "
                             f"rows for {B} samples are {cells} cells each")
        ld = scores.shape[1]
        if ld < 4 or ld > ops.GEO_SCORES_MAX_LD or ld % 4:
            raise ValueError(f"lc2is_amd.data: {who} scores need a pitch that is a multiple of 4 in 4..{ops.GEO_SCORES_MAX_LD}, got {ld}")
        L = label_size
        if teacher_weight is not None:
            if teacher_weight.dim() != 3 or teacher_weight.shape[0] != B or teacher_weight.shape[1] != teacher_weight.shape[2]:
                raise ValueError(f"lc2is_amd.data: {who} teacher_weight must be [{B}, L, L], got {tuple(teacher_weight.shape)}")
            if L is not None and L != teacher_weight.shape[1]:
                raise ValueError(f"lc2is_amd.data: {who} label_size {L} is not the teacher_weight's {teacher_weight.shape[1]}")
            L = int(teacher_weight.shape[1])
        if L is not None and (L < 1 or L > ops.AUG_MAX_SIDE or L % g):
            raise ValueError(f"lc2is_amd.data: {who} needs a label size that is a multiple of g = {g} in 1..{ops.AUG_MAX_SIDE}, got {L}")
        return g

    def warp_scores(self, scores, teacher_weight=None, label_size=None, params=None, out=None):
        """``(scores', teacher_weight' or None)``: a teacher's low-resolution scores fp32 [B*g*g, ld] (``model.head_scores`` of the
        weak view) under the maps of the last call - the geometry the student's view was given - in one launch (``ops.geo_scores``):
        bilinear with border padding, every column alike.  ``teacher_weight`` fp32 [B, L, L] follows as a ``pixel_weight`` does (0
        out of frame); ``label_size=L`` without it asks for the in-frame mask; with neither the second result is None.  ``params``:
        a table of ``ops.geo_params`` to use instead of ``last_params``; B is the table's, and g = isqrt(rows / B) must be exact.
        ``out``: (scores, weight) to write into.  This is the forward direction only: the teacher saw the unwarped view."""
        if params is None:
            params = self.last_params
        if params is None:
            raise RuntimeError("lc2is_amd.data: GeometricAugment.warp_scores needs the table of a view: call the augmenter first, or "
                               "pass params=")
        _tensor_type("GeometricAugment.warp_scores", params, torch.int32, "params")
        if params.dim() != 2 or params.shape[0] < 1 or params.shape[1] != ops.GEO_PARAM_WORDS:
            raise ValueError(f"lc2is_amd.data: GeometricAugment.warp_scores params must be [B, {ops.GEO_PARAM_WORDS}], got {tuple(params.shape)}")
        B = int(params.shape[0])
        g = self._scores_grid(scores, B, teacher_weight, label_size, "GeometricAugment.warp_scores")
        if not scores.is_cuda:
            raise RuntimeError("lc2is_amd.data: GeometricAugment runs on a HIP device; there is no CPU path "
                               "(tests/geo_scores_ref.py restates warp_scores in numpy, test-only)")
        return ops.geo_scores(scores, params, B, g, teacher_weight=teacher_weight, label_size=label_size, out=out)

    def view_distill(self, inputs: dict, labels, teacher_scores, keys, epoch, pixel_weight=None, teacher_weight=None):
        """The soft-teacher step under a geometric view: ``(inputs', labels', pixel_weight', teacher_scores', teacher_weight')`` -
        ``view`` and ``warp_scores`` under ONE table: three launches (params, apply, scores), no host read.  ``teacher_scores``:
        the teacher's ``head_scores`` of the unwarped view, fp32 [B*g*g, ld].  ``teacher_weight'`` is always returned, at the
        labels' size: the warped ``teacher_weight``, or the in-frame mask when none was given - what
        ``TrainStep.step_distill(inputs', labels', teacher_scores', teacher_weight=teacher_weight')`` takes, so that the cells the
        warp brought in from outside the frame cost no KL.  ``labels`` / ``pixel_weight`` may be None (and stay None), but one of
        labels, pixel_weight and teacher_weight must give the label size."""
        who = "GeometricAugment.view_distill"
        px = inputs["pixel_values"]
        sized = [t for t in (labels, pixel_weight, teacher_weight) if torch.is_tensor(t) and t.dim() == 3]
        if not torch.is_tensor(px) or px.dim() != 4 or px.shape[0] < 1:
            raise TypeError(f"lc2is_amd.data: {who} pixel_values must be a [B, 3, S, S] tensor")
        if not sized:
            raise ValueError(f"lc2is_amd.data: {who} needs labels, pixel_weight or teacher_weight [B, L, L] for the size of the mask")
        L = int(sized[0].shape[1])
        if any(t.shape[1] != L for t in sized):
            raise ValueError(f"lc2is_amd.data: {who} labels, pixel_weight and teacher_weight must have one size")
        B = int(px.shape[0])
        g = self._scores_grid(teacher_scores, B, teacher_weight, L, who)
        if not teacher_scores.is_cuda or not px.is_cuda:
            raise RuntimeError("lc2is_amd.data: GeometricAugment runs on a HIP device; there is no CPU path "
                               "(tests/geo_ref.py and tests/geo_scores_ref.py restate it in numpy, test-only)")
        _, _, outs = ops._geo_scores_batch(teacher_scores, B, g, teacher_weight, L, None)   # layout, alignment: before the first launch
        inputs_g, labels_g, pw_g = self.view(inputs, labels, pixel_weight, keys, epoch)
        scores_g, tw_g = self.warp_scores(teacher_scores, teacher_weight, L, out=outs)
        return inputs_g, labels_g, pw_g, scores_g, tw_g
