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
"""
from __future__ import annotations

import math

import torch

from .. import ops
from .augment import TrainAugment, _need_cuda, _threshold
from .preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
from .strong import _number, _pair


class GeometricAugment:
    """``geo(batch, keys, epoch, out=None) -> (pixel_values', labels', pixel_weight')``; see the module docstring for the definition.

    ``batch``: ``(pixel_values, labels or None, pixel_weight or None)`` on the device, contiguous: fp32 [B, 3, S, S], int64 [B, L, L],
    fp32 [B, L, L]; S % 4 == 0, S % L == 0, 8 <= S <= 4096.  An entry that is None stays None.  ``keys``: int64 [B], the dataset
    indices of the samples (a list or a device tensor); ``epoch``: an int or a device int32 scalar; ``out``: a triple of tensors to
    write into, none of which may overlap its input.  ``view(inputs, labels, pixel_weight, keys, epoch)`` returns
    ``({**inputs, "pixel_values": warped}, labels', pixel_weight')``.  ``rotate_deg`` (at most 180) and ``shear_deg`` (at most 45) are
    in degrees, ``scale_range`` lies inside [0.25, 4], ``translate`` (at most 0.5) is a share of the side.  ``last_params``: the
    device table int32 [B, 16] of the last call (ops.geo_params), never read back here."""

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
        if len(image_mean) != 3 or len(image_std) != 3 or min(image_std) <= 0:
            raise ValueError("lc2is_amd.data: image_mean / image_std must hold three values, std positive")
        if fill is not None:
            if not isinstance(fill, (tuple, list)) or len(fill) != 3:
                raise TypeError(f"lc2is_amd.data: fill must be None or an (r, g, b) triple on the 0..255 scale, got {fill!r}")
            fill = [_number(v, "fill") for v in fill]
            if min(fill) < 0.0 or max(fill) > 255.0:
                raise ValueError(f"lc2is_amd.data: fill must lie in 0..255, got {fill}")
        for v, what in ((ignore_index, "ignore_index"), (seed, "seed")):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"lc2is_amd.data: {what} must be an int, got {v!r}")
        if not -2 ** 63 <= ignore_index < 2 ** 63:
            raise ValueError(f"lc2is_amd.data: ignore_index must fit int64, got {ignore_index}")
        self.seed = seed & (2 ** 64 - 1)
        c = self.config = ops.GeoConfig()
        c.seed_lo, c.seed_hi = self.seed & 0xffffffff, self.seed >> 32
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
            if (t is not None or what == "pixel_values") and (not torch.is_tensor(t) or t.dtype != dtype):
                raise TypeError(f"lc2is_amd.data: GeometricAugment {what} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
        if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f"lc2is_amd.data: GeometricAugment pixel_values must be [B, 3, S, S], got {tuple(x.shape)}")
        B, S = int(x.shape[0]), int(x.shape[2])
        if S < ops.GEO_MIN_SIDE or S > ops.AUG_MAX_SIDE or S % 4:
            raise ValueError(f"lc2is_amd.data: GeometricAugment needs S a multiple of 4 in {ops.GEO_MIN_SIDE}..{ops.AUG_MAX_SIDE}, got {S}")
        for t, what in ((lab, "labels"), (pw, "pixel_weight")):
            if t is not None and (t.dim() != 3 or t.shape[0] != B or t.shape[1] != t.shape[2] or t.shape[1] < 1 or S % t.shape[1]):
                raise ValueError(f"lc2is_amd.data: GeometricAugment {what} must be [{B}, L, L] with L dividing {S}, got {tuple(t.shape)}")
        if lab is not None and pw is not None and lab.shape != pw.shape:
            raise ValueError(f"lc2is_amd.data: GeometricAugment labels {tuple(lab.shape)} and pixel_weight {tuple(pw.shape)} differ")
        if not x.is_cuda:
            raise RuntimeError("lc2is_amd.data: GeometricAugment runs on a HIP device; there is no CPU path "
                               "(tests/geo_ref.py restates it in numpy, test-only)")
        dev = _need_cuda(x.device)
        _, _, _, out = ops._geo_batch(batch, out)               # layout, alignment and overlap, before the first launch
        keys = TrainAugment._indices(keys, dev)
        if keys.numel() != B:
            raise ValueError(f"lc2is_amd.data: GeometricAugment got {keys.numel()} keys for {B} samples")
        params = ops.geo_params(keys, TrainAugment._epoch(epoch, dev), self.config)
        out = ops.geo_apply(batch, params, self.config, out=out)
        self.last_params = params
        return out

    def view(self, inputs: dict, labels, pixel_weight, keys, epoch, out=None):
        """``inputs`` with its ``pixel_values`` warped, and ``labels`` / ``pixel_weight`` (each may be None) under the same map;
        every other entry of ``inputs`` is passed on as it is."""
        px, labels, pixel_weight = self((inputs["pixel_values"], labels, pixel_weight), keys, epoch, out=out)
        return {**inputs, "pixel_values": px}, labels, pixel_weight
