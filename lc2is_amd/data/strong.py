"""Strong photometric views on the MI355X: colour jitter, random greyscale and Gaussian blur of a normalised batch in two
launches - the student's view in self-training (FixMatch, UniMatch, CPS, DACS, DAFormer all use this one).

    weak = TrainAugment(photometric=False, seed=1234)(pool, keys, epoch)      # the view the teacher labels
    strong = StrongAugment(seed=1234)
    student_inputs = strong.view(weak, keys, epoch)                           # the same geometry, another colour

The input is the fp32 ``pixel_values`` [B, 3, S, S] the step takes (normalised with ``image_mean`` / ``image_std``), so the view can be
made from a ``TrainAugment`` batch or, as in DACS and DAFormer, from the mixed batch after ``SampleMix``.  Per sample:

* colour jitter with probability ``jitter_prob``: brightness (add b on the 0..255 scale), contrast (multiply by c), saturation (blend
  with the 0.299 / 0.587 / 0.114 grey by s) and hue (rotation about the grey axis by h), all four, in this order;
* greyscale with probability ``gray_prob``;
* both folded into ONE 3 x 3 matrix plus offset and followed by ONE clamp to [0, 255].  This is a deliberate difference from recipes
  that clip to [0, 255] between the steps (torchvision's ColorJitter): intermediate values outside the range are carried, not cut, so
  the composition stays linear (and is one multiply-add per channel in the kernel).  Contrast scales about 0, not about the image's
  mean grey (that needs a reduction over the image), and the order of the steps is fixed;
* Gaussian blur with probability ``blur_prob``: sigma uniform in ``sigma_range`` (at most 2.0), radius min(8, ceil(4 sigma)), separable,
  borders reflected without repeating the edge (``F.pad(mode="reflect")``).

A sample for which nothing is drawn is copied bit for bit.  Every random number is a pure function of (seed, epoch, key, draw number)
on the counter RNG of ``TrainAugment``, with a stream constant of its own: a ``StrongAugment``, a ``TrainAugment`` and a ``SampleMix``
with one seed share no draw, a sample's view does not depend on the batch, and nothing is read back, so the launch pair captures
into a graph whose replays draw again from the device epoch / key tensors.  The exact definition is in include/lc2is_hip.h
(lc2is_strong_params / lc2is_strong_apply); tests/strong_ref.py restates it in numpy.  There is no CPU path.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ._shared import (_epoch, _int, _keys_for, _mean_std, _number, _pair, _pixel_shape, _require_device, _seed_words, _tensor_type,
                      _threshold)
from .preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD


class StrongAugment:
    """``strong(pixel_values, keys, epoch, out=None) -> pixel_values'``; see the module docstring for the definition.

    ``pixel_values``: fp32 [B, 3, S, S] on the device, contiguous, S % 4 == 0, 12 <= S <= 4096; ``keys``: int64 [B], the dataset
    indices of the samples (a list or a device tensor); ``epoch``: an int or a device int32 scalar; ``out``: a tensor to write into,
    which may not overlap the input.  ``view(inputs, keys, epoch)`` returns ``{**inputs, "pixel_values": strong view}``.
    ``brightness_delta`` is on the 0..255 scale, ``hue_delta`` in degrees (as ``TrainAugment``'s).  ``last_params``: the device
    table int32 [B, 32] of the last call (ops.strong_params), never read back here."""

    def __init__(self, jitter_prob: float = 0.8, brightness_delta: float = 64.0, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                 hue_delta: float = 90.0, gray_prob: float = 0.2, blur_prob: float = 0.5, sigma_range=(0.1, 2.0),
                 image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD, seed: int = 0):
        probs = [_threshold(_number(p, what), what) for p, what in ((jitter_prob, "jitter_prob"), (gray_prob, "gray_prob"),
                                                                    (blur_prob, "blur_prob"))]
        if _number(brightness_delta, "brightness_delta") < 0 or _number(hue_delta, "hue_delta") < 0:
            raise ValueError(f"lc2is_amd.data: brightness_delta {brightness_delta} and hue_delta {hue_delta} must not be negative")
        contrast, saturation = _pair(contrast_range, "contrast_range"), _pair(saturation_range, "saturation_range")
        if contrast[0] < 0 or saturation[0] < 0:
            raise ValueError(f"lc2is_amd.data: contrast_range {contrast} and saturation_range {saturation} must not be negative")
        sigma = _pair(sigma_range, "sigma_range")
        if not 0.0 < sigma[0] <= sigma[1] <= ops.STRONG_MAX_SIGMA:
            raise ValueError(f"lc2is_amd.data: sigma_range must be ordered inside (0, {ops.STRONG_MAX_SIGMA}] (the blur's radius is at "
                             f"most {ops.STRONG_MAX_RADIUS}), got {sigma}")
        _mean_std(image_mean, image_std)
        c = self.config = ops.StrongConfig()
        self.seed, c.seed_lo, c.seed_hi = _seed_words(_int(seed, "seed"))
        c.jitter_thr, c.gray_thr, c.blur_thr = probs
        c.brightness_delta, c.hue_delta = float(brightness_delta), math.radians(float(hue_delta))
        (c.contrast_lo, c.contrast_hi), (c.saturation_lo, c.saturation_hi), (c.sigma_lo, c.sigma_hi) = contrast, saturation, sigma
        for i in range(3):
            c.mean[i], c.std[i], c.inv_std[i] = float(image_mean[i]), float(image_std[i]), 1.0 / float(image_std[i])
        self.last_params = None

    def __call__(self, pixel_values, keys, epoch, out: torch.Tensor | None = None) -> torch.Tensor:
        x = pixel_values
        _tensor_type("StrongAugment", x, torch.float32, "pixel_values")
        B, _ = _pixel_shape("StrongAugment", x, ops.STRONG_MIN_SIDE, ops.AUG_MAX_SIDE)
        dev = _require_device("StrongAugment", "tests/strong_ref.py restates it in numpy", x)
        _, _, out = ops._strong_batch(x, out)                 # layout, alignment and overlap, before the first launch
        keys = _keys_for("StrongAugment", keys, dev, B)
        params = ops.strong_params(keys, _epoch(epoch, dev), self.config)
        out = ops.strong_apply(x, params, self.config, out=out)
        self.last_params = params
        return out

    def view(self, inputs: dict, keys, epoch, out: torch.Tensor | None = None) -> dict:
        """``inputs`` with its ``pixel_values`` replaced by their strong view; every other entry is passed on as it is."""
        return {**inputs, "pixel_values": self(inputs["pixel_values"], keys, epoch, out=out)}
