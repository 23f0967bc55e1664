"""Mixed-sample augmentation on the MI355X: ClassMix and CutMix of two batches in two launches, the step between the teacher's
pseudo-labels and the student's step in self-training (DACS and DAFormer mix with ClassMix; CPS, UniMatch and French et al. with
CutMix).

    mix = SampleMix("classmix", n_classes=151, exclude_label=0, seed=1234)
    px, labels, pw, info = mix((strong_view, labels_u, pw_u), (pixel_values, labels, None), keys, epoch)
    step.step({**inputs_u, "pixel_values": px}, labels, pw)

Output sample b is destination sample b with the masked region replaced by source sample ``src_index[b]``: pixels, labels and
per-pixel loss weights together, as selects (bit for bit the chosen side; a NaN on the other side does not spread).  The mask
lives on the L x L label cells and covers the (S / L)^2 pixels of each.

* ``classmix``: half (rounded up) of the classes present in the SOURCE label map, a uniformly random subset; every cell of a
  chosen class is pasted.  Labels outside 0 .. n_classes - 1, ``ignore_index`` and ``exclude_label`` are never chosen.
* ``cutmix``: one box whose area share is uniform in ``box_area`` and whose height is uniform among the heights that fit
  (CutMix-Seg draws the aspect ratio log-uniformly instead), at a uniform position.

Every random number is a pure function of (seed, epoch, key, draw number) on the counter RNG of ``TrainAugment``, with a stream
constant of its own: a sample's mask depends on its key, the epoch and its source label map only - not on the batch size, the
position in the batch or the rank - and nothing is read back, so the launch pair captures into a graph whose replays draw again
from the device epoch / key tensors.  The exact definition is in include/lc2is_hip.h (lc2is_mix_select / lc2is_mix_apply);
tests/mix_ref.py restates it in numpy.  There is no CPU path.
"""
from __future__ import annotations

import torch

from .. import ops
from ._shared import _epoch, _int, _keys_for, _require_device, _seed_words, _tensor_type

_MODES = {"none": ops.MIX_NONE, "classmix": ops.MIX_CLASSMIX, "cutmix": ops.MIX_CUTMIX}


class SampleMix:
    """``mix(dst, src, keys, epoch, src_index=None, out=None) -> (pixel_values, labels, pixel_weight, info)``.

    ``dst`` / ``src``: ``(pixel_values fp32 [n, 3, S, S], labels int64 [n, L, L], pixel_weight fp32 [n, L, L] or None)`` on the
    device, S % 4 == 0 and S % L == 0; None weighs every pixel 1 and the returned weights are always a tensor.  The source batch
    may hold another number of samples, and may be the destination batch itself (ClassMix within a batch: ``src_index`` a roll).
    ``keys``: int64 [B], the dataset indices of the destination samples; ``epoch``: an int or a device int32 scalar;
    ``src_index``: int64 [B], the source row pasted into each output sample (None: row b; a row outside the source batch leaves
    that sample as its destination and marks it in ``info``); ``out``: three tensors to write into, none of which may overlap an
    input.  ``info`` (also ``last_info``): the device tensor int32 [B, 4] = (classes present, classes chosen, masked cells, L * L)
    of the call, never read back here."""

    def __init__(self, mode: str = "classmix", n_classes: int = 151, ignore_index: int = -100, exclude_label: int | None = None,
                 box_area=(0.25, 0.5), seed: int = 0):
        if mode not in _MODES:
            raise ValueError(f"lc2is_amd.data: SampleMix mode must be one of {sorted(_MODES)}, got {mode!r}")
        if not 1 <= _int(n_classes, "n_classes") <= ops.MIX_MAX_CLASSES:
            raise ValueError(f"lc2is_amd.data: n_classes must be 1..{ops.MIX_MAX_CLASSES}, got {n_classes}")
        lo, hi = (float(v) for v in box_area)
        if not 0.0 < lo <= hi <= 1.0 or round(lo * 1024) < 1:
            raise ValueError(f"lc2is_amd.data: box_area must be an ordered pair of area shares in (0, 1] (at least 1/1024), got {tuple(box_area)}")
        self.mode, self.n_classes, self.ignore_index = mode, n_classes, _int(ignore_index, "ignore_index")
        self.exclude_label = None if exclude_label is None else _int(exclude_label, "exclude_label")
        self.box_area = (lo, hi)
        c = self.config = ops.MixConfig()
        self.seed, c.seed_lo, c.seed_hi = _seed_words(int(seed))
        c.mode, c.n_classes = _MODES[mode], n_classes
        c.ignore_index, c.exclude_label = self.ignore_index, -1 if self.exclude_label is None else self.exclude_label
        c.area_lo1024, c.area_hi1024 = int(round(lo * 1024)), int(round(hi * 1024))
        self.last_info = None

    @staticmethod
    def _batch(batch, name: str):
        """Dtypes and shapes of one (pixel_values, labels, pixel_weight | None), before any device work; returns (n, S, L)."""
        if not isinstance(batch, (tuple, list)) or len(batch) != 3:
            raise TypeError(f"lc2is_amd.data: SampleMix {name} must be (pixel_values, labels, pixel_weight or None)")
        px, lab, pw = batch
        for t, dtype, what in ((px, torch.float32, "pixel_values"), (lab, torch.int64, "labels"), (pw, torch.float32, "pixel_weight")):
            _tensor_type(f"SampleMix {name}", t, dtype, what, optional=what == "pixel_weight")
        if px.dim() != 4 or px.shape[1] != 3 or px.shape[2] != px.shape[3] or lab.dim() != 3 or lab.shape[1] != lab.shape[2] or \
                lab.shape[0] != px.shape[0] or px.shape[0] < 1 or (pw is not None and pw.shape != lab.shape):
            raise ValueError(f"lc2is_amd.data: SampleMix {name} must be pixel_values [n, 3, S, S], labels [n, L, L] and pixel_weight "
                             f"[n, L, L] or None, got {tuple(px.shape)}, {tuple(lab.shape)}, {None if pw is None else tuple(pw.shape)}")
        n, S, L = int(px.shape[0]), int(px.shape[2]), int(lab.shape[1])
        if S < 4 or S > ops.AUG_MAX_SIDE or S % 4 or L < 1 or S % L:
            raise ValueError(f"lc2is_amd.data: SampleMix needs S a multiple of 4 and of L, at most {ops.AUG_MAX_SIDE}; got S = {S}, L = {L}")
        return n, S, L

    def __call__(self, dst, src, keys, epoch, src_index=None, out=None):
        B, S, L = self._batch(dst, "dst")
        _, S2, L2 = self._batch(src, "src")
        if (S2, L2) != (S, L):
            raise ValueError(f"lc2is_amd.data: SampleMix dst is {S} px / {L} cells a side, src {S2} / {L2}")
        dev = _require_device("SampleMix", "tests/mix_ref.py restates it in numpy", dst[0], src[0])   # (mix_apply checks layout and overlap)
        keys = _keys_for("SampleMix", keys, dev, B, of="destination samples")
        if src_index is not None:
            src_index = _keys_for("SampleMix", src_index, dev, B, "source rows", "destination samples")
        plan, info = ops.mix_select(src[1], keys, _epoch(epoch, dev), self.config, src_index=src_index)
        px, lab, pw = ops.mix_apply(tuple(dst), tuple(src), plan, out=out)
        self.last_info = info
        return px, lab, pw, info
