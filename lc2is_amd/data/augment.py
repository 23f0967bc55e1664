"""Train-time augmentation on the MI355X: random rescale, random crop, horizontal flip and photometric jitter of a whole batch
in one launch, cut from decoded uint8 images that live in HBM.

The reference reserves the hook (data/dataset.py:144-149: one random ``transform`` applied to the image and to the label under a
shared RNG state) and leaves it to the host.  At the rate of the training step the host cannot keep up, and the decoded ADE20K
training split (about 27 GB of uint8) fits the device many times, so here

* ``DeviceImagePool`` holds the decoded pixels and label maps packed in two uint8 device buffers, with a descriptor per image;
* ``TrainAugment`` draws every sample's parameters on the device (``ops.aug_params``) and cuts the batch straight into the
  ``pixel_values`` [B,3,S,S] / ``label`` [B,L,L] tensors ``TrainStep.step`` takes (``ops.aug_apply``, one launch for images and
  labels together);
* ``AugmentedBatches`` iterates one epoch of such batches in ``ADE20KCollator``'s format.

    pool = DeviceImagePool.from_arrays(images_u8_HWC, labels_u8_HW)
    aug = TrainAugment(crop_size=512, label_size=128, seed=1234)
    for epoch in range(epochs):
        loader.set_epoch(epoch)                              # loader = AugmentedBatches(pool, aug, 32, shuffle_seed=0)
        for inputs, metas in loader:
            loss = step.step(inputs, inputs.pop("label"))

Every random number is a pure function of (seed, epoch, dataset index, draw number): an image gets the same augmentation in an
epoch whatever its batch, its position in the batch, the rank or the batch size, and no host value changes between steps, so the
launches can be captured in a graph whose replays draw fresh parameters from the static index / epoch tensors.

Geometry: the short edge is resized to ``base_size * ratio`` (ratio uniform in ``ratio_range``, bilinear without antialiasing,
``F.interpolate(..., align_corners=False)``), an S x S window is cut at a uniform position; where the resized image is smaller than
the window it sits at the top left and the rest is padding (0.0 = the mean colour after normalisation; ``pad_label`` for labels).
Labels take the same geometry with nearest-exact sampling at the centres of the (S / L)^2 cells.

Class-ratio re-draw (``cat_max_ratio``, mmseg's ``RandomCrop(cat_max_ratio=0.75)``): a crop in which one class covers that share
or more of the labelled cells, or which holds one class only, is rejected and its origin drawn again, up to ``cat_tries`` times; a
third launch (``ops.aug_crop_select``) between the two does it on the device.  It counts the L x L label cells the crop will
produce - the labels the loss sees - and not the full-resolution crop as mmseg does ((S / L)^2 times fewer reads); cells that are
padding or hold ``cat_ignore_label`` do not count.  ``None`` (the default) adds no launch and changes no bit.

Colour: brightness (add b), contrast (multiply by c), saturation (blend with the 0.299 / 0.587 / 0.114 grey by s) and hue
(rotation about the grey axis by h), each applied with its probability, in this order, folded into ONE 3 x 3 matrix plus offset per
image and followed by ONE clamp to [0, 255].  This is a deliberate difference from recipes that clip to [0, 255] between the
steps: intermediate values outside the range are carried, not cut, so the composition stays linear (and is one multiply-add per
channel in the kernel).  ``photometric=False`` gives the identity.

There is no CPU path: a non-CUDA device is an error, as for the evaluation preprocessors.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from ._shared import _epoch, _indices, _mean_std, _need_cuda, _seed_words, _threshold, _upload
from .preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD

ALIGN = 256                      # every image / label map starts on a multiple of this in its buffer
MAX_SIDE = ops.AUG_MAX_SIDE
_TAIL = 8                        # bytes readable after the last pixel of an image (a tap is one unaligned 8-byte read)
PHOTOMETRIC_DEFAULTS = dict(brightness_delta=32.0, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=36.0, prob=0.5)


def _up(n: int, a: int = ALIGN) -> int:
    return -(-n // a) * a


def pack_offsets(shapes, img_start: int = 0, lab_start: int = 0):
    """Byte offsets of images of the given (H, W) packed one after another at ALIGN-byte alignment: HWC pixels (3 * H * W bytes)
    in one buffer, HW labels in another.  Returns (img_offsets, lab_offsets, img_end, lab_end); the ends are aligned too (the
    next image starts there)."""
    img_offs, lab_offs = [], []
    io, lo = _up(img_start), _up(lab_start)
    for h, w in shapes:
        img_offs.append(io)
        lab_offs.append(lo)
        io, lo = _up(io + 3 * h * w), _up(lo + h * w)
    return img_offs, lab_offs, io, lo


def _as_u8(a, what: str) -> torch.Tensor:
    if isinstance(a, np.ndarray):
        if a.dtype != np.uint8:
            raise TypeError(f"lc2is_amd.data: {what} must be uint8 (decoded pixels or class ids), got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not torch.is_tensor(a) or a.dtype != torch.uint8:
        raise TypeError(f"lc2is_amd.data: {what} must be a uint8 array or tensor, got {getattr(a, 'dtype', type(a))}")
    return a.contiguous()


def _desc_rows(shapes, img_offs, lab_offs) -> torch.Tensor:
    """lc2is_aug_image rows as int64 [n, 3]: img_off, lab_off, H | W << 32."""
    return torch.tensor([[io, lo, h | (w << 32)] for (h, w), io, lo in zip(shapes, img_offs, lab_offs)],
                        dtype=torch.int64).reshape(-1, 3)


class DeviceImagePool:
    """Decoded uint8 images (HWC, 3 channels) and their label maps (HW), of any sizes up to 4096 px a side, packed at 256-byte
    alignment into one uint8 device buffer each, plus a descriptor table on the device.  The buffers grow by ``chunk_bytes``;
    growing moves them, so a graph captured over the pool must be captured again after images are added."""

    def __init__(self, device="cuda", chunk_bytes: int = 256 << 20):
        self.device = _need_cuda(device)
        self.chunk = max(int(chunk_bytes), ALIGN)
        self._img = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._lab = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._img_end = self._lab_end = 0
        self._shapes, self._img_offs, self._lab_offs = [], [], []
        self._desc = None

    @staticmethod
    def check(image, label) -> tuple[int, int]:
        """Validate one (image, label) pair; returns (H, W).  TypeError for a wrong dtype, ValueError for a wrong shape."""
        im, lb = _as_u8(image, "images"), _as_u8(label, "labels")
        if im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"lc2is_amd.data: images must be HWC with 3 channels, got shape {tuple(im.shape)}")
        h, w = int(im.shape[0]), int(im.shape[1])
        if tuple(lb.shape) != (h, w):
            raise ValueError(f"lc2is_amd.data: label shape {tuple(lb.shape)} does not match its image's ({h}, {w})")
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"lc2is_amd.data: image sides must be 1..{MAX_SIDE} px, got {h} x {w}")
        return h, w

    def _grow(self, buf: torch.Tensor, used: int, need: int) -> torch.Tensor:
        if need + ALIGN <= buf.numel():
            return buf
        new = torch.empty(_up(need + ALIGN, self.chunk), dtype=torch.uint8, device=self.device)
        new[:used].copy_(buf[:used])
        return new

    def reserve(self, img_bytes: int, lab_bytes: int) -> None:
        """Make room for this many more packed bytes at once (from_arrays does; saves the copies of repeated growth)."""
        self._img = self._grow(self._img, self._img_end, self._img_end + img_bytes)
        self._lab = self._grow(self._lab, self._lab_end, self._lab_end + lab_bytes)

    def add(self, image, label) -> int:
        """Append one image (uint8 HWC, host or device) with its label map (uint8 HW); returns its index in the pool."""
        h, w = self.check(image, label)
        im, lb = _as_u8(image, "images"), _as_u8(label, "labels")
        (io,), (lo,), img_end, lab_end = pack_offsets([(h, w)], self._img_end, self._lab_end)
        self.reserve(img_end - self._img_end, lab_end - self._lab_end)
        self._img[io:io + 3 * h * w].copy_(im.reshape(-1))
        self._lab[lo:lo + h * w].copy_(lb.reshape(-1))
        self._img_end, self._lab_end = img_end, lab_end
        self._shapes.append((h, w)); self._img_offs.append(io); self._lab_offs.append(lo)
        self._desc = None
        return len(self._shapes) - 1

    @classmethod
    def from_arrays(cls, images, labels, device="cuda", chunk_bytes: int = 256 << 20) -> "DeviceImagePool":
        if len(images) != len(labels):
            raise ValueError(f"lc2is_amd.data: {len(images)} images for {len(labels)} label maps")
        pool = cls(device, chunk_bytes)
        shapes = [cls.check(im, lb) for im, lb in zip(images, labels)]
        _, _, img_end, lab_end = pack_offsets(shapes)
        pool.reserve(img_end, lab_end)
        for im, lb in zip(images, labels):
            pool.add(im, lb)
        return pool

    @classmethod
    def _transient(cls, img, lab, desc, shapes) -> "DeviceImagePool":
        pool = cls.__new__(cls)
        pool.device, pool._img, pool._lab, pool._desc, pool._shapes = img.device, img, lab, desc, list(shapes)
        return pool

    def __len__(self) -> int:
        return len(self._shapes)

    @property
    def nbytes(self) -> int:
        """Packed bytes in use (pixels + labels, alignment gaps included)."""
        return self._img_end + self._lab_end

    def shape(self, index: int) -> tuple[int, int]:
        return self._shapes[index]

    def offsets(self, index: int) -> tuple[int, int]:
        return self._img_offs[index], self._lab_offs[index]

    @property
    def images(self) -> torch.Tensor:
        return self._img

    @property
    def labels(self) -> torch.Tensor:
        return self._lab

    def class_counts(self, indices=None, chunk: int = 4096) -> torch.Tensor:
        """Pixels per label value of the images `indices` (None: every image of the pool): int64 [n, 256] on the device
        (ops.label_histogram, `chunk` images per launch).  The input of ``class_weights``."""
        dev = _need_cuda(self.device)
        if indices is None:
            idx = torch.arange(len(self), dtype=torch.int64, device=dev)
        else:
            idx = TrainAugment._indices(indices, dev)
        out = torch.empty((idx.numel(), ops.LABEL_BINS), dtype=torch.int64, device=dev)
        if idx.numel():
            desc = self.desc
            for lo in range(0, idx.numel(), max(int(chunk), 1)):
                part = idx[lo:lo + max(int(chunk), 1)]
                out[lo:lo + part.numel()] = ops.label_histogram(self._lab, desc, part)
        return out

    @property
    def desc(self) -> torch.Tensor:
        """The descriptor table on the device: int64 [n, 3] = img_off, lab_off, H | W << 32 (lc2is_aug_image)."""
        if not self._shapes:
            raise RuntimeError("lc2is_amd.data: the image pool is empty")
        if self._desc is None:
            self._desc = _upload(_desc_rows(self._shapes, self._img_offs, self._lab_offs), self.device)
        return self._desc


def class_weights(counts: torch.Tensor, n_classes: int = 151, ignore_index: int | None = 0, mode: str = "median_freq",
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Class weights fp32 [n_classes] for ``CrossEntropyLoss(weight=)`` / ``TrainStep(criterion=)`` from per-image class counts
    [n, >= n_classes] (``DeviceImagePool.class_counts``), computed in fp64 with torch ops on the counts' device, no host read.
    Only the pixels of classes 0 .. n_classes - 1 other than ``ignore_index`` count.
    "median_freq" (Eigen & Fergus): f_c = pixels of c / counted pixels of the images in which c occurs; w_c = median of f over the
    classes that occur (the mean of the two middle values for an even number) / f_c.
    "enet" (Paszke et al.): w_c = 1 / ln(1.02 + p_c), p_c = the share of c in all counted pixels.
    A class that never occurs and ``ignore_index`` get weight 0.  ``dtype=torch.float64`` returns the values before the one rounding."""
    if mode not in ("median_freq", "enet"):
        raise ValueError(f"lc2is_amd.data: class_weights mode must be 'median_freq' or 'enet', got {mode!r}")
    if not torch.is_tensor(counts) or counts.dim() != 2 or counts.is_floating_point() or not 1 <= int(n_classes) <= counts.shape[1]:
        raise ValueError("lc2is_amd.data: class_weights takes integer counts [n, >= n_classes]")
    c = counts[:, :int(n_classes)].to(torch.int64).clone()
    if ignore_index is not None and 0 <= int(ignore_index) < int(n_classes):
        c[:, int(ignore_index)] = 0
    pix = c.sum(dim=0)
    occurs = pix > 0
    if mode == "median_freq":
        total = ((c > 0) * c.sum(dim=1, keepdim=True)).sum(dim=0)
        f = pix.double() / total.clamp(min=1).double()
        s = torch.sort(torch.where(occurs, f, torch.full_like(f, float("inf")))).values      # the occurring classes come first
        k = occurs.sum()
        mid = torch.stack([(k - 1).clamp(min=0) // 2, k // 2]).clamp(max=int(n_classes) - 1)
        w = 0.5 * s[mid].sum() / f
    else:
        w = 1.0 / torch.log(1.02 + pix.double() / pix.sum().clamp(min=1).double())
    return torch.where(occurs, w, torch.zeros_like(w)).to(dtype)


_PAD_LABEL = "pad_label"          # cat_ignore_label's default: whatever pad_label is


class TrainAugment:
    """Random rescale + crop + flip + photometric jitter of a batch on the device; see the module docstring for the definition.

    ``cat_max_ratio``: None, or the share in (0, 1) (mmseg: 0.75) a single class must stay below among the counted label cells of
    a crop; ``cat_ignore_label``: the label that is not counted (0..255; default: pad_label; None: every label counts);
    ``cat_tries``: the number of candidates that are checked (1..10) before one more is taken unchecked.  ``last_crop_info``: the
    device tensor int32 [B, 4] = (candidate taken, counted cells, largest class, classes) of the last call, never read back here.

    ``photometric``: True (PHOTOMETRIC_DEFAULTS), False (identity colour) or a dict overriding some of brightness_delta (0..255
    scale), contrast_range, saturation_range, hue_delta (degrees), prob (one probability, or four: brightness, contrast,
    saturation, hue)."""

    def __init__(self, crop_size: int = 512, label_size: int = 128, base_size: int = 512, ratio_range=(0.5, 2.0),
                 flip_prob: float = 0.5, photometric=True, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD,
                 pad_label: int = 0, seed: int = 0, cat_max_ratio: float | None = None, cat_ignore_label=_PAD_LABEL,
                 cat_tries: int = 10):
        S, L = int(crop_size), int(label_size)
        if S < 4 or S > MAX_SIDE or S % 4:
            raise ValueError(f"lc2is_amd.data: crop_size must be a multiple of 4 in 4..{MAX_SIDE}, got {S}")
        if L < 1 or S % L:
            raise ValueError(f"lc2is_amd.data: crop_size {S} must be a multiple of label_size {L}")
        lo, hi = (int(round(float(r) * 1024)) for r in ratio_range)
        if not 1 <= lo <= hi <= 1 << 20 or not 1 <= int(base_size) <= 65536:
            raise ValueError(f"lc2is_amd.data: bad base_size {base_size} / ratio_range {tuple(ratio_range)}")
        _mean_std(image_mean, image_std)
        self.crop_size, self.label_size, self.pad_label = S, L, int(pad_label)
        self.seed, seed_lo, seed_hi = _seed_words(int(seed))
        ignore = cat_ignore_label
        if isinstance(ignore, str) and ignore == _PAD_LABEL:      # defaulted: only a crop rule that is on needs it in range
            ignore = int(pad_label) if cat_max_ratio is not None or 0 <= int(pad_label) <= 255 else None
        if ignore is not None and not 0 <= int(ignore) <= 255:
            raise ValueError(f"lc2is_amd.data: cat_ignore_label must be a label 0..255 or None, got {ignore}")
        if not 1 <= int(cat_tries) <= ops.AUG_MAX_TRIES:
            raise ValueError(f"lc2is_amd.data: cat_tries must be 1..{ops.AUG_MAX_TRIES}, got {cat_tries}")
        if cat_max_ratio is not None and not (0.0 < float(cat_max_ratio) < 1.0 and 1 <= int(round(float(cat_max_ratio) * 1024)) <= 1023):
            raise ValueError(f"lc2is_amd.data: cat_max_ratio must lie in (0, 1) (in 1/1024 units: 1..1023), got {cat_max_ratio}")
        self.cat_max_ratio = None if cat_max_ratio is None else float(cat_max_ratio)
        self.cat_ratio1024 = None if cat_max_ratio is None else int(round(float(cat_max_ratio) * 1024))
        self.cat_ignore_label, self.cat_tries = -1 if ignore is None else int(ignore), int(cat_tries)
        self.last_crop_info = None
        ph = dict(PHOTOMETRIC_DEFAULTS)
        if isinstance(photometric, dict):
            unknown = set(photometric) - set(ph)
            if unknown:
                raise ValueError(f"lc2is_amd.data: unknown photometric settings {sorted(unknown)}")
            ph.update(photometric)
        probs = ph["prob"] if isinstance(ph["prob"], (tuple, list)) else (ph["prob"],) * 4
        if len(probs) != 4:
            raise ValueError("lc2is_amd.data: photometric prob must be one probability or four")
        if photometric is False:
            probs = (0.0,) * 4
        c = self.config = ops.AugConfig()
        c.seed_lo, c.seed_hi = seed_lo, seed_hi
        c.crop_size, c.base_size, c.ratio_lo1024, c.ratio_hi1024 = S, int(base_size), lo, hi
        c.flip_thr = _threshold(float(flip_prob), "flip_prob")
        for i, p in enumerate(probs):
            c.photo_thr[i] = _threshold(float(p), "photometric prob")
        c.brightness_delta = float(ph["brightness_delta"])
        c.contrast_lo, c.contrast_hi = (float(v) for v in ph["contrast_range"])
        c.saturation_lo, c.saturation_hi = (float(v) for v in ph["saturation_range"])
        c.hue_delta = math.radians(float(ph["hue_delta"]))
        n = self.norm = ops.AugNorm()
        for i in range(3):
            n.mean[i] = float(image_mean[i])
            n.inv_std[i] = 1.0 / float(image_std[i])
        self._stage = self._stage_free = None

    # ---- the launches ----
    _indices, _epoch = staticmethod(_indices), staticmethod(_epoch)      # (the key / epoch upload of _shared, under its old names)

    def params(self, pool: DeviceImagePool, indices, epoch, *, keys=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """The parameter table int32 [B, 20] of the samples `indices` of the pool in `epoch` (ops.aug_params).  keys: the dataset
        indices to draw for when they differ from the pool's (the streaming form)."""
        dev = _need_cuda(pool.device)
        idx = self._indices(indices, dev)
        return ops.aug_params(idx, self._epoch(epoch, dev), pool.desc, self.config,
                              keys=None if keys is None else self._indices(keys, dev), out=out)

    def select(self, pool: DeviceImagePool, indices, epoch, params: torch.Tensor, *, keys=None) -> torch.Tensor:
        """The class-ratio re-draw (ops.aug_crop_select): replaces top / left of `params` IN PLACE and returns it; the info
        tensor is kept in ``last_crop_info``.  With cat_max_ratio=None: nothing is launched."""
        if self.cat_ratio1024 is None:
            return params
        dev = _need_cuda(pool.device)
        self.last_crop_info = ops.aug_crop_select(pool.labels, pool.desc, self._indices(indices, dev), self._epoch(epoch, dev),
                                                  self.config, params, self.label_size, ratio1024=self.cat_ratio1024,
                                                  ignore_label=self.cat_ignore_label, tries=self.cat_tries,
                                                  keys=None if keys is None else self._indices(keys, dev))
        return params

    def apply(self, pool: DeviceImagePool, indices, params: torch.Tensor, out: dict | None = None) -> dict:
        """Cut the batch: {"pixel_values": fp32 [B,3,S,S], "label": int64 [B,L,L]} (ops.aug_apply), into `out`'s tensors if given."""
        dev = _need_cuda(pool.device)
        px, lb = ops.aug_apply(pool.images, pool.labels, pool.desc, self._indices(indices, dev), params, self.crop_size,
                               self.label_size, self.norm, pad_label=self.pad_label,
                               out_img=None if out is None else out["pixel_values"], out_lab=None if out is None else out["label"])
        return {"pixel_values": px, "label": lb}

    def __call__(self, pool: DeviceImagePool | None = None, indices=None, epoch=0, *, images=None, labels=None,
                 out: dict | None = None) -> dict:
        """Pool form: ``aug(pool, indices, epoch)``.  Streaming form: ``aug(images=[...], labels=[...], indices=..., epoch=...)``
        with host uint8 arrays and their DATASET indices: the batch is packed in one pinned staging buffer, crosses PCIe in one
        copy and gives the bits the pool form gives for the same indices.  (The staging buffer is reused: a call waits on the
        host for the previous call's copy, and nothing else.)"""
        if indices is None:
            raise ValueError("lc2is_amd.data: indices are required (the random numbers are a function of them)")
        if pool is not None:
            if images is not None or labels is not None:
                raise ValueError("lc2is_amd.data: give a pool or images / labels, not both")
            idx = self._indices(indices, _need_cuda(pool.device))
            epoch = self._epoch(epoch, idx.device)
            return self.apply(pool, idx, self.select(pool, idx, epoch, self.params(pool, idx, epoch)), out)
        if images is None or labels is None or len(images) != len(labels) or not len(images):
            raise ValueError("lc2is_amd.data: the streaming form takes as many images as labels, at least one")
        dev = indices.device if torch.is_tensor(indices) and indices.is_cuda else torch.device("cuda", torch.cuda.current_device())
        keys = self._indices(indices, dev)
        if keys.numel() != len(images):
            raise ValueError(f"lc2is_amd.data: {keys.numel()} indices for {len(images)} images")
        transient = self._stream_pool(images, labels, dev)
        slots = torch.arange(len(images), dtype=torch.int64, device=dev)
        epoch = self._epoch(epoch, dev)
        return self.apply(transient, slots, self.select(transient, slots, epoch, self.params(transient, slots, epoch, keys=keys), keys=keys), out)

    def _stream_pool(self, images, labels, dev) -> DeviceImagePool:
        shapes = [DeviceImagePool.check(im, lb) for im, lb in zip(images, labels)]
        img_offs, lab_offs, img_end, lab_end = pack_offsets(shapes)
        img_end = _up(img_end + _TAIL)
        desc_off, total = img_end + lab_end, img_end + lab_end + 24 * len(shapes)
        if self._stage is None or self._stage.numel() < total:
            self._stage = torch.empty(_up(total, 1 << 20), dtype=torch.uint8).pin_memory()
        elif self._stage_free is not None:
            self._stage_free.synchronize()       # the previous call's copy has left the staging buffer
        host = self._stage.numpy()
        for im, lb, (h, w), io, lo in zip(images, labels, shapes, img_offs, lab_offs):
            host[io:io + 3 * h * w] = _as_u8(im, "images").cpu().numpy().reshape(-1)
            host[img_end + lo:img_end + lo + h * w] = _as_u8(lb, "labels").cpu().numpy().reshape(-1)
        self._stage[desc_off:total].view(torch.int64).copy_(_desc_rows(shapes, img_offs, lab_offs).reshape(-1))
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        buf.copy_(self._stage[:total], non_blocking=True)
        self._stage_free = torch.cuda.Event()
        self._stage_free.record()
        return DeviceImagePool._transient(buf[:img_end], buf[img_end:desc_off], buf[desc_off:].view(torch.int64).view(-1, 3), shapes)


class AugmentedBatches:
    """One epoch of augmented batches from a pool, in ADE20KCollator's format: yields (inputs, metas) with inputs =
    {"pixel_values", "label", **extra_inputs} (extra_inputs: the tokenised class prompts) and metas = one dict per sample
    (its pool index and the epoch).  The epoch's order is a seeded permutation of the pool, cut to a multiple of `world` and
    strided over the ranks; ``set_epoch(e)`` selects the epoch (the permutation and the augmentation both depend on it).
    The only host -> device traffic is the epoch's index vector, once per epoch through pinned memory; nothing synchronises."""

    def __init__(self, pool: DeviceImagePool, augment: TrainAugment, batch_size: int, shuffle_seed: int, drop_last: bool = True,
                 rank: int = 0, world: int = 1, extra_inputs: dict | None = None):
        _need_cuda(pool.device)
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"lc2is_amd.data: bad batch_size {batch_size} / rank {rank} of {world}")
        self.pool, self.augment, self.batch_size, self.shuffle_seed = pool, augment, int(batch_size), int(shuffle_seed)
        self.drop_last, self.rank, self.world, self.extra_inputs = bool(drop_last), int(rank), int(world), dict(extra_inputs or {})
        self.epoch = 0

    @staticmethod
    def epoch_indices(n: int, shuffle_seed: int, epoch: int, rank: int = 0, world: int = 1) -> torch.Tensor:
        """The pool indices rank `rank` of `world` visits in `epoch`, in order (host int64): a permutation of range(n) seeded by
        (shuffle_seed, epoch), cut to a multiple of world, every world-th entry from `rank` on."""
        g = torch.Generator().manual_seed((int(shuffle_seed) * 0x9E3779B1 + int(epoch) * 0x85EBCA77 + 1) % (1 << 63))
        perm = torch.randperm(n, generator=g)
        return perm[:n - n % world][rank::world].contiguous()

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        n = len(self.pool) // self.world
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        dev, epoch = self.pool.device, self.epoch
        order = self.epoch_indices(len(self.pool), self.shuffle_seed, epoch, self.rank, self.world)
        order_dev = _upload(order, dev)
        epoch_dev = torch.full((1,), epoch, dtype=torch.int32, device=dev)
        host = order.tolist()
        for b in range(len(self)):
            lo, hi = b * self.batch_size, min((b + 1) * self.batch_size, len(host))
            batch = self.augment(self.pool, order_dev[lo:hi], epoch_dev)
            yield {**self.extra_inputs, **batch}, [dict(index=i, epoch=epoch) for i in host[lo:hi]]
