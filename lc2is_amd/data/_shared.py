"""What the device data classes (TrainAugment, SampleMix, StrongAugment, GeometricAugment) share: the checks of their settings, the
seed split, the key / epoch upload and the type, shape and device checks of a batch in front of ``ops``.  Private to ``lc2is_amd.data``."""
from __future__ import annotations

import math

import torch


# ---- settings ----
def _int(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"lc2is_amd.data: {what} must be an int, got {v!r}")
    return v


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"lc2is_amd.data: {what} must be a number, got {v!r}")
    if not math.isfinite(v):
        raise ValueError(f"lc2is_amd.data: {what} must be finite, got {v!r}")
    return float(v)


def _pair(v, what: str) -> tuple[float, float]:
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise TypeError(f"lc2is_amd.data: {what} must be a (lo, hi) pair, got {v!r}")
    lo, hi = _number(v[0], what), _number(v[1], what)
    if lo > hi:
        raise ValueError(f"lc2is_amd.data: {what} must be ordered, got {tuple(v)}")
    return lo, hi


def _threshold(p: float, what: str) -> int:
    """A probability as the 24-bit threshold its uniform draw is compared with."""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"lc2is_amd.data: {what} must be a probability, got {p}")
    return int(round(p * (1 << 24)))


def _seed_words(seed: int) -> tuple[int, int, int]:
    """(seed mod 2^64, seed_lo, seed_hi) as the config structs hold it.  What a seed may be is the caller's to check."""
    seed &= 2 ** 64 - 1
    return seed, seed & 0xffffffff, seed >> 32


def _mean_std(image_mean, image_std) -> None:
    if len(image_mean) != 3 or len(image_std) != 3 or min(image_std) <= 0:
        raise ValueError("lc2is_amd.data: image_mean / image_std must hold three values, std positive")


# ---- device ----
def _need_cuda(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("lc2is_amd.data: augmentation runs on a HIP device; there is no CPU path (tests/augment_ref.py restates it in numpy, test-only)")
    return device


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    """Host tensor -> device through pinned memory, asynchronously (no host synchronisation)."""
    return t.pin_memory().to(device, non_blocking=True)


def _indices(indices, device) -> torch.Tensor:
    """Keys / pool indices as a device int64 [n]: a device tensor is taken as it is, anything else is uploaded."""
    if torch.is_tensor(indices) and indices.is_cuda:
        if indices.dtype != torch.int64 or indices.dim() != 1:
            raise TypeError("lc2is_amd.data: device indices must be a 1-D int64 tensor")
        return indices.contiguous()
    return _upload(torch.as_tensor(indices, dtype=torch.int64).reshape(-1), device)


def _epoch(epoch, device) -> torch.Tensor:
    """The epoch as a device int32 [1]: a device tensor is taken as it is, an int is uploaded."""
    if torch.is_tensor(epoch) and epoch.is_cuda:
        if epoch.dtype != torch.int32 or epoch.numel() != 1:
            raise TypeError("lc2is_amd.data: a device epoch must be one int32")
        return epoch
    return _upload(torch.tensor([int(epoch)], dtype=torch.int32), device)


def _keys_for(who: str, keys, device, B: int, what: str = "keys", of: str = "samples") -> torch.Tensor:
    keys = _indices(keys, device)
    if keys.numel() != B:
        raise ValueError(f"lc2is_amd.data: {who} got {keys.numel()} {what} for {B} {of}")
    return keys


# ---- a batch in front of ops ----
def _tensor_type(who: str, t, dtype, what: str, optional: bool = False) -> None:
    if not (t is None and optional) and (not torch.is_tensor(t) or t.dtype != dtype):
        raise TypeError(f"lc2is_amd.data: {who} {what} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")


def _pixel_shape(who: str, x, min_side: int, max_side: int) -> tuple[int, int]:
    """(B, S) of pixel_values [B, 3, S, S], S a multiple of 4 in min_side..max_side."""
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f"lc2is_amd.data: {who} pixel_values must be [B, 3, S, S], got {tuple(x.shape)}")
    B, S = int(x.shape[0]), int(x.shape[2])
    if S < min_side or S > max_side or S % 4:
        raise ValueError(f"lc2is_amd.data: {who} needs S a multiple of 4 in {min_side}..{max_side}, got {S}")
    return B, S


def _require_device(who: str, ref: str, *tensors) -> torch.device:
    """Between a class's stage one (no device: TypeError for types, then ValueError for shapes) and its stage two (the ``ops`` check of
    layout, alignment and overlap, RuntimeError): every tensor must be on a HIP device; ``ref`` names the numpy restatement."""
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"lc2is_amd.data: {who} runs on a HIP device; there is no CPU path ({ref}, test-only)")
    return _need_cuda(tensors[0].device)
