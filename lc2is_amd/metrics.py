"""Device-side counterparts of the reference's segmentation metrics (metrics.py:45-102).

``compute_mIOU(outputs [N,K,h,w] logits, labels [N,h,w])`` (metrics.py:82-102): per image, bicubic x4 of the logits (HIP upsample
kernel), argmax (Softmax2d is monotone, so it is skipped), nearest x4 of the labels, per-class intersection / union counts in one
HIP pass, IoU averaged over the classes present in the label except ``ignore_index``, then over images.
Returns ``dict(mIOU_label=float)`` like the reference.  (torchmetrics is not needed.)

``compute_gt_mIOU(outputs, gt_list, sizes)`` (metrics.py:61-79): the same at each image's ORIGINAL size — bicubic resize of the
logits to ``sizes[i]`` (any size), argmax and counts against the original-resolution annotation ``gt_list[i]`` in one fused HIP
kernel (``ops.resize_argmax``) that never forms the [K, H, W] score map.  Returns ``dict(mIOU_gt=float)``.
``original_size_predictions(outputs, sizes)`` is the reference's ``original_size_interpolate`` (metrics.py:137-143) followed by
the argmax: a uint8 class map per image at its own size.
Past ``ops.RESIZE_KMAX`` = 192 classes (up to 1024) both go through ``ops.resize_argmax_wide``: the same arithmetic per class and
int16 class maps (``model.predict``'s convention).  ``compute_mIOU`` / ``per_image_mIOU`` stay at 192 classes (the narrow
``head_upsample_ce`` + ``miou_counts``); past them the model-size mIoU is ``forward_loss(..., seg_counts=)``.

``dataset_iou(counts_sum)``: the dataset-level scores of the published protocol (mmseg's IoUMetric: mIoU, mAcc, aAcc) from
{intersection, predicted, labelled} counts summed over all images, as ``slide.SlidingWindowInference.counts`` produces them."""
from __future__ import annotations

import torch

from . import ops


def _per_image_iou(counts: torch.Tensor, ignore_index: int | None) -> torch.Tensor:
    """float64 [N] from int32 [N, 3, K] {intersection, predicted, labelled} counts: IoU averaged over the classes the label holds,
    ``ignore_index`` excepted."""
    counts = counts.to(torch.float64)
    inter, pred, lab = counts[:, 0], counts[:, 1], counts[:, 2]
    union = pred + lab - inter
    iou = torch.where(union > 0, inter / union.clamp_min(1), torch.zeros_like(union))
    present = lab > 0
    if ignore_index is not None:
        present[:, ignore_index] = False
    # an image whose label holds nothing but ignore_index: the reference takes the mean of an EMPTY selection (metrics.py:94-97),
    # which is NaN, and the mean over images (:101) inherits it — 0 / 0 here reproduces that instead of scoring the image 0
    return (iou * present).sum(1) / present.sum(1).to(torch.float64)


def _resize_argmax_op(outputs: torch.Tensor):
    """``ops.resize_argmax``, or its wide form past 192 classes."""
    return ops.resize_argmax_wide if outputs.dim() == 4 and outputs.shape[1] > ops.RESIZE_KMAX else ops.resize_argmax


def per_image_mIOU(outputs: torch.Tensor, labels: torch.Tensor, n_cls: int = 151, ignore_index: int | None = 0) -> torch.Tensor:
    """The per-image values whose mean ``compute_mIOU`` returns (float64 [N] on the device; NaN for an image whose label holds
    nothing but ``ignore_index``).  ``Evaluator`` accumulates these batch by batch instead of keeping every batch's logits."""
    if not outputs.is_cuda:
        raise RuntimeError("lc2is_amd.metrics: outputs must be on the GPU (no CPU path)")
    N, K, h, w = outputs.shape
    ld = (K + 63) // 64 * 64
    lo = torch.zeros(N * h * w, ld, dtype=torch.float32, device=outputs.device)
    lo[:, :K] = outputs.float().permute(0, 2, 3, 1).reshape(N * h * w, K)
    _, _, hi = ops.head_upsample_ce(lo, None, N, h, w, K, 4, ops.INTERP_BICUBIC, want_scores=True, want_loss=False)
    return _per_image_iou(ops.miou_counts(hi, labels, 4), ignore_index)


def compute_mIOU(outputs: torch.Tensor, labels: torch.Tensor, n_cls: int = 151, ignore_index: int | None = 0) -> dict:
    return dict(mIOU_label=float(per_image_mIOU(outputs, labels, n_cls, ignore_index).mean().item()))


def per_image_gt_mIOU(outputs: torch.Tensor, gt_list, sizes=None, n_cls: int = 151, ignore_index: int | None = 0) -> torch.Tensor:
    """The per-image values whose mean ``compute_gt_mIOU`` returns (float64 [N] on the device; NaN for an image whose gt holds
    nothing but ``ignore_index``).  gt_list: N label maps [H_i, W_i] (uint8 / int32 / int64, host or device); sizes: N (H, W)
    pairs or an [N, 2] tensor, None = the gt maps' shapes (ValueError when they disagree)."""
    _, counts = _resize_argmax_op(outputs)(outputs, sizes, gt=list(gt_list), want_pred=False)
    return _per_image_iou(counts, ignore_index)


def compute_gt_mIOU(outputs: torch.Tensor, gt_list, sizes, n_cls: int = 151, ignore_index: int | None = 0) -> dict:
    return dict(mIOU_gt=float(per_image_gt_mIOU(outputs, gt_list, sizes, n_cls, ignore_index).mean().item()))


def original_size_predictions(outputs: torch.Tensor, sizes) -> list[torch.Tensor]:
    """The class map of each image at its original size: uint8 [H_i, W_i] on the device, int16 past 192 classes (the argmax of
    the bicubic resize of outputs[i] to sizes[i], exact ties to the lowest class)."""
    preds, _ = _resize_argmax_op(outputs)(outputs, sizes, want_pred=True)
    return preds


def dataset_iou(counts_sum: torch.Tensor, ignore_index: int | None = 0) -> dict:
    """Dataset-level scores from [3, K] {intersection, predicted, labelled} counts SUMMED over the images (int64; counted with
    ``ignore_index`` excluded, ``ops.resize_argmax_windows(ignore_index=)``).  float64 tensors on the counts' device, nothing is
    read to the host: ``IoU`` [K] (NaN for a class with an empty union), ``mIoU`` = its mean over the classes with a non-empty
    union, ``mAcc`` = the mean of intersection / labelled over the labelled classes, ``aAcc`` = all intersections / all labelled;
    ``ignore_index`` takes part in none of them."""
    if counts_sum.dim() != 2 or counts_sum.shape[0] != 3:
        raise ValueError(f"lc2is_amd.metrics.dataset_iou: counts must be [3, K] summed over images, got {tuple(counts_sum.shape)}")
    c = counts_sum.to(torch.float64)
    inter, pred, lab = c[0], c[1], c[2]
    keep = torch.ones_like(inter, dtype=torch.bool)
    if ignore_index is not None and 0 <= ignore_index < keep.numel():
        keep[ignore_index] = False
    union = pred + lab - inter
    nan = torch.full_like(inter, float("nan"))
    iou = torch.where(union > 0, inter / union.clamp_min(1), nan)
    acc = torch.where(lab > 0, inter / lab.clamp_min(1), nan)
    seen, labelled = keep & (union > 0), keep & (lab > 0)
    zero = torch.zeros_like(inter)
    return dict(mIoU=torch.where(seen, iou, zero).sum() / seen.sum(),
                mAcc=torch.where(labelled, acc, zero).sum() / labelled.sum(),
                aAcc=torch.where(keep, inter, zero).sum() / torch.where(keep, lab, zero).sum(),
                IoU=torch.where(keep, iou, nan))
