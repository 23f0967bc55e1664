"""The evaluation pass — this repo's counterpart of ``Engine.evaluate`` / ``Engine.eval_loop`` (reference
engine.py:125-168) plus the label-size metric it feeds (``metrics.segmentation_metrics`` -> ``compute_mIOU``,
metrics.py:45-58,82-102).

    ev = Evaluator(model, eval_loader, criterion, aux_criterion=None, compute_metrics=segmentation_metrics)
    metrics = ev.evaluate()        # {"eval_loss": ..., ["eval_aux_loss": ...], "eval_mIOU_label": ...}
    ev = Evaluator(..., gt_from_metas=lambda metas: [m["gt"] for m in metas])
    metrics = ev.evaluate()        # ... and "eval_mIOU_gt": the mIoU at each image's original size (compute_gt_mIOU)
    ev = SlideEvaluator(slide.SlidingWindowInference(model, text_inputs, flip=True), loader)   # loader: (images, gt_list)
    metrics = ev.evaluate()        # {"eval_mIoU", "eval_mAcc", "eval_aAcc"} over the dataset (sliding windows), "eval_mIOU_gt"

Semantics kept from the reference:
  * ``model.eval()``; per batch ``inputs, metas = data``; ``labels = inputs.pop("label")``; ``torch.no_grad()`` forward;
    ``eval_loss = criterion(outputs_dict["outputs"], labels)``; the aux loss (x 0.4) when the model returns
    ``low_score_map`` (engine.py:143-156);
  * the loss metrics are the MEAN OVER BATCHES of the per-batch losses (engine.py:158-165: a list of ``.item()``s,
    ``np.array(v).mean()``), not a pixel-weighted mean;
  * ``compute_metrics(outputs=all_outputs, labels=all_labels)`` on the concatenated outputs, keys prefixed ``eval_``
    (engine.py:128-130).
Differences (MI355X): outputs and labels stay ON THE DEVICE (the reference moves every batch to the host and re-concatenates
the growing tensor each step, engine.py:162-163 — O(n^2) host copies); the per-batch losses are kept as device scalars and
read once at the end (one sync per evaluation instead of one ``.item()`` per batch, engine.py:159); the metric is the HIP
``lc2is_amd.metrics.compute_mIOU`` (fused bicubic x4 + argmax + per-class counts).
"""
from __future__ import annotations

from typing import Callable, Iterable

import torch
from torch import nn

from . import metrics as _metrics


def segmentation_metrics(outputs: torch.Tensor, labels: torch.Tensor, gt_list=None, sizes=None, n_clas: int = 151,
                         ignore_index: int | None = 0, **_unused) -> dict:
    """metrics.segmentation_metrics (metrics.py:45-58): ``dict(mIOU_label=...)``, and ``mIOU_gt`` (``compute_gt_mIOU`` at each
    image's original size) when the original images' label maps ``gt_list`` are given — ``eval_loop`` supplies them only with
    ``Evaluator(gt_from_metas=...)``, as the reference's never does (engine.py:166; SURVEY.md §2 staleness).  ``sizes``: the
    (H, W) of each image, None = the gt maps' shapes."""
    m = _metrics.compute_mIOU(outputs=outputs, labels=labels, n_cls=n_clas, ignore_index=ignore_index)
    if gt_list is not None:
        m.update(_metrics.compute_gt_mIOU(outputs=outputs, gt_list=gt_list, sizes=sizes, n_cls=n_clas, ignore_index=ignore_index))
    return m


class Evaluator:
    """``Engine``'s evaluation half with the same constructor argument names (engine.py:15-21)."""

    def __init__(self, model: nn.Module, eval_loader: Iterable, criterion: nn.Module, aux_criterion: nn.Module | None = None,
                 compute_metrics: Callable | None = segmentation_metrics, device="cuda", keep_outputs: bool = False,
                 gt_from_metas: Callable | None = None) -> None:
        self.model = model
        self.eval_loader = eval_loader
        self.criterion = criterion
        self.aux_criterion = aux_criterion
        self.compute_metrics = compute_metrics
        self.device = torch.device(device)
        # With the default metric (a mean of per-image values) nothing but those values is kept between batches: the reference
        # concatenates every batch's logits (on the host, engine.py:162-163), which on the device would be ~20 GB (+ as much again
        # for the cat) over the 2000-image ADE20K validation split at 128 x 128.  ``keep_outputs=True`` (or a custom
        # ``compute_metrics``, whose contract is ``compute_metrics(outputs=..., labels=...)``) restores the concatenation.
        self.keep_outputs = keep_outputs or (compute_metrics is not None and compute_metrics is not segmentation_metrics)
        # ``gt_from_metas(metas) -> list of label maps [H_i, W_i]`` (the original images' annotations of one batch): adds
        # ``eval_mIOU_gt``, accumulated per image like ``per_image_mIOU``, or, when the outputs are kept, passed on to
        # ``compute_metrics`` as ``gt_list`` and ``sizes`` (the reference's metric signature).
        self.gt_from_metas = gt_from_metas
        self.model.to(self.device)

    def evaluate(self) -> dict:
        eval_metrics, eval_outputs = self.eval_loop()
        if self.compute_metrics is not None:
            if "per_image_mIOU" in eval_outputs:
                m = dict(mIOU_label=float(eval_outputs["per_image_mIOU"].mean().item()))
                if "per_image_mIOU_gt" in eval_outputs:
                    m["mIOU_gt"] = float(eval_outputs["per_image_mIOU_gt"].mean().item())
            else:
                m = self.compute_metrics(**eval_outputs)
            eval_metrics = {**eval_metrics, **{"eval_" + k: v for k, v in m.items()}}
        return eval_metrics

    def eval_loop(self) -> tuple[dict, dict]:
        self.model.eval()
        losses: dict[str, list[torch.Tensor]] = {}
        outs, labs, gts, gt_outs = [], [], [], []
        for data in self.eval_loader:
            inputs, metas = data
            inputs = {k: v.to(self.device, non_blocking=True) for k, v in inputs.items()}
            labels = inputs.pop("label")
            with torch.no_grad():
                outputs_dict = self.model(inputs)
                step = dict(eval_loss=self.criterion(outputs_dict["outputs"], labels))
                if "low_score_map" in outputs_dict.keys():
                    step["eval_aux_loss"] = self.aux_criterion(outputs_dict["low_score_map"], labels) * 0.4
            for k, v in step.items():
                losses.setdefault(k, []).append(v.detach().float().reshape(()))
            gt = None if self.gt_from_metas is None else list(self.gt_from_metas(metas))
            if self.keep_outputs or self.compute_metrics is None:
                outs.append(outputs_dict["outputs"])
                labs.append(labels)
                if gt is not None:
                    gts.extend(gt)
            else:
                outs.append(_metrics.per_image_mIOU(outputs_dict["outputs"], labels))
                if gt is not None:
                    gt_outs.append(_metrics.per_image_gt_mIOU(outputs_dict["outputs"], gt))
        eval_metrics = {k: float(torch.stack(v).mean().item()) for k, v in losses.items()}
        if self.keep_outputs or self.compute_metrics is None:
            eval_outputs = dict(outputs=torch.cat(outs), labels=torch.cat(labs))
            if self.gt_from_metas is not None:
                eval_outputs.update(gt_list=gts, sizes=torch.tensor([tuple(g.shape) for g in gts], dtype=torch.int64).view(-1, 2))
        else:
            eval_outputs = dict(per_image_mIOU=torch.cat(outs))
            if self.gt_from_metas is not None:
                eval_outputs["per_image_mIOU_gt"] = torch.cat(gt_outs)
        return eval_metrics, eval_outputs


class SlideEvaluator:
    """Whole-image evaluation by sliding windows (``slide.SlidingWindowInference``): the dataset-level mIoU / mAcc / aAcc of the
    published ADE20K protocol (``metrics.dataset_iou`` of the counts summed over all images, mmseg's counting rule: an ignored
    or out-of-range pixel counts nowhere) and the reference's per-image mean over the same predictions (``eval_mIOU_gt``,
    metrics.py:61-79, counted as ``Evaluator``'s: every pixel counts in "predicted", ``ignore_index`` only leaves the mean — a
    second fused launch over the same window forwards).  ``loader`` yields ``(images, gt_list)``: decoded uint8 HWC
    images and their label maps at the same sizes.  The counts stay on the device; the four scores are read once at the end."""

    def __init__(self, inference, loader: Iterable, ignore_index: int | None = 0) -> None:
        self.inference, self.loader, self.ignore_index = inference, loader, ignore_index

    def evaluate(self) -> dict:
        total, per_image = None, []
        for images, gt_list in self.loader:
            if self.ignore_index is None:
                c = c_ref = self.inference.counts(images, gt_list, ignore_index=None)
            else:
                c, c_ref = self.inference.counts_both(images, gt_list, self.ignore_index)
            s = c.sum(0, dtype=torch.int64)
            total = s if total is None else total + s
            per_image.append(_metrics._per_image_iou(c_ref, self.ignore_index))
        if total is None:
            raise ValueError("lc2is_amd.evalloop.SlideEvaluator: the loader yielded nothing")
        d = _metrics.dataset_iou(total, self.ignore_index)
        vals = torch.stack([d["mIoU"], d["mAcc"], d["aAcc"], torch.cat(per_image).mean()]).tolist()   # the one host read
        return dict(zip(("eval_mIoU", "eval_mAcc", "eval_aAcc", "eval_mIOU_gt"), vals))
