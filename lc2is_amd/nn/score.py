"""Score-map tail of the FTN / hierarchical compositions on MI355X.

Reference (model/final.py:350-356; the same four lines at model/model.py:204-212 and model/ftn.py:56-62):
    visual = rearrange(visual_embeddings, "b (h w) c -> b c h w"); visual = F.normalize(visual, dim=1)
    text   = F.normalize(text_embeddings, dim=-1)
    score_map = einsum('bchw,bkc->bkhw', visual, text);  score_map = F.interpolate(score_map, "bilinear", x4)
followed by nn.CrossEntropyLoss()(score_map, labels) in the engine (engine.py:94).

HIP path: L2-normalise both sides (one wave per row), one strided-batched MFMA GEMM launch for the per-image K class scores at the low
resolution, then the fused bilinear-x4 + softmax-CE kernel: the [B,K,4h,4w] fp32 map (157 MB/img at 512x512,
K=150 — "the" bandwidth-bound tensor of config 5) is only materialised when the caller asks for it.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .base import require_cuda
from .loss import check_ohem
from .model import (_reduce, fused_dice_options, fused_focal_options, fused_loss_options, fused_sigmoid_options, head_scores_hi,
                    head_scores_hi_bwd, wide_refuse)

KPAD = 192   # class pitch up to 192 classes; past them ops.class_pad(K)


def _scores_lo(visual, text):
    B, P, C = visual.shape
    K = text.shape[1]
    if K > ops.HEAD_WIDE_CMAX or C % 64:
        raise NotImplementedError(f"lc2is_amd ScoreMapTail: at most {ops.HEAD_WIDE_CMAX} classes ({ops.HEAD_CMAX} for every criterion "
                                  "but the plain cross-entropy), channel count a multiple of 64")
    kpad = ops.class_pad(K)
    v32 = visual.reshape(B * P, C).float().contiguous()
    t32 = text.reshape(B * K, C).float().contiguous()
    _, vn16, vinv = ops.l2norm_fwd(v32, want_f32=False)
    _, tn16, tinv = ops.l2norm_fwd(t32, want_f32=False)
    tpad = torch.zeros(B, kpad, C, dtype=torch.bfloat16, device=visual.device)
    tpad[:, :K] = tn16.view(B, K, C)
    # per-image class embeddings: ONE strided-batched NT launch (blockIdx.y = image)
    _, scores = ops.gemm_nt_batched(vn16.view(B, P, C), tpad)
    scores = scores.view(B * P, kpad)
    return scores, dict(v32=v32, t32=t32, vn16=vn16, tpad=tpad, vinv=vinv, tinv=tinv, dims=(B, P, C, K))


def _scores_bwd(ds32, sv):
    """ds32: gradient wrt the low-resolution scores [B*P, class_pad(K)] (fp32)."""
    B, P, C, K = sv["dims"]
    kpad = ops.class_pad(K)
    ds16 = ops.cast_bf16(ds32)
    dtn = torch.empty(B, kpad, C, dtype=torch.float32, device=ds32.device)
    tT = ops.transpose_bf16_batched(sv["tpad"])                                    # [B, C, KPAD]
    _, dvn = ops.gemm_nt_batched(ds16.view(B, P, kpad), tT)                         # d(normalised visual) [B, P, C]
    dvn = dvn.view(B * P, C)
    vn16 = sv["vn16"]
    probs = [(ds16[b * P:(b + 1) * P], vn16[b * P:(b + 1) * P], dtn[b], None, False) for b in range(B)]
    gmax = ops.GROUP_MAX
    for i in range(0, B, gmax):                                                    # the B weight-gradient-shaped products: one grid
        ops.gemm_tn_grouped(probs[i:i + gmax])
    dv = ops.l2norm_bwd(dvn, sv["v32"], sv["vinv"])
    dt = ops.l2norm_bwd(dtn[:, :K].reshape(B * K, C).contiguous(), sv["t32"], sv["tinv"])
    return dv.view(B, P, C), dt.view(B, K, C)


class _ScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, visual, text, labels, scale, ignore_index, save, loss_opts=None, ohem=None, owner=None, dice=None, seg_counts=None,
                accum=None, focal=None, sigmoid=None):
        B, P, C = visual.shape
        K = text.shape[1]
        h = int(round(P ** 0.5))
        scores, sv = _scores_lo(visual, text)
        if labels is None:
            hi = head_scores_hi(scores, B, h, h, K, scale, ops.INTERP_BILINEAR)
            ctx.sv, ctx.fused, ctx.meta = (sv if save else None), None, (B, h, K, scale)
            return hi
        if seg_counts is not None:   # accuracy / IoU counts of the batch: the ORIGINAL labels (before OHEM relabels), the loss's scores
            ops.seg_counts_add(seg_counts, scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR, ignore_index)
        if K > ops.HEAD_CMAX:   # the chunked cross-entropy (loss() refused every other criterion before anything ran)
            weight, _, reduction = loss_opts if loss_opts is not None else (None, 0.0, "mean")
            loss2, dlo = ops.head_upsample_ce_wide(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR, want_grad=save,
                                                   ignore_index=ignore_index, grad_scale=1.0, class_weight=weight)
            loss, inv = _reduce(loss2, reduction, save)
            if accum is not None:
                ops.accum_add(accum, loss2)
            elif inv is not None:
                dlo.mul_(inv)
            ctx.sv, ctx.fused, ctx.meta = (sv if save else None), dlo, (B, h, K, scale)
            return loss
        if dice is not None:   # CE + soft Dice: dlo is the gradient of the scalar loss
            ce_weight, dice_weight, smooth, present_only = dice
            loss4, stats, dlo = ops.head_upsample_ce_dice(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR,
                                                          want_grad=save, ignore_index=ignore_index, ce_weight=ce_weight,
                                                          dice_weight=dice_weight, smooth=smooth, present_only=present_only)
            owner.last_dice = (stats[0], stats[1], stats[2], loss4)
            ctx.sv, ctx.fused, ctx.meta = (sv if save else None), dlo, (B, h, K, scale)
            return loss4[0]
        if ohem is not None:   # hard-pixel selection: per-pixel loss pass, selection, then the same fused call on the new labels
            labels, info = ops.ohem_labels(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR, ignore_index, ohem)
            owner.last_ohem = (labels, info)
        if loss_opts is not None or focal is not None or sigmoid is not None:   # class weights / label smoothing / 'sum' (loss2[1] = sum_i w_{y_i})
            weight, label_smoothing, reduction = loss_opts if loss_opts is not None else (None, 0.0, "mean")
            if sigmoid is not None:   # sigmoid focal / sigmoid CE: per-class binary terms, [sum, NUMBER of counted pixels]
                loss2, dlo = ops.head_upsample_sigmoid(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR,
                                                       want_grad=save, ignore_index=ignore_index, grad_scale=1.0, class_weight=weight,
                                                       gamma=sigmoid[0], alpha=sigmoid[1],
                                                       class_scale=ops.sigmoid_class_scale(sigmoid[2], reduction, K))
            elif focal is not None:   # focal / poly-1: the CE gradient times one scalar per pixel, the same [sum, weighted count] pair
                loss2, dlo = ops.head_upsample_focal(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR,
                                                     want_grad=save, ignore_index=ignore_index, grad_scale=1.0, class_weight=weight,
                                                     gamma=focal[0], poly_eps=focal[1])
            else:
                loss2, dlo, _ = ops.head_upsample_ce(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR,
                                                     want_grad=save, ignore_index=ignore_index, grad_scale=1.0,
                                                     class_weight=weight, label_smoothing=label_smoothing)
            loss, inv = _reduce(loss2, reduction, save)
            if accum is not None:   # accumulation cycle: dlo stays the gradient of the SUM, the cycle's update divides
                ops.accum_add(accum, loss2)
            elif inv is not None:
                dlo.mul_(inv)
            ctx.sv, ctx.fused, ctx.meta = (sv if save else None), dlo, (B, h, K, scale)
            return loss
        n = float(B * h * scale * h * scale)
        loss2, dlo, _ = ops.head_upsample_ce(scores, labels.contiguous(), B, h, h, K, scale, ops.INTERP_BILINEAR,
                                             want_grad=save, ignore_index=ignore_index, grad_scale=1.0 / n)
        if accum is not None:   # accumulation cycle: undo the kernel's 1/n, dlo is the gradient of the SUM; the update divides
            ops.accum_add(accum, loss2)
            if save:
                dlo.mul_(n)
        elif save:   # mean over the pixels the kernel counted (negative / ignore_index / out-of-range labels are skipped)
            dlo.mul_(n / loss2[1].clamp_min(1.0))
        ctx.sv, ctx.fused, ctx.meta = (sv if save else None), dlo, (B, h, K, scale)
        return loss2[0] / loss2[1]

    @staticmethod
    def backward(ctx, gout):
        B, h, K, scale = ctx.meta
        if ctx.fused is not None:
            ds = ctx.fused * gout
        else:
            ds = head_scores_hi_bwd(gout, B, h, h, K, scale, ops.INTERP_BILINEAR, ops.class_pad(K))
        dv, dt = _scores_bwd(ds, ctx.sv)
        ctx.sv = ctx.fused = None
        return dv, dt, None, None, None, None, None, None, None, None, None, None, None, None


class ScoreMapTail(nn.Module):
    """``forward(visual_embeddings [B,h*w,C], text_embeddings [B,K,C]) -> score_map [B,K,S*h,S*w]`` (the reference's
    return value) and ``loss(visual, text, labels)`` = CrossEntropyLoss()(score_map, labels) without ever writing the map."""

    def __init__(self, scale_factor: int = 4) -> None:
        super().__init__()
        self.scale_factor = scale_factor

    def forward(self, visual_embeddings: torch.Tensor, text_embeddings: torch.Tensor) -> torch.Tensor:
        require_cuda(visual_embeddings, "visual_embeddings")
        save = torch.is_grad_enabled() and (visual_embeddings.requires_grad or text_embeddings.requires_grad)
        return _ScoreFn.apply(visual_embeddings, text_embeddings, None, self.scale_factor, -100, save)

    def loss(self, visual_embeddings: torch.Tensor, text_embeddings: torch.Tensor, labels: torch.Tensor,
             ignore_index: int = -100, *, weight=None, label_smoothing: float = 0.0, reduction: str = "mean",
             ohem=None, dice=None, seg_counts=None, accum=None, focal=None, sigmoid=None) -> torch.Tensor:
        """``weight`` / ``label_smoothing`` / ``reduction`` ('mean' or 'sum') as in nn.CrossEntropyLoss.  ``ohem=(thresh, min_kept
        per image)``: the loss over the hard pixels only (OhemCrossEntropyLoss's rule); ``self.last_ohem`` then holds (the labels
        the head saw, the device info block).  ``dice=(ce_weight, dice_weight, smooth, present_only)``: ce_weight * mean CE +
        dice_weight * soft Dice over the batch (DiceCrossEntropyLoss's definition), not combinable with the other options;
        ``self.last_dice`` then holds the device tensors (I, P, T, loss block).  ``seg_counts``: an int64 [3, K] device tensor that
        takes ``+= counts.sum(0)`` of this batch ({intersection, predicted, labelled} of the argmax of the same upsampled scores
        against ``labels`` as given, over the pixels the loss counts; ``BaseModelWithText.forward_loss`` has the details).
        ``accum``: the device block of a gradient-accumulation cycle (``ops.accum_add``): the head's [sum of losses, count] joins it,
        the backward leaves the gradient of the SUM of the pixel losses; not combinable with ``dice=``.
        ``focal=(gamma, poly_eps)``: the focal / poly-1 loss per counted pixel in place of the cross-entropy (FocalLoss's
        definition; ``BaseModelWithText.forward_loss`` has the details); keeps ``weight``, ``reduction``, ``ohem``, ``seg_counts`` and
        ``accum``, not combinable with ``dice=`` or ``label_smoothing``.
        ``sigmoid=(gamma, alpha, normalize)``: the sigmoid focal / sigmoid cross-entropy loss, summed over the classes of each
        counted pixel, in place of the cross-entropy (SigmoidFocalLoss's definition: 'mean' divides by a count of elements or of
        pixels, never a weight sum; ``BaseModelWithText.forward_loss`` has the details); keeps ``weight``, ``reduction``, ``ohem``,
        ``seg_counts`` and ``accum``, not combinable with ``dice=``, ``focal=`` or ``label_smoothing``."""
        if accum is not None and dice is not None:
            raise ValueError("lc2is_amd: accum= cannot be combined with dice= (the Dice statistics of micro-batches do not add)")
        sigmoid = fused_sigmoid_options(sigmoid, label_smoothing, dice, focal)
        focal = fused_focal_options(focal, label_smoothing, dice)
        opts = fused_loss_options(weight, label_smoothing, reduction)
        if ohem is not None:
            ohem = check_ohem(*ohem)
        dice = fused_dice_options(dice, opts, ohem)
        if seg_counts is not None:
            ops.check_seg_counts(seg_counts, text_embeddings.shape[1])
        wide_refuse("ScoreMapTail.loss", text_embeddings.shape[1], self.scale_factor, label_smoothing, ohem, dice, focal, sigmoid)
        require_cuda(visual_embeddings, "visual_embeddings")
        save = torch.is_grad_enabled() and (visual_embeddings.requires_grad or text_embeddings.requires_grad)
        if sigmoid is not None:
            return _ScoreFn.apply(visual_embeddings, text_embeddings, labels, self.scale_factor, ignore_index, save, opts, ohem, self,
                                  dice, seg_counts, accum, None, sigmoid)
        if focal is not None:
            return _ScoreFn.apply(visual_embeddings, text_embeddings, labels, self.scale_factor, ignore_index, save, opts, ohem, self,
                                  dice, seg_counts, accum, focal)
        if accum is None:
            return _ScoreFn.apply(visual_embeddings, text_embeddings, labels, self.scale_factor, ignore_index, save, opts, ohem, self,
                                  dice, seg_counts)
        return _ScoreFn.apply(visual_embeddings, text_embeddings, labels, self.scale_factor, ignore_index, save, opts, ohem, self, dice,
                              seg_counts, accum)

    @torch.no_grad()
    def predict(self, visual_embeddings: torch.Tensor, text_embeddings: torch.Tensor) -> torch.Tensor:
        """The class map of the score map, uint8 [B, S*h, S*w] (int16 past 192 classes): ``forward(visual, text).argmax(1)`` (exact
        ties to the lowest class) without writing the map — the argmax is taken in the fused head (``ops.head_upsample_argmax``,
        ``ops.head_upsample_argmax_wide``)."""
        require_cuda(visual_embeddings, "visual_embeddings")
        B, P, _ = visual_embeddings.shape
        K = text_embeddings.shape[1]
        h = int(round(P ** 0.5))
        scores, _ = _scores_lo(visual_embeddings, text_embeddings)
        argmax = ops.head_upsample_argmax_wide if K > ops.HEAD_CMAX else ops.head_upsample_argmax
        pred, _ = argmax(scores, None, B, h, h, K, self.scale_factor, ops.INTERP_BILINEAR, want_counts=False)
        return pred
