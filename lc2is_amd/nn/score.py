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
from .head_loss import HeadCriterion, fused_head_loss, head_criterion
from .model import head_scores_hi, head_scores_hi_bwd

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
    def forward(ctx, visual, text, labels, scale, ignore_index, save, crit=HeadCriterion(), owner=None, seg_counts=None, accum=None):
        B, P, C = visual.shape
        K = text.shape[1]
        h = int(round(P ** 0.5))
        scores, sv = _scores_lo(visual, text)
        ctx.sv, ctx.fused, ctx.meta = (sv if save else None), None, (B, h, K, scale)
        if labels is None:
            return head_scores_hi(scores, B, h, h, K, scale, ops.INTERP_BILINEAR)
        # plain_n: this site's plain cross-entropy has always launched with grad_scale 1/n and rescaled by n/count afterwards
        loss, dlo, mul, dice_stats, ohem_sel = fused_head_loss(scores, labels, B, h, h, K, scale, ops.INTERP_BILINEAR, ignore_index,
                                                               crit, save, seg_counts, accum,
                                                               plain_n=float(B * h * scale * h * scale))
        if dice_stats is not None:
            owner.last_dice = dice_stats
        if ohem_sel is not None:
            owner.last_ohem = ohem_sel
        if mul is not None:   # the 1/count of the mean goes into the saved gradient here: the backward is one multiply by gout
            dlo.mul_(mul)
        ctx.fused = dlo
        return loss

    @staticmethod
    def backward(ctx, gout):
        B, h, K, scale = ctx.meta
        if ctx.fused is not None:
            ds = ctx.fused * gout
        else:
            ds = head_scores_hi_bwd(gout, B, h, h, K, scale, ops.INTERP_BILINEAR, ops.class_pad(K))
        dv, dt = _scores_bwd(ds, ctx.sv)
        ctx.sv = ctx.fused = None
        return (dv, dt) + (None,) * 8


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
             ohem=None, dice=None, seg_counts=None, accum=None, focal=None, sigmoid=None, pixel_weight=None,
             distill=None) -> torch.Tensor:
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
        ``seg_counts`` and ``accum``, not combinable with ``dice=``, ``focal=`` or ``label_smoothing``.
        ``pixel_weight``: a contiguous fp32 device tensor of the labels' shape (finite, >= 0, no grad) that multiplies each counted
        pixel's cross-entropy but not its count — 'mean' still divides by the sum of w_y (``BaseModelWithText.forward_loss`` has the
        details); keeps ``weight``, ``label_smoothing``, ``reduction``, ``seg_counts`` and ``accum``, not combinable with ``ohem=``,
        ``dice=``, ``focal=`` or ``sigmoid=``, limited to 192 classes.
        ``distill``: a ``head_loss.Distill(scores, weight, temperature, region, pixel_weight)`` — adds weight * the mean per-pixel
        T^2 KL(teacher || student) of the upsampled scores to the loss of whatever criterion is chosen; ``scores`` are a teacher's
        ``scores_lo(visual, text)``, fp32 [B*h*w, class_pad(K)], no grad (``BaseModelWithText.forward_loss`` has the details).  Not
        combinable with ``accum=``, limited to 192 classes."""
        B, P = visual_embeddings.shape[0], visual_embeddings.shape[1]
        crit = head_criterion("ScoreMapTail.loss", weight=weight, label_smoothing=label_smoothing, reduction=reduction, ohem=ohem,
                              dice=dice, focal=focal, sigmoid=sigmoid, seg_counts=seg_counts, accum=accum,
                              n_classes=lambda: text_embeddings.shape[1], scale=self.scale_factor, pixel_weight=pixel_weight,
                              distill=distill, rows=B * P, device=visual_embeddings.device)
        require_cuda(visual_embeddings, "visual_embeddings")
        save = torch.is_grad_enabled() and (visual_embeddings.requires_grad or text_embeddings.requires_grad)
        return _ScoreFn.apply(visual_embeddings, text_embeddings, labels, self.scale_factor, ignore_index, save, crit, self, seg_counts,
                              accum)

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

    @torch.no_grad()
    def scores_lo(self, visual_embeddings: torch.Tensor, text_embeddings: torch.Tensor) -> torch.Tensor:
        """The low-resolution class scores of the score map, fp32 [B*h*w, class_pad(K)] (channels at and past K are padding), under
        no_grad: what ``loss(distill=Distill(scores, ...))`` consumes as the teacher's side of a distillation step."""
        require_cuda(visual_embeddings, "visual_embeddings")
        return _scores_lo(visual_embeddings, text_embeddings)[0]

    @torch.no_grad()
    def predict_confidence(self, visual_embeddings: torch.Tensor, text_embeddings: torch.Tensor, thresh=None,
                           ignore_index: int = -100):
        """``(pred, conf)``: the class map of ``predict`` and its softmax probability ``forward(visual, text).softmax(1).max(1)``,
        fp32 [B, S*h, S*w], without writing the map (``ops.head_upsample_conf``).  With ``thresh``: ``(pred, conf, pseudo, counts)``
        as ``BaseModelWithText.predict_confidence``.  Limited to 192 classes."""
        if thresh is not None:
            thresh = ops.conf_thresh(thresh)
        K = text_embeddings.shape[1]
        if K > ops.HEAD_CMAX:
            raise NotImplementedError(f"lc2is_amd ScoreMapTail.predict_confidence: limited to {ops.HEAD_CMAX} classes, got {K} "
                                      "(the chunked head past them gives the class map only: predict)")
        require_cuda(visual_embeddings, "visual_embeddings")
        B, P, _ = visual_embeddings.shape
        h = int(round(P ** 0.5))
        scores, _ = _scores_lo(visual_embeddings, text_embeddings)
        out = ops.head_upsample_conf(scores, B, h, h, K, self.scale_factor, ops.INTERP_BILINEAR, thresh=thresh,
                                     ignore_index=ignore_index, want_counts=thresh is not None)
        return out[:2] if thresh is None else out
