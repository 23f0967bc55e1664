"""``TextToPatch`` and the ``BaseModelWithText`` composition on MI355X.

Reference: model/text_patch.py:4-19, model/model.py:12-56 (the only caller of the hot path for BASELINE
configs 1-4) and the engine contract of engine.py:81-100 (``model(inputs)`` -> ``outputs_dict["outputs"]``).

Head algebra: bicubic x4 has taps summing to 1, so it commutes with the affine
``pixel_patch.visual`` and with the prototype matmul:
    logits = up4(dec_v) W_v^T + b_v) F_t^T  ==  up4( (dec_v W_v^T + b_v) F_t^T )
The HIP path evaluates the right-hand side: two small MFMA GEMMs at 32x32 resolution, then ONE fused kernel
that upsamples the 151 class scores, and (training) computes the cross-entropy and its gradient in the same
pass.  ``literal_order=True`` is not needed for parity (the tolerance is stated in tests/) and is not provided.
"""
from __future__ import annotations

from pathlib import Path

import torch
from torch import nn

from .. import ops
from .base import HipModule, grad_buf, linear_bwd_params, require_cuda, vec_grad
from .clip import ClipArch, ImageEncoderCLIP, TextEncoderCLIP, TextEncoderCLIPPooler
from .decoder import DecoderBlock, DecoderLayer
from .head_loss import HeadCriterion, fused_head_loss, head_criterion
from .head_loss import (fused_dice_options, fused_focal_options, fused_loss_options,   # noqa: F401  (the pieces of head_criterion:
                        fused_sigmoid_options, wide_refuse)                            # part of this module's surface)

_DATA = Path(__file__).resolve().parent.parent / "data"
KPAD = 192  # class dimension padded to a multiple of 64 (MFMA K-step of the dgrad product); past 192 classes: ops.class_pad(K)


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b through the bf16 MFMA GEMM; x fp32 [..., K]."""

    @staticmethod
    def forward(ctx, x, weight, bias, w16, w16T, save):
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1]).float().contiguous()
        x16 = ops.cast_bf16(x2)
        _, y, _ = ops.gemm_nt(x16, w16, bias, out_bf16=None, out_f32=True)
        if save:
            ctx.x16, ctx.weight, ctx.bias, ctx.w16T, ctx.lead = x16, weight, bias, w16T, lead
        return y.view(*lead, weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        g2 = gy.reshape(-1, gy.shape[-1]).float().contiguous()
        g16 = ops.cast_bf16(g2)
        linear_bwd_params(g16, ctx.x16, ctx.weight, ctx.bias)
        _, dx, _ = ops.gemm_nt(g16, ctx.w16T, None, out_bf16=None, out_f32=True)
        return dx.view(*ctx.lead, dx.shape[-1]), None, None, None, None, None


class TextToPatch(HipModule):
    """Drop-in for model/text_patch.py:4-19.  forward(img, text) -> (t_feature, v_feature) — text FIRST."""

    def __init__(self, img_in: int, text_in: int, out: int = 512) -> None:
        super().__init__()
        self.textual = nn.Linear(in_features=text_in, out_features=out)
        self.visual = nn.Linear(in_features=img_in, out_features=out)

    def _build_shadows(self, device):
        bf = dict(dtype=torch.bfloat16, device=device)
        t, v = self.textual.weight, self.visual.weight
        s = dict(wt=torch.empty(*t.shape, **bf), wtT=torch.empty(t.shape[1], t.shape[0], **bf),
                 wv=torch.empty(*v.shape, **bf), wvT=torch.empty(v.shape[1], v.shape[0], **bf))
        return s, [(t, s["wt"], s["wtT"]), (v, s["wv"], s["wvT"])]

    def forward(self, img: torch.Tensor, text: torch.Tensor):
        require_cuda(img, "img")
        sh = self._ensure_ready()
        save = torch.is_grad_enabled()
        t_feature = _LinearFn.apply(text, self.textual.weight, self.textual.bias, sh["wt"], sh["wtT"], save)
        v_feature = _LinearFn.apply(img, self.visual.weight, self.visual.bias, sh["wv"], sh["wvT"], save)
        return t_feature, v_feature


def head_scores_hi(scores, B: int, h: int, w: int, K: int, S: int, mode: int):
    """The materialised [B, K, S h, S w] map of low-resolution scores [B*h*w, ld].  Past 192 classes: contiguous 192-channel slices
    through the same kernel, concatenated (the reference composition of the wide head; the loss and prediction paths never form it)."""
    if K <= ops.HEAD_CMAX:
        return ops.head_upsample_ce(scores, None, B, h, w, K, S, mode, want_scores=True, want_loss=False)[2]
    outs = []
    for c0 in range(0, K, ops.HEAD_CMAX):
        n = min(ops.HEAD_CMAX, K - c0)
        part = scores[:, c0:c0 + (n + 63) // 64 * 64].contiguous()
        outs.append(ops.head_upsample_ce(part, None, B, h, w, n, S, mode, want_scores=True, want_loss=False)[2])
    return torch.cat(outs, dim=1)


def head_scores_hi_bwd(gout, B: int, h: int, w: int, K: int, S: int, mode: int, ld: int):
    """Gradient of head_scores_hi wrt the low-resolution scores, fp32 [B*h*w, ld] (zero padded columns)."""
    gout = gout.float()
    if K <= ops.HEAD_CMAX:
        return ops.upsample_bwd_nchw(gout.contiguous(), B, h, w, K, S, mode, ld)
    ds = torch.zeros(B * h * w, ld, dtype=torch.float32, device=gout.device)
    for c0 in range(0, K, ops.HEAD_CMAX):
        n = min(ops.HEAD_CMAX, K - c0)
        ds[:, c0:c0 + n] = ops.upsample_bwd_nchw(gout[:, c0:c0 + n].contiguous(), B, h, w, n, S, mode, (n + 63) // 64 * 64)[:, :n]
    return ds


class _HeadFn(torch.autograd.Function):
    """dec_v [B,P,C] (+ class prototypes) -> NCHW logits [B,K,4g,4g]  or, with labels, the mean CE loss."""

    @staticmethod
    def forward(ctx, dec, anchor, model, labels, save, ignore_index, crit=HeadCriterion(), seg_counts=None, accum=None):
        out, saved = model._head_fwd(dec, labels, save, ignore_index, crit, seg_counts, accum)
        ctx.model, ctx.saved = model, saved
        return out

    @staticmethod
    def backward(ctx, gout):
        ddec = ctx.model._head_bwd(gout, ctx.saved)
        ctx.saved = None
        return (ddec,) + (None,) * 8


class BaseModelWithText(HipModule):
    """Drop-in for model/model.py:12-56.

    ``forward(inputs)`` returns ``dict(outputs=logits [B,K,out,out])`` — the dict contract ``Engine`` indexes
    (engine.py:82,94,150); ``forward_tuple(inputs)`` returns the legacy
    ``(feature_t, feature_v, logits)`` of model/model.py:56; ``forward_loss(inputs, labels)`` is the fused
    training head (mean cross-entropy, identical to ``CrossEntropyLoss()(forward(inputs)["outputs"], labels)``).
    """

    def __init__(self, patch_size: int = 16, in_size: int = 224, out_size: int = 224, dropout: float = 0,
                 num_layers: int = 1, *, prototypes: torch.Tensor | str | None = None,
                 vision_arch: ClipArch | None = None, text_arch: ClipArch | None = None, nhead: int = 8,
                 dim_feedforward: int = 2048, out_dim: int = 512) -> None:
        super().__init__()
        self.patch_size, self.in_size, self.out_size = patch_size, in_size, out_size
        if out_size != 4 * (in_size // patch_size):
            raise ValueError("BaseModelWithText: out_size must be 4 * (in_size // patch_size) "
                             "(model/model.py:41-44 upsamples the patch grid by 4)")
        self.vision_encoder = ImageEncoderCLIP(in_size=in_size, patch_size=patch_size, arch=vision_arch)
        self.text_encoder = TextEncoderCLIP(patch_size=patch_size, arch=text_arch)
        if prototypes is None:
            prototypes = _DATA / "ade20k_prototypes.pt"  # model/model.py:22 (cwd-relative in the reference)
        if not isinstance(prototypes, torch.Tensor):
            prototypes = torch.load(prototypes, weights_only=True)
        self.class_prototypes = nn.Parameter(prototypes.detach().clone().float(), requires_grad=True)
        cv, ct = self.vision_encoder.hidden_size(), self.text_encoder.hidden_size()
        layer = DecoderLayer(d_model=cv, d_kv=ct, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                             batch_first=True, norm_first=True)
        self.vision_decoder = DecoderBlock(decoder_layer=layer, num_layers=num_layers)
        self.pixel_patch = TextToPatch(out=out_dim, img_in=cv, text_in=self.class_prototypes.shape[1])
        if self.class_prototypes.shape[0] > ops.HEAD_WIDE_CMAX:
            raise ValueError(f"BaseModelWithText: at most {ops.HEAD_WIDE_CMAX} classes are supported by the fused head "
                             f"({ops.HEAD_CMAX} by every criterion, more by the plain cross-entropy)")
        self.overlap_text = True     # text tower on a side stream (set False to serialise, e.g. under graph capture)
        self._text_stream = None

    # -- shadows owned by the composition: padded bf16 prototypes -------------------------------------------
    def _params_for_version(self):
        return [self.class_prototypes]

    def _grad_params(self):
        """What the head's backward writes: the prototypes and TextToPatch's two Linears (the towers and the decoder are
        modules of their own)."""
        return [self.class_prototypes, *self.pixel_patch.parameters()]

    def _build_shadows(self, device):
        K, Ct = self.class_prototypes.shape
        p16 = torch.zeros(ops.class_pad(K), Ct, dtype=torch.bfloat16, device=device)
        return dict(p16=p16, K=K), [(self.class_prototypes, p16[:K], None)]

    # -- head ------------------------------------------------------------------------------------------------
    def _head_scores(self, dec16, ready: bool = False):
        sh = self._sh if ready else self._ensure_ready()     # ready: the caller has just made the check (forward, forward_loss)
        pp = self.pixel_patch
        psh = pp._ensure_ready()
        ft16, _, _ = ops.gemm_nt(sh["p16"], psh["wt"], pp.textual.bias)            # [KPAD, out]
        fv16, _, _ = ops.gemm_nt(dec16, psh["wv"], pp.visual.bias)                  # [B*P, out]
        _, scores, _ = ops.gemm_nt(fv16, ft16, None, out_bf16=None, out_f32=True)   # [B*P, KPAD]
        return ft16, fv16, scores

    def _head_fwd(self, dec, labels, save, ignore_index, crit=HeadCriterion(), seg_counts=None, accum=None):
        B, P, C = dec.shape
        g = self.in_size // self.patch_size
        K = self.class_prototypes.shape[0]
        dec16 = ops.cast_bf16(dec.reshape(B * P, C).float().contiguous())
        ft16, fv16, scores = self._head_scores(dec16, ready=True)
        saved = dict(dec16=dec16, ft16=ft16, fv16=fv16, dims=(B, P, C, g, K), fused=None) if save else None
        if labels is None:
            return head_scores_hi(scores, B, g, g, K, 4, ops.INTERP_BICUBIC), saved
        loss, dlo, inv_count, dice_stats, ohem_sel = fused_head_loss(scores, labels, B, g, g, K, 4, ops.INTERP_BICUBIC, ignore_index,
                                                                     crit, save, seg_counts, accum)
        if dice_stats is not None:
            self.last_dice = dice_stats
        if ohem_sel is not None:
            self.last_ohem = ohem_sel
        if save:   # the 1/count of the mean is folded into the upstream-gradient multiply of _head_bwd
            saved.update(fused=dlo, inv_count=inv_count)
        return loss, saved

    def _head_bwd(self, gout, saved):
        B, P, C, g, K = saved["dims"]
        pp = self.pixel_patch
        psh, sh = pp._sh, self._sh
        if saved["fused"] is not None:
            ds = saved["fused"]   # d(sum of pixel losses)/d(scores); gout: scalar upstream gradient of the mean loss
            inv = saved["inv_count"]   # None: reduction='sum'
            if inv is None:
                ds16 = ops.cast_bf16(ds if gout is None else ds * gout)
            else:
                ds16 = ops.cast_bf16(ds * (inv if gout is None else gout * inv))
        else:
            ds = head_scores_hi_bwd(gout, B, g, g, K, 4, ops.INTERP_BICUBIC, ops.class_pad(K))
            ds16 = ops.cast_bf16(ds)
        ft16, fv16, dec16 = saved["ft16"], saved["fv16"], saved["dec16"]
        ftT = ops.transpose_bf16(ft16)                                   # [out, KPAD]
        dfv, _, _ = ops.gemm_nt(ds16, ftT, None)                         # [B*P, out]
        dft = ops.gemm_tn(ds16, fv16)                                    # [KPAD, out] fp32
        linear_bwd_params(dfv, dec16, pp.visual.weight, pp.visual.bias)
        _, ddec, _ = ops.gemm_nt(dfv, psh["wvT"], None, out_bf16=None, out_f32=True)
        dft16 = ops.cast_bf16(dft)
        linear_bwd_params(dft16, sh["p16"], pp.textual.weight, pp.textual.bias)
        if self.class_prototypes.requires_grad:
            _, dp, _ = ops.gemm_nt(dft16, psh["wtT"], None, out_bf16=None, out_f32=True)   # [KPAD, Ct]
            gp, acc = grad_buf(self.class_prototypes)
            if acc:
                gp.add_(dp[:K])
            else:
                gp.copy_(dp[:K])
        pp._grads_ready()
        self._grads_ready()
        return ddec.view(B, P, C)

    # -- composition -----------------------------------------------------------------------------------------
    def _decode(self, inputs):
        vision_inputs = {k: v for k, v in inputs.items() if k in ["pixel_values"]}
        text_inputs = {k: v for k, v in inputs.items() if k in ["input_ids", "attention_mask"]}
        if self.overlap_text and text_inputs["input_ids"].is_cuda:
            # The text tower is ~400 tiny launches (B*L = 512 tokens at config 2) that leave most of the 256 CUs idle:
            # it runs on a side HIP stream under the vision tower's large kernels (autograd replays its backward on
            # the same stream, again beside the vision backward).
            dev = text_inputs["input_ids"].device
            main = torch.cuda.current_stream(dev)
            if self._text_stream is None or self._text_stream.device != dev:
                # HIGH priority (round 5): HIP multiplexes streams onto a few hardware queues, and two streams on one queue run
                # in order.  Which queue a pool stream lands on depends on what else created streams before it — with a
                # process group on `nccl` the side stream of this class shared the main stream's queue and the tower ran
                # SERIALISED (34.0 instead of 30.7 ms per step, profiles/r05_dp_one_gpu.txt).  Priority levels have queues of
                # their own, so a high-priority stream never shares one with the (normal-priority) stream the vision tower is on;
                # its launches are tiny and few CUs wide.  LC2IS_TEXT_STREAM_PRIO=0: a normal-priority pool stream as before.
                prio = int(__import__("os").environ.get("LC2IS_TEXT_STREAM_PRIO", "-1"))
                self._text_stream = torch.cuda.Stream(dev, priority=prio)
            side = self._text_stream
            side.wait_stream(main)
            with torch.cuda.stream(side):
                for t in text_inputs.values():
                    t.record_stream(side)
                enc_t = self.text_encoder(**text_inputs)                                      # model.py:32
            enc_v = self.vision_encoder(**vision_inputs)                                      # model.py:35
            main.wait_stream(side)
            enc_t.record_stream(main)
        else:
            enc_t = self.text_encoder(**text_inputs)                                          # model.py:32
            enc_v = self.vision_encoder(**vision_inputs)                                      # model.py:35
        kpm = text_inputs["attention_mask"] != 1    # model.py:38 `torch.where(mask == 1, False, True)`: the same bool tensor in one launch instead of four
        return self.vision_decoder(tgt=enc_v, memory=enc_t, memory_key_padding_mask=kpm)

    def forward(self, inputs: dict) -> dict:
        dec_v = self._decode(inputs)
        self._ensure_ready()
        anchor, save = self._anchor_save(dec_v)
        logits = _HeadFn.apply(dec_v, anchor, self, None, save, -100)
        return dict(outputs=logits)

    def forward_loss(self, inputs: dict, labels: torch.Tensor, ignore_index: int = -100, *, weight=None,
                     label_smoothing: float = 0.0, reduction: str = "mean", ohem=None, dice=None,
                     seg_counts=None, accum=None, focal=None, sigmoid=None, pixel_weight=None, distill=None) -> torch.Tensor:
        """Cross-entropy of the model output against ``labels`` [B,out,out] — CE(engine.py:94) fused with the head; never
        materialises the fp32 logits.  ``weight`` / ``label_smoothing`` / ``reduction`` ('mean' or 'sum') as in
        nn.CrossEntropyLoss.  ``ohem=(thresh, min_kept per image)``: the loss over the hard pixels only, selected on the device
        (OhemCrossEntropyLoss's rule); ``self.last_ohem`` then holds (the labels the head saw, the device info block).
        ``dice=(ce_weight, dice_weight, smooth, present_only)``: ce_weight * mean CE + dice_weight * soft Dice over the batch
        (DiceCrossEntropyLoss's definition), not combinable with the other options; ``self.last_dice`` then holds the device
        tensors (I, P, T, loss block = [loss, CE mean, Dice, n_valid]).
        ``seg_counts``: an int64 [3, K] device tensor that takes ``+= counts.sum(0)`` of this batch — {intersection, predicted,
        labelled} of the argmax of the same upsampled scores against ``labels`` as given (under ``ohem=``: before relabelling), over
        the pixels the loss counts (``ops.head_upsample_argmax``; ``metrics.dataset_iou`` turns them into aAcc / mAcc / mIoU).  One
        more forward pass of the head and a small device add, no host read; loss and gradients are unchanged.  None: no launch.
        ``accum``: the fp64 [4] device block of a gradient-accumulation cycle (``ops.accum_add``; ``TrainStep(accumulate=N)``).  The
        head's [sum of losses, count] — after ``ohem=``, that of the relabelled call — is added to the block, the returned value is
        this batch's usual loss, and the backward writes the gradient of the SUM of the pixel losses whatever ``reduction`` says:
        the update that closes the cycle divides by the block's count.  Not combinable with ``dice=``.  None: no launch.
        ``focal=(gamma, poly_eps)``: the focal / poly-1 loss w_y ((1 - p_y)^gamma (-log p_y) + poly_eps (1 - p_y)) per counted
        pixel in place of the cross-entropy (FocalLoss's definition: 'mean' divides by the sum of w_y), one forward + backward
        launch of the head.  Keeps ``weight``, ``reduction``, ``seg_counts``, ``accum`` (a per-pixel loss: the sums add) and ``ohem``
        (the selection still ranks by the plain CE; the relabelled call is the focal one); not combinable with ``dice=`` or
        ``label_smoothing``.  None: the cross-entropy.
        ``sigmoid=(gamma, alpha, normalize)``: the sigmoid focal loss (gamma = 0, alpha None: binary cross-entropy with logits on
        one-hot targets) in place of the cross-entropy — per counted pixel the sum over the K classes of w_c a_t (1 - p_t)^gamma
        (-log p_t) with p = sigmoid(score), no softmax (SigmoidFocalLoss's definition), one forward + backward launch of the head.
        'mean' divides by a COUNT — counted pixels x K with normalize 'elements', counted pixels with 'pixels' — not by a weight sum:
        torch's and mmseg's rule for binary losses, deliberately different from the softmax losses above.  Keeps ``weight`` (on
        class c's binary term), ``reduction``, ``seg_counts``, ``accum`` and ``ohem`` (the selection still ranks by the plain softmax
        CE; the relabelled call is the sigmoid one); not combinable with ``dice=``, ``focal=`` or ``label_smoothing``
        (``ValueError`` before the towers run).  None: the softmax losses above.
        ``pixel_weight``: a contiguous fp32 device tensor of the labels' shape, finite and >= 0 (not checked: no host sync), not
        requiring grad — each counted pixel's cross-entropy is multiplied by its weight (pseudo-label quality or confidence weights,
        ``selftrain.PseudoLabeler``; boundary-weight maps), in one forward + backward launch of the head
        (``ops.head_upsample_ce_pw``).  The pixel's COUNT is not: 'mean' still divides by the sum of w_y over the counted pixels, so
        an all-ones weight is the plain loss and a per-image weight scales that image's loss (mmseg's ``weight_reduce_loss``) rather
        than cancelling; ``seg_counts`` and ``accum`` keep their meaning.  Keeps ``weight``, ``label_smoothing`` and ``reduction``;
        not combinable with ``ohem=``, ``dice=``, ``focal=`` or ``sigmoid=`` (``ValueError``), and limited to 192 classes
        (``NotImplementedError``).  None: no weight, the calls above.
        ``distill``: a ``head_loss.Distill(scores, weight, temperature, region, pixel_weight)`` — ADDS weight * the mean over the
        counted pixels of pw_i T^2 KL(softmax(teacher / T) || softmax(student / T)) on the upsampled scores to the loss of whatever
        criterion the other options choose (Hinton's distillation per pixel; the soft consistency of a mean teacher), in one more
        forward + backward launch of the head on the same low-resolution scores (``ops.head_upsample_kd``): neither logit map is
        formed.  ``scores`` are the teacher's ``head_scores(inputs)`` (this model under ``TrainStep.ema_weights()``, or another one
        with the same classes and patch grid), fp32 [B*g*g, class_pad(K)], no grad: nothing flows to the teacher.  ``region``
        'all': every pixel; 'labelled': the pixels ``labels`` counts (as given: before ``ohem=`` relabels).  The term has its own
        denominator, the number of pixels it counts, so it is not combinable with ``accum=`` and is limited to 192 classes
        (``NotImplementedError``); a bad weight, temperature, region or teacher tensor is a ``ValueError`` before the towers run.
        None: no term, the calls above."""
        rows = None if distill is None else inputs["pixel_values"].shape[0] * (self.in_size // self.patch_size) ** 2
        crit = head_criterion("BaseModelWithText.forward_loss", weight=weight, label_smoothing=label_smoothing, reduction=reduction,
                              ohem=ohem, dice=dice, focal=focal, sigmoid=sigmoid, seg_counts=seg_counts, accum=accum,
                              n_classes=lambda: self.class_prototypes.shape[0], scale=4, pixel_weight=pixel_weight, distill=distill,
                              rows=rows, device=None if distill is None else self.class_prototypes.device)
        dec_v = self._decode(inputs)
        self._ensure_ready()
        anchor, save = self._anchor_save(dec_v)
        return _HeadFn.apply(dec_v, anchor, self, labels, save, ignore_index, crit, seg_counts, accum)

    @torch.no_grad()
    def predict(self, inputs: dict) -> torch.Tensor:
        """The class map of the model output, uint8 [B, out, out] (int16 past 192 classes): ``forward(inputs)["outputs"].argmax(1)``
        (exact ties to the lowest class) without forming the logits — the argmax is taken in the fused head
        (``ops.head_upsample_argmax``, ``ops.head_upsample_argmax_wide``)."""
        dec_v = self._decode(inputs)
        B, P, C = dec_v.shape
        g = self.in_size // self.patch_size
        K = self.class_prototypes.shape[0]
        dec16 = ops.cast_bf16(dec_v.reshape(B * P, C).float().contiguous())
        _, _, scores = self._head_scores(dec16)
        argmax = ops.head_upsample_argmax_wide if K > ops.HEAD_CMAX else ops.head_upsample_argmax
        pred, _ = argmax(scores, None, B, g, g, K, 4, ops.INTERP_BICUBIC, want_counts=False)
        return pred

    @torch.no_grad()
    def head_scores(self, inputs: dict) -> torch.Tensor:
        """The low-resolution class scores of the model output, fp32 [B*g*g, class_pad(K)] (g = in_size // patch_size; channels at
        and past K are padding): what the fused head upsamples, taken under no_grad as ``predict`` takes them.  This is the layout
        ``forward_loss(distill=Distill(scores, ...))`` consumes — the teacher's side of a distillation step."""
        dec_v = self._decode(inputs)
        B, P, C = dec_v.shape
        dec16 = ops.cast_bf16(dec_v.reshape(B * P, C).float().contiguous())
        return self._head_scores(dec16)[2]

    @torch.no_grad()
    def predict_confidence(self, inputs: dict, thresh=None, ignore_index: int = -100):
        """``(pred uint8 [B, out, out], conf fp32 [B, out, out])``: the class map of ``predict`` and its softmax probability,
        ``forward(inputs)["outputs"].softmax(1).max(1)``, without forming the logits (``ops.head_upsample_conf``).  With ``thresh``
        (a number in [0, 1]): ``(pred, conf, pseudo, counts)`` — ``pseudo`` int64 = the class where conf >= thresh, else
        ``ignore_index``; ``counts`` int32 [B, 2] = per image {pixels with conf >= thresh, pixels of the image}.  No host read."""
        if thresh is not None:
            thresh = ops.conf_thresh(thresh)
        K = self.class_prototypes.shape[0]
        if K > ops.HEAD_CMAX:
            raise NotImplementedError(f"lc2is_amd BaseModelWithText.predict_confidence: limited to {ops.HEAD_CMAX} classes, got {K} "
                                      "(the chunked head past them gives the class map only: predict)")
        dec_v = self._decode(inputs)
        B, P, C = dec_v.shape
        g = self.in_size // self.patch_size
        dec16 = ops.cast_bf16(dec_v.reshape(B * P, C).float().contiguous())
        _, _, scores = self._head_scores(dec16)
        out = ops.head_upsample_conf(scores, B, g, g, K, 4, ops.INTERP_BICUBIC, thresh=thresh, ignore_index=ignore_index,
                                     want_counts=thresh is not None)
        return out[:2] if thresh is None else out

    @torch.no_grad()
    def forward_tuple(self, inputs: dict):
        """Legacy return of model/model.py:56: (feature_t [K,out], feature_v [B,out_size²,out], logits)."""
        dec_v = self._decode(inputs)
        B, P, C = dec_v.shape
        g = self.in_size // self.patch_size
        K = self.class_prototypes.shape[0]
        dec16 = ops.cast_bf16(dec_v.reshape(B * P, C).float().contiguous())
        ft16, fv16, scores = self._head_scores(dec16)
        logits = head_scores_hi(scores, B, g, g, K, 4, ops.INTERP_BICUBIC)
        fv = fv16.float()
        outs = []
        for c0 in range(0, fv.shape[1], KPAD):  # upsample the visual features 192 channels at a time
            c1 = min(c0 + KPAD, fv.shape[1])
            ld = (c1 - c0 + 63) // 64 * 64
            chunk = torch.zeros(B * P, ld, dtype=torch.float32, device=fv.device)
            chunk[:, :c1 - c0] = fv[:, c0:c1]
            _, _, hi = ops.head_upsample_ce(chunk, None, B, g, g, c1 - c0, 4, ops.INTERP_BICUBIC, want_scores=True,
                                            want_loss=False)
            outs.append(hi)
        feature_v = torch.cat(outs, dim=1).flatten(2).transpose(1, 2).contiguous()
        return ft16[:K].float(), feature_v, logits


class _ContrastiveHeadFn(torch.autograd.Function):
    """(enc_v [B,P,Cv], enc_t [Nt,Ct]) -> logits [B, (4g)^2, Nt] through the commuted head (scores at the patch grid, then
    ONE bicubic x4 of the Nt class channels)."""

    @staticmethod
    def forward(ctx, enc_v, enc_t, anchor, model, save):
        logits, saved = model._head_fwd(enc_v, enc_t, save)
        ctx.model, ctx.saved = model, saved
        return logits

    @staticmethod
    def backward(ctx, gout):
        dv, dt = ctx.model._head_bwd(gout, ctx.saved)
        ctx.saved = None
        return dv, dt, None, None, None


class ContrastiveModel(HipModule):
    """Drop-in for model/model.py:58-103: CLIP vision tower, POOLED CLIP text tower (one embedding per prompt), TextToPatch,
    ``logits[b, pixel, prompt] = feature_v @ feature_t^T`` on the bicubically x4-upsampled patch grid.

    ``forward(inputs) -> (feature_t, feature_v, logits)`` like the reference; ``feature_v`` ([B, out^2, out] — the tensor the
    commuted head exists to avoid) is only materialised when ``return_features`` is True (default False -> ``None``).
    Trains with ``lc2is_amd.nn.ContrastiveLoss`` (model/loss.py:39-64, which hard-codes 151 prompts)."""

    def __init__(self, patch_size: int = 16, in_size: int = 224, out_size: int = 224, dropout: float = 0, num_layers: int = 1,
                 *, vision_arch: ClipArch | None = None, text_arch: ClipArch | None = None, out_dim: int = 512) -> None:
        super().__init__()
        self.patch_size, self.in_size, self.out_size = patch_size, in_size, out_size
        if out_size != 4 * (in_size // patch_size):
            raise ValueError("ContrastiveModel: out_size must be 4 * (in_size // patch_size) (model/model.py:83-86)")
        self.vision_encoder = ImageEncoderCLIP(in_size=in_size, patch_size=patch_size, arch=vision_arch)
        self.text_encoder = TextEncoderCLIPPooler(patch_size=patch_size, arch=text_arch)
        self.pixel_patch = TextToPatch(out=out_dim, img_in=self.vision_encoder.hidden_size(),
                                       text_in=self.text_encoder.hidden_size())
        self.return_features = False

    def _params_for_version(self):
        return []

    def _head_fwd(self, enc_v, enc_t, save):
        B, P, C = enc_v.shape
        g = self.in_size // self.patch_size
        Nt, Ct = enc_t.shape
        if Nt > KPAD:
            raise ValueError(f"ContrastiveModel: at most {KPAD} prompts are supported by the fused head")
        pp = self.pixel_patch
        psh = pp._ensure_ready()
        dec16 = ops.cast_bf16(enc_v.reshape(B * P, C).float().contiguous())
        t16 = torch.zeros(KPAD, Ct, dtype=torch.bfloat16, device=enc_v.device)
        ops.cast_bf16(enc_t.float().contiguous(), t16[:Nt])
        ft16, _, _ = ops.gemm_nt(t16, psh["wt"], pp.textual.bias)                   # [KPAD, out]
        fv16, _, _ = ops.gemm_nt(dec16, psh["wv"], pp.visual.bias)                  # [B*P, out]
        _, scores, _ = ops.gemm_nt(fv16, ft16, None, out_bf16=None, out_f32=True)   # [B*P, KPAD]
        _, _, hi = ops.head_upsample_ce(scores, None, B, g, g, Nt, 4, ops.INTERP_BICUBIC, want_scores=True, want_loss=False)
        logits = hi.flatten(2).transpose(1, 2)                                       # [B, (4g)^2, Nt] (view of NCHW scores)
        saved = dict(dec16=dec16, t16=t16, ft16=ft16, fv16=fv16, dims=(B, P, C, g, Nt)) if save else None
        return logits, saved

    def _head_bwd(self, gout, saved):
        B, P, C, g, Nt = saved["dims"]
        pp = self.pixel_patch
        psh = pp._sh
        gn = gout.transpose(1, 2).reshape(B, Nt, 4 * g, 4 * g).float().contiguous()
        ds16 = ops.cast_bf16(ops.upsample_bwd_nchw(gn, B, g, g, Nt, 4, ops.INTERP_BICUBIC, KPAD))
        ft16, fv16, dec16, t16 = saved["ft16"], saved["fv16"], saved["dec16"], saved["t16"]
        dfv, _, _ = ops.gemm_nt(ds16, ops.transpose_bf16(ft16), None)               # [B*P, out]
        dft16 = ops.cast_bf16(ops.gemm_tn(ds16, fv16))                               # [KPAD, out]
        linear_bwd_params(dfv, dec16, pp.visual.weight, pp.visual.bias)
        _, dv, _ = ops.gemm_nt(dfv, psh["wvT"], None, out_bf16=None, out_f32=True)
        linear_bwd_params(dft16[:Nt], t16[:Nt], pp.textual.weight, pp.textual.bias)
        _, dt, _ = ops.gemm_nt(dft16, psh["wtT"], None, out_bf16=None, out_f32=True)   # [KPAD, Ct]
        pp._grads_ready()
        return dv.view(B, P, C), dt[:Nt].contiguous()

    def forward(self, inputs: dict):
        vision_inputs = {k: v for k, v in inputs.items() if k in ["pixel_values"]}
        text_inputs = {k: v for k, v in inputs.items() if k in ["input_ids", "attention_mask"]}
        enc_t = self.text_encoder(**text_inputs)                                                # model.py:77
        enc_v = self.vision_encoder(**vision_inputs)                                            # model.py:80
        require_cuda(enc_v, "pixel_values")
        self.pixel_patch._ensure_ready()
        anchor, save = self.pixel_patch._anchor_save(enc_v, enc_t)     # the head's own parameters are TextToPatch's
        logits = _ContrastiveHeadFn.apply(enc_v, enc_t, anchor, self, save)
        feature_t = feature_v = None
        if self.return_features:
            with torch.no_grad():
                feature_t, feature_v = self._features(enc_v, enc_t)
        return feature_t, feature_v, logits

    def _features(self, enc_v, enc_t):
        B, P, C = enc_v.shape
        g = self.in_size // self.patch_size
        pp = self.pixel_patch
        psh = pp._ensure_ready()
        ft16, _, _ = ops.gemm_nt(ops.cast_bf16(enc_t.float().contiguous()), psh["wt"], pp.textual.bias)
        fv16, _, _ = ops.gemm_nt(ops.cast_bf16(enc_v.reshape(B * P, C).float().contiguous()), psh["wv"], pp.visual.bias)
        fv = fv16.float()
        outs = []
        for c0 in range(0, fv.shape[1], KPAD):   # upsample the visual features 192 channels at a time
            c1 = min(c0 + KPAD, fv.shape[1])
            ld = (c1 - c0 + 63) // 64 * 64
            chunk = torch.zeros(B * P, ld, dtype=torch.float32, device=fv.device)
            chunk[:, :c1 - c0] = fv[:, c0:c1]
            _, _, hi = ops.head_upsample_ce(chunk, None, B, g, g, c1 - c0, 4, ops.INTERP_BICUBIC, want_scores=True, want_loss=False)
            outs.append(hi)
        return ft16.float(), torch.cat(outs, dim=1).flatten(2).transpose(1, 2).contiguous()
