"""Thin tensor-level wrappers over the C ABI (``include/lc2is_hip.h``).

Each function validates dtype / device / layout (raising ``RuntimeError`` like the reference's torch calls
would), takes raw device pointers + leading dimensions from the tensors and launches on the caller's
current HIP stream.  Outputs and workspaces are allocated here with ``torch.empty`` (PyTorch is the
allocator, nothing else).  There is no CPU path: a non-CUDA tensor is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib

ACT_NONE, ACT_QUICK_GELU, ACT_RELU, ACT_DQUICK_GELU, ACT_DRELU, ACT_QUICK_GELU_GRAD, ACT_MUL_AUX = 0, 1, 2, 3, 4, 5, 6
ACT_GELU_ERF, ACT_DGELU_ERF, ACT_ADD_AUX = 7, 8, 9

_P, _I, _F, _Z, _L, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_long, C.c_ulonglong
_ARGTYPES = {
    "lc2is_gemm_nt_bf16": [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P],
    "lc2is_gemm_nt_plan": [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I],
    "lc2is_gemm_nt_ln_xchg_bytes": [_I, _I],
    "lc2is_gemm_nt_ln_bf16": [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _F, _P, _I, _P, _P, _P, _Z, _I, _I, _I, _P],
    "lc2is_gemm_nt_bf16_batched": [_P, _I, _L, _P, _I, _L, _P, _I, _L, _P, _I, _L, _I, _I, _I, _I, _P],
    "lc2is_transpose_bf16_batched": [_P, _I, _L, _P, _I, _L, _I, _I, _I, _P],
    "lc2is_gemm_tn_workspace_bytes": [_I, _I, _I],
    "lc2is_gemm_tn_bf16": [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _Z, _P],
    "lc2is_gemm_tn_plan": [_I, _I, _I, _P],
    "lc2is_gemm_tn_grouped_plan": [_P, _I, _P, _P, _I],
    "lc2is_colsum_workspace_bytes": [_I, _I],
    "lc2is_colsum_bf16": [_P, _I, _P, _I, _I, _I, _P, _Z, _P],
    "lc2is_layernorm_fwd": [_P, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _F, _P],
    "lc2is_layernorm_bwd_partials": [_I, _I],
    "lc2is_ln_partials_reduce": [_P, _I, _P],
    "lc2is_layernorm_bwd_workspace_bytes": [_I, _I],
    "lc2is_layernorm_bwd": [_P, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I,
                            _P, _Z, _P],
    "lc2is_attention_fwd": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P],
    "lc2is_attention_bwd": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P,
                            _I, _I, _I, _I, _I, _F, _I, _P],
    "lc2is_attention_fwd_dropout": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _I, _F, _U64, _P],
    "lc2is_attention_bwd_dropout": [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P,
                                    _I, _I, _I, _I, _I, _F, _I, _F, _U64, _P],
    "lc2is_dropout_rows_f32": [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _F, _U64, _P],
    "lc2is_dropout_rows_bf16": [_P, _I, _P, _I, _I, _I, _F, _U64, _P],
    "lc2is_dropout_mask": [_P, _L, _I, _F, _U64, _P],
    "lc2is_shadow_refresh": [_P, _I, _I, _P],
    "lc2is_set_cu_budget": [_I],
    "lc2is_get_cu_budget": [],
    "lc2is_cast_f32_bf16": [_P, _I, _P, _I, _I, _I, _P],
    "lc2is_transpose_bf16": [_P, _I, _P, _I, _I, _I, _P],
    "lc2is_patchify": [_P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_vit_embed_fwd": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P],
    "lc2is_vit_embed_bwd": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_text_embed_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_text_embed_bwd": [_P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_rows_copy_bf16": [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_rows_copy_f32": [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_sgd_step": [_P, _P, _P, _Z, _F, _F, _F, _F, _P],
    "lc2is_adamw_step": [_P, _P, _P, _P, _Z, _F, _F, _F, _F, _F, _I, _F, _P],
    "lc2is_grad_sumsq_blocks": [_Z],
    "lc2is_grad_sumsq_workspace_bytes": [_Z],
    "lc2is_grad_sumsq": [_P, _Z, _P, _Z, _P],
    "lc2is_optim_ctrl_update": [_P, _P, _P, _I, _P, _I, _F, _F, _I, _F, _F, _P],
    "lc2is_accum_add": [_P, _P, _P],
    "lc2is_optim_ctrl_update_accum": [_P, _P, _I, _P, _P, _I, _P, _I, _F, _F, _I, _F, _F, _P],
    "lc2is_sgd_step_ctrl": [_P, _P, _P, _Z, _P, _F, _F, _I, _P],
    "lc2is_adamw_step_ctrl": [_P, _P, _P, _P, _Z, _P, _F, _F, _F, _F, _I, _P],
    "lc2is_sgd_step_groups": [_P, _P, _P, _Z, _P, _P, _P, _I, _F, _I, _P],
    "lc2is_adamw_step_groups": [_P, _P, _P, _P, _Z, _P, _P, _P, _I, _F, _F, _F, _I, _P],
    "lc2is_ema_update_ctrl": [_P, _P, _Z, _P, _F, _I, _I, _I, _P],
    "lc2is_swap_f32": [_P, _P, _Z, _P],
    "lc2is_head_upsample_ce_workspace_bytes": [_I, _I, _I, _I, _I, _I, _I],
    "lc2is_head_upsample_ce": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_long, _F, _P, _Z, _P],
    "lc2is_ce_nchw_fwd": [_P, _P, _P, _P, _I, _I, C.c_long, C.c_long, _P],
    "lc2is_ce_nchw_bwd": [_P, _P, _P, _P, _F, _P, _I, _I, C.c_long, C.c_long, _P],
    "lc2is_head_upsample_ce_opts": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_long, _F, _P, _F, _P, _Z, _P],
    "lc2is_ce_nchw_fwd_opts": [_P, _P, _P, _P, _P, _I, _I, C.c_long, C.c_long, _P, _F, _P],
    "lc2is_ce_nchw_fwd_workspace_bytes": [_I, C.c_long],
    "lc2is_ce_nchw_fwd_ordered": [_P, _P, _P, _P, _P, _I, _I, C.c_long, C.c_long, _P, _F, _P, _Z, _P],
    "lc2is_ce_nchw_bwd_opts": [_P, _P, _P, _P, _F, _P, _P, _I, _I, C.c_long, C.c_long, _P, _F, _P],
    "lc2is_upsample_bwd_nchw": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "lc2is_head_upsample_px": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _L, _P],
    "lc2is_head_upsample_argmax_workspace_bytes": [_I, _I, _I, _I, _I, _I],
    "lc2is_head_upsample_argmax": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _P, _Z, _P],
    "lc2is_ohem_select_workspace_bytes": [_L],
    "lc2is_ohem_select": [_P, _P, _P, _L, _I, _L, _F, _L, _P, _P, _Z, _P],
    "lc2is_head_upsample_ce_dice_workspace_bytes": [_I, _I, _I, _I, _I, _I, _I],
    "lc2is_head_upsample_ce_dice": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _F, _F, _F, _I, _F, _P, _Z, _P],
    "lc2is_ce_dice_nchw_workspace_bytes": [_I, _I, _L],
    "lc2is_ce_dice_nchw_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _L, _L, _F, _F, _F, _I, _P, _Z, _P],
    "lc2is_ce_dice_nchw_bwd": [_P, _P, _P, _P, _P, _F, _P, _I, _I, _L, _L, _P],
    "lc2is_head_upsample_focal": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _F, _P, _F, _F, _P, _Z, _P],
    "lc2is_focal_nchw_fwd": [_P, _P, _P, _P, _P, _I, _I, _L, _L, _P, _F, _F, _P, _Z, _P],
    "lc2is_focal_nchw_bwd": [_P, _P, _P, _P, _F, _P, _P, _I, _I, _L, _L, _P, _F, _F, _P],
    "lc2is_head_upsample_sigmoid": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _F, _P, _F, _F, _F, _P, _Z, _P],
    "lc2is_sigmoid_focal_nchw_fwd": [_P, _P, _P, _P, _I, _I, _L, _L, _P, _F, _F, _F, _P, _Z, _P],
    "lc2is_sigmoid_focal_nchw_bwd": [_P, _P, _P, _F, _P, _P, _I, _I, _L, _L, _P, _F, _F, _F, _P],
    "lc2is_head_upsample_ce_wide_workspace_bytes": [_I, _I, _I, _I, _I, _I, _I, _I],
    "lc2is_head_upsample_ce_wide": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _F, _P, _P, _Z, _P],
    "lc2is_head_upsample_argmax_wide_workspace_bytes": [_I, _I, _I, _I, _I, _I],
    "lc2is_head_upsample_argmax_wide": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _P, _Z, _P],
    "lc2is_head_upsample_conf_workspace_bytes": [_I, _I, _I, _I, _I, _I],
    "lc2is_head_upsample_conf": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _L, _P, _Z, _P],
    "lc2is_head_upsample_ce_pw": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _F, _P, _F, _P, _Z, _P],
    "lc2is_head_upsample_kd": [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _F, _F, _P, _Z, _P],
    "lc2is_bilinear_up_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_bilinear_up_bwd": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "lc2is_sr_gather": [_P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_sr_scatter_add_f32": [_P, _P, _I, _I, _I, _I, _P],
    "lc2is_l2norm_fwd": [_P, _P, _P, _P, _I, _I, _F, _P],
    "lc2is_l2norm_bwd": [_P, _P, _P, _P, _I, _I, _F, _P],
    "lc2is_add_n": [_P, _P, _P, _P, _P, _P, _Z, _P],
    "lc2is_rows_ce": [_P, _P, _P, _P, _P, _F, _I, _I, _I, _P],
    "lc2is_cols_ce": [_P, _P, _P, _P, _F, _I, _I, _I, _I, _P],
    "lc2is_npair": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "lc2is_miou_counts": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lc2is_resize_argmax_workspace_bytes": [_L, _I],
    "lc2is_resize_argmax": [_P, _I, _I, _I, _I, _I, _P, _L, _L, _P, _I, _P, _P, _P, _Z, _P],
    "lc2is_resize_argmax_windows": [_P, _I, _I, _I, _I, _I, _P, _I, _P, _L, _L, _L, _P, _I, _I, _P, _P, _P, _Z, _P],
    "lc2is_resize_argmax_multiscale": [_P, _I, _I, _I, _I, _I, _P, _I, _P, _L, _P, _L, _L, _L, _P, _I, _I, _I, _P, _P, _P, _Z, _P],
    "lc2is_resize_argmax_wide_workspace_bytes": [_L, _I],
    "lc2is_resize_argmax_wide": [_P, _I, _I, _I, _I, _I, _P, _L, _L, _P, _I, _P, _P, _P, _Z, _P],
    "lc2is_resize_argmax_windows_wide": [_P, _I, _I, _I, _I, _I, _P, _I, _P, _L, _L, _L, _P, _I, _I, _P, _P, _P, _Z, _P],
    "lc2is_resize_argmax_multiscale_wide": [_P, _I, _I, _I, _I, _I, _P, _I, _P, _L, _P, _L, _L, _L, _P, _I, _I, _I, _P, _P, _P, _Z,
                                            _P],
    "lc2is_npair_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "lc2is_gemm_tn_grouped_workspace_bytes": [_P, _I],
    "lc2is_gemm_tn_grouped": [_P, _I, _P, _Z, _P],
    "lc2is_release_captured_tables": [],
    "lc2is_captured_tables_mark": [],
    "lc2is_release_captured_tables_range": [_I, _I],
    "lc2is_rows_gather": [_P, _I, _I, _P, _I, _I, _P, _P, _I, _I, _I, _P],
    "lc2is_resample_u8": [_P, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P],
    "lc2is_gather2d_u8": [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P],
    "lc2is_crop_lut": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "lc2is_aug_params": [_P, _P, _I, _P, _P, _L, _P, _P, _P],
    "lc2is_aug_apply": [_P, _Z, _P, _Z, _P, _L, _P, _P, _I, _I, _I, _P, _L, _P, _P, _P],
    "lc2is_aug_crop_select": [_P, _Z, _P, _L, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "lc2is_label_histogram": [_P, _Z, _P, _L, _P, _I, _P, _P],
    "lc2is_mix_select": [_P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _P],
    "lc2is_mix_apply": [_P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P],
    "lc2is_strong_params": [_P, _I, _P, _P, _P, _P],
    "lc2is_strong_apply": [_P, _P, _P, _I, _I, _P, _P],
    "lc2is_geo_params": [_P, _I, _P, _P, _P, _P],
    "lc2is_geo_apply": [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    "lc2is_geo_scores": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "lc2is_swin_attn_fwd": [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P],
    "lc2is_swin_bias_table_grad": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "lc2is_swin_attn_bwd_workspace_bytes": [_I, _I, _I],
    "lc2is_swin_attn_bwd": [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F,
                            _P, _Z, _P],
}
_bound = {}


def _fn(name: str):
    f = _bound.get(name)
    if f is None:
        f = getattr(_lib.load(), name)
        if name in _ARGTYPES:
            f.argtypes = _ARGTYPES[name]
        if name.endswith("_bytes"):
            f.restype = C.c_size_t
        _bound[name] = f
    return f


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor | None, dtype, name: str, ndim: int | None = 2):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"lc2is_amd: {name} must be a CUDA(HIP) tensor; there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"lc2is_amd: {name} must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"lc2is_amd: {name} must be {ndim}-D, got shape {tuple(t.shape)}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise RuntimeError(f"lc2is_amd: {name} must have unit stride in its last dimension")


def _dims(who: str, t: torch.Tensor, name: str, ndim: int = 2, dtype=None):
    """The shape of an operand that DEFINES sizes of the call.  With ``dtype``: the call's first operand, which also gives the device
    every other operand is held to — it has to be on the GPU and passes everything _chk_op asks of rows (its shape being its own)."""
    if t.dim() == ndim:
        if dtype is None:
            return t.shape
        if t.is_cuda and t.dtype is dtype:
            st = t.stride()
            if st[-1] == 1 and t.data_ptr() % (8 if dtype is torch.bfloat16 and st[-2] % 8 else 16) == 0:
                return t.shape
    if dtype is not None and not t.is_cuda:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be a CUDA(HIP) tensor; there is no CPU path")
    if t.dim() != ndim:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be {ndim}-D, got shape {tuple(t.shape)}")
    _chk_op(who, t, name, dtype, t.shape, t.device)      # (raises: names the rule)
    raise AssertionError("unreachable")


def _chk_op(who: str, t: torch.Tensor | None, name: str, dtype, shape, dev, vec: int = 0):
    """One operand of a dense hot-path launcher.  The kernels index every tensor by the call's integers alone and issue 8- and
    16-byte accesses, so a tensor on another device, of another dtype or shape, or with a base below the alignment rule of
    include/lc2is_hip.h is refused here, before any launch.  ``vec`` = 0: rows with a leading dimension (unit inner stride;
    16-byte base, 8 for bf16 rows whose ld is only a multiple of 4).  ``vec`` > 0: a tensor the kernel takes no ld for — it must be
    contiguous with a ``vec``-byte base (16 where the kernel reads it as float4, else 4)."""
    if t is None:
        return
    if t.device == dev and t.dtype is dtype and t.shape == shape:
        if vec:
            if t.is_contiguous() and t.data_ptr() % vec == 0:
                return
        else:
            st = t.stride()   # (one call: cheaper than two stride(i))
            if st[-1] == 1 and t.data_ptr() % (8 if dtype is torch.bfloat16 and st[-2] % 8 else 16) == 0:
                return
    # the slow path: which rule it was
    if t.device != dev:
        raise RuntimeError(f"lc2is_amd.{who}: {name} is on {t.device}, the first operand on {dev}")
    if t.dtype != dtype:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be {dtype}, got {t.dtype}")
    if t.shape != shape:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if vec and not t.is_contiguous():
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be contiguous (the kernel takes no leading dimension for it)")
    if not vec and t.stride(-1) != 1:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must have unit stride in its last dimension")
    raise RuntimeError(f"lc2is_amd.{who}: {name} has a base address below the alignment its accesses need "
                       f"(data_ptr % 16 = {t.data_ptr() % 16}, strides {tuple(t.stride())})")


def _chk_ld8(who: str, t: torch.Tensor, name: str):
    """bf16 rows the attention kernels store as whole 16-byte chunks and have no narrower path for: every row has to begin on a
    16-byte boundary, i.e. ld % 8 == 0 (the launchers refuse the same)."""
    if t.stride(0) % 8:
        raise RuntimeError(f"lc2is_amd.{who}: {name} needs a leading dimension that is a multiple of 8 (16-byte stores), "
                           f"got {t.stride(0)}")


# ---- the device data views (aug_*, mix_*, strong_*, geo_*): what their wrappers ask of an operand, each rule once ----
def _overlap(a: torch.Tensor, b: torch.Tensor | None) -> bool:
    """The byte ranges of two tensors share a byte (lc2is_bytes_overlap of csrc/common.h)."""
    a0, b0 = a.data_ptr(), 0 if b is None else b.data_ptr()
    return b is not None and a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _view_table(who: str, t, name: str, B: int, words: int, dev=None, new_on=None) -> torch.Tensor:
    """A parameter, plan or info table: contiguous int32 [B, words], on ``dev`` where one is named; None is allocated on ``new_on``."""
    if t is None and new_on is not None:
        t = torch.empty((B, words), dtype=torch.int32, device=new_on)
    _chk(t, torch.int32, name)
    if tuple(t.shape) != (B, words) or not t.is_contiguous() or (dev is not None and t.device != dev):
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be contiguous int32 [{B}, {words}]" + ("" if dev is None else f" on {dev}"))
    return t


def _view_keys(who: str, keys, epoch, B: int | None = None) -> int:
    """epoch: one int32 on the device; keys: one int64 per sample (B None: the keys give B, at least one).  Returns B."""
    _chk(keys, torch.int64, "keys", 1); _chk(epoch, torch.int32, "epoch", None)
    n = keys.numel() if B is None else B
    if n < 1 or epoch.numel() != 1 or (keys is not None and keys.numel() != n):
        raise RuntimeError(f"lc2is_amd.{who}: epoch must hold one int32 and keys one int64 per sample, at least one")
    return n


def _view_pixels(who: str, x, name: str, align: int = 16):
    """A pixel batch: fp32 [B, 3, S, S], contiguous, with an ``align``-byte base; returns (B, S).  The side rule is _view_side's."""
    _chk(x, torch.float32, name, 4)
    B, S = x.shape[0], x.shape[2]
    if B < 1 or tuple(x.shape) != (B, 3, S, S) or not x.is_contiguous() or x.data_ptr() % align:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be contiguous fp32 [B, 3, S, S] with a {align}-byte base, got {tuple(x.shape)}, strides {tuple(x.stride())}")
    return B, S


def _view_side(who: str, B: int, S: int, L: int | None, min_side: int) -> None:
    """S a multiple of 4 (and of the label size L, where there is one) in min_side..AUG_MAX_SIDE; at most 65535 samples (one per blockIdx.y)."""
    if S < min_side or S > AUG_MAX_SIDE or S % 4 or (L is not None and (L < 1 or S % L)):
        raise ValueError(f"lc2is_amd.{who}: the size {S} must be a multiple of 4" + ("" if L is None else f" and of the label size {L}") + f", in {min_side}..{AUG_MAX_SIDE}")
    if not 1 <= B <= 65535:
        raise ValueError(f"lc2is_amd.{who}: 1..65535 samples per call, got {B}")


def _view_cells(who: str, m, name: str, dtype, B: int, L: int, dev=None) -> None:
    """A label (int64) or weight (fp32) map on the cells: contiguous [B, L, L] with an aligned base, on ``dev`` where one is named."""
    _chk(m, dtype, name, 3)
    if m is not None and (tuple(m.shape) != (B, L, L) or not m.is_contiguous() or m.data_ptr() % m.element_size() or (dev is not None and m.device != dev)):
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be contiguous {dtype} [{B}, L, L], labels and weights of one L" +
                           ("" if dev is None else " on the first operand's device") + f", got {tuple(m.shape)}, strides {tuple(m.stride())}")


def _view_out(who: str, o, name: str, shape, dtype, new_on, align: int = 1, inputs=(), refusal: str = "", dev=None) -> torch.Tensor:
    """None is allocated on ``new_on``; else contiguous ``shape``, ``align``-byte base (on ``dev`` if named), no byte shared with ``inputs``."""
    if o is None:
        o = torch.empty(shape, dtype=dtype, device=new_on)
    _chk(o, dtype, name, len(shape))
    if tuple(o.shape) != tuple(shape) or not o.is_contiguous() or o.data_ptr() % align or (dev is not None and o.device != dev):
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be contiguous {dtype} {tuple(shape)}, {align}-byte base" + ("" if dev is None else ", on the input's device"))
    if any(_overlap(o, i) for i in inputs):
        raise RuntimeError(f"lc2is_amd.{who}: {name} {refusal}")
    return o


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _ld(t: torch.Tensor | None) -> int:
    return 0 if t is None else (t.stride(0) if t.dim() == 2 else t.shape[-1])


def _out(spec, shape, dtype, dev):
    if spec is True:
        return torch.empty(shape, dtype=dtype, device=dev)
    if spec is None or spec is False:
        return None
    return spec



_ws_cache: dict = {}


def workspace(nbytes: int, device, tag: str = "default") -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream, tag); stream-ordered reuse is safe because every
    consumer of a workspace is enqueued on the same stream before the next producer."""
    key = (str(device), _stream(), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def gemm_nt(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, *, act: int = ACT_NONE,
            resid: torch.Tensor | None = None, aux_in: torch.Tensor | None = None,
            out_bf16: torch.Tensor | bool | None = True, out_f32: torch.Tensor | bool | None = None,
            aux_out: torch.Tensor | bool | None = None, tile_cfg: int = 0):
    """out = epi(a @ w.T + bias) (+ resid).  a [M,K] bf16, w [N,K] bf16, bias fp32 [N], resid fp32 [M,N] — or bf16 (a bf16
    residual stream: the add runs as the ACT_ADD_AUX epilogue, needs act == ACT_NONE and no other aux_in).
    ``out_bf16`` / ``out_f32`` / ``aux_out``: True = allocate, tensor = write into it, None/False = skip.
    Returns (out_bf16, out_f32, aux_out) with None for skipped outputs."""
    who, bf, f32, aux_name = "gemm_nt", torch.bfloat16, torch.float32, "aux_in"
    M, K = _dims(who, a, "a", 2, bf)
    dev = a.device
    N = _dims(who, w, "w")[0]
    mn = (M, N)
    _chk_op(who, w, "w", bf, (N, K), dev)
    if resid is not None and resid.dtype == bf:
        if act != ACT_NONE or aux_in is not None:
            raise RuntimeError("lc2is_amd.gemm_nt: resid in bf16 needs act == ACT_NONE and no aux_in")
        act, aux_in, resid, aux_name = ACT_ADD_AUX, resid, None, "resid"
    _chk_op(who, bias, "bias", f32, (N,), dev, 16); _chk_op(who, resid, "resid", f32, mn, dev)
    _chk_op(who, aux_in, aux_name, bf, mn, dev)
    ob = _out(out_bf16, mn, bf, dev)
    of = _out(out_f32, mn, f32, dev)
    ao = _out(aux_out, mn, bf, dev)
    if out_bf16 is not True:   # (what _out allocated above needs no check)
        _chk_op(who, ob, "out_bf16", bf, mn, dev)
    if out_f32 is not True:
        _chk_op(who, of, "out_f32", f32, mn, dev)
    if aux_out is not True:
        _chk_op(who, ao, "aux_out", bf, mn, dev)
    rc = _fn("lc2is_gemm_nt_bf16")(_ptr(a), _ld(a), _ptr(w), _ld(w), _ptr(bias), _ptr(resid), _ld(resid),
                                   _ptr(aux_in), _ld(aux_in), _ptr(ob), _ld(ob), _ptr(of), _ld(of), _ptr(ao),
                                   _ld(ao), M, N, K, act, tile_cfg, _stream())
    _lib.check(rc, f"gemm_nt M={M} N={N} K={K}")
    return ob, of, ao


class _GemmNtLaunch(C.Structure):   # lc2is_gemm_nt_launch
    _fields_ = [(n, _I) for n in ("cfg", "row0", "rows", "tail_rows", "staged_epi")] + \
               [(n, C.c_longlong) for n in ("off_a", "off_resid", "off_aux_in", "off_out_bf16", "off_out_f32", "off_aux_out")]


def gemm_nt_plan(M: int, N: int, K: int, *, act: int = ACT_NONE, resid: bool = False, aux_in: bool = False, out_bf16: bool = True,
                 out_f32: bool = False, aux_out: bool = False, tile_cfg: int = 0, ld: int | None = None):
    """The launches gemm_nt runs for this problem under the present CU budget: a list of (cfg, row0, rows, tail_rows, staged_epi,
    offsets) tuples, offsets = the bytes by which that launch's (a, resid, aux_in, out_bf16, out_f32, aux_out) pointers lie past the
    caller's.  ``ld`` = leading dimension of resid / aux_in / the outputs (default N).  Nothing is launched and no GPU is needed;
    raises what gemm_nt would raise for arguments the library refuses."""
    ld = N if ld is None else ld
    opt = [v for on in (resid, aux_in, out_bf16, out_f32, aux_out) for v in ((1 << 40 if on else None), (ld if on else 0))]
    recs = (_GemmNtLaunch * 2)()   # (pointers are only tested for NULL)
    n = _fn("lc2is_gemm_nt_plan")(1 << 40, K, 1 << 40, K, None, *opt, M, N, K, act, tile_cfg, recs, 2)
    if n < 0:
        _lib.check(n, f"gemm_nt_plan M={M} N={N} K={K}")
    return [(r.cfg, r.row0, r.rows, r.tail_rows, r.staged_epi,
             (r.off_a, r.off_resid, r.off_aux_in, r.off_out_bf16, r.off_out_f32, r.off_aux_out)) for r in recs[:n]]


_xchg_cache = {}
# the GEMM + LayerNorm launch (round 5): LC2IS_LN_FUSE=0 keeps the two launches everywhere; rows from which the fused form is taken
_LN_FUSE = os.environ.get("LC2IS_LN_FUSE", "1") != "0"
# 0 = where the 256x384 tiles fill the chip anyway: 224 tiles (7/8 of a round of the 256 CUs, the large-tile rule of lc2is_gemm_nt_bf16) —
# M >= 28 672 at N = 768; below that the unfused plan's smaller tiles keep more CUs busy than 2 x M / 256 blocks would
_LN_FUSE_MIN_ROWS = int(os.environ.get("LC2IS_LN_FUSE_MIN_ROWS", "0"))


def gemm_nt_ln_ok(M: int, N: int, K: int) -> bool:
    """Should this problem take gemm_nt_ln (else: gemm_nt + layernorm_fwd)?"""
    if not (_LN_FUSE and N in (384, 768) and K % 64 == 0 and M >= 256 and M % 256 <= 64):
        return False
    if _LN_FUSE_MIN_ROWS > 0:
        return M >= _LN_FUSE_MIN_ROWS
    return (M // 256) * (N // 384) >= 224


def gemm_nt_ln(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, resid: torch.Tensor | None, gamma: torch.Tensor,
               beta: torch.Tensor | None, eps: float = 1e-5, *, save_stats: bool = True,
               out_f32: torch.Tensor | None = None, ln_out: torch.Tensor | None = None):
    """x = a @ w.T + bias (+ resid) in fp32 AND h = bf16(LayerNorm(x) * gamma + beta) in ONE launch (256x384 tiles, the two column
    tiles of a row tile exchange row statistics).  a [M,K] bf16, w [N,K] bf16 with N in (384, 768), resid fp32 [M,N].
    Returns (x_f32, h_bf16, mean, rstd) — what gemm_nt(..., out_f32=True) followed by layernorm_fwd returns."""
    who, bf, f32 = "gemm_nt_ln", torch.bfloat16, torch.float32
    M, K = _dims(who, a, "a", 2, bf)
    dev = a.device
    N = _dims(who, w, "w")[0]
    _chk_op(who, w, "w", bf, (N, K), dev); _chk_op(who, bias, "bias", f32, (N,), dev, 16)
    _chk_op(who, resid, "resid", f32, (M, N), dev)
    if gamma is None:
        raise RuntimeError("lc2is_amd.gemm_nt_ln: gamma is required")
    _chk_op(who, gamma, "gamma", f32, (N,), dev, 16); _chk_op(who, beta, "beta", f32, (N,), dev, 16)
    xf = _out(out_f32 if out_f32 is not None else True, (M, N), f32, dev)
    h = _out(ln_out if ln_out is not None else True, (M, N), bf, dev)
    _chk_op(who, out_f32, "out_f32", f32, (M, N), dev); _chk_op(who, ln_out, "ln_out", bf, (M, N), dev)
    mean = torch.empty((M,), dtype=torch.float32, device=dev) if save_stats else None
    rstd = torch.empty((M,), dtype=torch.float32, device=dev) if save_stats else None
    nb = _fn("lc2is_gemm_nt_ln_xchg_bytes")(M, N)
    xc = None
    if nb:
        key = (str(dev), _stream())
        xc = _xchg_cache.get(key)
        if xc is None or xc.numel() < nb:
            xc = torch.zeros(max(int(nb), 1 << 21), dtype=torch.uint8, device=dev)   # all zero once; every launch leaves it all zero
            _xchg_cache[key] = xc
    rc = _fn("lc2is_gemm_nt_ln_bf16")(_ptr(a), _ld(a), _ptr(w), _ld(w), _ptr(bias), _ptr(resid), _ld(resid), _ptr(xf), _ld(xf),
                                      _ptr(gamma), _ptr(beta), float(eps), _ptr(h), _ld(h), _ptr(mean), _ptr(rstd), _ptr(xc),
                                      xc.numel() if xc is not None else 0, M, N, K, _stream())
    _lib.check(rc, f"gemm_nt_ln M={M} N={N} K={K}")
    return xf, h, mean, rstd


def gemm_nt_batched(a: torch.Tensor, w: torch.Tensor, *, out_bf16: torch.Tensor | bool | None = None,
                    out_f32: torch.Tensor | bool | None = True):
    """out[b] = a[b] @ w[b].T for every b in ONE launch.  a [B,M,K] bf16, w [B,N,K] bf16 (unit inner stride; any row /
    batch strides that are multiples of 8 elements).  Returns (out_bf16 [B,M,N] or None, out_f32 [B,M,N] or None)."""
    who, dev = "gemm_nt_batched", a.device
    Bn, M, K = _dims(who, a, "a", 3, torch.bfloat16)
    N = _dims(who, w, "w", 3)[1]
    _chk_op(who, w, "w", torch.bfloat16, (Bn, N, K), dev)
    ob = _out(out_bf16, (Bn, M, N), torch.bfloat16, dev)
    of = _out(out_f32, (Bn, M, N), torch.float32, dev)
    if out_bf16 is not True:
        _chk_op(who, ob, "out_bf16", torch.bfloat16, (Bn, M, N), dev)
    if out_f32 is not True:
        _chk_op(who, of, "out_f32", torch.float32, (Bn, M, N), dev)
    st = lambda t: (0, 0) if t is None else (t.stride(1), t.stride(0))  # noqa: E731
    rc = _fn("lc2is_gemm_nt_bf16_batched")(_ptr(a), a.stride(1), a.stride(0), _ptr(w), w.stride(1), w.stride(0),
                                           _ptr(ob), *st(ob), _ptr(of), *st(of), M, N, K, Bn, _stream())
    _lib.check(rc, f"gemm_nt_batched B={Bn} M={M} N={N} K={K}")
    return ob, of


def transpose_bf16_batched(x: torch.Tensor) -> torch.Tensor:
    """x [B,R,C] bf16 -> [B,C,R] contiguous, one launch."""
    _chk(x, torch.bfloat16, "x", 3)
    Bn, R, Cc = x.shape
    out = torch.empty((Bn, Cc, R), dtype=torch.bfloat16, device=x.device)
    rc = _fn("lc2is_transpose_bf16_batched")(_ptr(x), x.stride(1), x.stride(0), _ptr(out), R, Cc * R, R, Cc, Bn, _stream())
    _lib.check(rc, f"transpose_bf16_batched B={Bn} R={R} C={Cc}")
    return out


def gemm_tn(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor | None = None, accumulate: bool = False,
            db: torch.Tensor | None = None):
    """dw[N,K] (fp32) = dy[M,N]^T @ x[M,K]; optional fused bias gradient db[N] = dy.sum(0) (same accumulate flag)."""
    who, dev = "gemm_tn", dy.device
    M, N = _dims(who, dy, "dy", 2, torch.bfloat16)
    K = _dims(who, x, "x")[1]
    _chk_op(who, x, "x", torch.bfloat16, (M, K), dev)
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dev)
        accumulate = False
    else:
        _chk_op(who, dw, "dw", torch.float32, (N, K), dev)
    _chk_op(who, db, "db", torch.float32, (N,), dev, 4)
    nbytes = _fn("lc2is_gemm_tn_workspace_bytes")(M, N, K)
    ws = workspace(nbytes, dy.device, "gemm_tn")
    rc = _fn("lc2is_gemm_tn_bf16")(_ptr(dy), _ld(dy), _ptr(x), _ld(x), _ptr(dw), _ld(dw), _ptr(db), M, N, K,
                                   int(accumulate), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, f"gemm_tn M={M} N={N} K={K}")
    return dw


class _TnPlan(C.Structure):   # lc2is_tn_plan
    _fields_ = [(n, _I) for n in ("big", "ntn", "ntk", "splits", "chunk", "grid", "red_grid")] + [("workspace_bytes", C.c_longlong)]


def gemm_tn_plan(M: int, N: int, K: int) -> dict:
    """The plan gemm_tn runs for densely packed [M,N] / [M,K] operands under the present CU budget: dict(big, ntn, ntk, splits,
    chunk, grid, red_grid, workspace_bytes).  Nothing is launched and no GPU is needed; raises what gemm_tn would raise."""
    rec = _TnPlan()
    _lib.check(_fn("lc2is_gemm_tn_plan")(M, N, K, C.addressof(rec)), f"gemm_tn_plan M={M} N={N} K={K}")
    return {n: getattr(rec, n) for n, _ in _TnPlan._fields_}


class TnProblem(C.Structure):
    _fields_ = [("dY", C.c_void_p), ("X", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p), ("ldy", C.c_int),
                ("ldx", C.c_int), ("ldw", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("accumulate", C.c_int)]


GROUP_MAX = 128        # LC2IS_TN_GROUP_MAX


# rows (tokens) from which a weight gradient joins a grouped launch: the text tower (151 prompts x 16 tokens = 2416 rows, 72
# problems of 4..16 tiles) stays 76 small launches on its side stream: grouping them (1024) measured neutral on the step
_GROUP_MIN_ROWS = int(os.environ.get("LC2IS_GROUP_MIN_ROWS", "4096"))


def gemm_tn_groupable(dy: torch.Tensor, x: torch.Tensor) -> bool:
    return dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0 and dy.shape[0] >= _GROUP_MIN_ROWS


def gemm_tn_grouped(problems):
    """problems: list of (dy [M,N] bf16, x [M,K] bf16, dw [N,K] fp32, db [N] fp32 or None, accumulate) with N, K
    multiples of 8 (check with gemm_tn_groupable; groups whose N, K are all multiples of 256 take the 256x256 LDS-DMA tiles) — the weight gradients of one layer, or of a whole tower, in one grid."""
    if not 1 <= len(problems) <= GROUP_MAX:
        raise RuntimeError(f"lc2is_amd.gemm_tn_grouped: 1..{GROUP_MAX} problems per launch")
    arr = (TnProblem * len(problems))()
    who, dev = "gemm_tn_grouped", problems[0][0].device
    for i, (dy, x, dw, db, acc) in enumerate(problems):
        try:
            M, N = _dims(who, dy, "dy", 2, torch.bfloat16)
            K = _dims(who, x, "x")[1]
            if i:
                _chk_op(who, dy, "dy", torch.bfloat16, (M, N), dev)      # (on the first problem's device)
            _chk_op(who, x, "x", torch.bfloat16, (M, K), dev)
            if dw is None:
                raise RuntimeError("lc2is_amd.gemm_tn_grouped: dw is required")
            _chk_op(who, dw, "dw", torch.float32, (N, K), dev); _chk_op(who, db, "db", torch.float32, (N,), dev, 4)
        except RuntimeError as e:
            raise RuntimeError(f"{e} (problem {i})") from None
        arr[i] = TnProblem(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ld(dy), _ld(x), _ld(dw), M, N, K, int(acc))
    nbytes = _fn("lc2is_gemm_tn_grouped_workspace_bytes")(arr, len(problems))
    ws = workspace(nbytes, problems[0][0].device, "gemm_tn_grouped")
    rc = _fn("lc2is_gemm_tn_grouped")(arr, len(problems), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, f"gemm_tn_grouped n={len(problems)}")


class _TnGroupPlan(C.Structure):   # lc2is_tn_group_plan
    _fields_ = [(n, _I) for n in ("small", "table", "grid", "red_grid")] + [(n, C.c_longlong) for n in ("workspace_bytes", "table_bytes")]


class _TnGroupRec(C.Structure):   # lc2is_tn_group_rec
    _fields_ = [(n, _I) for n in ("index", "ntn", "ntk", "splits", "chunk", "blk_end", "red_end", "red_blocks")] + \
               [(n, C.c_longlong) for n in ("slab_offset", "bias_offset")]


def gemm_tn_grouped_plan(shapes, M: int, lds=None, db=True):
    """The plan gemm_tn_grouped runs for problems of ``shapes`` = [(N, K), ...] over M rows each under the present CU budget:
    (summary dict, [record dict per problem, in grid order]).  ``lds`` = [(ldy, ldx, ldw), ...] (default: densely packed), ``db``:
    with bias gradients (one bool, or one per problem).  Nothing is launched and no GPU is needed; raises what gemm_tn_grouped would raise."""
    n = len(shapes)
    arr = (TnProblem * max(n, 1))()
    for i, (N, K) in enumerate(shapes):
        ldy, ldx, ldw = lds[i] if lds is not None else (N, K, K)
        arr[i] = TnProblem(1 << 40, 1 << 40, 1 << 40, (1 << 40) if (db[i] if isinstance(db, (list, tuple)) else db) else None, ldy, ldx, ldw, M, N, K, 0)   # (only tested for NULL)
    summary, recs = _TnGroupPlan(), (_TnGroupRec * max(n, 1))()
    _lib.check(_fn("lc2is_gemm_tn_grouped_plan")(arr, n, C.addressof(summary), recs, n), f"gemm_tn_grouped_plan n={n}")
    return ({f: getattr(summary, f) for f, _ in _TnGroupPlan._fields_},
            [{f: getattr(r, f) for f, _ in _TnGroupRec._fields_} for r in recs[:n]])


def release_captured_tables() -> int:
    """Free the pinned descriptor-table images that captured grouped weight-gradient launches left behind (call after the
    graphs that captured them are destroyed).  Returns the number freed."""
    f = _fn("lc2is_release_captured_tables")
    f.restype = C.c_int
    return int(f())


def captured_tables_mark() -> int:
    """Number of captured descriptor-table images registered so far (bracket a capture with two marks)."""
    return int(_fn("lc2is_captured_tables_mark")())


def release_captured_tables_range(first: int, last: int) -> int:
    """Free the images registered between two marks (the ones ONE captured graph owns), after that graph is destroyed."""
    return int(_fn("lc2is_release_captured_tables_range")(int(first), int(last)))


def colsum(dy: torch.Tensor, db: torch.Tensor | None = None, accumulate: bool = False):
    """db[N] (fp32) = dy[M,N].sum(0)."""
    M, N = _dims("colsum", dy, "dy", 2, torch.bfloat16)
    if db is None:
        db = torch.empty((N,), dtype=torch.float32, device=dy.device)
        accumulate = False
    else:
        _chk_op("colsum", db, "db", torch.float32, (N,), dy.device, 4)
    nbytes = _fn("lc2is_colsum_workspace_bytes")(M, N)
    ws = workspace(nbytes, dy.device, "colsum")
    rc = _fn("lc2is_colsum_bf16")(_ptr(dy), _ld(dy), _ptr(db), M, N, int(accumulate), _ptr(ws), ws.numel(),
                                  _stream())
    _lib.check(rc, f"colsum M={M} N={N}")
    return db


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor | None, eps: float = 1e-5, *,
                  save_stats: bool = True, out_bf16: torch.Tensor | bool | None = True,
                  out_f32: torch.Tensor | bool | None = None):
    """x fp32 or bf16 [M,C] (the residual stream) -> (y_bf16, y_f32, mean, rstd)."""
    who, bf, f32 = "layernorm_fwd", torch.bfloat16, torch.float32
    xb = x.dtype == bf
    M, Cc = _dims(who, x, "x", 2, bf if xb else f32)
    dev = x.device
    if gamma is None:
        raise RuntimeError("lc2is_amd.layernorm_fwd: gamma is required")
    _chk_op(who, gamma, "gamma", f32, (Cc,), dev, 16); _chk_op(who, beta, "beta", f32, (Cc,), dev, 16)
    yb = _out(out_bf16, (M, Cc), bf, dev)
    yf = _out(out_f32, (M, Cc), f32, dev)
    if out_bf16 is not True:
        _chk_op(who, yb, "out_bf16", bf, (M, Cc), dev)
    if out_f32 is not True:
        _chk_op(who, yf, "out_f32", f32, (M, Cc), dev)
    mean = torch.empty((M,), dtype=torch.float32, device=dev) if save_stats else None
    rstd = torch.empty((M,), dtype=torch.float32, device=dev) if save_stats else None
    rc = _fn("lc2is_layernorm_fwd")(_ptr(x), _ld(x), int(xb), _ptr(gamma), _ptr(beta), _ptr(yb), _ld(yb), _ptr(yf),
                                    _ld(yf), _ptr(mean), _ptr(rstd), M, Cc, float(eps), _stream())
    _lib.check(rc, f"layernorm_fwd M={M} C={Cc}")
    return yb, yf, mean, rstd


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor,
                  rstd: torch.Tensor, *, dres: torch.Tensor | None = None, dgamma: torch.Tensor | None = None,
                  dbeta: torch.Tensor | None = None, accumulate: bool = False, want_f32: bool = True,
                  want_bf16: bool = True, need_param_grads: bool = True):
    """Returns (dx_f32, dx_bf16, dgamma, dbeta).  dy, x (the residual stream the forward normalised) and dres (the gradient
    arriving over the residual path) are each bf16 or fp32 [M,C]."""
    who, bf, f32 = "layernorm_bwd", torch.bfloat16, torch.float32
    xb = x.dtype == bf
    M, Cc = _dims(who, x, "x", 2, bf if xb else f32)
    dev = x.device
    dyb = dy if dy.dtype == bf else None
    dyf = dy if dy.dtype == f32 else None
    if dyb is None and dyf is None:
        raise RuntimeError("lc2is_amd.layernorm_bwd: dy must be bf16 or fp32")
    rb = dres is not None and dres.dtype == bf
    _chk_op(who, dy, "dy", dy.dtype, (M, Cc), dev)
    _chk_op(who, dres, "dres", bf if rb else f32, (M, Cc), dev)
    if gamma is None or mean is None or rstd is None:
        raise RuntimeError("lc2is_amd.layernorm_bwd: gamma, mean and rstd are required")
    _chk_op(who, gamma, "gamma", f32, (Cc,), dev, 16); _chk_op(who, mean, "mean", f32, (M,), dev, 4); _chk_op(who, rstd, "rstd", f32, (M,), dev, 4)
    _chk_op(who, dgamma, "dgamma", f32, (Cc,), dev, 4); _chk_op(who, dbeta, "dbeta", f32, (Cc,), dev, 4)
    dxf = torch.empty((M, Cc), dtype=torch.float32, device=dev) if want_f32 else None
    dxb = torch.empty((M, Cc), dtype=torch.bfloat16, device=dev) if want_bf16 else None
    if need_param_grads:
        if dgamma is None:
            dgamma = torch.empty((Cc,), dtype=torch.float32, device=dev)
            accumulate = False
            if dbeta is None:
                dbeta = torch.empty((Cc,), dtype=torch.float32, device=dev)
    nbytes = _fn("lc2is_layernorm_bwd_workspace_bytes")(M, Cc)
    defer = _ln_defer if (need_param_grads and (dgamma is not None or dbeta is not None)) else None
    if defer is not None:
        # parameter gradients deferred (ln_defer_begin/flush): the partial sums stay in a buffer of their own until the
        # grouped reduce at the end of the layer group
        ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        defer.append((ws, _fn("lc2is_layernorm_bwd_partials")(M, Cc), Cc, dgamma, dbeta, bool(accumulate)))
        pg, pb = None, None
    else:
        ws = workspace(nbytes, dev, "ln_bwd")
        pg, pb = dgamma, dbeta
    rc = _fn("lc2is_layernorm_bwd")(_ptr(dyb), _ld(dyb), _ptr(dyf), _ld(dyf), _ptr(x), _ld(x), int(xb), _ptr(gamma),
                                    _ptr(mean), _ptr(rstd), _ptr(dres), _ld(dres), int(rb), _ptr(dxf), _ld(dxf),
                                    _ptr(dxb), _ld(dxb), _ptr(pg), _ptr(pb), int(accumulate), M, Cc,
                                    _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, f"layernorm_bwd M={M} C={Cc}")
    return dxf, dxb, dgamma, dbeta


class LnPartials(C.Structure):
    _fields_ = [("partials", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("nparts", C.c_int),
                ("C", C.c_int), ("accumulate", C.c_int)]


LN_PARTIALS_MAX = 64   # LC2IS_LN_PARTIALS_MAX
_LN_DEFER = os.environ.get("LC2IS_LN_DEFER", "1") != "0"   # A/B switch: 0 = every layernorm_bwd reduces its own partials
_ln_defer = None       # list of deferred (ws, nparts, C, dgamma, dbeta, accumulate) while a deferral scope is open


def ln_defer_begin():
    """Open a deferral scope: layernorm_bwd calls that are handed dgamma / dbeta buffers keep their partial sums and the
    reductions leave together at ln_defer_flush (nn.base.WgradBatch opens / flushes one with the weight gradients).
    Returns the previous scope (pass it to ln_defer_end)."""
    global _ln_defer
    prev, _ln_defer = _ln_defer, ([] if _LN_DEFER else None)
    return prev


def ln_defer_flush():
    """One grouped launch per <= LN_PARTIALS_MAX deferred calls (two calls that write the same vector are never put in
    the same launch: the second waits for the next one)."""
    global _ln_defer
    items = _ln_defer
    if not items:
        return
    _ln_defer = []
    while items:
        chunk, rest, seen = [], [], set()
        for it in items:
            outs = {t.data_ptr() for t in (it[3], it[4]) if t is not None}
            if len(chunk) < LN_PARTIALS_MAX and not (outs & seen) and not rest:
                chunk.append(it); seen |= outs
            else:
                rest.append(it)
        arr = (LnPartials * len(chunk))()
        for i, (ws, nparts, Cc, dg, db, acc) in enumerate(chunk):
            _chk(dg, torch.float32, "dgamma", 1); _chk(db, torch.float32, "dbeta", 1)
            arr[i] = LnPartials(_ptr(ws), _ptr(dg), _ptr(db), nparts, Cc, int(acc))
        rc = _fn("lc2is_ln_partials_reduce")(arr, len(chunk), _stream())
        _lib.check(rc, f"ln_partials_reduce n={len(chunk)}")
        items = rest


def ln_defer_end(prev):
    global _ln_defer
    ln_defer_flush()
    _ln_defer = prev


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, H: int, Sq: int, Sk: int, D: int,
                  scale: float, *, causal: bool = False, kbias: torch.Tensor | None = None,
                  save_lse: bool = True, out: torch.Tensor | None = None, dropout_p: float = 0.0, seed: int = 0):
    """q [B*Sq, H*D], k/v [B*Sk, H*D] bf16 2-D views (any row stride).  Returns (o [B*Sq, H*D] bf16, lse2).
    dropout_p > 0: dropout on the attention probabilities, decisions = f(seed, (b,h,q), key) (pass the same to attention_bwd).
    kbias: fp32 contiguous [B,Sk] additive key bias, per key any finite value or -inf (masked); any subset of the keys may be
    masked.  A query row with no visible key gives O = 0 and lse2 = -inf (torch gives NaN).  The K / V rows of masked keys
    do not matter as long as they are finite."""
    who, bf = "attention_fwd", torch.bfloat16
    dev, qs, ks = q.device, (B * Sq, H * D), (B * Sk, H * D)
    if _dims(who, q, "q", 2, bf) != qs:
        raise RuntimeError(f"lc2is_amd.attention_fwd: q must have shape {qs}, got {tuple(q.shape)}")
    _chk_op(who, k, "k", bf, ks, dev); _chk_op(who, v, "v", bf, ks, dev)
    _chk_op(who, kbias, "kbias", torch.float32, (B, Sk), dev, 4)
    o = out
    if o is None:
        o = torch.empty(qs, dtype=bf, device=dev)
    else:
        _chk_op(who, o, "out", bf, qs, dev); _chk_ld8(who, o, "out")
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device) if save_lse else None
    if dropout_p > 0.0:
        rc = _fn("lc2is_attention_fwd_dropout")(_ptr(q), _ld(q), _ptr(k), _ld(k), _ptr(v), _ld(v), _ptr(o), _ld(o),
                                                _ptr(lse), _ptr(kbias), B, H, Sq, Sk, D, float(scale), int(causal),
                                                float(dropout_p), int(seed), _stream())
    else:
        rc = _fn("lc2is_attention_fwd")(_ptr(q), _ld(q), _ptr(k), _ld(k), _ptr(v), _ld(v), _ptr(o), _ld(o),
                                        _ptr(lse), _ptr(kbias), B, H, Sq, Sk, D, float(scale), int(causal),
                                        _stream())
    _lib.check(rc, f"attention_fwd B={B} H={H} Sq={Sq} Sk={Sk} D={D}")
    return o, lse


def attention_bwd(q, k, v, o, do, lse2, B: int, H: int, Sq: int, Sk: int, D: int, scale: float, *,
                  causal: bool = False, kbias: torch.Tensor | None = None, dq=None, dk=None, dv=None,
                  dropout_p: float = 0.0, seed: int = 0):
    """Returns (dq, dk, dv) bf16; dq/dk/dv may be preallocated 2-D views (e.g. slices of a packed dQKV).
    kbias / causal / dropout_p / seed as passed to attention_fwd.  A row whose lse2 is -inf (no visible key) gets dq = 0 and
    gives nothing to dk / dv; the dk / dv rows of masked keys are 0."""
    who, bf = "attention_bwd", torch.bfloat16
    dev, qs, ks = q.device, (B * Sq, H * D), (B * Sk, H * D)
    if _dims(who, q, "q", 2, bf) != qs:
        raise RuntimeError(f"lc2is_amd.attention_bwd: q must have shape {qs}, got {tuple(q.shape)}")
    for t, n, s in ((k, "k", ks), (v, "v", ks), (o, "o", qs), (do, "do", qs)):
        if t is None:
            raise RuntimeError(f"lc2is_amd.attention_bwd: {n} is required")
        _chk_op(who, t, n, bf, s, dev)
    _chk_op(who, dq, "dq", bf, qs, dev); _chk_op(who, dk, "dk", bf, ks, dev); _chk_op(who, dv, "dv", bf, ks, dev)
    if dq is None:
        dq = torch.empty(qs, dtype=bf, device=dev)
    else:
        _chk_ld8(who, dq, "dq")   # (dk / dv leave as 8-byte stores: ld % 4 is enough for them)
    dk = dk if dk is not None else torch.empty(ks, dtype=bf, device=dev)
    dv = dv if dv is not None else torch.empty(ks, dtype=bf, device=dev)
    if lse2 is None:
        raise RuntimeError("lc2is_amd.attention_bwd: lse2 is required")
    _chk_op(who, lse2, "lse2", torch.float32, (B, H, Sq), dev, 4); _chk_op(who, kbias, "kbias", torch.float32, (B, Sk), dev, 4)
    delta = torch.empty((B, H, Sq), dtype=torch.float32, device=dev)
    args = (_ptr(q), _ld(q), _ptr(k), _ld(k), _ptr(v), _ld(v), _ptr(o), _ld(o), _ptr(do), _ld(do), _ptr(dq), _ld(dq),
            _ptr(dk), _ld(dk), _ptr(dv), _ld(dv), _ptr(lse2), _ptr(delta), _ptr(kbias), B, H, Sq, Sk, D, float(scale),
            int(causal))
    if dropout_p > 0.0:
        rc = _fn("lc2is_attention_bwd_dropout")(*args, float(dropout_p), int(seed), _stream())
    else:
        rc = _fn("lc2is_attention_bwd")(*args, _stream())
    _lib.check(rc, f"attention_bwd B={B} H={H} Sq={Sq} Sk={Sk} D={D}")
    return dq, dk, dv


def dropout_rows_f32(x: torch.Tensor, p: float, seed: int, *, resid: torch.Tensor | None = None,
                     out_f32: torch.Tensor | bool | None = True, out_bf16: torch.Tensor | bool | None = None,
                     rows_per_sample: int = 0):
    """y = resid + keep * x / (1 - p) on fp32 rows [M,C]; one decision per element, or per sample of `rows_per_sample` rows
    (drop-path).  Returns (y_f32 or None, y_bf16 or None).  Applied to a gradient with the forward's (p, seed) it is the
    backward of the same site."""
    who, dev = "dropout_rows_f32", x.device
    M, Cc = _dims(who, x, "x", 2, torch.float32)
    _chk_op(who, resid, "resid", torch.float32, (M, Cc), dev)
    yf = _out(out_f32, (M, Cc), torch.float32, dev)
    yb = _out(out_bf16, (M, Cc), torch.bfloat16, dev)
    if out_f32 is not True:
        _chk_op(who, yf, "out_f32", torch.float32, (M, Cc), dev)
    if out_bf16 is not True:
        _chk_op(who, yb, "out_bf16", torch.bfloat16, (M, Cc), dev)
    rc = _fn("lc2is_dropout_rows_f32")(_ptr(x), _ld(x), _ptr(resid), _ld(resid), _ptr(yf), _ld(yf), _ptr(yb), _ld(yb), M, Cc,
                                       int(rows_per_sample), float(p), int(seed), _stream())
    _lib.check(rc, f"dropout_rows_f32 M={M} C={Cc}")
    return yf, yb


def dropout_rows_bf16(x: torch.Tensor, p: float, seed: int, out: torch.Tensor | None = None):
    """bf16 [M,C] -> keep * x / (1 - p), in place unless `out` is given."""
    M, Cc = _dims("dropout_rows_bf16", x, "x", 2, torch.bfloat16)
    y = x if out is None else out
    _chk_op("dropout_rows_bf16", out, "out", torch.bfloat16, (M, Cc), x.device)
    rc = _fn("lc2is_dropout_rows_bf16")(_ptr(x), _ld(x), _ptr(y), _ld(y), M, Cc, float(p), int(seed), _stream())
    _lib.check(rc, f"dropout_rows_bf16 M={M} C={Cc}")
    return y


def dropout_mask(rows: int, cols: int, p: float, seed: int, device) -> torch.Tensor:
    """The decisions keep(seed, r, c) as a uint8 [rows, cols] tensor — for tests (the product path never stores a mask)."""
    out = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    _lib.check(_fn("lc2is_dropout_mask")(_ptr(out), rows, cols, float(p), int(seed), _stream()), "dropout_mask")
    return out


INTERP_BICUBIC, INTERP_BILINEAR = 0, 1


class ShadowDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("dstT", C.c_void_p), ("N", C.c_int), ("K", C.c_int),
                ("ld_dst", C.c_int), ("ld_dstT", C.c_int), ("tile_start", C.c_int), ("flags", C.c_int)]


class ShadowTable:
    """Device-resident descriptor table for ``lc2is_shadow_refresh`` (built once; pointers must stay valid)."""

    def __init__(self, entries, device):
        # entries: list of (src_f32 [N,K] contiguous, dst_bf16 2-D view or None, dstT_bf16 2-D view or None)
        descs = (ShadowDesc * len(entries))()
        start = 0
        self._keep = []
        for i, (src, dst, dstT) in enumerate(entries):
            if src.dim() == 1:  # vectors are copied as [1,K] rows
                src = src.unsqueeze(0)
                dst = dst.unsqueeze(0) if dst is not None and dst.dim() == 1 else dst
            f32copy = dst is not None and dst.dtype == torch.float32
            _chk(src, torch.float32, "shadow src")
            _chk(dst, torch.float32 if f32copy else torch.bfloat16, "shadow dst")
            _chk(dstT, torch.bfloat16, "shadow dstT")
            if f32copy and dstT is not None:
                raise RuntimeError("lc2is_amd: fp32 shadow copies have no transposed twin")
            if not src.is_contiguous():
                raise RuntimeError("lc2is_amd: shadow source must be contiguous")
            N, K = src.shape
            if K % 4 or (dstT is not None and N % 4):
                raise RuntimeError(f"lc2is_amd: shadow shape [{N},{K}] not supported")
            if dst is not None and tuple(dst.shape) != (N, K):
                raise RuntimeError("lc2is_amd: shadow dst shape mismatch")
            if dstT is not None and tuple(dstT.shape) != (K, N):
                raise RuntimeError("lc2is_amd: shadow dstT shape mismatch")
            descs[i] = ShadowDesc(src.data_ptr(), _ptr(dst), _ptr(dstT), N, K, _ld(dst), _ld(dstT), start, int(f32copy))
            start += ((N + 63) // 64) * ((K + 63) // 64)
            self._keep.append((src, dst, dstT))
        self.n = len(entries)
        self.total_tiles = start
        raw = bytes(descs)
        self.dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)

    def refresh(self):
        rc = _fn("lc2is_shadow_refresh")(self.dev.data_ptr(), self.n, self.total_tiles, _stream())
        _lib.check(rc, "shadow_refresh")


def cast_bf16(src: torch.Tensor, out: torch.Tensor | None = None):
    _chk(src, torch.float32, "src")
    M, Cc = src.shape
    out = out if out is not None else torch.empty((M, Cc), dtype=torch.bfloat16, device=src.device)
    _chk(out, torch.bfloat16, "out")
    _lib.check(_fn("lc2is_cast_f32_bf16")(_ptr(src), _ld(src), _ptr(out), _ld(out), M, Cc, _stream()), "cast")
    return out


def transpose_bf16(src: torch.Tensor, out: torch.Tensor | None = None):
    _chk(src, torch.bfloat16, "src")
    R, Cc = src.shape
    out = out if out is not None else torch.empty((Cc, R), dtype=torch.bfloat16, device=src.device)
    _chk(out, torch.bfloat16, "out")
    _lib.check(_fn("lc2is_transpose_bf16")(_ptr(src), _ld(src), _ptr(out), _ld(out), R, Cc, _stream()),
               "transpose")
    return out


def patchify(pixels: torch.Tensor, patch: int, kpad: int | None = None):
    """pixels fp32 [B,3,H,W] contiguous -> bf16 [B*G*G, kpad]."""
    _chk(pixels, torch.float32, "pixel_values", 4)
    if not pixels.is_contiguous() or pixels.shape[1] != 3:
        raise RuntimeError("lc2is_amd.patchify: pixel_values must be contiguous [B,3,H,W]")
    B, _, H, W = pixels.shape
    G = H // patch
    k = 3 * patch * patch
    kpad = kpad or ((k + 63) // 64) * 64
    out = torch.empty((B * G * G, kpad), dtype=torch.bfloat16, device=pixels.device)
    _lib.check(_fn("lc2is_patchify")(_ptr(pixels), _ptr(out), kpad, B, H, W, patch, _stream()), "patchify")
    return out


def _chk_rows(who: str, t, name: str, rows: int, what: str):
    """The row-streaming kernels index a tensor by their integer arguments alone: a tensor with another row count is read or
    written out of bounds, so it is refused here, before any launch."""
    if t.shape[0] != rows:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must have {what} = {rows} rows, got shape {tuple(t.shape)}")


def _chk_table(who: str, t, name: str, like, min_rows: int | None, Cc: int):
    """A parameter or gradient table the kernels address as dense fp32 [rows, C] (a [C] vector when ``min_rows`` is None)."""
    _chk(t, torch.float32, name, 1 if min_rows is None else 2)
    if t.device != like.device:
        raise RuntimeError(f"lc2is_amd.{who}: {name} is on {t.device}, the data on {like.device}")
    if not t.is_contiguous():
        raise RuntimeError(f"lc2is_amd.{who}: {name} must be contiguous")
    if t.shape[-1] != Cc:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must have C = {Cc} columns, got shape {tuple(t.shape)}")
    if min_rows is not None and t.shape[0] < min_rows:
        raise RuntimeError(f"lc2is_amd.{who}: {name} must have at least {min_rows} rows, got shape {tuple(t.shape)}")


def vit_embed_fwd(patch_f32, cls, pos, B: int, P: int):
    _chk(patch_f32, torch.float32, "patch")
    Cc = patch_f32.shape[1]
    _chk_rows("vit_embed_fwd", patch_f32, "patch", B * P, "B*P")
    _chk_table("vit_embed_fwd", cls, "cls", patch_f32, None, Cc)
    _chk_table("vit_embed_fwd", pos, "pos", patch_f32, P + 1, Cc)
    x = torch.empty((B * (P + 1), Cc), dtype=torch.float32, device=patch_f32.device)
    _lib.check(_fn("lc2is_vit_embed_fwd")(_ptr(patch_f32), _ld(patch_f32), _ptr(cls), _ptr(pos), _ptr(x), Cc, B,
                                          P, Cc, _stream()), "vit_embed_fwd")
    return x


def vit_embed_bwd(dx, dpos, dcls, B: int, P: int, accumulate: bool = False):
    _chk(dx, torch.float32, "dx")
    Cc = dx.shape[1]
    _chk_rows("vit_embed_bwd", dx, "dx", B * (P + 1), "B*(P+1)")
    _chk_table("vit_embed_bwd", dcls, "dcls", dx, None, Cc)
    _chk_table("vit_embed_bwd", dpos, "dpos", dx, P + 1, Cc)
    dpatch = torch.empty((B * P, Cc), dtype=torch.bfloat16, device=dx.device)
    _lib.check(_fn("lc2is_vit_embed_bwd")(_ptr(dx), _ld(dx), _ptr(dpos), _ptr(dcls), _ptr(dpatch), Cc, B, P, Cc,
                                          int(accumulate), _stream()), "vit_embed_bwd")
    return dpatch


def text_embed_fwd(ids, tok, pos):
    _chk(ids, torch.int64, "input_ids"); _chk(tok, torch.float32, "tok")
    if not ids.is_contiguous():
        raise RuntimeError("lc2is_amd.text_embed_fwd: input_ids must be contiguous")
    B, L = ids.shape
    V, Cc = tok.shape
    _chk_table("text_embed_fwd", tok, "tok", ids, 1, Cc)
    _chk_table("text_embed_fwd", pos, "pos", ids, L, Cc)
    x = torch.empty((B * L, Cc), dtype=torch.float32, device=tok.device)
    _lib.check(_fn("lc2is_text_embed_fwd")(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(x), Cc, B, L, Cc, V, _stream()),
               "text_embed_fwd")
    return x


def text_embed_bwd(ids, dx, dtok, dpos, accumulate: bool = False):
    """dtok must already hold the running gradient (or zeros); per-token sums in row order, no atomics (reproducible).
    ids outside [0, rows of dtok) are clamped into it, as the forward clamps them — and callers rely on it: a tower whose token
    table is frozen hands a ONE-row scratch as dtok, every id then lands on row 0 and only dpos is kept (nn/clip.py)."""
    _chk(ids, torch.int64, "input_ids"); _chk(dx, torch.float32, "dx")
    if not ids.is_contiguous():
        raise RuntimeError("lc2is_amd.text_embed_bwd: input_ids must be contiguous")
    B, L = ids.shape
    Cc = dx.shape[1]
    _chk_rows("text_embed_bwd", dx, "dx", B * L, "B*L")
    if dx.device != ids.device:
        raise RuntimeError(f"lc2is_amd.text_embed_bwd: dx is on {dx.device}, input_ids on {ids.device}")
    _chk_table("text_embed_bwd", dtok, "dtok", ids, 1, Cc)
    _chk_table("text_embed_bwd", dpos, "dpos", ids, L, Cc)
    V = dtok.shape[0]
    _lib.check(_fn("lc2is_text_embed_bwd")(_ptr(ids), _ptr(dx), _ld(dx), _ptr(dtok), _ptr(dpos), B, L, Cc, V,
                                           int(accumulate), _stream()), "text_embed_bwd")


def rows_copy(src, S_src: int, src_off: int, S_dst: int, dst_off: int, B: int, n: int, *, dst_f32=None,
              dst_bf16=None):
    sb = src.dtype == torch.bfloat16
    _chk(src, torch.bfloat16 if sb else torch.float32, "src")
    Cc = src.shape[1]
    if not src.is_contiguous() or src.shape[0] != B * S_src:
        raise RuntimeError("lc2is_amd.rows_copy: src must be contiguous [B*S_src, C]")
    for t in (dst_f32, dst_bf16):
        if t is not None and (not t.is_contiguous() or tuple(t.shape) != (B * S_dst, Cc)):
            raise RuntimeError("lc2is_amd.rows_copy: dst must be contiguous [B*S_dst, C]")
    _lib.check(_fn("lc2is_rows_copy_bf16" if sb else "lc2is_rows_copy_f32")(_ptr(src), S_src, src_off, _ptr(dst_f32), _ptr(dst_bf16),
                                                                            S_dst, dst_off, B, n, Cc, _stream()), "rows_copy")


def sgd_step(params, grads, momentum_buf, lr, momentum=0.0, weight_decay=0.0, grad_scale=1.0):
    _chk(params, torch.float32, "params", 1); _chk(grads, torch.float32, "grads", 1)
    _lib.check(_fn("lc2is_sgd_step")(_ptr(params), _ptr(grads), _ptr(momentum_buf), params.numel(), lr, momentum,
                                     weight_decay, grad_scale, _stream()), "sgd_step")


def adamw_step(params, grads, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _chk(params, torch.float32, "params", 1); _chk(grads, torch.float32, "grads", 1)
    _lib.check(_fn("lc2is_adamw_step")(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), lr, beta1,
                                       beta2, eps, weight_decay, int(step), grad_scale, _stream()), "adamw_step")


# ---- the device-held optimizer path: the lc2is_optim_ctrl block as an int32 [OPTIM_CTRL_WORDS] tensor (floats through .view) ----
OPTIM_CTRL_WORDS = 12
(CTRL_CALLS, CTRL_APPLIED, CTRL_SKIPPED, CTRL_FINITE, CTRL_GRAD_NORM, CTRL_CLIP_COEF, CTRL_LR, CTRL_BC1, CTRL_BC2, CTRL_GRAD_MUL,
 CTRL_APPLY) = range(11)


def _chk_ctrl(ctrl):
    _chk(ctrl, torch.int32, "ctrl", 1)
    if ctrl.numel() != OPTIM_CTRL_WORDS:
        raise RuntimeError(f"lc2is_amd: ctrl must be an int32 [{OPTIM_CTRL_WORDS}] control block (lc2is_optim_ctrl)")


def _chk_same_numel(name, params, *others):
    for t in others:
        if t is not None:
            _chk(t, torch.float32, name + " buffer", 1)
            if t.numel() != params.numel():
                raise RuntimeError(f"lc2is_amd.{name}: every buffer must have params' {params.numel()} elements, got {t.numel()}")


def grad_sumsq(grads):
    """Pass 1 of the device-held optimizer path over a flat fp32 gradient (numel % 4 == 0): returns (partials fp32 [blocks],
    flags int32 [blocks]) — per-block sums of squares and "saw an inf / NaN" flags — as views of the stream's workspace, valid
    until the next grad_sumsq on this stream.  Fixed grid and summation order: bitwise reproducible."""
    _chk(grads, torch.float32, "grads", 1)
    n = grads.numel()
    nb = _fn("lc2is_grad_sumsq_blocks")(n)
    if nb <= 0:
        raise RuntimeError(f"lc2is_amd.grad_sumsq: numel must be a positive multiple of 4, got {n}")
    need = _fn("lc2is_grad_sumsq_workspace_bytes")(n)
    ws = workspace(need, grads.device, "grad_sumsq")
    _lib.check(_fn("lc2is_grad_sumsq")(_ptr(grads), n, _ptr(ws), ws.numel(), _stream()), "grad_sumsq")
    return ws[:4 * nb].view(torch.float32), ws[4 * nb:8 * nb].view(torch.int32)


def optim_ctrl_update(ctrl, partials, flags, lr_table, *, grad_scale=1.0, max_norm=float("inf"), skip_nonfinite=False,
                      beta1=0.0, beta2=0.0):
    """The one small launch between grad_sumsq and a _ctrl optimizer: global norm, clip coefficient, finite verdict, this call's
    rate from the DEVICE fp32 ``lr_table``, counters and AdamW bias corrections, all written into ``ctrl`` on the device."""
    _chk_ctrl(ctrl); _chk(partials, torch.float32, "partials", 1); _chk(flags, torch.int32, "flags", 1)
    _chk(lr_table, torch.float32, "lr_table", 1)
    if flags.numel() != partials.numel() or not partials.is_contiguous() or not flags.is_contiguous():
        raise RuntimeError("lc2is_amd.optim_ctrl_update: partials and flags must be contiguous and of one length")
    if lr_table.numel() < 1 or not lr_table.is_contiguous():
        raise RuntimeError("lc2is_amd.optim_ctrl_update: lr_table must be a non-empty contiguous fp32 tensor")
    _lib.check(_fn("lc2is_optim_ctrl_update")(_ptr(ctrl), _ptr(partials), _ptr(flags), partials.numel(), _ptr(lr_table),
                                              lr_table.numel(), grad_scale, max_norm, int(bool(skip_nonfinite)), beta1, beta2,
                                              _stream()), "optim_ctrl_update")


# ---- gradient accumulation: the lc2is_accum_block as an fp64 [4] tensor (32 bytes; ints and floats through .view) ----
ACCUM_BLOCK_BYTES = 32
ACCUM_LOSS_SUM, ACCUM_DENOM = 0, 1          # fp64 words
ACCUM_MICRO = 4                             # int32 word
ACCUM_LAST_LOSS, ACCUM_LAST_DENOM = 6, 7    # fp32 words


def _chk_accum(block):
    _chk(block, torch.float64, "accum block", 1)
    if block.numel() * 8 != ACCUM_BLOCK_BYTES or block.data_ptr() % 8:
        raise RuntimeError(f"lc2is_amd: the accumulation block must be an 8-byte aligned fp64 [{ACCUM_BLOCK_BYTES // 8}] tensor "
                           "(lc2is_accum_block)")


def accum_add(block, loss2):
    """One micro-batch joins an accumulation cycle: ``block`` (fp64 [4], lc2is_accum_block) takes ``loss_sum += loss2[0]``,
    ``denom += loss2[1]``, ``micro += 1`` in fp64 on the device.  ``loss2``: the fp32 [2] the fused head returns."""
    if block is None or loss2 is None:
        raise RuntimeError("lc2is_amd.accum_add: block and loss2 are required")
    _chk_accum(block); _chk(loss2, torch.float32, "loss2", 1)
    if loss2.numel() != 2 or loss2.device != block.device:
        raise RuntimeError("lc2is_amd.accum_add: loss2 must be the head's fp32 [2] (sum of losses, count) on the block's device")
    _lib.check(_fn("lc2is_accum_add")(_ptr(block), _ptr(loss2), _stream()), "accum_add")


def optim_ctrl_update_accum(ctrl, block, use_denom, partials, flags, lr_table, *, grad_scale=1.0, max_norm=float("inf"),
                            skip_nonfinite=False, beta1=0.0, beta2=0.0):
    """optim_ctrl_update for the call that closes an accumulation cycle: the gradient scale is ``grad_scale / block.denom`` (formed
    in fp64; 1 in place of a zero denominator, ``grad_scale`` alone with ``use_denom=False``), and the block then holds the cycle's
    mean loss and count in its ``last_*`` words and zeroed sums."""
    if block is None:
        raise RuntimeError("lc2is_amd.optim_ctrl_update_accum: block is required")
    _chk_ctrl(ctrl); _chk_accum(block); _chk(partials, torch.float32, "partials", 1); _chk(flags, torch.int32, "flags", 1)
    _chk(lr_table, torch.float32, "lr_table", 1)
    if flags.numel() != partials.numel() or not partials.is_contiguous() or not flags.is_contiguous():
        raise RuntimeError("lc2is_amd.optim_ctrl_update_accum: partials and flags must be contiguous and of one length")
    if lr_table.numel() < 1 or not lr_table.is_contiguous():
        raise RuntimeError("lc2is_amd.optim_ctrl_update_accum: lr_table must be a non-empty contiguous fp32 tensor")
    _lib.check(_fn("lc2is_optim_ctrl_update_accum")(_ptr(ctrl), _ptr(block), int(bool(use_denom)), _ptr(partials), _ptr(flags),
                                                    partials.numel(), _ptr(lr_table), lr_table.numel(), grad_scale, max_norm,
                                                    int(bool(skip_nonfinite)), beta1, beta2, _stream()),
               "optim_ctrl_update_accum")


def sgd_step_ctrl(params, grads, momentum_buf, ctrl, momentum=0.0, weight_decay=0.0, reverse=False):
    _chk(params, torch.float32, "params", 1); _chk_same_numel("sgd_step_ctrl", params, grads, momentum_buf); _chk_ctrl(ctrl)
    _lib.check(_fn("lc2is_sgd_step_ctrl")(_ptr(params), _ptr(grads), _ptr(momentum_buf), params.numel(), _ptr(ctrl), momentum,
                                          weight_decay, int(bool(reverse)), _stream()), "sgd_step_ctrl")


def adamw_step_ctrl(params, grads, m, v, ctrl, beta1, beta2, eps, weight_decay, reverse=False):
    _chk(params, torch.float32, "params", 1); _chk_same_numel("adamw_step_ctrl", params, grads, m, v); _chk_ctrl(ctrl)
    _lib.check(_fn("lc2is_adamw_step_ctrl")(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), _ptr(ctrl), beta1,
                                            beta2, eps, weight_decay, int(bool(reverse)), _stream()), "adamw_step_ctrl")


# ---- parameter groups: one launch over the arena, a learning-rate factor and a weight decay per 64-element granule ----
GROUP_GRANULE, MAX_PARAM_GROUPS, GROUP_SKIP = 64, 255, 255


def _chk_groups(name, params, granule_group, groups):
    _chk(granule_group, torch.uint8, "granule_group", 1); _chk(groups, torch.float32, "groups", 2)
    if granule_group is None or groups is None:
        raise RuntimeError(f"lc2is_amd.{name}: granule_group and groups are required")
    n = params.numel()
    if n == 0 or n % GROUP_GRANULE:
        raise RuntimeError(f"lc2is_amd.{name}: numel must be a positive multiple of {GROUP_GRANULE}, got {n}")
    if not params.is_contiguous() or not granule_group.is_contiguous() or granule_group.numel() != n // GROUP_GRANULE:
        raise RuntimeError(f"lc2is_amd.{name}: granule_group must be a contiguous uint8 [{n // GROUP_GRANULE}] map (one id per "
                           f"{GROUP_GRANULE} elements), got {tuple(granule_group.shape)}")
    if not groups.is_contiguous() or groups.shape[1] != 2 or not 1 <= groups.shape[0] <= MAX_PARAM_GROUPS:
        raise RuntimeError(f"lc2is_amd.{name}: groups must be a contiguous fp32 [ngroups, 2] table of (lr_scale, weight_decay), "
                           f"1 <= ngroups <= {MAX_PARAM_GROUPS}, got {tuple(groups.shape)}")


def sgd_step_groups(params, grads, momentum_buf, ctrl, granule_group, groups, momentum=0.0, reverse=False):
    """sgd_step_ctrl in one launch over the whole arena with per-group constants: ``granule_group`` (uint8 [numel / 64]) names the
    group of each 64-element granule (GROUP_SKIP = 255: the granule is neither read nor written), ``groups`` (fp32 [ngroups, 2])
    holds (lr_scale, weight_decay); the rate of a group is ctrl's lr * lr_scale."""
    _chk(params, torch.float32, "params", 1); _chk_same_numel("sgd_step_groups", params, grads, momentum_buf); _chk_ctrl(ctrl)
    _chk_groups("sgd_step_groups", params, granule_group, groups)
    _lib.check(_fn("lc2is_sgd_step_groups")(_ptr(params), _ptr(grads), _ptr(momentum_buf), params.numel(), _ptr(ctrl),
                                            _ptr(granule_group), _ptr(groups), groups.shape[0], momentum, int(bool(reverse)),
                                            _stream()), "sgd_step_groups")


def adamw_step_groups(params, grads, m, v, ctrl, granule_group, groups, beta1, beta2, eps, reverse=False):
    """adamw_step_ctrl in one launch over the whole arena with per-group (lr_scale, weight_decay): see sgd_step_groups."""
    _chk(params, torch.float32, "params", 1); _chk_same_numel("adamw_step_groups", params, grads, m, v); _chk_ctrl(ctrl)
    _chk_groups("adamw_step_groups", params, granule_group, groups)
    _lib.check(_fn("lc2is_adamw_step_groups")(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), _ptr(ctrl),
                                              _ptr(granule_group), _ptr(groups), groups.shape[0], beta1, beta2, eps,
                                              int(bool(reverse)), _stream()), "adamw_step_groups")


# ---- weight EMA on the device: follows the control block's verdict and counter; evaluated through an in-place exchange ----
def ema_update_ctrl(ema, params, ctrl, one_minus_decay, warmup=False, every=1, reverse=False):
    """ema += w * (params - ema) over two flat fp32 buffers of one length, unless ``ctrl`` says this step was skipped or
    ``applied % every != 0`` (then nothing is read or written).  ``one_minus_decay``: 1 - decay, formed in fp64 by the caller (it is
    rounded to fp32 once, here); ``warmup``: the j-th update takes max(w, 9 / (10 + j)).  Elements equal to the parameter bit for
    bit keep their bits."""
    _chk(ema, torch.float32, "ema", 1); _chk_same_numel("ema_update_ctrl", ema, params); _chk_ctrl(ctrl)
    if params is None:
        raise RuntimeError("lc2is_amd.ema_update_ctrl: params is required")
    _lib.check(_fn("lc2is_ema_update_ctrl")(_ptr(ema), _ptr(params), ema.numel(), _ptr(ctrl), float(one_minus_decay),
                                            int(bool(warmup)), int(every), int(bool(reverse)), _stream()), "ema_update_ctrl")


def swap_f32(a, b):
    """Exchange the contents of two equal-length, non-overlapping flat fp32 buffers in place, bit for bit."""
    _chk(a, torch.float32, "a", 1); _chk_same_numel("swap_f32", a, b)
    if b is None:
        raise RuntimeError("lc2is_amd.swap_f32: b is required")
    _lib.check(_fn("lc2is_swap_f32")(_ptr(a), _ptr(b), a.numel(), _stream()), "swap_f32")


def finite_ge(v, lo: float = 0.0) -> bool:
    """``v`` is a finite number >= lo and not a bool: the test every option validator of the losses applies."""
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v) and v >= lo


def _head_front(who: str, scores_lo, labels, B: int, h: int, w: int, C: int, S: int, *, need_labels: bool, scales=None,
                cmax: int = 0, cmin: int | None = None):
    """The checks every ``head_upsample_*`` wrapper runs on its tensors, in one order: scores contiguous, labels [B, h S, w S] and
    contiguous (required or optional), then — where the wrapper names its ``scales``, (4,) or (4, 8, 16) — S among them and scores_lo [B h w, ld] with
    (cmin <=) C <= ld <= cmax, ld a multiple of 64.  Returns ld."""
    if scores_lo is None or not scores_lo.is_contiguous():
        raise RuntimeError(f"lc2is_amd.{who}: scores_lo must be contiguous")
    if (need_labels or labels is not None) and (labels is None or tuple(labels.shape) != (B, h * S, w * S)
                                                or not labels.is_contiguous()):
        raise RuntimeError(f"lc2is_amd.{who}: labels must be contiguous [{B},{h*S},{w*S}]")
    ld = scores_lo.shape[1]
    if scales is None:
        return ld
    if S not in scales:
        raise RuntimeError(f"lc2is_amd.{who}: S must be {'4' if scales == (4,) else '4, 8 or 16'}, got {S}")
    if scores_lo.shape[0] != B * h * w or (cmin is not None and C < cmin) or not C <= ld <= cmax or ld % 64:
        raise RuntimeError(f"lc2is_amd.{who}: scores_lo must be [{B * h * w}, ld] with C <= ld <= {cmax}, ld % 64 == 0, "
                           f"got {tuple(scores_lo.shape)}")
    return ld


def _head_alloc(who: str, scores_lo, nbytes: int, want_grad: bool, geom, nloss: int = 2):
    """(loss block, dscores_lo or None, workspace) of a head call whose launches hand partials to a fixed-order finish launch: all
    overwritten, the workspace per call (its slabs live until the last launch, in stream order).  ``nbytes`` == 0: the C side does
    not take this geometry."""
    if nbytes == 0:
        B, h, w, C, S, mode = geom
        raise RuntimeError(f"lc2is_amd.{who}: unsupported call B={B} h={h} w={w} C={C} S={S} mode={mode}")
    dev = scores_lo.device
    loss = torch.empty(nloss, dtype=torch.float32, device=dev)
    dlo = torch.empty(scores_lo.shape, dtype=torch.float32, device=dev) if want_grad else None
    return loss, dlo, torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _nchw_front(who: str, logits, labels, *, bwd: bool = False, lse=(), cmax: int | None = None):
    """The checks of the ``*_nchw_fwd`` / ``*_nchw_bwd`` wrappers on contiguous logits [B,C,H,W] and labels [B,H,W] (a backward: and
    the forward's ``lse``, given as a 1-tuple, in one message); ``cmax``: the class limit of a forward.  Returns (B, C, H, W)."""
    if not bwd and (logits is None or labels is None or not logits.is_contiguous() or not labels.is_contiguous()):
        raise RuntimeError(f"lc2is_amd.{who}: logits/labels must be contiguous")
    B, Cc, H, W = logits.shape
    if not bwd and tuple(labels.shape) != (B, H, W):
        raise RuntimeError(f"lc2is_amd.{who}: labels must be [{B},{H},{W}]")
    if bwd and (not logits.is_contiguous() or not labels.is_contiguous() or tuple(labels.shape) != (B, H, W)
                or any(tuple(t.shape) != (B, H, W) or not t.is_contiguous() for t in lse)):
        raise RuntimeError(f"lc2is_amd.{who}: contiguous logits [B,C,H,W] with labels{' / lse' if lse else ''} [{B},{H},{W}] required")
    if cmax is not None and not 1 <= Cc <= cmax:
        raise RuntimeError(f"lc2is_amd.{who}: 1 <= C <= {cmax} required, got {Cc}")
    return B, Cc, H, W


def _chk_grad_px(who: str, grad_px, B: int, H: int, W: int) -> None:
    if grad_px is not None:
        _chk(grad_px, torch.float32, "grad_px", 3)
        if tuple(grad_px.shape) != (B, H, W) or not grad_px.is_contiguous():
            raise RuntimeError(f"lc2is_amd.{who}: grad_px must be contiguous [{B},{H},{W}]")


def _chk_nchw_bwd(logits, labels, lse, grad_scale_dev) -> None:
    """The dtype checks every ``*_nchw_bwd`` opens with (``lse``: None for the sigmoid losses, which save none)."""
    _chk(logits, torch.float32, "logits", 4); _chk(labels, torch.int64, "labels", 3)
    _chk(lse, torch.float32, "lse", 3); _chk(grad_scale_dev, torch.float32, "grad_scale_dev", 1)


def _nchw_fwd_alloc(logits, B: int, H: int, W: int, per_pixel: bool, lse: bool = True):
    """What an ordered ``*_nchw_fwd`` allocates: loss[2] (overwritten: block partials summed in a fixed order), the partials
    workspace (per call, like head_upsample_ce's slabs) and its byte count, lse [B,H,W] or None, the per-pixel map or None."""
    dev = logits.device
    nbytes = _fn("lc2is_ce_nchw_fwd_workspace_bytes")(B, H * W)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lse_map = torch.empty((B, H, W), dtype=torch.float32, device=dev) if lse else None
    lpx = torch.empty((B, H, W), dtype=torch.float32, device=dev) if per_pixel else None
    return loss, ws, nbytes, lse_map, lpx


def _ce_options(class_weight, label_smoothing: float, C: int, dev):
    """Validate F.cross_entropy's weight / label_smoothing for a C-class call; True when either is set."""
    if not 0.0 <= label_smoothing <= 1.0:
        raise RuntimeError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
    if class_weight is None:
        return label_smoothing != 0.0
    if class_weight.dim() != 1 or class_weight.numel() != C:   # torch's message (aten LossNLL.cpp)
        raise RuntimeError(f"weight tensor should be defined either for all {C} classes or no classes but got weight "
                           f"tensor of shape: {list(class_weight.shape)}")
    _chk(class_weight, torch.float32, "class_weight", 1)
    if class_weight.device != dev:
        raise RuntimeError(f"lc2is_amd: class_weight must be on {dev}, got {class_weight.device}")
    return True


def head_upsample_ce(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                     want_grad: bool = False, want_scores: bool = False, want_loss: bool = True,
                     ignore_index: int = -100, grad_scale: float = 1.0, class_weight=None, label_smoothing: float = 0.0):
    """scores_lo fp32 [B*h*w, ld].  Returns (loss_sum[2] or None, dscores_lo or None, scores_hi NCHW or None).
    class_weight (fp32 [C] on the device) / label_smoothing: F.cross_entropy's options (S = 4 / 8 / 16); loss_sum[1] is then
    the weighted count sum_i w_{y_i}, the denominator of the mean."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    opts = _ce_options(class_weight, label_smoothing, C, scores_lo.device) and want_loss
    ld = _head_front("head_upsample_ce", scores_lo, labels, B, h, w, C, S, need_labels=False)
    dev = scores_lo.device
    # S = 4 / 8 / 16: per-block partials in a workspace + a fixed-order second launch (reproducible; outputs overwritten);
    # other S: the atomic path adds into cleared buffers
    nbytes = _fn("lc2is_head_upsample_ce_workspace_bytes")(B, h, w, C, S, mode, int(want_grad)) if want_loss else 0
    alloc = torch.empty if nbytes else torch.zeros
    loss = alloc(2, dtype=torch.float32, device=dev) if want_loss else None
    dlo = alloc(scores_lo.shape, dtype=torch.float32, device=dev) if want_grad else None
    hi = torch.empty((B, C, h * S, w * S), dtype=torch.float32, device=dev) if want_scores else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None   # (per call: the slabs live until the second launch, in stream order)
    if opts:
        rc = _fn("lc2is_head_upsample_ce_opts")(_ptr(scores_lo), ld, _ptr(labels), _ptr(dlo), _ptr(hi), _ptr(loss), B, h,
                                                w, C, S, mode, ignore_index, grad_scale, _ptr(class_weight),
                                                label_smoothing, _ptr(ws), nbytes, _stream())
    else:
        rc = _fn("lc2is_head_upsample_ce")(_ptr(scores_lo), ld, _ptr(labels), _ptr(dlo), _ptr(hi), _ptr(loss), B, h,
                                           w, C, S, mode, ignore_index, grad_scale, _ptr(ws), nbytes, _stream())
    _lib.check(rc, f"head_upsample_ce B={B} h={h} w={w} C={C} S={S}")
    return loss, dlo, hi


# ---- online hard example mining: per-pixel loss of the fused head, exact k-th largest on the device, relabelling ----
def head_upsample_px(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                     ignore_index: int = -100):
    """scores_lo fp32 [B*h*w, ld], labels int64 [B, h*S, w*S] -> per-pixel plain CE of the upsampled scores, fp32 [B, h*S, w*S]
    (0 where the pixel is not counted): head_upsample_ce's forward alone (S = 4 / 8 / 16), one launch, no gradient."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    ld = _head_front("head_upsample_px", scores_lo, labels, B, h, w, C, S, need_labels=True)
    lpx = torch.empty((B, h * S, w * S), dtype=torch.float32, device=scores_lo.device)
    _lib.check(_fn("lc2is_head_upsample_px")(_ptr(scores_lo), ld, _ptr(labels), _ptr(lpx), B, h, w, C, S, mode,
                                             ignore_index, _stream()), f"head_upsample_px B={B} h={h} w={w} C={C} S={S}")
    return lpx


# ---- class map and accuracy / IoU counts of the fused head: the argmax sibling of head_upsample_px ----
def head_upsample_argmax(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                         ignore_index: int = -100, want_pred: bool = True, want_counts: bool = True):
    """scores_lo fp32 [B*h*w, ld], labels int64 [B, h*S, w*S] or None -> (pred uint8 [B, h*S, w*S] or None, counts int32 [B, 3, C]
    or None): the argmax over the C classes of the upsampled scores (S = 4 / 8 / 16; exact ties to the lowest class) and, per image,
    the {intersection, predicted, labelled} counts over the pixels the loss counts (label != ignore_index and 0 <= label < C).  The
    [B, C, H, W] map is never formed; nothing syncs, no atomics, the same bytes every run, captures into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    if not want_pred and not want_counts:
        raise ValueError("lc2is_amd.head_upsample_argmax: want_pred and want_counts are both False")
    if want_counts and labels is None:
        raise ValueError("lc2is_amd.head_upsample_argmax: want_counts needs labels")
    ld = _head_front("head_upsample_argmax", scores_lo, labels, B, h, w, C, S, need_labels=False, scales=(4, 8, 16), cmax=HEAD_CMAX)
    dev = scores_lo.device
    nbytes = 0
    if want_counts:
        nbytes = _fn("lc2is_head_upsample_argmax_workspace_bytes")(B, h, w, C, S, mode)
        if nbytes == 0:
            raise RuntimeError(f"lc2is_amd.head_upsample_argmax: unsupported call B={B} h={h} w={w} C={C} S={S} mode={mode}")
    pred = torch.empty((B, h * S, w * S), dtype=torch.uint8, device=dev) if want_pred else None
    counts = torch.empty((B, 3, C), dtype=torch.int32, device=dev) if want_counts else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None   # (per call: the slabs live until the second launch)
    _lib.check(_fn("lc2is_head_upsample_argmax")(_ptr(scores_lo), ld, _ptr(labels), _ptr(pred), _ptr(counts), B, h, w, C, S, mode,
                                                 ignore_index, _ptr(ws), nbytes, _stream()),
               f"head_upsample_argmax B={B} h={h} w={w} C={C} S={S}")
    return pred, counts


# ---- the fused head past 192 classes: the class axis walked in chunks of 192 channels (head_wide.hip) ----
HEAD_CMAX = 192            # classes the narrow head kernels take (every criterion, S = 4 / 8 / 16)
HEAD_WIDE_CMAX = 1024      # LC2IS_HEAD_WIDE_CMAX: classes the wide cross-entropy / argmax kernels take (S = 4)


def class_pad(K: int) -> int:
    """Channel pitch of the low-resolution score map of a K-class head: 192 up to 192 classes (the narrow kernels' one shape),
    else K rounded up to 64."""
    return HEAD_CMAX if K <= HEAD_CMAX else (K + 63) // 64 * 64


def head_upsample_ce_wide(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                          want_grad: bool = False, ignore_index: int = -100, grad_scale: float = 1.0, class_weight=None):
    """Cross-entropy of the x4-upsampled scores for up to 1024 classes: scores_lo fp32 [B*h*w, ld], labels int64 [B, 4h, 4w].
    Returns (loss2 = [sum of w_y (lse - z_y), sum of w_y over the counted pixels], dscores_lo or None = grad_scale * d loss2[0] /
    d scores_lo, every one of the ld channels written).  ``head_upsample_ce(class_weight=...)`` without label smoothing, the class
    axis walked in chunks of 192 channels: an online-softmax sweep, a gradient sweep and the finish launch; nothing syncs, no
    atomics, the same bytes every run, captures into a graph.  C <= 192 is taken too (the narrow call is the faster one there)."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    ld = _head_front("head_upsample_ce_wide", scores_lo, labels, B, h, w, C, S, need_labels=True, scales=(4,), cmax=HEAD_WIDE_CMAX,
                     cmin=1)
    _ce_options(class_weight, 0.0, C, scores_lo.device)
    nbytes = _fn("lc2is_head_upsample_ce_wide_workspace_bytes")(B, h, w, C, ld, S, mode, int(want_grad))
    loss, dlo, ws = _head_alloc("head_upsample_ce_wide", scores_lo, nbytes, want_grad, (B, h, w, C, S, mode))
    _lib.check(_fn("lc2is_head_upsample_ce_wide")(_ptr(scores_lo), ld, _ptr(labels), _ptr(dlo), _ptr(loss), B, h, w, C, S, mode,
                                                  ignore_index, grad_scale, _ptr(class_weight), _ptr(ws), nbytes, _stream()),
               f"head_upsample_ce_wide B={B} h={h} w={w} C={C} S={S}")
    return loss, dlo


def head_upsample_argmax_wide(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                              ignore_index: int = -100, want_pred: bool = True, want_counts: bool = True):
    """``head_upsample_argmax`` for up to 1024 classes (S = 4): (pred int16 [B, 4h, 4w] or None, counts int32 [B, 3, C] or None).
    The class axis is walked in chunks of 192 channels with a running (value, class) per pixel; exact ties go to the lowest class."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    if not want_pred and not want_counts:
        raise ValueError("lc2is_amd.head_upsample_argmax_wide: want_pred and want_counts are both False")
    if want_counts and labels is None:
        raise ValueError("lc2is_amd.head_upsample_argmax_wide: want_counts needs labels")
    ld = _head_front("head_upsample_argmax_wide", scores_lo, labels, B, h, w, C, S, need_labels=False, scales=(4,),
                     cmax=HEAD_WIDE_CMAX, cmin=1)
    dev = scores_lo.device
    nbytes = 0
    if want_counts:
        nbytes = _fn("lc2is_head_upsample_argmax_wide_workspace_bytes")(B, h, w, C, S, mode)
        if nbytes == 0:
            raise RuntimeError(f"lc2is_amd.head_upsample_argmax_wide: unsupported call B={B} h={h} w={w} C={C} S={S} mode={mode}")
    pred = torch.empty((B, h * S, w * S), dtype=torch.int16, device=dev) if want_pred else None
    counts = torch.empty((B, 3, C), dtype=torch.int32, device=dev) if want_counts else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None   # (per call: the slabs live until the second launch)
    _lib.check(_fn("lc2is_head_upsample_argmax_wide")(_ptr(scores_lo), ld, _ptr(labels), _ptr(pred), _ptr(counts), B, h, w, C, S,
                                                      mode, ignore_index, _ptr(ws), nbytes, _stream()),
               f"head_upsample_argmax_wide B={B} h={h} w={w} C={C} S={S}")
    return pred, counts


# ---- self-training: the teacher's confidence and pseudo-labels, and the cross-entropy with a per-pixel weight (head_selftrain.hip) ----
def conf_thresh(thresh) -> float:
    """``thresh`` of a pseudo-labelling call, validated: a number in [0, 1] (a NaN is refused)."""
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not 0.0 <= thresh <= 1.0:
        raise ValueError(f"lc2is_amd: the confidence threshold must be a number in [0, 1], got {thresh!r}")
    return float(thresh)


def head_upsample_conf(scores_lo, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *, thresh=None,
                       ignore_index: int = -100, want_pred: bool = True, want_conf: bool = True, want_counts: bool = False):
    """scores_lo fp32 [B*h*w, ld] -> (pred uint8 [B, h*S, w*S], conf fp32 [B, h*S, w*S], pseudo int64 [B, h*S, w*S], counts int32
    [B, 2]), None for what was not asked: the argmax over the C classes of the upsampled scores (S = 4 / 8 / 16; the bytes of
    ``head_upsample_argmax``) and its softmax probability.  With ``thresh`` (a number in [0, 1]): ``pseudo`` = the class where
    conf >= thresh, else ``ignore_index``, and (``want_counts``) per image {pixels with conf >= thresh, pixels of the image}.  A
    pixel whose scores are all -inf or hold a NaN / +inf gets conf = 1 / C: conf is always finite and in (0, 1].  The [B, C, H, W]
    map is never formed; nothing syncs, no atomics, the same bytes every run, captures into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo")
    if thresh is None:
        if want_counts:
            raise ValueError("lc2is_amd.head_upsample_conf: want_counts needs thresh")
        if not want_pred and not want_conf:
            raise ValueError("lc2is_amd.head_upsample_conf: nothing requested (want_pred and want_conf are False, no thresh)")
    else:
        thresh = conf_thresh(thresh)
    ld = _head_front("head_upsample_conf", scores_lo, None, B, h, w, C, S, need_labels=False, scales=(4, 8, 16), cmax=HEAD_CMAX)
    dev = scores_lo.device
    nbytes = 0
    if want_counts:
        nbytes = _fn("lc2is_head_upsample_conf_workspace_bytes")(B, h, w, C, S, mode)
        if nbytes == 0:
            raise RuntimeError(f"lc2is_amd.head_upsample_conf: unsupported call B={B} h={h} w={w} C={C} S={S} mode={mode}")
    shape = (B, h * S, w * S)
    pred = torch.empty(shape, dtype=torch.uint8, device=dev) if want_pred else None
    conf = torch.empty(shape, dtype=torch.float32, device=dev) if want_conf else None
    pseudo = torch.empty(shape, dtype=torch.int64, device=dev) if thresh is not None else None
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev) if want_counts else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None   # (per call: the slabs live until the second launch)
    _lib.check(_fn("lc2is_head_upsample_conf")(_ptr(scores_lo), ld, _ptr(pred), _ptr(conf), _ptr(pseudo), _ptr(counts), B, h, w, C, S,
                                               mode, 0.0 if thresh is None else thresh, ignore_index, _ptr(ws), nbytes, _stream()),
               f"head_upsample_conf B={B} h={h} w={w} C={C} S={S}")
    return pred, conf, pseudo, counts


def check_pixel_weight(who: str, pixel_weight, shape, dev=None) -> None:
    """``pixel_weight`` of a loss call: a contiguous fp32 tensor of the labels' shape that does not require grad (on ``dev`` where
    given).  Its values must be finite and >= 0, which is documented and not checked (no host sync)."""
    if not isinstance(pixel_weight, torch.Tensor) or pixel_weight.dtype != torch.float32:
        raise ValueError(f"lc2is_amd {who}: pixel_weight must be a float32 tensor, got "
                         f"{getattr(pixel_weight, 'dtype', type(pixel_weight).__name__)}")
    if pixel_weight.requires_grad:
        raise ValueError(f"lc2is_amd {who}: pixel_weight must not require grad (the loss is not differentiated with respect to it)")
    if shape is not None and (tuple(pixel_weight.shape) != tuple(shape) or not pixel_weight.is_contiguous()):
        raise ValueError(f"lc2is_amd {who}: pixel_weight must be contiguous {list(shape)} (the labels' shape), got "
                         f"{list(pixel_weight.shape)}")
    if dev is not None and pixel_weight.device != dev:
        raise ValueError(f"lc2is_amd {who}: pixel_weight must be on {dev}, got {pixel_weight.device}")


def head_upsample_ce_pw(scores_lo, labels, pixel_weight, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                        want_grad: bool = False, ignore_index: int = -100, grad_scale: float = 1.0, class_weight=None,
                        label_smoothing: float = 0.0):
    """``head_upsample_ce`` (class_weight / label_smoothing) with a per-pixel weight: scores_lo fp32 [B*h*w, ld], labels int64 and
    pixel_weight fp32 (contiguous, finite and >= 0: not checked) [B, h*S, w*S].  Returns (loss2, dscores_lo or None): loss2[0] =
    sum_i pw_i l_i over the counted pixels, loss2[1] = sum_i w_{y_i} — NOT multiplied by pw_i: the denominator of the mean stays the
    unweighted call's, so pixel_weight == 1 is that loss and a per-image weight scales the image's loss instead of cancelling.
    dscores_lo = grad_scale * d loss2[0] / d scores_lo.  One forward + backward launch and the finish launch of ``head_upsample_ce``
    (S = 4 / 8 / 16, C <= 192); nothing syncs, no atomics, the same bytes every run, captures into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    _ce_options(class_weight, label_smoothing, C, scores_lo.device)
    ld = _head_front("head_upsample_ce_pw", scores_lo, labels, B, h, w, C, S, need_labels=True, scales=(4, 8, 16), cmax=HEAD_CMAX)
    check_pixel_weight("head_upsample_ce_pw", pixel_weight, labels.shape, scores_lo.device)
    nbytes = _fn("lc2is_head_upsample_ce_workspace_bytes")(B, h, w, C, S, mode, int(want_grad))
    loss, dlo, ws = _head_alloc("head_upsample_ce_pw", scores_lo, nbytes, want_grad, (B, h, w, C, S, mode))
    _lib.check(_fn("lc2is_head_upsample_ce_pw")(_ptr(scores_lo), ld, _ptr(labels), _ptr(pixel_weight), _ptr(dlo), _ptr(loss), B, h, w,
                                                C, S, mode, ignore_index, grad_scale, _ptr(class_weight), label_smoothing, _ptr(ws),
                                                nbytes, _stream()), f"head_upsample_ce_pw B={B} h={h} w={w} C={C} S={S}")
    return loss, dlo


# ---- distillation: per-pixel KL to a teacher's low-resolution scores (head_distill.hip) ----
def kd_temperature(temperature) -> float:
    """``temperature`` of a distillation call, validated: a finite number > 0."""
    if not finite_ge(temperature) or temperature <= 0:
        raise ValueError(f"lc2is_amd: the distillation temperature must be a finite number > 0, got {temperature!r}")
    return float(temperature)


def check_teacher_scores(who: str, teacher_lo, shape=None, dev=None) -> None:
    """``teacher_lo`` of a distillation call: a contiguous fp32 tensor that does not require grad, of the student's low-resolution
    shape and on its device where those are given."""
    if not isinstance(teacher_lo, torch.Tensor) or teacher_lo.dtype != torch.float32:
        raise ValueError(f"lc2is_amd {who}: the teacher's scores must be a float32 tensor, got "
                         f"{getattr(teacher_lo, 'dtype', type(teacher_lo).__name__)}")
    if teacher_lo.requires_grad:
        raise ValueError(f"lc2is_amd {who}: the teacher's scores must not require grad (nothing flows to the teacher; take them "
                         "under no_grad or detach them)")
    if not teacher_lo.is_contiguous() or (shape is not None and tuple(teacher_lo.shape) != tuple(shape)):
        raise ValueError(f"lc2is_amd {who}: the teacher's scores must be contiguous{'' if shape is None else ' ' + str(list(shape))} "
                         f"(the student's low-resolution scores' shape), got {list(teacher_lo.shape)}")
    if dev is not None and teacher_lo.device != dev:
        raise ValueError(f"lc2is_amd {who}: the teacher's scores must be on {dev}, got {teacher_lo.device}")


def head_upsample_kd(scores_lo, teacher_lo, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                     temperature: float = 1.0, labels=None, pixel_weight=None, want_grad: bool = False, ignore_index: int = -100,
                     grad_scale: float = 1.0):
    """Per-pixel KL(teacher || student) of the upsampled scores at a temperature T: scores_lo and teacher_lo fp32 [B*h*w, ld]
    (the teacher contiguous, the student's shape and device, no grad).  Counted pixels: every pixel without ``labels``; with them
    (int64 [B, h*S, w*S]) the pixels the cross-entropy counts.  ``pixel_weight`` fp32 [B, h*S, w*S] (finite, >= 0: not checked) or
    None.  Returns (loss2, dscores_lo or None): loss2[0] = sum_i pw_i T^2 KL_i, loss2[1] = the number of counted pixels (NOT
    multiplied by pw_i), dscores_lo = grad_scale * d loss2[0] / d scores_lo = grad_scale pw_i T (p_s - p_t) pulled through the
    upsample; the teacher gets no gradient.  teacher_lo == scores_lo gives exactly 0 and 0.  One forward + backward launch and the
    finish launch of ``head_upsample_ce`` (S = 4 / 8 / 16, C <= 192); nothing syncs, no atomics, the same bytes every run, captures
    into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    temperature = kd_temperature(temperature)
    ld = _head_front("head_upsample_kd", scores_lo, labels, B, h, w, C, S, need_labels=False, scales=(4, 8, 16), cmax=HEAD_CMAX)
    check_teacher_scores("head_upsample_kd", teacher_lo, scores_lo.shape, scores_lo.device)
    if pixel_weight is not None:
        check_pixel_weight("head_upsample_kd", pixel_weight, (B, h * S, w * S), scores_lo.device)
    nbytes = _fn("lc2is_head_upsample_ce_workspace_bytes")(B, h, w, C, S, mode, int(want_grad))
    loss, dlo, ws = _head_alloc("head_upsample_kd", scores_lo, nbytes, want_grad, (B, h, w, C, S, mode))
    _lib.check(_fn("lc2is_head_upsample_kd")(_ptr(scores_lo), _ptr(teacher_lo), ld, _ptr(labels), _ptr(pixel_weight), _ptr(dlo),
                                             _ptr(loss), B, h, w, C, S, mode, ignore_index, temperature, grad_scale, _ptr(ws), nbytes,
                                             _stream()), f"head_upsample_kd B={B} h={h} w={w} C={C} S={S}")
    return loss, dlo


def seg_counts_add(seg_counts, scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int, ignore_index: int):
    """``seg_counts += counts.sum(0)`` for the batch behind ``scores_lo``: what every fused head does for ``seg_counts=``.  int64
    [3, C] on the device, added in place by one small device op (no host read).  Past 192 classes the wide kernel counts."""
    check_seg_counts(seg_counts, C)
    argmax = head_upsample_argmax_wide if C > HEAD_CMAX else head_upsample_argmax
    _, counts = argmax(scores_lo, labels, B, h, w, C, S, mode, ignore_index=ignore_index, want_pred=False)
    seg_counts.add_(counts.sum(0))


def check_seg_counts(seg_counts, C: int | None = None) -> None:
    """``seg_counts`` of the fused heads: an int64 [3, C] tensor on a HIP device (TypeError / ValueError / RuntimeError otherwise)."""
    if not isinstance(seg_counts, torch.Tensor) or seg_counts.dtype != torch.int64:
        raise TypeError("lc2is_amd: seg_counts must be an int64 [3, K] tensor on the device")
    if seg_counts.dim() != 2 or seg_counts.shape[0] != 3 or (C is not None and seg_counts.shape[1] != C) or not seg_counts.is_contiguous():
        raise ValueError(f"lc2is_amd: seg_counts must be a contiguous int64 [3, {'K' if C is None else C}] tensor, "
                         f"got {tuple(seg_counts.shape)}")
    if not seg_counts.is_cuda:
        raise RuntimeError("lc2is_amd: seg_counts must be a CUDA(HIP) tensor; there is no CPU path")


OHEM_INFO_WORDS = 3   # lc2is_ohem_info as int64 [3]: n_valid, k, then (L, L_eff) as the two fp32 halves of the third word


def ohem_loss_thresh(thresh: float) -> float:
    """-log(thresh) formed in fp64 and rounded to fp32 once: the loss a pixel must exceed when the threshold binds."""
    if not 0.0 < thresh <= 1.0:
        raise ValueError(f"OHEM thresh must be in (0, 1], got {thresh}")
    return float(torch.tensor(-math.log(thresh), dtype=torch.float64).to(torch.float32))


def ohem_select(loss_px, labels, C: int, thresh: float, min_kept_total: int, ignore_index: int = -100):
    """Hard-pixel selection over all ``loss_px.numel()`` pixels: returns (labels_out, info).  A pixel is valid iff
    label != ignore_index and 0 <= label < C; k = min(min_kept_total, n_valid - 1); L = the valid loss of rank k (descending);
    L_eff = min(L, fp32(-log(thresh))); labels_out = label where valid and loss > L_eff, ignore_index elsewhere.  ``info``: the
    device block lc2is_ohem_info as int64 [3] (``ohem_info_fields`` reads it; nothing here syncs).  Exact, no atomics, the same
    bytes every run; captures into a graph."""
    _chk(loss_px, torch.float32, "loss_px", None); _chk(labels, torch.int64, "labels", None)
    if loss_px is None or labels is None or loss_px.shape != labels.shape or not loss_px.is_contiguous() or not labels.is_contiguous():
        raise RuntimeError("lc2is_amd.ohem_select: loss_px (fp32) and labels (int64) must be contiguous and of one shape")
    if int(min_kept_total) < 0:
        raise ValueError(f"OHEM min_kept must be >= 0, got {min_kept_total}")
    tau = ohem_loss_thresh(thresh)
    n = loss_px.numel()
    need = _fn("lc2is_ohem_select_workspace_bytes")(n)
    if need == 0:
        raise RuntimeError(f"lc2is_amd.ohem_select: 1 <= numel < 2^31 required, got {n}")
    dev = loss_px.device
    ws = workspace(need, dev, "ohem_select")
    out = torch.empty_like(labels)
    info = torch.empty(OHEM_INFO_WORDS, dtype=torch.int64, device=dev)
    _lib.check(_fn("lc2is_ohem_select")(_ptr(loss_px), _ptr(labels), _ptr(out), n, C, ignore_index, tau, int(min_kept_total),
                                        _ptr(info), _ptr(ws), ws.numel(), _stream()), f"ohem_select n={n}")
    return out, info


def ohem_info_fields(info) -> dict:
    """The info block of ``ohem_select`` on the host (this reads the device: a sync): n_valid, k, L, L_eff."""
    host = info.detach().cpu()
    L, L_eff = host[2:3].view(torch.float32).tolist()
    return dict(n_valid=int(host[0]), k=int(host[1]), L=L, L_eff=L_eff)


def ohem_labels(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int, ignore_index: int, ohem):
    """The two launches every fused head shares in front of its CE call: per-pixel loss of the upsampled scores, then the
    selection.  ``ohem`` = (thresh, min_kept per image).  Returns (labels_out, info)."""
    thresh, min_kept = ohem
    lpx = head_upsample_px(scores_lo, labels, B, h, w, C, S, mode, ignore_index=ignore_index)
    return ohem_select(lpx, labels, C, thresh, int(min_kept) * B, ignore_index)


# ---- soft Dice + cross-entropy: batch statistics on the device, then the gradient pass ----
DICE_CMAX = 192   # classes the Dice kernels take (the fused head's limit)


def dice_options(ce_weight, dice_weight, smooth, present_only) -> tuple[float, float, float, bool]:
    """(ce_weight, dice_weight, smooth, present_only) of a Dice + CE loss, validated: finite numbers >= 0, the two weights not
    both 0, present_only a bool."""
    for name, v in (("ce_weight", ce_weight), ("dice_weight", dice_weight), ("smooth", smooth)):
        if not finite_ge(v):
            raise ValueError(f"Dice + CE: {name} must be a finite number >= 0, got {v!r}")
    if float(ce_weight) == 0.0 and float(dice_weight) == 0.0:
        raise ValueError("Dice + CE: ce_weight and dice_weight must not both be 0")
    if not isinstance(present_only, bool):
        raise ValueError(f"Dice + CE: present_only must be a bool, got {present_only!r}")
    return float(ce_weight), float(dice_weight), float(smooth), present_only


def head_upsample_ce_dice(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                          want_grad: bool = False, ignore_index: int = -100, ce_weight: float = 1.0, dice_weight: float = 1.0,
                          smooth: float = 1.0, present_only: bool = True, grad_scale: float = 1.0):
    """ce_weight * mean CE + dice_weight * soft Dice of the upsampled scores (S = 4 / 8 / 16): scores_lo fp32 [B*h*w, ld], labels
    int64 [B, h*S, w*S].  Returns (loss_out fp32 [4] = loss, CE mean, Dice, n_valid; class_stats fp32 [3, ld] = I, P, T;
    dscores_lo or None = grad_scale * d loss / d scores_lo, the gradient of the scalar loss).  The per-class sums run over the
    whole batch of the call; nothing syncs, the same bytes every run, captures into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    ce_weight, dice_weight, smooth, present_only = dice_options(ce_weight, dice_weight, smooth, present_only)
    if not math.isfinite(grad_scale):
        raise ValueError(f"lc2is_amd.head_upsample_ce_dice: grad_scale must be finite, got {grad_scale}")
    ld = _head_front("head_upsample_ce_dice", scores_lo, labels, B, h, w, C, S, need_labels=True, scales=(4, 8, 16), cmax=DICE_CMAX)
    nbytes = _fn("lc2is_head_upsample_ce_dice_workspace_bytes")(B, h, w, C, S, mode, int(want_grad))
    loss, dlo, ws = _head_alloc("head_upsample_ce_dice", scores_lo, nbytes, want_grad, (B, h, w, C, S, mode), nloss=4)
    stats = torch.empty((3, ld), dtype=torch.float32, device=scores_lo.device)
    _lib.check(_fn("lc2is_head_upsample_ce_dice")(_ptr(scores_lo), ld, _ptr(labels), _ptr(dlo), _ptr(loss), _ptr(stats), B, h, w,
                                                  C, S, mode, ignore_index, ce_weight, dice_weight, smooth, int(present_only),
                                                  grad_scale, _ptr(ws), nbytes, _stream()),
               f"head_upsample_ce_dice B={B} h={h} w={w} C={C} S={S}")
    return loss, stats, dlo


def ce_dice_nchw_fwd(logits, labels, ignore_index: int = -100, *, ce_weight: float = 1.0, dice_weight: float = 1.0,
                     smooth: float = 1.0, present_only: bool = True):
    """The same loss on NCHW fp32 logits (C <= 192).  Returns (loss_out [4], class_stats [3, C], lse [B,H,W], coef): ``coef`` is
    the device coefficient block ``ce_dice_nchw_bwd`` takes."""
    _chk(logits, torch.float32, "logits", 4); _chk(labels, torch.int64, "labels", 3)
    ce_weight, dice_weight, smooth, present_only = dice_options(ce_weight, dice_weight, smooth, present_only)
    B, Cc, H, W = _nchw_front("ce_dice_nchw_fwd", logits, labels, cmax=DICE_CMAX)
    dev = logits.device
    nbytes = _fn("lc2is_ce_dice_nchw_workspace_bytes")(B, Cc, H * W)
    loss = torch.empty(4, dtype=torch.float32, device=dev)
    stats = torch.empty((3, Cc), dtype=torch.float32, device=dev)
    lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    coef = torch.empty(2 * ((Cc + 3) // 4 * 4) + 4, dtype=torch.float32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(_fn("lc2is_ce_dice_nchw_fwd")(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(loss), _ptr(stats), _ptr(coef), B, Cc,
                                             H * W, ignore_index, ce_weight, dice_weight, smooth, int(present_only), _ptr(ws),
                                             nbytes, _stream()), "ce_dice_nchw_fwd")
    return loss, stats, lse, coef


def ce_dice_nchw_bwd(logits, labels, lse, coef, grad_scale_dev, grad_scale: float = 1.0, ignore_index: int = -100):
    """dlogits = grad_scale * grad_scale_dev (device scalar or None) * d loss / d logits, from ``ce_dice_nchw_fwd``'s lse and coef."""
    _chk_nchw_bwd(logits, labels, lse, grad_scale_dev); _chk(coef, torch.float32, "coef", 1)
    B, Cc, H, W = _nchw_front("ce_dice_nchw_bwd", logits, labels, bwd=True, lse=(lse,))
    if not 1 <= Cc <= DICE_CMAX or coef.numel() != 2 * ((Cc + 3) // 4 * 4) + 4:
        raise RuntimeError(f"lc2is_amd.ce_dice_nchw_bwd: coef must be ce_dice_nchw_fwd's block for C={Cc} (C <= {DICE_CMAX})")
    d = torch.empty_like(logits)
    _lib.check(_fn("lc2is_ce_dice_nchw_bwd")(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(coef), _ptr(grad_scale_dev), grad_scale,
                                             _ptr(d), B, Cc, H * W, ignore_index, _stream()), "ce_dice_nchw_bwd")
    return d


# ---- focal / poly-1 cross-entropy: per-pixel losses of the label's probability alone, one pass ----
def focal_options(gamma, poly_eps) -> tuple[float, float]:
    """(gamma, poly_eps) of a focal / poly-1 loss, validated: gamma a finite number >= 0, poly_eps a finite number >= -1."""
    for name, v, lo in (("gamma", gamma, 0.0), ("poly_eps", poly_eps, -1.0)):
        if not finite_ge(v, lo):
            raise ValueError(f"focal loss: {name} must be a finite number >= {lo:g}, got {v!r}")
    return float(gamma), float(poly_eps)


def _focal_weight(class_weight, C: int, dev):
    if class_weight is not None:
        _ce_options(class_weight, 0.0, C, dev)


def head_upsample_focal(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                        want_grad: bool = False, ignore_index: int = -100, grad_scale: float = 1.0, class_weight=None,
                        gamma: float = 2.0, poly_eps: float = 0.0):
    """Focal / poly-1 cross-entropy of the upsampled scores (S = 4 / 8 / 16): scores_lo fp32 [B*h*w, ld], labels int64
    [B, h*S, w*S].  Per counted pixel, with p the label's softmax probability and q = 1 - p:
    l = w_y (q^gamma (-ln p) + poly_eps q).  Returns (loss2 = [sum of l, sum of w_y over the counted pixels], dscores_lo or None =
    grad_scale * d(sum of l) / d scores_lo).  One forward + backward launch and the finish launch of ``head_upsample_ce``; nothing
    syncs, no atomics, the same bytes every run, captures into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    gamma, poly_eps = focal_options(gamma, poly_eps)
    ld = _head_front("head_upsample_focal", scores_lo, labels, B, h, w, C, S, need_labels=True, scales=(4, 8, 16), cmax=HEAD_CMAX)
    _focal_weight(class_weight, C, scores_lo.device)
    nbytes = _fn("lc2is_head_upsample_ce_workspace_bytes")(B, h, w, C, S, mode, int(want_grad))
    loss, dlo, ws = _head_alloc("head_upsample_focal", scores_lo, nbytes, want_grad, (B, h, w, C, S, mode))
    _lib.check(_fn("lc2is_head_upsample_focal")(_ptr(scores_lo), ld, _ptr(labels), _ptr(dlo), _ptr(loss), B, h, w, C, S, mode,
                                                ignore_index, grad_scale, _ptr(class_weight), gamma, poly_eps, _ptr(ws), nbytes,
                                                _stream()), f"head_upsample_focal B={B} h={h} w={w} C={C} S={S}")
    return loss, dlo


def focal_nchw_fwd(logits, labels, ignore_index: int = -100, *, class_weight=None, gamma: float = 2.0, poly_eps: float = 0.0,
                   per_pixel: bool = False):
    """The same loss on NCHW fp32 logits.  Returns (loss2 = [sum of l, sum of w_y], lse [B,H,W]) and, with per_pixel=True, a third
    tensor: the per-pixel losses [B,H,W] (0 where not counted)."""
    _chk(logits, torch.float32, "logits", 4); _chk(labels, torch.int64, "labels", 3)
    gamma, poly_eps = focal_options(gamma, poly_eps)
    B, Cc, H, W = _nchw_front("focal_nchw_fwd", logits, labels)
    _focal_weight(class_weight, Cc, logits.device)
    loss, ws, nbytes, lse, lpx = _nchw_fwd_alloc(logits, B, H, W, per_pixel)
    _lib.check(_fn("lc2is_focal_nchw_fwd")(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(loss), _ptr(lpx), B, Cc, H * W, ignore_index,
                                           _ptr(class_weight), gamma, poly_eps, _ptr(ws), nbytes, _stream()), "focal_nchw_fwd")
    return (loss, lse, lpx) if per_pixel else (loss, lse)


def focal_nchw_bwd(logits, labels, lse, grad_scale_dev, grad_scale: float = 1.0, ignore_index: int = -100, *, class_weight=None,
                   gamma: float = 2.0, poly_eps: float = 0.0, grad_px=None):
    """dlogits = grad_scale * grad_scale_dev (device scalar or None) * grad_px (per pixel, [B,H,W] fp32, optional) * dl_i/dlogits,
    from ``focal_nchw_fwd``'s lse."""
    _chk_nchw_bwd(logits, labels, lse, grad_scale_dev)
    gamma, poly_eps = focal_options(gamma, poly_eps)
    B, Cc, H, W = _nchw_front("focal_nchw_bwd", logits, labels, bwd=True, lse=(lse,))
    _focal_weight(class_weight, Cc, logits.device)
    _chk_grad_px("focal_nchw_bwd", grad_px, B, H, W)
    d = torch.empty_like(logits)
    _lib.check(_fn("lc2is_focal_nchw_bwd")(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(grad_scale_dev), grad_scale, _ptr(grad_px),
                                           _ptr(d), B, Cc, H * W, ignore_index, _ptr(class_weight), gamma, poly_eps, _stream()),
               "focal_nchw_bwd")
    return d


# ---- sigmoid cross-entropy / sigmoid focal loss: per-class binary terms, no softmax, one pass ----
def sigmoid_options(gamma, alpha, normalize: str = "elements"):
    """(gamma, alpha, normalize) of a sigmoid focal / sigmoid cross-entropy loss, validated: gamma a finite number >= 0 (returned as
    a float), alpha None or a number in [0, 1] (returned as None or a float), normalize 'elements' or 'pixels'."""
    if not finite_ge(gamma):
        raise ValueError(f"sigmoid focal loss: gamma must be a finite number >= 0, got {gamma!r}")
    if alpha is not None and not (finite_ge(alpha) and alpha <= 1.0):
        raise ValueError(f"sigmoid focal loss: alpha must be None or a number in [0, 1], got {alpha!r}")
    if normalize not in ("elements", "pixels"):
        raise ValueError(f"sigmoid focal loss: normalize must be 'elements' or 'pixels', got {normalize!r}")
    return float(gamma), None if alpha is None else float(alpha), normalize


def sigmoid_class_scale(normalize: str, reduction: str, C: int) -> float:
    """The factor on a pixel's sum over its C classes: 1 / C for a 'mean' over elements (torch's mean of a binary loss), else 1."""
    return 1.0 / C if (normalize == "elements" and reduction == "mean") else 1.0


def _sigmoid_args(gamma, alpha, class_scale):
    gamma, alpha, _ = sigmoid_options(gamma, alpha)
    if not finite_ge(class_scale) or class_scale == 0:
        raise ValueError(f"sigmoid focal loss: class_scale must be a finite number > 0, got {class_scale!r}")
    return gamma, -1.0 if alpha is None else alpha, float(class_scale)   # (the C entry points read any negative alpha as "none")


def head_upsample_sigmoid(scores_lo, labels, B: int, h: int, w: int, C: int, S: int, mode: int = INTERP_BICUBIC, *,
                          want_grad: bool = False, ignore_index: int = -100, grad_scale: float = 1.0, class_weight=None,
                          gamma: float = 2.0, alpha=0.25, class_scale: float = 1.0):
    """Sigmoid focal loss / sigmoid cross-entropy of the upsampled scores (S = 4 / 8 / 16): scores_lo fp32 [B*h*w, ld], labels int64
    [B, h*S, w*S].  Per counted pixel and class c, with t = [c == label], p = sigmoid(z), p_t = t ? p : 1 - p:
    l_c = w_c a_t (1 - p_t)^gamma (-ln p_t), a_t = alpha / 1 - alpha (1 when alpha is None); the pixel's loss is class_scale * sum_c
    l_c.  Returns (loss2 = [sum of the pixel losses, NUMBER of counted pixels], dscores_lo or None = grad_scale * d(sum) / d
    scores_lo).  One forward + backward launch and the finish launch of ``head_upsample_ce``; nothing syncs, no atomics, the same
    bytes every run, captures into a graph."""
    _chk(scores_lo, torch.float32, "scores_lo"); _chk(labels, torch.int64, "labels", 3)
    gamma, alpha, class_scale = _sigmoid_args(gamma, alpha, class_scale)
    ld = _head_front("head_upsample_sigmoid", scores_lo, labels, B, h, w, C, S, need_labels=True, scales=(4, 8, 16), cmax=HEAD_CMAX)
    _focal_weight(class_weight, C, scores_lo.device)
    nbytes = _fn("lc2is_head_upsample_ce_workspace_bytes")(B, h, w, C, S, mode, int(want_grad))
    loss, dlo, ws = _head_alloc("head_upsample_sigmoid", scores_lo, nbytes, want_grad, (B, h, w, C, S, mode))
    _lib.check(_fn("lc2is_head_upsample_sigmoid")(_ptr(scores_lo), ld, _ptr(labels), _ptr(dlo), _ptr(loss), B, h, w, C, S, mode,
                                                  ignore_index, grad_scale, _ptr(class_weight), gamma, alpha, class_scale, _ptr(ws),
                                                  nbytes, _stream()), f"head_upsample_sigmoid B={B} h={h} w={w} C={C} S={S}")
    return loss, dlo


def sigmoid_focal_nchw_fwd(logits, labels, ignore_index: int = -100, *, class_weight=None, gamma: float = 2.0, alpha=0.25,
                           class_scale: float = 1.0, per_pixel: bool = False):
    """The same loss on NCHW fp32 logits.  Returns loss2 = [sum of the pixel losses, number of counted pixels] and, with
    per_pixel=True, (loss2, the per-pixel losses [B,H,W], 0 where not counted).  Nothing is saved for the backward."""
    _chk(logits, torch.float32, "logits", 4); _chk(labels, torch.int64, "labels", 3)
    gamma, alpha, class_scale = _sigmoid_args(gamma, alpha, class_scale)
    B, Cc, H, W = _nchw_front("sigmoid_focal_nchw_fwd", logits, labels)
    _focal_weight(class_weight, Cc, logits.device)
    loss, ws, nbytes, _, lpx = _nchw_fwd_alloc(logits, B, H, W, per_pixel, lse=False)
    _lib.check(_fn("lc2is_sigmoid_focal_nchw_fwd")(_ptr(logits), _ptr(labels), _ptr(loss), _ptr(lpx), B, Cc, H * W, ignore_index,
                                                   _ptr(class_weight), gamma, alpha, class_scale, _ptr(ws), nbytes, _stream()),
               "sigmoid_focal_nchw_fwd")
    return (loss, lpx) if per_pixel else loss


def sigmoid_focal_nchw_bwd(logits, labels, grad_scale_dev, grad_scale: float = 1.0, ignore_index: int = -100, *, class_weight=None,
                           gamma: float = 2.0, alpha=0.25, class_scale: float = 1.0, grad_px=None):
    """dlogits = grad_scale * grad_scale_dev (device scalar or None) * grad_px (per pixel, [B,H,W] fp32, optional) * dl_i/dlogits."""
    _chk_nchw_bwd(logits, labels, None, grad_scale_dev)
    gamma, alpha, class_scale = _sigmoid_args(gamma, alpha, class_scale)
    B, Cc, H, W = _nchw_front("sigmoid_focal_nchw_bwd", logits, labels, bwd=True)
    _focal_weight(class_weight, Cc, logits.device)
    _chk_grad_px("sigmoid_focal_nchw_bwd", grad_px, B, H, W)
    d = torch.empty_like(logits)
    _lib.check(_fn("lc2is_sigmoid_focal_nchw_bwd")(_ptr(logits), _ptr(labels), _ptr(grad_scale_dev), grad_scale, _ptr(grad_px),
                                                   _ptr(d), B, Cc, H * W, ignore_index, _ptr(class_weight), gamma, alpha, class_scale,
                                                   _stream()), "sigmoid_focal_nchw_bwd")
    return d


def ce_nchw_fwd(logits, labels, ignore_index: int = -100, *, class_weight=None, label_smoothing: float = 0.0,
                per_pixel: bool = False):
    """Returns (loss_sum[2], lse [B,H,W]) — loss_sum = (sum of per-pixel losses, sum of w_y over the counted pixels) — and,
    with per_pixel=True, a third tensor: the per-pixel losses [B,H,W] (reduction="none"; 0 where not counted)."""
    _chk(logits, torch.float32, "logits", 4); _chk(labels, torch.int64, "labels", 3)
    B, Cc, H, W = _nchw_front("ce_nchw_fwd", logits, labels)
    _ce_options(class_weight, label_smoothing, Cc, logits.device)   # (validation; the C side picks the kernel variant)
    loss, ws, nbytes, lse, lpx = _nchw_fwd_alloc(logits, B, H, W, per_pixel)
    _lib.check(_fn("lc2is_ce_nchw_fwd_ordered")(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(loss), _ptr(lpx), B, Cc, H * W,
                                                ignore_index, _ptr(class_weight), label_smoothing, _ptr(ws), nbytes,
                                                _stream()), "ce_nchw_fwd")
    return (loss, lse, lpx) if per_pixel else (loss, lse)


def ce_nchw_bwd(logits, labels, lse, grad_scale_dev, grad_scale: float, ignore_index: int = -100, *, class_weight=None,
                label_smoothing: float = 0.0, grad_px=None):
    """dlogits = grad_scale * grad_scale_dev * grad_px (per pixel, [B,H,W] fp32, optional) * dloss_i/dlogits, from
    ``ce_nchw_fwd``'s lse.  With every option unset the C side launches the plain kernel."""
    _chk_nchw_bwd(logits, labels, lse, grad_scale_dev)
    B, Cc, H, W = _nchw_front("ce_nchw_bwd", logits, labels, bwd=True, lse=(lse,))
    _ce_options(class_weight, label_smoothing, Cc, logits.device)
    _chk_grad_px("ce_nchw_bwd", grad_px, B, H, W)
    d = torch.empty_like(logits)
    _lib.check(_fn("lc2is_ce_nchw_bwd_opts")(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(grad_scale_dev), grad_scale,
                                             _ptr(grad_px), _ptr(d), B, Cc, H * W, ignore_index, _ptr(class_weight),
                                             label_smoothing, _stream()), "ce_nchw_bwd")
    return d


def upsample_bwd_nchw(dhi, B: int, h: int, w: int, C: int, S: int, mode: int, ld: int):
    """dhi fp32 NCHW [B,C,h*S,w*S] -> dlo fp32 [B*h*w, ld] (zero padded columns)."""
    _chk(dhi, torch.float32, "dhi", 4)
    if not dhi.is_contiguous() or tuple(dhi.shape) != (B, C, h * S, w * S):
        raise RuntimeError("lc2is_amd.upsample_bwd_nchw: dhi must be contiguous [B,C,h*S,w*S]")
    dlo = torch.zeros((B * h * w, ld), dtype=torch.float32, device=dhi.device)
    _lib.check(_fn("lc2is_upsample_bwd_nchw")(_ptr(dhi), _ptr(dlo), ld, B, h, w, C, S, mode, _stream()),
               "upsample_bwd_nchw")
    return dlo


def _dense(t, dtype, name):
    _chk(t, dtype, name)
    if t is not None and not t.is_contiguous():
        raise RuntimeError(f"lc2is_amd: {name} must be contiguous")


def bilinear_up_fwd(x, B: int, h: int, w: int, S: int, *, want_f32: bool = True, want_bf16: bool = False):
    """x fp32 [B*h*w, C] channels-last tokens -> ([B*h*S*w*S, C] fp32 or None, bf16 twin or None)."""
    _dense(x, torch.float32, "x")
    Cc = x.shape[1]
    _chk_rows("bilinear_up_fwd", x, "x", B * h * w, "B*h*w")
    n = B * h * S * w * S
    of = torch.empty((n, Cc), dtype=torch.float32, device=x.device) if want_f32 else None
    ob = torch.empty((n, Cc), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    _lib.check(_fn("lc2is_bilinear_up_fwd")(_ptr(x), _ptr(of), _ptr(ob), B, h, w, Cc, S, _stream()), "bilinear_up_fwd")
    return of, ob


def bilinear_up_bwd(dout, B: int, h: int, w: int, S: int, *, din=None, accumulate: bool = False, want_bf16: bool = False):
    _dense(dout, torch.float32, "dout")
    Cc = dout.shape[1]
    _chk_rows("bilinear_up_bwd", dout, "dout", B * h * S * w * S, "B*h*S*w*S")
    if din is None:
        din = torch.empty((B * h * w, Cc), dtype=torch.float32, device=dout.device)
        accumulate = False
    _dense(din, torch.float32, "din")
    if tuple(din.shape) != (B * h * w, Cc) or din.device != dout.device:
        raise RuntimeError(f"lc2is_amd.bilinear_up_bwd: din must be [B*h*w, C] = [{B * h * w}, {Cc}] on {dout.device}, got shape "
                           f"{tuple(din.shape)} on {din.device}")
    d16 = torch.empty((B * h * w, Cc), dtype=torch.bfloat16, device=dout.device) if want_bf16 else None
    _lib.check(_fn("lc2is_bilinear_up_bwd")(_ptr(dout), _ptr(din), _ptr(d16), B, h, w, Cc, S, int(accumulate), _stream()),
               "bilinear_up_bwd")
    return din, d16


def sr_gather(x16, B: int, h: int, w: int, scatter: bool = False):
    """gather: bf16 [B*h*w, C] -> [B*h*w/4, 4C];  scatter: bf16 [B*h*w/4, 4C] -> [B*h*w, C]."""
    _dense(x16, torch.bfloat16, "x")
    if h % 2 or w % 2:
        raise RuntimeError(f"lc2is_amd.sr_gather: h and w must be even, got {h} x {w}")
    if scatter:
        _chk_rows("sr_gather", x16, "x", B * h * w // 4, "B*h*w/4")
        if x16.shape[1] % 4:
            raise RuntimeError(f"lc2is_amd.sr_gather: scatter rows hold 4 pixels of C, got shape {tuple(x16.shape)}")
        Cc = x16.shape[1] // 4
        out = torch.empty((B * h * w, Cc), dtype=torch.bfloat16, device=x16.device)
    else:
        _chk_rows("sr_gather", x16, "x", B * h * w, "B*h*w")
        Cc = x16.shape[1]
        out = torch.empty((B * h * w // 4, 4 * Cc), dtype=torch.bfloat16, device=x16.device)
    _lib.check(_fn("lc2is_sr_gather")(_ptr(x16), _ptr(out), B, h, w, Cc, int(scatter), _stream()), "sr_gather")
    return out


def l2norm_fwd(x, eps: float = 1e-12, *, want_f32: bool = True, want_bf16: bool = True):
    _dense(x, torch.float32, "x")
    M, Cc = x.shape
    yf = torch.empty_like(x) if want_f32 else None
    yb = torch.empty((M, Cc), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    inv = torch.empty((M,), dtype=torch.float32, device=x.device)
    _lib.check(_fn("lc2is_l2norm_fwd")(_ptr(x), _ptr(yf), _ptr(yb), _ptr(inv), M, Cc, eps, _stream()), "l2norm_fwd")
    return yf, yb, inv


def l2norm_bwd(dy, x, inv, eps: float = 1e-12):
    _dense(dy, torch.float32, "dy"); _dense(x, torch.float32, "x")
    M, Cc = x.shape
    if dy.shape != x.shape or dy.device != x.device:
        raise RuntimeError(f"lc2is_amd.l2norm_bwd: dy must match x {tuple(x.shape)} on {x.device}, got {tuple(dy.shape)} on {dy.device}")
    _chk(inv, torch.float32, "inv", None)
    if inv.numel() != M or not inv.is_contiguous() or inv.device != x.device:
        raise RuntimeError(f"lc2is_amd.l2norm_bwd: inv must hold M = {M} contiguous values on {x.device}, got shape "
                           f"{tuple(inv.shape)} on {inv.device}")
    dx = torch.empty_like(x)
    _lib.check(_fn("lc2is_l2norm_bwd")(_ptr(dy), _ptr(x), _ptr(inv), _ptr(dx), M, Cc, eps, _stream()), "l2norm_bwd")
    return dx


def add_n(tensors, *, want_f32: bool = True, want_bf16: bool = False):
    """Elementwise sum of 2..4 fp32 tensors of equal shape."""
    if not 2 <= len(tensors) <= 4:
        raise RuntimeError("lc2is_amd.add_n takes 2 to 4 tensors")
    for t in tensors:
        _chk(t, torch.float32, "addend", None)
        if not t.is_contiguous() or t.shape != tensors[0].shape:
            raise RuntimeError("lc2is_amd.add_n: addends must be contiguous and equally shaped")
    ps = [_ptr(t) for t in tensors] + [None] * (4 - len(tensors))
    of = torch.empty_like(tensors[0]) if want_f32 else None
    ob = torch.empty(tensors[0].shape, dtype=torch.bfloat16, device=tensors[0].device) if want_bf16 else None
    _lib.check(_fn("lc2is_add_n")(*ps, _ptr(of), _ptr(ob), tensors[0].numel(), _stream()), "add_n")
    return of, ob


def sr_scatter_add(src16, dst32, B: int, h: int, w: int):
    """dst32 [B*h*w, C] fp32 += scatter(src16 [B*h*w/4, 4C] bf16)."""
    _dense(src16, torch.bfloat16, "src"); _dense(dst32, torch.float32, "dst")
    Cc = dst32.shape[1]
    if h % 2 or w % 2:
        raise RuntimeError(f"lc2is_amd.sr_scatter_add: h and w must be even, got {h} x {w}")
    _chk_rows("sr_scatter_add", dst32, "dst", B * h * w, "B*h*w")
    if tuple(src16.shape) != (B * h * w // 4, 4 * Cc) or src16.device != dst32.device:
        raise RuntimeError(f"lc2is_amd.sr_scatter_add: src must be [B*h*w/4, 4C] = [{B * h * w // 4}, {4 * Cc}] on {dst32.device}, "
                           f"got shape {tuple(src16.shape)} on {src16.device}")
    _lib.check(_fn("lc2is_sr_scatter_add_f32")(_ptr(src16), _ptr(dst32), B, h, w, Cc, _stream()), "sr_scatter_add")


def _labels(labels, n: int, name: str):
    _chk(labels, torch.int64, "labels", None)
    if not labels.is_contiguous() or labels.numel() != n:
        raise RuntimeError(f"lc2is_amd.{name}: labels must be contiguous int64 with {n} elements, got {tuple(labels.shape)}")


def rows_ce(x, labels, *, loss_sum=None, dx=None, grad_scale: float = 1.0, accumulate_dx: bool = False, want_lse=False):
    """Softmax-CE over the K classes of each row of x [M,K]; a label outside [0, K) adds nothing to loss_sum or dx."""
    _dense(x, torch.float32, "x")
    M, K = x.shape
    _labels(labels, M, "rows_ce")
    _dense(dx, torch.float32, "dx")
    if dx is not None and dx.shape != x.shape:
        raise RuntimeError("lc2is_amd.rows_ce: dx must match x")
    lse = torch.empty((M,), dtype=torch.float32, device=x.device) if want_lse else None
    _lib.check(_fn("lc2is_rows_ce")(_ptr(x), _ptr(labels), _ptr(lse), _ptr(loss_sum), _ptr(dx), grad_scale, M, K,
                                    int(accumulate_dx), _stream()), "rows_ce")
    return lse


def cols_ce(x, labels, B: int, H: int, W: int, K: int, loss_sum, dx=None, grad_scale: float = 1.0):
    _dense(x, torch.float32, "x")
    if x.numel() != B * H * W * K or x.shape[1] != K:
        raise RuntimeError(f"lc2is_amd.cols_ce: x {tuple(x.shape)} is not [B*H*W, K] for B={B} H={H} W={W} K={K}")
    _labels(labels, B * H * W, "cols_ce")
    _dense(dx, torch.float32, "dx")
    if dx is not None and dx.shape != x.shape:
        raise RuntimeError("lc2is_amd.cols_ce: dx must match x")
    _lib.check(_fn("lc2is_cols_ce")(_ptr(x), _ptr(labels), _ptr(loss_sum), _ptr(dx), grad_scale, B, H, W, K, _stream()),
               "cols_ce")


def npair(x, x_pos, x_neg):
    for t, n in ((x, "x"), (x_pos, "x_pos"), (x_neg, "x_neg")):
        _dense(t, torch.float32, n)
    res = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    _lib.check(_fn("lc2is_npair")(_ptr(x), _ptr(x_pos), _ptr(x_neg), _ptr(res), x.shape[0], x_pos.shape[0],
                                  x_neg.shape[0], x.shape[1], _stream()), "npair")
    return res



def npair_bwd(x, x_pos, x_neg, dres):
    """Gradients of npair's res [n] wrt (x, x_pos, x_neg), all fp32."""
    for t, n in ((x, "x"), (x_pos, "x_pos"), (x_neg, "x_neg")):
        _dense(t, torch.float32, n)
    _chk(dres, torch.float32, "dres", 1)
    n, d = x.shape
    dx, dxp, dxn = torch.empty_like(x), torch.empty_like(x_pos), torch.empty_like(x_neg)
    ws = torch.empty(n * (x_pos.shape[0] + 1), dtype=torch.float32, device=x.device)
    _lib.check(_fn("lc2is_npair_bwd")(_ptr(x), _ptr(x_pos), _ptr(x_neg), _ptr(dres.contiguous()), _ptr(dx), _ptr(dxp), _ptr(dxn),
                                      _ptr(ws), n, x_pos.shape[0], x_neg.shape[0], d, _stream()), "npair_bwd")
    return dx, dxp, dxn

def miou_counts(scores_hi, labels_lo, S: int):
    _chk(scores_hi, torch.float32, "scores_hi", 4); _chk(labels_lo, torch.int64, "labels", 3)
    B, K, H, W = scores_hi.shape
    if S <= 0 or H % S or W % S or tuple(labels_lo.shape) != (B, H // S, W // S):
        raise RuntimeError(f"lc2is_amd.miou_counts: labels {tuple(labels_lo.shape)} do not match scores {tuple(scores_hi.shape)} / {S}")
    counts = torch.zeros((B, 3, K), dtype=torch.int32, device=scores_hi.device)
    _lib.check(_fn("lc2is_miou_counts")(_ptr(scores_hi.contiguous()), _ptr(labels_lo.contiguous()), _ptr(counts), B, K, H,
                                        W, S, _stream()), "miou_counts")
    return counts


RESIZE_TILE, RESIZE_KMAX = 16, 192      # LC2IS_RESIZE_TILE; the largest class count of lc2is_resize_argmax
RESIZE_WIDE_KMAX = 1024                 # LC2IS_RESIZE_WIDE_KMAX: the largest class count of the lc2is_resize_argmax*_wide entries
_GT_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}


def resize_sizes(N: int, sizes, gt=None) -> list[tuple[int, int]]:
    """N (H, W) pairs as ints from a sequence or an [N, 2] tensor (None: the shapes of the N gt maps).  ValueError when they
    disagree with N or with the gt maps' shapes."""
    if gt is not None and len(gt) != N:
        raise ValueError(f"lc2is_amd: {len(gt)} gt maps for {N} images")
    if sizes is None:
        if gt is None:
            raise ValueError("lc2is_amd: sizes are needed when no gt maps are given")
        sizes = [tuple(g.shape) for g in gt]
    hw = [tuple(int(v) for v in s) for s in (sizes.tolist() if torch.is_tensor(sizes) else sizes)]
    if len(hw) != N or any(len(s) != 2 or s[0] < 1 or s[1] < 1 for s in hw):
        raise ValueError(f"lc2is_amd: sizes must be {N} (H, W) pairs of positive ints, got {hw}")
    if gt is not None:
        bad = [i for i, (g, s) in enumerate(zip(gt, hw)) if tuple(g.shape) != s]
        if bad:
            raise ValueError(f"lc2is_amd: gt maps {bad} do not have the shapes given by sizes "
                             f"({[tuple(gt[i].shape) for i in bad]} vs {[hw[i] for i in bad]})")
    return hw


def _resize_layout(hw):
    """Per image the pixel count, first pixel and first tile of the packed pred / gt buffers, and the totals."""
    T = RESIZE_TILE
    tiles = [-(-H // T) * -(-W // T) for H, W in hw]
    px = [H * W for H, W in hw]
    first_px = [sum(px[:i]) for i in range(len(hw))]
    first_tile = [sum(tiles[:i]) for i in range(len(hw))]
    return px, first_px, first_tile, sum(tiles), sum(px)


def _resize_gt(gt, dts, N, K, n_tiles, dev, wide=False):
    """(packed gt, counts, workspace, its bytes) of a call with gt maps (wide: the workspace query of the wide entries)."""
    dt = dts.pop() if len(dts) == 1 else torch.int64
    flat = [x.reshape(-1) for x in gt]
    if all(not x.is_cuda for x in flat):
        g = torch.cat([x.to(dt) for x in flat]).to(dev)          # one host -> device copy
    else:
        g = torch.cat([x.to(dev, dt) for x in flat])
    counts = torch.empty((N, 3, K), dtype=torch.int32, device=dev)
    nbytes = _fn("lc2is_resize_argmax_wide_workspace_bytes" if wide else "lc2is_resize_argmax_workspace_bytes")(n_tiles, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)     # per-tile counts (per call: live until the second launch)
    return g, counts, ws, nbytes


def _resize_front(who, x, what, kmax=RESIZE_KMAX):
    """The first checks of the resize + argmax wrappers: x is NCHW with 1 <= K <= kmax (192; the wide wrappers pass 1024).
    Returns its shape."""
    if x.dim() != 4:
        raise RuntimeError(f"{who}: {what}, got shape {tuple(x.shape)}")
    K = x.shape[1]
    if not 1 <= K <= kmax:
        raise RuntimeError(f"{who}: K = {K} classes is not supported (1 <= K <= {kmax})")
    return tuple(x.shape)


def _resize_ignore_index(who, ignore_index):
    if ignore_index is not None and (int(ignore_index) != ignore_index or ignore_index < 0):
        raise ValueError(f"{who}: ignore_index must be None or an int >= 0, got {ignore_index!r}")


def _resize_windows(who, where, wl, canvas, V, h, w, rows, overhang):
    """Validates one window list against its (Hc, Wc) canvas and appends its (view, oy, ox, mirrored) rows to ``rows``.
    overhang=False: every window lies on the canvas; True: its origin does, and only its on-canvas part covers cells."""
    Hc, Wc = canvas
    if not 1 <= len(wl) <= SLIDE_MAX_WIN:
        raise ValueError(f"{who}: {where} has {len(wl)} windows (1 to {SLIDE_MAX_WIN})")
    cover = torch.zeros(Hc, Wc, dtype=torch.bool)
    for view, oy, ox, mirrored in wl:
        view, oy, ox = int(view), int(oy), int(ox)
        if not 0 <= view < V:
            raise ValueError(f"{who}: {where}: view index {view} is not in [0, {V})")
        if overhang and not (0 <= oy < Hc and 0 <= ox < Wc):
            raise ValueError(f"{who}: {where}: window origin ({oy}, {ox}) is outside the {Hc} x {Wc} canvas")
        if not overhang and not (0 <= oy <= Hc - h and 0 <= ox <= Wc - w):
            raise ValueError(f"{who}: {where}: window origin ({oy}, {ox}) is outside [0, {Hc - h}] x [0, {Wc - w}]")
        cover[oy:oy + h, ox:ox + w] = True
        rows.append((view, oy, ox, 1 if mirrored else 0))
    if not bool(cover.all()):
        raise ValueError(f"{who}: {where}: {int((~cover).sum())} canvas cells are covered by no window")


def _resize_back(who, x, what, gt, want_pred):
    """The last host checks, in their order: gt dtypes, something to compute, and (last of all) x on the GPU.  Returns the gt
    dtypes (None without gt)."""
    dts = None
    if gt is not None:
        dts = {g.dtype for g in gt}
        if not dts <= set(_GT_BYTES):
            raise RuntimeError(f"{who}: gt maps must be uint8, int32 or int64, got {sorted(map(str, dts))}")
    if not want_pred and gt is None:
        raise ValueError(f"{who}: nothing to compute (want_pred=False and no gt)")
    if not x.is_cuda:
        raise RuntimeError(f"{who}: {what} must be a CUDA(HIP) tensor; there is no CPU path")
    return dts


def _resize_channels_last(x):
    """(fp32 [N, h, w, ld] copy of NCHW x with the channels padded by zeros to ld, a multiple of 4; ld)."""
    N, K, h, w = x.shape
    ld = (K + 3) // 4 * 4
    lo = torch.empty((N, h, w, ld), dtype=torch.float32, device=x.device)
    lo[..., :K] = x.permute(0, 2, 3, 1)
    if ld > K:
        lo[..., K:] = 0
    return lo, ld


def _resize_run(hw, K, gt, dts, want_pred, dev, launch, wide=False):
    """The common tail: the packed layout, pred (uint8; wide: int16) / gt / counts / workspace, the launch and the split of the
    packed pred.
    launch(layout, pred, g, gt_bytes, counts, ws, nbytes) makes the descriptors from layout = (first_px, first_tile, n_tiles,
    total_px), calls the library and checks its return code."""
    N = len(hw)
    px, first_px, first_tile, n_tiles, total_px = _resize_layout(hw)
    pred = torch.empty(total_px, dtype=torch.int16 if wide else torch.uint8, device=dev) if want_pred else None
    counts = g = ws = None
    nbytes = 0
    if gt is not None:
        g, counts, ws, nbytes = _resize_gt(gt, dts, N, K, n_tiles, dev, wide)
    launch((first_px, first_tile, n_tiles, total_px), pred, g, _GT_BYTES[g.dtype] if g is not None else 0, counts, ws, nbytes)
    preds = None if pred is None else [x.view(H, W) for x, (H, W) in zip(torch.split(pred, px), hw)]
    return preds, counts


def resize_argmax(scores, sizes, gt=None, want_pred: bool = True):
    """Per image, F.interpolate(scores[i:i+1], size=sizes[i], mode="bicubic", align_corners=False) and the argmax over the classes
    (exact ties: the lowest index), fused: the [K, H, W] score map is never formed (lc2is_resize_argmax).
    scores: the model's NCHW [N, K, h, w] logits on the GPU (any float dtype; the channels-last fp32 copy is made here), K <= 192
    (193 to 1024 classes: ``resize_argmax_wide``).
    sizes: N (H, W) pairs (sequence or [N, 2] tensor) or None (the gt maps' shapes).  gt: None or N label maps [H_i, W_i]
    (uint8 / int32 / int64, host or device).
    Returns (pred, counts): pred a list of uint8 [H_i, W_i] (views of one packed buffer) or None (want_pred=False);
    counts int32 [N, 3, K] = {intersection, predicted, labelled} (labelled: 0 <= gt < K) when gt is given, else None."""
    return _resize_argmax(scores, sizes, gt, want_pred, wide=False)


def _resize_argmax(scores, sizes, gt, want_pred, wide):
    """``resize_argmax`` (wide=False) and ``resize_argmax_wide``: one body, the entry point, class limit and pred dtype differ."""
    name = "resize_argmax_wide" if wide else "resize_argmax"
    who = f"lc2is_amd.{name}"
    N, K, h, w = _resize_front(who, scores, "scores must be NCHW [N, K, h, w]", RESIZE_WIDE_KMAX if wide else RESIZE_KMAX)
    hw = resize_sizes(N, sizes, gt)
    dts = _resize_back(who, scores, "scores", gt, want_pred)
    dev = scores.device
    lo, ld = _resize_channels_last(scores)

    def launch(layout, pred, g, gt_bytes, counts, ws, nbytes):
        first_px, first_tile, n_tiles, total_px = layout
        desc = torch.tensor([[H, W, p0, t0] for (H, W), p0, t0 in zip(hw, first_px, first_tile)], dtype=torch.int64).to(dev)
        rc = _fn(f"lc2is_{name}")(_ptr(lo), ld, N, h, w, K, _ptr(desc), n_tiles, total_px, _ptr(g), gt_bytes, _ptr(pred),
                                  _ptr(counts), _ptr(ws), nbytes, _stream())
        _lib.check(rc, f"{name} N={N} K={K} h={h} w={w}")
    return _resize_run(hw, K, gt, dts, want_pred, dev, launch, wide)


def resize_argmax_wide(scores, sizes, gt=None, want_pred: bool = True):
    """``resize_argmax`` for 1 <= K <= 1024 classes (lc2is_resize_argmax_wide): the same arguments and checks; pred is a list of
    int16 [H_i, W_i] views, counts int32 [N, 3, K].  With K <= 192 it returns ``resize_argmax``'s class indices and counts, which
    is then the faster call (its count epilogue holds the three rows of a tile at once).  The per-tile count workspace is
    n_tiles * 3 * K * 4 bytes: 14 MB for one 683 x 512 image at K = 847."""
    return _resize_argmax(scores, sizes, gt, want_pred, wide=True)


SLIDE_MAX_WIN = 64                      # LC2IS_SLIDE_MAX_WIN: windows per image of lc2is_resize_argmax_windows


def resize_argmax_windows(views, windows, canvases, sizes, gt=None, want_pred: bool = True, ignore_index: int | None = None):
    """``resize_argmax`` for sliding-window evaluation (lc2is_resize_argmax_windows): image i is resized from a canvas of
    canvases[i] = (Hc, Wc) score cells that is never formed, each cell the mean of the window views covering it.
    views: the model's NCHW [V, K, h, w] logits on the GPU, one score grid per window forward (the channels-last fp32 copy is made
    here).  windows: per image a list of (view, oy, ox, mirrored): the view's index, its origin on the canvas in cells, and whether
    it is stored mirrored along x (a forward of the flipped window).  At most 64 windows per image, every canvas cell covered.
    sizes, gt, want_pred and the returned (pred, counts): as ``resize_argmax``.  ignore_index: None = its counting rule; an int
    >= 0 = mmseg's: a pixel whose gt is ignore_index or outside [0, K) counts in none of the three rows.
    Everything is validated on the host before anything is allocated."""
    return _resize_argmax_windows(views, windows, canvases, sizes, gt, want_pred, ignore_index, wide=False)


def _resize_argmax_windows(views, windows, canvases, sizes, gt, want_pred, ignore_index, wide):
    """``resize_argmax_windows`` (wide=False) and ``resize_argmax_windows_wide``: one body."""
    name = "resize_argmax_windows_wide" if wide else "resize_argmax_windows"
    who = f"lc2is_amd.{name}"
    V, K, h, w = _resize_front(who, views, "views must be NCHW [V, K, h, w]", RESIZE_WIDE_KMAX if wide else RESIZE_KMAX)
    N = len(windows)
    if N < 1 or len(canvases) != N:
        raise ValueError(f"{who}: {N} window lists for {len(canvases)} canvases")
    hw = resize_sizes(N, sizes, gt)
    _resize_ignore_index(who, ignore_index)
    canv, rows, first_win = [], [], []
    for i, (wl, cv) in enumerate(zip(windows, canvases)):
        Hc, Wc = (int(v) for v in cv)
        if Hc < h or Wc < w:
            raise ValueError(f"{who}: canvas {i} ({Hc} x {Wc}) is smaller than a view ({h} x {w})")
        first_win.append(len(rows))
        _resize_windows(who, f"image {i}", wl, (Hc, Wc), V, h, w, rows, overhang=False)
        canv.append((Hc, Wc))
    dts = _resize_back(who, views, "views", gt, want_pred)
    dev = views.device
    lo, ld = _resize_channels_last(views)

    def launch(layout, pred, g, gt_bytes, counts, ws, nbytes):
        first_px, first_tile, n_tiles, total_px = layout
        desc = torch.tensor([[H, W, p0, t0, Hc, Wc, w0, len(wl)] for (H, W), p0, t0, (Hc, Wc), w0, wl in
                             zip(hw, first_px, first_tile, canv, first_win, windows)], dtype=torch.int64).to(dev)
        win = torch.tensor(rows, dtype=torch.int32).to(dev)
        rc = _fn(f"lc2is_{name}")(_ptr(lo), ld, V, h, w, K, _ptr(desc), N, _ptr(win), len(rows), n_tiles, total_px, _ptr(g),
                                  gt_bytes, -1 if ignore_index is None else int(ignore_index), _ptr(pred), _ptr(counts), _ptr(ws),
                                  nbytes, _stream())
        _lib.check(rc, f"{name} N={N} V={V} K={K} h={h} w={w}")
    return _resize_run(hw, K, gt, dts, want_pred, dev, launch, wide)


def resize_argmax_windows_wide(views, windows, canvases, sizes, gt=None, want_pred: bool = True,
                               ignore_index: int | None = None):
    """``resize_argmax_windows`` for 1 <= K <= 1024 classes (lc2is_resize_argmax_windows_wide): the same arguments and checks;
    pred is int16, and with K <= 192 the class indices and counts are ``resize_argmax_windows``'s (the faster call there)."""
    return _resize_argmax_windows(views, windows, canvases, sizes, gt, want_pred, ignore_index, wide=True)


MS_MAX_CANVAS = 16                      # LC2IS_MS_MAX_CANVAS: canvases per image of lc2is_resize_argmax_multiscale
_MS_MODES = {"logit": 0, "prob": 1}     # LC2IS_MS_LOGIT, LC2IS_MS_PROB


def resize_argmax_multiscale(views, canvases, sizes, gt=None, want_pred: bool = True, ignore_index: int | None = None,
                             mode: str = "prob"):
    """``resize_argmax_windows`` over several canvases per image (lc2is_resize_argmax_multiscale): multi-scale / flip evaluation.
    canvases[i]: the ordered list of ((Hc, Wc), windows) of image i, 1 to 16 of them, ``windows`` as in ``resize_argmax_windows``
    (1 to 64 per canvas, every canvas cell covered).  Every canvas is the window mean, resized to sizes[i]; the resized canvases
    are summed per class in list order, as logits (mode="logit") or after a softmax over the classes of each (mode="prob", mmseg's
    aug_test), and the argmax of the sum is taken.  No canvas and no [K, H, W] map is formed.
    A canvas may be smaller than a view (a scale below the crop): a window's origin must lie on the canvas, and only the part of
    the view that lies on the canvas is read (its top-left min(h, Hc - oy) x min(w, Wc - ox) cells; a mirrored view is mirrored
    over that part).
    views, sizes, gt, want_pred, ignore_index and the returned (pred, counts): as ``resize_argmax_windows``.
    Everything is validated on the host before anything is allocated."""
    return _resize_argmax_multiscale(views, canvases, sizes, gt, want_pred, ignore_index, mode, wide=False)


def _resize_argmax_multiscale(views, canvases, sizes, gt, want_pred, ignore_index, mode, wide):
    """``resize_argmax_multiscale`` (wide=False) and ``resize_argmax_multiscale_wide``: one body."""
    name = "resize_argmax_multiscale_wide" if wide else "resize_argmax_multiscale"
    who = f"lc2is_amd.{name}"
    V, K, h, w = _resize_front(who, views, "views must be NCHW [V, K, h, w]", RESIZE_WIDE_KMAX if wide else RESIZE_KMAX)
    if mode not in _MS_MODES:
        raise ValueError(f"{who}: mode must be 'prob' or 'logit', got {mode!r}")
    N = len(canvases)
    if N < 1:
        raise ValueError(f"{who}: no images")
    hw = resize_sizes(N, sizes, gt)
    _resize_ignore_index(who, ignore_index)
    crows, rows, first_canvas = [], [], []
    for i, cl in enumerate(canvases):
        if not 1 <= len(cl) <= MS_MAX_CANVAS:
            raise ValueError(f"{who}: image {i} has {len(cl)} canvases (1 to {MS_MAX_CANVAS})")
        first_canvas.append(len(crows))
        for a, (cv, wl) in enumerate(cl):
            Hc, Wc = (int(v) for v in cv)
            if Hc < 1 or Wc < 1:
                raise ValueError(f"{who}: image {i} canvas {a}: size ({Hc}, {Wc}) is not positive")
            crows.append((Hc, Wc, len(rows), len(wl)))
            _resize_windows(who, f"image {i} canvas {a}", wl, (Hc, Wc), V, h, w, rows, overhang=True)
    dts = _resize_back(who, views, "views", gt, want_pred)
    dev = views.device
    lo, ld = _resize_channels_last(views)

    def launch(layout, pred, g, gt_bytes, counts, ws, nbytes):
        first_px, first_tile, n_tiles, total_px = layout
        desc = torch.tensor([[H, W, p0, t0, c0, len(cl)] for (H, W), p0, t0, c0, cl in
                             zip(hw, first_px, first_tile, first_canvas, canvases)], dtype=torch.int64).to(dev)
        canv = torch.tensor(crows, dtype=torch.int64).to(dev)
        win = torch.tensor(rows, dtype=torch.int32).to(dev)
        rc = _fn(f"lc2is_{name}")(_ptr(lo), ld, V, h, w, K, _ptr(desc), N, _ptr(canv), len(crows), _ptr(win), len(rows), n_tiles,
                                  total_px, _ptr(g), gt_bytes, -1 if ignore_index is None else int(ignore_index), _MS_MODES[mode],
                                  _ptr(pred), _ptr(counts), _ptr(ws), nbytes, _stream())
        _lib.check(rc, f"{name} N={N} V={V} K={K} h={h} w={w} canvases={len(crows)} mode={mode}")
    return _resize_run(hw, K, gt, dts, want_pred, dev, launch, wide)


def resize_argmax_multiscale_wide(views, canvases, sizes, gt=None, want_pred: bool = True, ignore_index: int | None = None,
                                  mode: str = "prob"):
    """``resize_argmax_multiscale`` for 1 <= K <= 1024 classes (lc2is_resize_argmax_multiscale_wide): the same arguments, checks
    and modes; pred is int16, and with K <= 192 the class indices and counts are ``resize_argmax_multiscale``'s (the faster call
    there)."""
    return _resize_argmax_multiscale(views, canvases, sizes, gt, want_pred, ignore_index, mode, wide=True)


# ---- Swin backbone ----------------------------------------------------------------------------------------------
def rows_gather(src: torch.Tensor, index_map: torch.Tensor, *, out: torch.Tensor | None = None, out_dtype=None,
                add: torch.Tensor | None = None, cols: int | None = None):
    """out[r, :cols] = (map[r] >= 0 ? src[map[r], :cols] : 0) (+ add[r, :cols]).  src/out fp32 or bf16 2-D (row
    strides allowed), map int32 [rows], add fp32."""
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("lc2is_amd.rows_gather: src must be fp32 or bf16")
    _chk(src, src.dtype, "src"); _chk(index_map, torch.int32, "map", 1); _chk(add, torch.float32, "add")
    rows = index_map.numel()
    cols = src.shape[1] if cols is None else cols
    if out is None:
        out = torch.empty((rows, cols), dtype=out_dtype or src.dtype, device=src.device)
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("lc2is_amd.rows_gather: out must be fp32 or bf16")
    _chk(out, out.dtype, "out")
    if out.shape[0] != rows or out.shape[1] < cols or src.shape[1] < cols or (add is not None and add.shape[0] != rows):
        raise RuntimeError("lc2is_amd.rows_gather: shape mismatch")
    rc = _fn("lc2is_rows_gather")(_ptr(src), _ld(src), int(src.dtype == torch.bfloat16), _ptr(out), _ld(out),
                                  int(out.dtype == torch.bfloat16), _ptr(index_map), _ptr(add), _ld(add), rows, cols,
                                  _stream())
    _lib.check(rc, f"rows_gather rows={rows} cols={cols}")
    return out


def swin_attn_fwd(qkv: torch.Tensor, bias: torch.Tensor, nwin: int, win_per_img: int, nwx: int, Hp: int, Wp: int,
                  ws: int, shift: int, nH: int, scale: float, *, save_lse: bool = True, out: torch.Tensor | None = None):
    """qkv bf16 [nwin*ws*ws, 3C]; bias fp32 [nH, S, S].  Returns (o bf16 [nwin*S, C], lse [nwin, nH, S])."""
    who, dev = "swin_attn_fwd", qkv.device
    S, Cc = ws * ws, _dims(who, qkv, "qkv", 2, torch.bfloat16)[1] // 3
    if qkv.shape != (nwin * S, 3 * Cc):
        raise RuntimeError(f"lc2is_amd.swin_attn_fwd: qkv must have shape {(nwin * S, 3 * Cc)}, got {tuple(qkv.shape)}")
    if bias is None:
        raise RuntimeError("lc2is_amd.swin_attn_fwd: bias is required")
    _chk_op(who, bias, "bias", torch.float32, (nH, S, S), dev, 4)
    _chk_op(who, out, "out", torch.bfloat16, (nwin * S, Cc), dev)
    o = out if out is not None else torch.empty((nwin * S, Cc), dtype=torch.bfloat16, device=dev)
    lse = torch.empty((nwin, nH, S), dtype=torch.float32, device=qkv.device)
    rc = _fn("lc2is_swin_attn_fwd")(_ptr(qkv), _ld(qkv), _ptr(o), _ld(o), _ptr(lse), _ptr(bias), nwin, win_per_img, nwx,
                                    Hp, Wp, ws, shift, nH, Cc, float(scale), _stream())
    _lib.check(rc, f"swin_attn_fwd nwin={nwin} nH={nH} ws={ws}")
    return o, (lse if save_lse else None)


def swin_attn_bwd(qkv, o, do, lse, bias, nwin: int, win_per_img: int, nwx: int, Hp: int, Wp: int, ws: int, shift: int,
                  nH: int, scale: float, *, dbias: torch.Tensor | None = None, accumulate_dbias: bool = False,
                  dqkv: torch.Tensor | None = None):
    """Returns dqkv bf16 [nwin*S, 3C]; dbias fp32 [nH,S,S] is written (or accumulated) when given."""
    who, dev, bf, f32 = "swin_attn_bwd", qkv.device, torch.bfloat16, torch.float32
    S, Cc = ws * ws, _dims(who, qkv, "qkv", 2, bf)[1] // 3
    rows = nwin * S
    if qkv.shape != (rows, 3 * Cc):
        raise RuntimeError(f"lc2is_amd.swin_attn_bwd: qkv must have shape {(rows, 3 * Cc)}, got {tuple(qkv.shape)}")
    _chk_op(who, dqkv, "dqkv", bf, (rows, 3 * Cc), dev)
    if dqkv is None:
        dqkv = torch.empty((rows, 3 * Cc), dtype=bf, device=dev)
    for t, n, s in ((o, "o", (rows, Cc)), (do, "do", (rows, Cc))):
        if t is None:
            raise RuntimeError(f"lc2is_amd.swin_attn_bwd: {n} is required")
        _chk_op(who, t, n, bf, s, dev)
    if lse is None or bias is None:
        raise RuntimeError("lc2is_amd.swin_attn_bwd: lse and bias are required")
    _chk_op(who, lse, "lse", f32, (nwin, nH, S), dev, 4); _chk_op(who, bias, "bias", f32, (nH, S, S), dev, 4)
    _chk_op(who, dbias, "dbias", f32, (nH, S, S), dev, 4)
    ws_b = None
    if dbias is not None:
        nbytes = _fn("lc2is_swin_attn_bwd_workspace_bytes")(nwin, ws, nH)
        ws_b = workspace(nbytes, qkv.device, "swin_attn")
    rc = _fn("lc2is_swin_attn_bwd")(_ptr(qkv), _ld(qkv), _ptr(o), _ld(o), _ptr(do), _ld(do), _ptr(lse), _ptr(bias),
                                    _ptr(dqkv), _ld(dqkv), _ptr(dbias), int(accumulate_dbias), nwin, win_per_img, nwx,
                                    Hp, Wp, ws, shift, nH, Cc, float(scale), _ptr(ws_b),
                                    0 if ws_b is None else ws_b.numel(), _stream())
    _lib.check(rc, f"swin_attn_bwd nwin={nwin} nH={nH} ws={ws}")
    return dqkv


# ---- preprocessing (uint8 images) ---------------------------------------------------------------------------------
def swin_bias_table_grad(dbias: torch.Tensor, offsets: torch.Tensor, positions: torch.Tensor, dtable: torch.Tensor,
                         accumulate: bool = False):
    """dtable [T, nH] (+)= sum of dbias [nH, S, S] over the pairs of each relative offset (CSR index, fixed order)."""
    _chk(dbias, torch.float32, "dbias", 3); _chk(dtable, torch.float32, "dtable", 2)
    _chk(offsets, torch.int32, "offsets", 1); _chk(positions, torch.int32, "positions", 1)
    nH, S, S2 = dbias.shape
    T = dtable.shape[0]
    if S2 != S or dtable.shape[1] != nH or offsets.numel() != T + 1 or positions.numel() != S * S \
            or not dbias.is_contiguous() or not dtable.is_contiguous():
        raise RuntimeError("lc2is_amd.swin_bias_table_grad: shape mismatch")
    rc = _fn("lc2is_swin_bias_table_grad")(_ptr(dbias), _ptr(offsets), _ptr(positions), _ptr(dtable), nH, S * S, T,
                                           int(accumulate), _stream())
    _lib.check(rc, "swin_bias_table_grad")
    return dtable


def _u8(t, name):
    if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 3 or not t.is_contiguous():
        raise RuntimeError(f"lc2is_amd: {name} must be a contiguous uint8 HWC tensor on a HIP device")


def resample_u8(src: torch.Tensor, out_size: int, axis: int, bounds: torch.Tensor, kk: torch.Tensor):
    """One separable 8-bit Pillow resampling pass over an HWC uint8 image (axis 1 = width, 0 = height)."""
    _u8(src, "src"); _chk(bounds, torch.int32, "bounds"); _chk(kk, torch.int32, "kk")
    H, W, Cc = src.shape
    if tuple(bounds.shape) != (out_size, 2) or kk.shape[0] != out_size or not (bounds.is_contiguous() and kk.is_contiguous()):
        raise RuntimeError("lc2is_amd.resample_u8: coefficient tables do not match out_size")
    out = torch.empty((out_size, W, Cc) if axis == 0 else (H, out_size, Cc), dtype=torch.uint8, device=src.device)
    rc = _fn("lc2is_resample_u8")(_ptr(src), H, W, Cc, _ptr(out), out_size, axis, _ptr(bounds), _ptr(kk), kk.shape[1], _stream())
    _lib.check(rc, f"resample_u8 {H}x{W}x{Cc} -> {out_size} axis {axis}")
    return out


def gather2d_u8(src: torch.Tensor, yi: torch.Tensor, xi: torch.Tensor):
    _u8(src, "src"); _chk(yi, torch.int32, "yi", 1); _chk(xi, torch.int32, "xi", 1)
    H, W, Cc = src.shape
    out = torch.empty((yi.numel(), xi.numel(), Cc), dtype=torch.uint8, device=src.device)
    rc = _fn("lc2is_gather2d_u8")(_ptr(src), H, W, Cc, _ptr(out), yi.numel(), xi.numel(), _ptr(yi), _ptr(xi), _stream())
    _lib.check(rc, "gather2d_u8")
    return out


def crop_lut(src: torch.Tensor, top: int, left: int, S: int, *, lut_f32: torch.Tensor | None = None,
             out_f32: torch.Tensor | None = None, lut_i64: torch.Tensor | None = None, out_i64: torch.Tensor | None = None):
    """S x S crop + lookup: float32 CHW pixel values (lut_f32 [C,256]) and / or int64 label ids of channel 0 (lut_i64 [256])."""
    _u8(src, "src")
    H, W, Cc = src.shape
    if lut_f32 is not None:
        _chk(lut_f32, torch.float32, "lut_f32")
        if tuple(lut_f32.shape) != (Cc, 256) or not lut_f32.is_contiguous():
            raise RuntimeError("lc2is_amd.crop_lut: lut_f32 must be [C,256]")
        out_f32 = out_f32 if out_f32 is not None else torch.empty((Cc, S, S), dtype=torch.float32, device=src.device)
        if tuple(out_f32.shape) != (Cc, S, S) or not out_f32.is_contiguous() or out_f32.dtype != torch.float32:
            raise RuntimeError("lc2is_amd.crop_lut: out_f32 must be contiguous float32 [C,S,S]")
    if lut_i64 is not None:
        _chk(lut_i64, torch.int64, "lut_i64", 1)
        out_i64 = out_i64 if out_i64 is not None else torch.empty((S, S), dtype=torch.int64, device=src.device)
        if tuple(out_i64.shape) != (S, S) or not out_i64.is_contiguous() or out_i64.dtype != torch.int64:
            raise RuntimeError("lc2is_amd.crop_lut: out_i64 must be contiguous int64 [S,S]")
    rc = _fn("lc2is_crop_lut")(_ptr(src), H, W, Cc, top, left, S, _ptr(lut_f32), _ptr(out_f32 if lut_f32 is not None else None),
                               _ptr(lut_i64), _ptr(out_i64 if lut_i64 is not None else None), _stream())
    _lib.check(rc, f"crop_lut {H}x{W} crop {S}@({top},{left})")
    return out_f32, out_i64


# ---- train-time augmentation (device image pool) -------------------------------------------------------------------
AUG_PARAM_WORDS, AUG_MAX_SIDE = 20, 4096      # LC2IS_AUG_PARAM_WORDS, LC2IS_AUG_MAX_SIDE
AUG_NH, AUG_NW, AUG_TOP, AUG_LEFT, AUG_FLIP, AUG_M, AUG_O = 0, 1, 2, 3, 4, 5, 14
AUG_MAX_TRIES, LABEL_BINS = 10, 256                # LC2IS_AUG_MAX_TRIES; one histogram bin per uint8 label value


class AugConfig(C.Structure):
    """lc2is_aug_config (include/lc2is_hip.h): host struct, passed by value into aug_params_kernel."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("crop_size", C.c_int32), ("base_size", C.c_int32),
                ("ratio_lo1024", C.c_int32), ("ratio_hi1024", C.c_int32), ("flip_thr", C.c_uint32), ("photo_thr", C.c_uint32 * 4),
                ("brightness_delta", C.c_float), ("contrast_lo", C.c_float), ("contrast_hi", C.c_float),
                ("saturation_lo", C.c_float), ("saturation_hi", C.c_float), ("hue_delta", C.c_float)]


class AugNorm(C.Structure):
    """lc2is_aug_norm: out_c = (v / 255 - mean_c) * inv_std_c."""
    _fields_ = [("mean", C.c_float * 3), ("inv_std", C.c_float * 3)]


def _aug_tables(desc, slots, name):
    _chk(desc, torch.int64, "desc"); _chk(slots, torch.int64, "indices", 1)
    if desc.shape[1] != 3 or not desc.is_contiguous() or desc.shape[0] < 1 or slots.numel() < 1:
        raise RuntimeError(f"lc2is_amd.{name}: desc must be a contiguous int64 [n_images, 3] table (img_off, lab_off, H | W << 32) "
                           "and indices non-empty")


def aug_params(slots: torch.Tensor, epoch: torch.Tensor, desc: torch.Tensor, cfg: AugConfig, *, keys: torch.Tensor | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Draw one row of augmentation parameters per sample (lc2is_aug_params): int32 [B, AUG_PARAM_WORDS] = nh, nw, top, left, flip,
    fp32 colour matrix M[3][3] and offset o[3] (bit patterns; view the tensor as float32 to read them).  slots int64 [B]: rows of
    desc; keys int64 [B] or None: the dataset indices the random numbers are a function of (None: the slots); epoch: DEVICE int32
    scalar.  Nothing but device memory decides the result, so a captured call draws again on replay."""
    _aug_tables(desc, slots, "aug_params")
    B = _view_keys("aug_params", keys, epoch, slots.numel())
    out = _view_table("aug_params", out, "out", B, AUG_PARAM_WORDS, new_on=slots.device)
    rc = _fn("lc2is_aug_params")(_ptr(slots), _ptr(keys), B, _ptr(epoch), _ptr(desc), desc.shape[0], C.addressof(cfg), _ptr(out),
                                 _stream())
    _lib.check(rc, f"aug_params B={B}")
    return out


def aug_apply(img: torch.Tensor, lab: torch.Tensor, desc: torch.Tensor, slots: torch.Tensor, params: torch.Tensor, S: int, L: int,
              norm: AugNorm, *, pad_label: int = 0, out_img: torch.Tensor | None = None, out_lab: torch.Tensor | None = None):
    """One launch for the batch (lc2is_aug_apply): bilinear resize to (nh, nw) + zero pad + S x S crop + flip + colour + normalise of
    the pool's uint8 HWC pixels -> fp32 [B, 3, S, S], and the nearest-exact labels of the same geometry at the centres of the
    (S / L)^2 cells -> int64 [B, L, L].  img / lab: the pool's packed uint8 buffers; desc / slots as in aug_params; params its table."""
    _aug_tables(desc, slots, "aug_apply")
    _chk(img, torch.uint8, "img", 1); _chk(lab, torch.uint8, "lab", 1)
    B = slots.numel()
    _view_table("aug_apply", params, "params", B, AUG_PARAM_WORDS)
    if S < 1 or S > AUG_MAX_SIDE or S % 4 or L < 1 or S % L:
        raise ValueError(f"lc2is_amd.aug_apply: crop size {S} must be a multiple of 4 and of the label size {L}, at most {AUG_MAX_SIDE}")
    out_img = _view_out("aug_apply", out_img, "out_img", (B, 3, S, S), torch.float32, img.device)
    out_lab = _view_out("aug_apply", out_lab, "out_lab", (B, L, L), torch.int64, img.device)
    rc = _fn("lc2is_aug_apply")(_ptr(img), img.numel(), _ptr(lab), lab.numel(), _ptr(desc), desc.shape[0], _ptr(slots), _ptr(params),
                                B, S, L, C.addressof(norm), int(pad_label), _ptr(out_img), _ptr(out_lab), _stream())
    _lib.check(rc, f"aug_apply B={B} S={S} L={L}")
    return out_img, out_lab


def aug_crop_select(lab: torch.Tensor, desc: torch.Tensor, slots: torch.Tensor, epoch: torch.Tensor, cfg: AugConfig,
                    params: torch.Tensor, L: int, *, ratio1024: int, ignore_label: int = -1, tries: int = AUG_MAX_TRIES,
                    keys: torch.Tensor | None = None, info: torch.Tensor | None = None) -> torch.Tensor:
    """The class-ratio re-draw of the crop origin (lc2is_aug_crop_select), between aug_params and aug_apply: for every sample the
    candidates 0 (the row's own top / left) .. tries - 1 are checked in order on the L x L label cells aug_apply would write, the
    first one with more than one class and max count * 1024 < ratio1024 * counted cells is taken, else candidate `tries`
    unchecked.  `params` int32 [B, AUG_PARAM_WORDS] is changed IN PLACE (words AUG_TOP, AUG_LEFT).  Cells that are padding or
    hold ignore_label (0..255; -1: none) are not counted.  Returns info int32 [B, 4] = t*, n, m, d on the device ({tries, 0, 0, 0}:
    none accepted; {-1, 0, 0, 0}: a row out of range, left untouched).  lab: the pool's packed label buffer; desc / slots / keys /
    epoch / cfg as in aug_params.  Nothing but device memory decides the result."""
    _aug_tables(desc, slots, "aug_crop_select")
    _chk(lab, torch.uint8, "lab", 1)
    B, S, L = _view_keys("aug_crop_select", keys, epoch, slots.numel()), int(cfg.crop_size), int(L)
    _view_table("aug_crop_select", params, "params", B, AUG_PARAM_WORDS)
    if S < 1 or S > AUG_MAX_SIDE or L < 1 or S % L:
        raise ValueError(f"lc2is_amd.aug_crop_select: crop size {S} must be a multiple of the label size {L}, at most {AUG_MAX_SIDE}")
    if not 1 <= int(ratio1024) <= 1023 or not -1 <= int(ignore_label) <= 255 or not 1 <= int(tries) <= AUG_MAX_TRIES:
        raise ValueError(f"lc2is_amd.aug_crop_select: ratio1024 {ratio1024} must be 1..1023, ignore_label {ignore_label} -1..255 and "
                         f"tries {tries} 1..{AUG_MAX_TRIES}")
    info = _view_table("aug_crop_select", info, "info", B, 4, new_on=slots.device)
    rc = _fn("lc2is_aug_crop_select")(_ptr(lab), lab.numel(), _ptr(desc), desc.shape[0], _ptr(slots), _ptr(keys), B, _ptr(epoch),
                                      C.addressof(cfg), _ptr(params), L, int(ratio1024), int(ignore_label), int(tries), _ptr(info),
                                      _stream())
    _lib.check(rc, f"aug_crop_select B={B} S={S} L={L}")
    return info


def label_histogram(lab: torch.Tensor, desc: torch.Tensor, slots: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-image class counts (lc2is_label_histogram): int32 [B, 256], out[b, v] = pixels of image slots[b] whose label is v.  lab:
    the pool's packed label buffer; desc / slots as in aug_params.  A slot outside the table gives a row of zeros.  Exact, no atomics."""
    _aug_tables(desc, slots, "label_histogram")
    _chk(lab, torch.uint8, "lab", 1)
    B = slots.numel()
    out = _view_table("label_histogram", out, "out", B, LABEL_BINS, new_on=slots.device)
    rc = _fn("lc2is_label_histogram")(_ptr(lab), lab.numel(), _ptr(desc), desc.shape[0], _ptr(slots), B, _ptr(out), _stream())
    _lib.check(rc, f"label_histogram B={B}")
    return out


# ---- mixed-sample augmentation (ClassMix / CutMix) -------------------------------------------------------------------
MIX_NONE, MIX_CLASSMIX, MIX_CUTMIX = 0, 1, 2       # LC2IS_MIX_*
MIX_MAX_CLASSES, MIX_PLAN_WORDS, MIX_BITMAP, MIX_STREAM = 1024, 40, 8, 0x4D495831


class MixConfig(C.Structure):
    """lc2is_mix_config (include/lc2is_hip.h): host struct, passed by value into mix_select_kernel."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("mode", C.c_int32), ("n_classes", C.c_int32),
                ("ignore_index", C.c_int64), ("exclude_label", C.c_int64), ("area_lo1024", C.c_int32), ("area_hi1024", C.c_int32)]


def _mix_batch(px, lab, pw, name):
    n, S = _view_pixels("mix_apply", px, f"{name} pixels", align=4)
    _chk(lab, torch.int64, f"{name} labels", 3)
    L = lab.shape[1]
    _view_cells("mix_apply", lab, f"{name} labels", torch.int64, n, L)
    _view_cells("mix_apply", pw, f"{name} weights", torch.float32, n, L)
    return n, S, L


def mix_select(src_lab: torch.Tensor, keys: torch.Tensor, epoch: torch.Tensor, cfg: MixConfig, *,
               src_index: torch.Tensor | None = None, plan: torch.Tensor | None = None, info: torch.Tensor | None = None):
    """Draw one mixing plan per output sample (lc2is_mix_select): plan int32 [B, MIX_PLAN_WORDS] = mode, source row, cutmix box (top,
    left, bh, bw), classes present, classes chosen, and the chosen-class bitmap; info int32 [B, 4] = classes present, classes chosen,
    masked cells, L * L ({-1, 0, 0, 0}: the source row lies outside the source batch; that sample keeps its destination).  src_lab
    int64 [Bs, L, L]: the source batch's label maps; keys int64 [B]: the indices the random numbers are a function of; epoch: DEVICE
    int32 scalar; src_index int64 [B] or None (row b).  Nothing but device memory decides the result: a captured call draws again."""
    _chk(src_lab, torch.int64, "src_lab", 3); _chk(src_index, torch.int64, "src_index", 1)
    B = _view_keys("mix_select", keys, epoch)
    Bs, L = src_lab.shape[0], src_lab.shape[1]
    if Bs < 1 or src_lab.shape[2] != L or not src_lab.is_contiguous() or (src_index is not None and src_index.numel() != B):
        raise RuntimeError("lc2is_amd.mix_select: src_lab must be contiguous int64 [Bs, L, L] and src_index one int64 per output sample")
    if not 1 <= L <= AUG_MAX_SIDE:
        raise ValueError(f"lc2is_amd.mix_select: label size {L} must be 1..{AUG_MAX_SIDE}")
    if cfg.mode not in (MIX_NONE, MIX_CLASSMIX, MIX_CUTMIX) or not 1 <= cfg.n_classes <= MIX_MAX_CLASSES or \
            not 1 <= cfg.area_lo1024 <= cfg.area_hi1024 <= 1024:
        raise ValueError(f"lc2is_amd.mix_select: mode {cfg.mode} must be MIX_NONE / MIX_CLASSMIX / MIX_CUTMIX, n_classes {cfg.n_classes} "
                         f"1..{MIX_MAX_CLASSES} and the area range ({cfg.area_lo1024}, {cfg.area_hi1024}) ordered inside 1..1024")
    plan = _view_table("mix_select", plan, "plan", B, MIX_PLAN_WORDS, new_on=keys.device)
    info = _view_table("mix_select", info, "info", B, 4, new_on=keys.device)
    rc = _fn("lc2is_mix_select")(_ptr(src_lab), Bs, _ptr(src_index), _ptr(keys), B, _ptr(epoch), C.addressof(cfg), L, _ptr(plan),
                                 _ptr(info), _stream())
    _lib.check(rc, f"mix_select B={B} Bs={Bs} L={L}")
    return plan, info


def mix_apply(dst, src, plan: torch.Tensor, out=None):
    """One launch (lc2is_mix_apply): out = mask ? src[plan's source row] : dst for pixels fp32 [B, 3, S, S], labels int64 [B, L, L] and
    per-pixel weights fp32 [B, L, L], the mask on the L x L cells from `plan` (mix_select).  dst / src: (pixels, labels, weights or
    None = ones); the source batch may hold another number of samples and may be the destination batch itself.  out: (pixels,
    labels, weights) to write into; an output that overlaps an input is refused.  A select, never a blend: bit for bit the chosen
    side, whatever the other side holds."""
    (dpx, dlab, dpw), (spx, slab, spw) = dst, src
    B, S, L = _mix_batch(dpx, dlab, dpw, "destination")
    Bs, S2, L2 = _mix_batch(spx, slab, spw, "source")
    if (S2, L2) != (S, L):
        raise RuntimeError(f"lc2is_amd.mix_apply: the destination is {S} px / {L} cells a side, the source {S2} / {L2}")
    _view_side("mix_apply", B, S, L, 4)
    _view_table("mix_apply", plan, "plan", B, MIX_PLAN_WORDS)
    why = "may not alias an input (the source batch may be the destination batch)"
    opx, olab, opw = out or (None, None, None)
    opx = _view_out("mix_apply", opx, "out pixels", dpx.shape, torch.float32, dpx.device, inputs=(dpx, spx), refusal=why)
    olab = _view_out("mix_apply", olab, "out labels", dlab.shape, torch.int64, dlab.device, inputs=(dlab, slab), refusal=why)
    opw = _view_out("mix_apply", opw, "out weights", dlab.shape, torch.float32, dlab.device, inputs=(dpw, spw), refusal=why)
    rc = _fn("lc2is_mix_apply")(_ptr(dpx), _ptr(dlab), _ptr(dpw), _ptr(spx), _ptr(slab), _ptr(spw), Bs, _ptr(plan), B, S, L,
                                _ptr(opx), _ptr(olab), _ptr(opw), _stream())
    _lib.check(rc, f"mix_apply B={B} Bs={Bs} S={S} L={L}")
    return opx, olab, opw


# ---- strong photometric views (colour jitter, greyscale, Gaussian blur) ----------------------------------------------
STRONG_MAX_RADIUS, STRONG_PARAM_WORDS, STRONG_STREAM = 8, 32, 0x53545231      # LC2IS_STRONG_*
STRONG_FLAGS, STRONG_R, STRONG_SIGMA, STRONG_M, STRONG_O, STRONG_W = 0, 1, 2, 3, 12, 15
STRONG_COLOUR, STRONG_GREY, STRONG_BLUR = 1, 2, 4
STRONG_MIN_SIDE, STRONG_MAX_SIGMA = 12, 2.0


class StrongConfig(C.Structure):
    """lc2is_strong_config (include/lc2is_hip.h): host struct, passed by value into both kernels."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("jitter_thr", C.c_uint32), ("gray_thr", C.c_uint32),
                ("blur_thr", C.c_uint32), ("brightness_delta", C.c_float), ("contrast_lo", C.c_float), ("contrast_hi", C.c_float),
                ("saturation_lo", C.c_float), ("saturation_hi", C.c_float), ("hue_delta", C.c_float), ("sigma_lo", C.c_float),
                ("sigma_hi", C.c_float), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("inv_std", C.c_float * 3)]


def strong_params(keys: torch.Tensor, epoch: torch.Tensor, cfg: StrongConfig, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """Draw one row of strong-view parameters per sample (lc2is_strong_params): int32 [B, STRONG_PARAM_WORDS] = flags (bit 0 colour,
    bit 1 grey, bit 2 blur), the blur radius R, then fp32 bit patterns: sigma, the colour matrix M[3][3] and offset o[3], the blur taps
    w[0..8]; the rest 0.  keys int64 [B]: the indices the random numbers are a function of; epoch: DEVICE int32 scalar.  Nothing but
    device memory decides the result: a captured call draws again on replay."""
    B = _view_keys("strong_params", keys, epoch)
    if max(cfg.jitter_thr, cfg.gray_thr, cfg.blur_thr) > 1 << 24 or not 0.0 < cfg.sigma_lo <= cfg.sigma_hi <= STRONG_MAX_SIGMA:
        raise ValueError(f"lc2is_amd.strong_params: thresholds must be at most 2^24 and the sigma range ({cfg.sigma_lo}, {cfg.sigma_hi}) "
                         f"ordered inside (0, {STRONG_MAX_SIGMA}]")
    out = _view_table("strong_params", out, "out", B, STRONG_PARAM_WORDS, new_on=keys.device)
    rc = _fn("lc2is_strong_params")(_ptr(keys), B, _ptr(epoch), C.addressof(cfg), _ptr(out), _stream())
    _lib.check(rc, f"strong_params B={B}")
    return out


def _strong_batch(x: torch.Tensor, out: torch.Tensor | None):
    """Everything strong_apply asks of its input and output, before any device work; returns (B, S, out), out allocated if None."""
    B, S = _view_pixels("strong_apply", x, "pixel_values")
    _view_side("strong_apply", B, S, None, STRONG_MIN_SIDE)
    out = _view_out("strong_apply", out, "out", x.shape, torch.float32, x.device, 16, (x,), "may not overlap the input (the blur reads a halo: no in-place form)")
    return B, S, out


def strong_apply(x: torch.Tensor, params: torch.Tensor, cfg: StrongConfig, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """One launch (lc2is_strong_apply): the strong view of a normalised batch fp32 [B, 3, S, S] as the rows of `params`
    (strong_params) say: colour map on the 0..255 scale with one clamp, separable Gaussian blur with reflected borders, re-normalise;
    a row with no flag gives the input bit for bit.  S % 4 == 0, 12 <= S <= 4096.  x must be contiguous with a 16-byte base (a batch
    slice x[i:j] is; a strided or permuted view is refused, not copied); out: a tensor to write into, which may not overlap x (the
    blur reads a halo)."""
    B, S, out = _strong_batch(x, out)
    _view_table("strong_apply", params, "params", B, STRONG_PARAM_WORDS)
    rc = _fn("lc2is_strong_apply")(_ptr(x), _ptr(params), C.addressof(cfg), B, S, _ptr(out), _stream())
    _lib.check(rc, f"strong_apply B={B} S={S}")
    return out


# ---- geometric views (random affine warp; labels and weights follow) --------------------------------------------------
GEO_PARAM_WORDS, GEO_STREAM = 16, 0x47454F31                                   # LC2IS_GEO_*
GEO_FLAGS, GEO_M, GEO_T, GEO_REC = 0, 1, 5, 7
GEO_WARP, GEO_FLIP = 1, 2
GEO_ONE, GEO_MAX_M, GEO_MAX_T, GEO_MIN_SIDE = 65536, 524288, 65536, 8
GEO_MAX_ROTATE, GEO_MAX_SHEAR = C.c_float(math.pi).value, C.c_float(math.pi / 4).value      # the fp32 neighbours of pi, pi / 4
GEO_MIN_SCALE, GEO_MAX_SCALE, GEO_MAX_TRANSLATE = 0.25, 4.0, 0.5
_GATHERS = "may not overlap its input (a warp gathers: no in-place form)"


class GeoConfig(C.Structure):
    """lc2is_geo_config (include/lc2is_hip.h): host struct, passed by value into both kernels."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("warp_thr", C.c_uint32), ("flip_thr", C.c_uint32),
                ("rotate", C.c_float), ("scale_lo", C.c_float), ("scale_hi", C.c_float), ("shear", C.c_float),
                ("translate", C.c_float), ("fill", C.c_float * 3), ("ignore_index", C.c_int64)]


def _geo_config(cfg: GeoConfig, who: str) -> None:
    """The limits of include/lc2is_hip.h (they keep every |m| <= GEO_MAX_M); a NaN fails its comparison."""
    if max(cfg.warp_thr, cfg.flip_thr) > 1 << 24:
        raise ValueError(f"lc2is_amd.{who}: thresholds must be at most 2^24, got {cfg.warp_thr}, {cfg.flip_thr}")
    if not (0.0 <= cfg.rotate <= GEO_MAX_ROTATE and GEO_MIN_SCALE <= cfg.scale_lo <= cfg.scale_hi <= GEO_MAX_SCALE
            and 0.0 <= cfg.shear <= GEO_MAX_SHEAR and 0.0 <= cfg.translate <= GEO_MAX_TRANSLATE):
        raise ValueError(f"lc2is_amd.{who}: rotate {cfg.rotate} must be 0..pi, the scale range ({cfg.scale_lo}, {cfg.scale_hi}) ordered "
                         f"inside [{GEO_MIN_SCALE}, {GEO_MAX_SCALE}], shear {cfg.shear} 0..pi/4 and translate {cfg.translate} "
                         f"0..{GEO_MAX_TRANSLATE}")


def geo_params(keys: torch.Tensor, epoch: torch.Tensor, cfg: GeoConfig, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """Draw one affine map per sample (lc2is_geo_params): int32 [B, GEO_PARAM_WORDS] = flags (bit 0 warp, bit 1 flip), the output-to-
    source matrix m00 m01 m10 m11 and the translation tx ty in Q16, the fp32 bit patterns of theta, s, phi, fx, fy as drawn; the
    rest 0.  keys int64 [B]: the indices the random numbers are a function of; epoch: DEVICE int32 scalar.  Nothing but device
    memory decides the result: a captured call draws again on replay."""
    B = _view_keys("geo_params", keys, epoch)
    _geo_config(cfg, "geo_params")
    out = _view_table("geo_params", out, "out", B, GEO_PARAM_WORDS, new_on=keys.device)
    rc = _fn("lc2is_geo_params")(_ptr(keys), B, _ptr(epoch), C.addressof(cfg), _ptr(out), _stream())
    _lib.check(rc, f"geo_params B={B}")
    return out


def _geo_batch(batch, out):
    """Everything geo_apply asks of its batch and outputs, before any device work; returns (B, S, L, out) with the missing outputs
    allocated.  An entry of the batch that is None has None as its output."""
    if not isinstance(batch, (tuple, list)) or len(batch) != 3:
        raise TypeError("lc2is_amd.geo_apply: batch must be (pixel_values, labels or None, pixel_weight or None)")
    px, lab, pw = batch
    if px is None:
        raise RuntimeError("lc2is_amd.geo_apply: pixel_values are required")
    _chk(px, torch.float32, "pixel_values", 4); _chk(lab, torch.int64, "labels", 3); _chk(pw, torch.float32, "pixel_weight", 3)
    B, S = _view_pixels("geo_apply", px, "pixel_values")
    L = next((m.shape[1] for m in (lab, pw) if m is not None), S)
    _view_cells("geo_apply", lab, "labels", torch.int64, B, L, px.device)
    _view_cells("geo_apply", pw, "pixel_weight", torch.float32, B, L, px.device)
    _view_side("geo_apply", B, S, L, GEO_MIN_SIDE)
    if out is None:
        out = (None, None, None)
    if not isinstance(out, (tuple, list)) or len(out) != 3:
        raise TypeError("lc2is_amd.geo_apply: out must be (pixel_values, labels or None, pixel_weight or None)")
    outs = tuple(None if i is None else _view_out("geo_apply", o, name, i.shape, i.dtype, i.device, align, (i,), _GATHERS, dev=i.device)
                 for o, i, align, name in ((out[0], px, 16, "out pixel_values"), (out[1], lab, 8, "out labels"),
                                           (out[2], pw, 4, "out pixel_weight")))
    return B, S, L, outs


def geo_apply(batch, params: torch.Tensor, cfg: GeoConfig, *, out=None):
    """One launch (lc2is_geo_apply): the affine warp of batch = (pixel_values fp32 [B, 3, S, S], labels int64 [B, L, L] or None,
    pixel_weight fp32 [B, L, L] or None) as the rows of `params` (geo_params) say, all three under the same map: pixels bilinear with
    cfg.fill out of frame, labels and weights nearest with cfg.ignore_index / 0.0 out of frame.  A row with no flag, or one out of
    range, gives the sample bit for bit.  S % 4 == 0, S % L == 0, 8 <= S <= 4096.  Tensors must be contiguous (a batch slice is; a
    strided or permuted view is refused, not copied); out: (pixels, labels, weights) to write into, none of which may overlap its
    input.  Returns (pixels, labels, weights); an entry that was None stays None."""
    B, S, L, (opx, olab, opw) = _geo_batch(batch, out)
    _geo_config(cfg, "geo_apply")
    _view_table("geo_apply", params, "params", B, GEO_PARAM_WORDS)
    px, lab, pw = batch
    rc = _fn("lc2is_geo_apply")(_ptr(px), _ptr(lab), _ptr(pw), _ptr(params), C.addressof(cfg), B, S, L, _ptr(opx), _ptr(olab),
                                _ptr(opw), _stream())
    _lib.check(rc, f"geo_apply B={B} S={S} L={L}")
    return opx, olab, opw


GEO_SCORES_MAX_G, GEO_SCORES_MAX_LD = 512, 1024                               # lc2is_geo_scores' limits


def _geo_scores_batch(scores, B, g, teacher_weight, label_size, out):
    """Everything geo_scores asks of its operands and outputs, before any device work (as _geo_batch for geo_apply); returns
    (ld, L or None, (scores', weight' or None)) with the missing outputs allocated."""
    for v, what in ((B, "B"), (g, "g"), (label_size, "label_size")):
        if (v is not None or what != "label_size") and (isinstance(v, bool) or not isinstance(v, int)):
            raise TypeError(f"lc2is_amd.geo_scores: {what} must be an int, got {v!r}")
    if out is None:
        out = (None, None)
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise TypeError("lc2is_amd.geo_scores: out must be (scores or None, weight or None)")
    for t, what in ((scores, "scores"), (teacher_weight, "teacher_weight"), (out[0], "out scores"), (out[1], "out weight")):
        if (t is not None or what == "scores") and not torch.is_tensor(t):
            raise TypeError(f"lc2is_amd.geo_scores: {what} must be a tensor, got {type(t).__name__}")
    _chk(scores, torch.float32, "scores", 2); _chk(teacher_weight, torch.float32, "teacher_weight", 3)
    ld = scores.shape[1]
    if not 1 <= B <= 65535 or not 1 <= g <= GEO_SCORES_MAX_G or ld < 4 or ld > GEO_SCORES_MAX_LD or ld % 4:
        raise ValueError(f"lc2is_amd.geo_scores: B {B} must be 1..65535, g {g} 1..{GEO_SCORES_MAX_G} and the pitch {ld} a multiple of 4 in "
                         f"4..{GEO_SCORES_MAX_LD}")
    if scores.shape[0] != B * g * g or not scores.is_contiguous() or scores.data_ptr() % 16:
        raise RuntimeError(f"lc2is_amd.geo_scores: scores must be contiguous fp32 [{B}*{g}*{g}, ld] with a 16-byte base, got shape "
                           f"{tuple(scores.shape)}, strides {tuple(scores.stride())}")
    L = label_size
    if teacher_weight is not None:
        Lw = teacher_weight.shape[1]
        _view_cells("geo_scores", teacher_weight, "teacher_weight", torch.float32, B, Lw, scores.device)
        if L is not None and L != Lw:
            raise ValueError(f"lc2is_amd.geo_scores: label_size {L} is not the teacher_weight's {Lw}")
        L = Lw
    if L is not None and (L < 1 or L > AUG_MAX_SIDE or L % g):
        raise ValueError(f"lc2is_amd.geo_scores: the label size {L} must be a multiple of g = {g} in 1..{AUG_MAX_SIDE}")
    if L is None and out[1] is not None:
        raise ValueError("lc2is_amd.geo_scores: an out weight without teacher_weight or label_size: no weight map is made")
    osc = _view_out("geo_scores", out[0], "out scores", scores.shape, torch.float32, scores.device, 16, (scores,), _GATHERS, dev=scores.device)
    otw = None if L is None else _view_out("geo_scores", out[1], "out weight", (B, L, L), torch.float32, scores.device, 4,
                                           (teacher_weight,), _GATHERS, dev=scores.device)
    return ld, L, (osc, otw)


def geo_scores(scores: torch.Tensor, params: torch.Tensor, B: int, g: int, *, teacher_weight: torch.Tensor | None = None,
               label_size: int | None = None, out=None):
    """One launch (lc2is_geo_scores): a teacher's low-resolution scores fp32 [B*g*g, ld] (model.head_scores' layout, every column
    alike) under the rows of `params` (geo_params) - the map geo_apply gave the student's pixels - bilinear with BORDER padding:
    F.grid_sample(padding_mode="border", align_corners=False) of the recorded matrix on the [B, ld, g, g] view.  A row with no flag,
    or one out of range, gives the sample bit for bit.  teacher_weight fp32 [B, L, L] follows under geo_apply's cell rule (0.0 out
    of frame); label_size=L without it asks for the in-frame mask (1.0 / 0.0) at that size; with neither no weight map is made.
    g <= 512, ld % 4 == 0 in 4..1024, L % g == 0.  Tensors must be contiguous (refused, not copied); out: (scores, weight) to write
    into, neither of which may overlap its input.  Returns (scores', weight' or None)."""
    ld, L, (osc, otw) = _geo_scores_batch(scores, B, g, teacher_weight, label_size, out)
    _view_table("geo_scores", params, "params", B, GEO_PARAM_WORDS, dev=scores.device)
    rc = _fn("lc2is_geo_scores")(_ptr(scores), _ptr(teacher_weight), _ptr(params), B, g, ld, L or 0, int(L is not None), _ptr(osc),
                                 _ptr(otw), _stream())
    _lib.check(rc, f"geo_scores B={B} g={g} ld={ld} L={L}")
    return osc, otw


def set_cu_budget(ncu: int) -> None:
    """Compute units the GEMM tile planners may count on (0 = all 256): include/lc2is_hip.h lc2is_set_cu_budget."""
    _lib.check(_fn("lc2is_set_cu_budget")(int(ncu)), "set_cu_budget")


def get_cu_budget() -> int:
    return int(_fn("lc2is_get_cu_budget")())
