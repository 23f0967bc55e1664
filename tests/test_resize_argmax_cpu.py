"""CPU-side checks of the original-size resize + argmax (lc2is_resize_argmax): the C ABI is declared and bound, its workspace query
is a pure host function with the stated formula, the C entry point refuses bad arguments before any launch, and the Python layer
refuses CPU outputs, sizes that disagree with the gt maps, K > 192 and other gt dtypes before it allocates anything."""
import inspect

import pytest
import torch

from lc2is_amd import _lib, evalloop, metrics, ops


def test_header_declares_and_ops_binds_both_entry_points():
    syms = _lib.header_symbols()
    for s in ("lc2is_resize_argmax", "lc2is_resize_argmax_workspace_bytes"):
        assert s in syms and s in ops._ARGTYPES
        assert hasattr(_lib.load(), s)


def test_workspace_query_is_a_pure_host_function():
    ws = ops._fn("lc2is_resize_argmax_workspace_bytes")
    # n_tiles * 3 * K * 4: one int32 {intersection, predicted, labelled} slab per 16 x 16 tile
    for n_tiles, K in ((1, 1), (1376, 151), (12288, 151), (5, 192)):
        assert ws(n_tiles, K) == n_tiles * 3 * K * 4
    assert ws(0, 151) == 0 and ws(10, 0) == 0 and ws(10, 193) == 0
    tiles = lambda H, W: -(-H // 16) * -(-W // 16)
    assert tiles(683, 512) == 43 * 32 and tiles(1, 1) == 1 and tiles(2048, 1536) == 12288


def test_c_entry_point_refuses_before_launching():
    """Error codes come back from argument checks alone: the pointers (never dereferenced) need not be device memory."""
    f = ops._fn("lc2is_resize_argmax")
    P = 0x10000   # 16-byte aligned stand-in
    ok = dict(scores=P, ld=152, N=1, h=128, w=128, K=151, desc=P, n_tiles=1376, total_px=683 * 512, gt=P, gt_bytes=1, pred=P,
              counts=P, ws=P, ws_bytes=1376 * 3 * 151 * 4)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["scores"], a["ld"], a["N"], a["h"], a["w"], a["K"], a["desc"], a["n_tiles"], a["total_px"], a["gt"],
                 a["gt_bytes"], a["pred"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert call(K=193, ld=196) == -3                      # LC2IS_ERR_UNSUPPORTED: K > 192
    assert call(gt_bytes=2) == -3                         # gt neither uint8 nor int32 nor int64
    assert call(scores=None) == -2 and call(desc=None) == -2 and call(pred=None, counts=None) == -2
    assert call(gt=None) == -2 and call(ws=None) == -2    # counts need gt and the workspace
    assert call(ld=150) == -1 and call(ld=154) == -1 and call(scores=P + 4) == -1 and call(n_tiles=0) == -1
    assert call(ws_bytes=1376 * 3 * 151 * 4 - 1) == -4    # LC2IS_ERR_WORKSPACE


def _gt(H, W, dtype=torch.int64):
    return torch.zeros(H, W, dtype=dtype)


def test_python_layer_refuses_bad_calls_before_allocating():
    x = torch.zeros(2, 151, 8, 8)                         # CPU outputs
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.compute_gt_mIOU(x, [_gt(5, 7), _gt(9, 3)], [(5, 7), (9, 3)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.original_size_predictions(x, [(5, 7), (9, 3)])
    with pytest.raises(ValueError, match="shapes"):
        metrics.compute_gt_mIOU(x, [_gt(5, 7), _gt(9, 3)], [(5, 7), (3, 9)])
    with pytest.raises(ValueError):
        metrics.per_image_gt_mIOU(x, [_gt(5, 7)], [(5, 7)])           # one gt map for two images
    with pytest.raises(ValueError):
        metrics.original_size_predictions(x, [(5, 7), (0, 3)])
    with pytest.raises(RuntimeError, match="192"):
        ops.resize_argmax(torch.zeros(1, 193, 8, 8), [(16, 16)])
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        ops.resize_argmax(x, None, gt=[_gt(5, 7, torch.int16), _gt(9, 3)])
    with pytest.raises(RuntimeError, match="uint8, int32 or int64"):
        ops.resize_argmax(x, None, gt=[_gt(5, 7, torch.float32), _gt(9, 3)])


def test_sizes_come_from_sequences_tensors_or_the_gt_maps():
    gt = [_gt(5, 7, torch.uint8), _gt(9, 3, torch.int32)]
    assert ops.resize_sizes(2, None, gt) == [(5, 7), (9, 3)]
    assert ops.resize_sizes(2, torch.tensor([[5, 7], [9, 3]]), gt) == [(5, 7), (9, 3)]
    assert ops.resize_sizes(2, [(5, 7), (9, 3)]) == [(5, 7), (9, 3)]


def test_segmentation_metrics_accepts_gt_list_and_sizes():
    params = inspect.signature(evalloop.segmentation_metrics).parameters
    assert list(params)[:6] == ["outputs", "labels", "gt_list", "sizes", "n_clas", "ignore_index"]
    assert params["gt_list"].default is None and params["sizes"].default is None
    assert list(inspect.signature(metrics.compute_gt_mIOU).parameters) == ["outputs", "gt_list", "sizes", "n_cls", "ignore_index"]
    assert inspect.signature(evalloop.Evaluator).parameters["gt_from_metas"].default is None
