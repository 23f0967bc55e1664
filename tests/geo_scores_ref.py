"""Numpy restatement of lc2is_geo_scores (include/lc2is_hip.h), test-only, written from the header on top of tests/geo_ref.py
(source_uv, cell_index, row_is_mapped): the score rule with int64 positions that are clamped BEFORE they are split into index and
fraction (border padding: no fill exists) and a float64 blend; the weight rule is geo_ref's cell rule with 0.0 out of frame, ones
standing in for a weight map that is not given.  Shared by tests/test_geo_scores_cpu.py and tests/test_gpu_geo_scores.py."""
import numpy as np

import geo_ref as GR


def split(row, g):
    """(y0, x0, fyi, fxi, in_frame) int64 / bool [g, g]: the near tap and the 17-bit fractions of every output cell, and whether the
    UNCLAMPED position lies in [0, (g - 1) 2^17]^2 - there the four taps are geo_apply's pixel taps, none of them outside."""
    U, V = GR.source_uv(row, g)
    X, Y = U + (g - 1) * GR.ONE, V + (g - 1) * GR.ONE
    last = (g - 1) << 17
    in_frame = (X >= 0) & (X <= last) & (Y >= 0) & (Y <= last)
    X, Y = np.clip(X, 0, last), np.clip(Y, 0, last)
    return Y >> 17, X >> 17, Y & 0x1FFFF, X & 0x1FFFF, in_frame


def is_exact(row, g):
    """Every fraction of the row is 0 at side g: the warp selects, and moves bits."""
    _, _, fyi, fxi, _ = split(row, g)
    return not fyi.any() and not fxi.any()


def warp_scores(x, row):
    """One sample: x [g, g, ld] (any float dtype) -> float64 [g, g, ld]; the near tap selected where a fraction is 0 (NaN / inf in a
    tap that is not selected does not reach the output).  A far tap that is used has an index of at most g - 1."""
    x = np.asarray(x)
    g = x.shape[0]
    y0, x0, fyi, fxi, _ = split(row, g)
    assert (x0[fxi != 0] <= g - 2).all() and (y0[fyi != 0] <= g - 2).all() and x0.min() >= 0 and y0.min() >= 0 and max(x0.max(), y0.max()) <= g - 1
    x1, y1 = np.minimum(x0 + 1, g - 1), np.minimum(y0 + 1, g - 1)
    p = x.astype(np.float64)
    p00, p01, p10, p11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    fx, fy = (fxi / 131072.0)[..., None], (fyi / 131072.0)[..., None]
    hx, hy = (fxi != 0)[..., None], (fyi != 0)[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        top = np.where(hx, p00 + fx * (p01 - p00), p00)
        bot = np.where(hx, p10 + fx * (p11 - p10), p10)
        return np.where(hy, top + fy * (bot - top), top)


def select_scores(x, row):
    """The near taps alone, in x's dtype: what an exact row (is_exact) gives, bit for bit."""
    y0, x0, _, _, _ = split(row, np.asarray(x).shape[0])
    return np.asarray(x)[y0, x0]


def warp_weight(tw, row, L):
    """One sample: tw fp32 [L, L] or None (ones: the in-frame mask) -> fp32 [L, L], nearest, 0.0 out of frame."""
    tw = np.ones((L, L), dtype=np.float32) if tw is None else np.asarray(tw, dtype=np.float32)
    return GR.warp_cells(tw, row, 0.0)


def scores_ref(scores, tw, rows, B, g, L=None):
    """Restatement of lc2is_geo_scores.  scores fp32 [B*g*g, ld]; tw fp32 [B, L, L] or None; rows int32 [B, 16]; L: the side of the
    weight map (None: no weight map).  Returns (float64 [B*g*g, ld], fp32 [B, L, L] or None); a copy row holds exactly its input."""
    scores = np.asarray(scores)
    rows = np.asarray(rows, dtype=np.int32)
    x = scores.reshape(B, g, g, -1)
    out = x.astype(np.float64)
    out_tw = None
    if L is not None:
        out_tw = np.ones((B, L, L), dtype=np.float32) if tw is None else np.array(tw, dtype=np.float32)
    for b in range(B):
        if not GR.row_is_mapped(rows[b]):
            continue
        out[b] = warp_scores(x[b], rows[b])
        if L is not None:
            out_tw[b] = warp_weight(None if tw is None else tw[b], rows[b], L)
    return out.reshape(scores.shape), out_tw
