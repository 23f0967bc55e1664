"""Numpy restatement of the geometric views (include/lc2is_hip.h, lc2is_geo_params / lc2is_geo_apply), test-only, written from the
header: the draws with uint32 / int64 integers (switches bit for bit; the five fp32 values as the one-rounding numbers the header
defines, so tx, ty are exact), the matrix in float64, and the apply definition with int64 indices and a float64 blend.  Shared by
tests/test_geo_cpu.py and tests/test_gpu_geo.py; the RNG is tests/augment_ref.py's."""
import numpy as np

from augment_ref import sample_hash, u24

STREAM = np.uint32(0x47454F31)
P_WORDS, FLAGS, M0, T0, REC0 = 16, 0, 1, 5, 7
WARP, FLIP = 1, 2
ONE, MAX_M, MAX_T = 65536, 8 * 65536, 65536
REC_NAMES = ("theta", "s", "phi", "fx", "fy")


def geo_hash(seed, epoch, keys):
    """The geometric view's stream: the sample hash of the augmentation XOR a constant of its own."""
    return sample_hash(seed, epoch, keys) ^ STREAM


def config_dict(cfg):
    """The fields of an ops.GeoConfig as Python numbers (floats are the struct's fp32 values)."""
    d = {name: getattr(cfg, name) for name, _ in cfg._fields_ if name != "fill"}
    d["fill"] = [float(v) for v in cfg.fill]
    return d


def draw_range(t24, lo, hi):
    """fma(hi - lo, t, lo) in fp32, t = u24 * 2^-24: the difference is rounded to fp32; the product of two fp32 numbers and its sum
    with lo are exact in float64 for the symmetric ranges [-a, a] (hi - lo = 2a: at most 49 significant bits apart), so theta, phi,
    fx and fy are the kernel's numbers and the one rounding is the cast; s, whose range may be narrow next to its lo, can be off by
    an ulp through a double rounding and is only held to a tolerance."""
    lo, hi = np.float32(lo), np.float32(hi)
    span = np.float64(np.float32(hi - lo))
    return (span * (np.asarray(t24, dtype=np.float64) / 16777216.0) + np.float64(lo)).astype(np.float32)


def draw_params(cfg, keys, epoch):
    """cfg: config_dict(...).  Returns int64 arrays warp, flip, flags, tx, ty; fp32 theta, s, phi, fx, fy; float64 M [n,2,2] (times
    65536, before rounding, the flip applied) and int64 m [n,4] = rint(M)."""
    h = geo_hash(cfg["seed_lo"] | (cfg["seed_hi"] << 32), epoch, keys)
    n = len(h)
    warp, flip = u24(h, 0) < cfg["warp_thr"], u24(h, 6) < cfg["flip_thr"]
    theta = draw_range(u24(h, 1), -np.float32(cfg["rotate"]), cfg["rotate"])
    s = draw_range(u24(h, 2), cfg["scale_lo"], cfg["scale_hi"])
    phi = draw_range(u24(h, 3), -np.float32(cfg["shear"]), cfg["shear"])
    fx = draw_range(u24(h, 4), -np.float32(cfg["translate"]), cfg["translate"])
    fy = draw_range(u24(h, 5), -np.float32(cfg["translate"]), cfg["translate"])
    th, sc, ph = theta.astype(np.float64), s.astype(np.float64), phi.astype(np.float64)
    cs, sn, tn = np.cos(th), np.sin(th), np.tan(ph)
    M = np.stack([cs, cs * tn - sn, sn, sn * tn + cs], axis=1) / sc[:, None] * ONE       # (1/s) R(theta) H(phi)
    M = np.where(warp[:, None], M, np.array([ONE, 0.0, 0.0, ONE])[None])
    M[flip, 0] *= -1.0
    M[flip, 2] *= -1.0
    # fx * 65536 is exact in fp32 (a power of two), rintf rounds half to even as np.rint does
    tx = np.where(warp, np.rint(fx.astype(np.float64) * ONE), 0.0).astype(np.int64)
    ty = np.where(warp, np.rint(fy.astype(np.float64) * ONE), 0.0).astype(np.int64)
    flags = np.where(warp, WARP, 0) | np.where(flip, FLIP, 0)
    return dict(warp=warp.astype(np.int64), flip=flip.astype(np.int64), flags=flags.astype(np.int64), tx=tx, ty=ty, theta=theta, s=s,
                phi=phi, fx=fx, fy=fy, M=M.reshape(n, 2, 2), m=np.rint(M).astype(np.int64))


def param_rows(p):
    """The int32 [n, 16] table the kernel writes for draw_params' result (m rounded from the float64 matrix)."""
    n = len(p["flags"])
    rows = np.zeros((n, P_WORDS), dtype=np.int32)
    rows[:, FLAGS] = p["flags"]
    rows[:, M0:M0 + 4] = p["m"]
    rows[:, T0], rows[:, T0 + 1] = p["tx"], p["ty"]
    for j, name in enumerate(REC_NAMES):
        rows[:, REC0 + j] = np.asarray(p[name], dtype=np.float32).view(np.int32)
    return rows


def make_row(flags, m=(ONE, 0, 0, ONE), t=(0, 0), rec=(0.0, 1.0, 0.0, 0.0, 0.0)):
    """One hand-written int32 row."""
    row = np.zeros(P_WORDS, dtype=np.int32)
    row[FLAGS] = flags
    row[M0:M0 + 4] = np.asarray(m, dtype=np.int64)
    row[T0:T0 + 2] = np.asarray(t, dtype=np.int64)
    row[REC0:REC0 + 5] = np.asarray(rec, dtype=np.float32).view(np.int32)
    return row


def affine_row(theta_deg=0.0, s=1.0, phi_deg=0.0, fx=0.0, fy=0.0, flip=False):
    """The row lc2is_geo_params would write for these values (float64 matrix, rounded once)."""
    th, ph = np.radians(theta_deg), np.radians(phi_deg)
    cs, sn, tn = np.cos(th), np.sin(th), np.tan(ph)
    m = np.rint(np.array([cs, cs * tn - sn, sn, sn * tn + cs]) / s * ONE).astype(np.int64)
    if flip:
        m[0], m[2] = -m[0], -m[2]
    return make_row(WARP | (FLIP if flip else 0), m, (int(np.rint(fx * ONE)), int(np.rint(fy * ONE))), (th, s, ph, fx, fy))


def row_is_mapped(row):
    """False: lc2is_geo_apply renders the row as the copy."""
    row = np.asarray(row, dtype=np.int64)
    return bool(row[FLAGS] != 0 and not row[FLAGS] & ~(WARP | FLIP) and (np.abs(row[M0:M0 + 4]) <= MAX_M).all()
                and (np.abs(row[T0:T0 + 2]) <= MAX_T).all())


def source_uv(row, n):
    """U, V int64 [n, n] of the header for a map of side n (python integers would do; |U| < 2^36)."""
    m00, m01, m10, m11, tx, ty = (int(v) for v in np.asarray(row, dtype=np.int64)[M0:M0 + 6])
    c = 2 * np.arange(n, dtype=np.int64) + 1 - n
    u, v = c[None, :], c[:, None]
    return m00 * u + m01 * v + 2 * tx * n, m10 * u + m11 * v + 2 * ty * n


def theta_of(row):
    """The 2 x 3 matrix F.affine_grid takes for this row (float64)."""
    m00, m01, m10, m11, tx, ty = (float(v) for v in np.asarray(row, dtype=np.int64)[M0:M0 + 6])
    return np.array([[m00, m01, 2 * tx], [m10, m11, 2 * ty]]) / ONE


def warp_pixels(x, row, fill):
    """One sample: x [3, S, S] (any float dtype) -> float64 [3, S, S]; integer indices and fractions, the blend in float64, the near tap
    selected where a fraction is 0.  NaN / inf in a tap that is not selected does not reach the output."""
    x = np.asarray(x)
    S = x.shape[-1]
    U, V = source_uv(row, S)
    X, Y = U + (S - 1) * ONE, V + (S - 1) * ONE
    x0, y0 = X >> 17, Y >> 17
    fxi, fyi = X & 0x1FFFF, Y & 0x1FFFF
    fx, fy = fxi / 131072.0, fyi / 131072.0
    out = np.empty((3, S, S), dtype=np.float64)
    for c in range(3):
        p = x[c].astype(np.float64)

        def tap(yy, xx):
            ok = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
            return np.where(ok, p[np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)], float(fill[c]))

        p00, p01, p10, p11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        with np.errstate(invalid="ignore", over="ignore"):
            top = np.where(fxi != 0, p00 + fx * (p01 - p00), p00)
            bot = np.where(fxi != 0, p10 + fx * (p11 - p10), p10)
            out[c] = np.where(fyi != 0, top + fy * (bot - top), top)
    return out


def cell_index(row, L):
    """(ys, xs, inside) int64 / bool [L, L]: the source cell of every output cell."""
    U, V = source_uv(row, L)
    xs, ys = (U + L * ONE) >> 17, (V + L * ONE) >> 17
    return ys, xs, (xs >= 0) & (xs < L) & (ys >= 0) & (ys < L)


def warp_cells(m, row, outside):
    """One sample: a map [L, L] of any dtype -> the same dtype, nearest, `outside` out of frame."""
    m = np.asarray(m)
    L = m.shape[-1]
    ys, xs, inside = cell_index(row, L)
    return np.where(inside, m[np.clip(ys, 0, L - 1), np.clip(xs, 0, L - 1)], np.asarray(outside, dtype=m.dtype))


TILE, BOX_WORDS = 32, 4096


def tile_box(row, S, ty, tx):
    """(w, h, bx, by) of the source box geo_apply_kernel forms for output tile (ty, tx) of a mapped row, as include/lc2is_hip.h says: the near
    taps of the tile's four corners, + 1 for the far taps, clipped to the image, the width in whole quads from bx = xlo & ~3; (4, 0, 0, 0) when the tile
    looks outside the image altogether.  The block stages the box when w * h <= BOX_WORDS and gathers directly otherwise."""
    m00, m01, m10, m11, t_x, t_y = (int(v) for v in np.asarray(row, dtype=np.int64)[M0:M0 + 6])
    x0, y0 = tx * TILE, ty * TILE
    xe, ye = min(x0 + TILE, S) - 1, min(y0 + TILE, S) - 1
    xs, ys = [], []
    for cx in (x0, xe):
        for cy in (y0, ye):
            u, v = 2 * cx + 1 - S, 2 * cy + 1 - S
            xs.append((m00 * u + m01 * v + 2 * t_x * S + (S - 1) * ONE) >> 17)
            ys.append((m10 * u + m11 * v + 2 * t_y * S + (S - 1) * ONE) >> 17)
    xlo, xhi, ylo, yhi = max(min(xs), 0), min(max(xs) + 1, S - 1), max(min(ys), 0), min(max(ys) + 1, S - 1)
    if xlo > xhi or ylo > yhi:
        return 4, 0, 0, 0
    bx = xlo & ~3
    return (xhi - bx + 1 + 3) & ~3, yhi - ylo + 1, bx, ylo


def direct_tiles(row, S):
    """The output tiles of a mapped row whose box does not fit and which therefore take the direct form."""
    n = (S + TILE - 1) // TILE
    return [(ty, tx) for ty in range(n) for tx in range(n) if np.prod(tile_box(row, S, ty, tx)[:2]) > BOX_WORDS]


def apply_ref(px, lab, pw, rows, fill, ignore_index):
    """Restatement of lc2is_geo_apply.  px fp32 [B,3,S,S]; lab int64 [B,L,L] or None; pw fp32 [B,L,L] or None; rows int32 [B,16].
    Returns (float64 [B,3,S,S], int64 or None, fp32 or None); a sample that is copied holds exactly the fp32 input values."""
    px = np.asarray(px)
    rows = np.asarray(rows, dtype=np.int32)
    out_px = px.astype(np.float64)
    out_lab = None if lab is None else np.array(lab, dtype=np.int64)
    out_pw = None if pw is None else np.array(pw, dtype=np.float32)
    for b in range(px.shape[0]):
        if not row_is_mapped(rows[b]):
            continue
        out_px[b] = warp_pixels(px[b], rows[b], fill)
        if lab is not None:
            out_lab[b] = warp_cells(lab[b], rows[b], ignore_index)
        if pw is not None:
            out_pw[b] = warp_cells(pw[b], rows[b], 0.0)
    return out_px, out_lab, out_pw
