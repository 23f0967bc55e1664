"""Numpy restatement of the device augmentation (include/lc2is_hip.h, lc2is_aug_params / lc2is_aug_apply), test-only: the
parameter draw with uint32 / int64 integers (bit for bit what the kernel computes) and float64 colour fields, and the apply
definition in float64.  Shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py, like golden_util.py."""
import numpy as np

GOLD = np.uint32(0x9E3779B9)
MAX_RESIZED = 262143
P_WORDS, NH, NW, TOP, LEFT, FLIP, M0, O0 = 20, 0, 1, 2, 3, 4, 5, 14


def mix32(x):
    """lowbias32 (lc2is_amd/csrc/common.h mix32) on uint32 arrays, wrap-around arithmetic."""
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def sample_hash(seed, epoch, keys):
    keys = np.asarray(keys, dtype=np.int64).astype(np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = np.uint32(seed & 0xffffffff), np.uint32(seed >> 32)
    epoch = (np.asarray(epoch, dtype=np.int64) & 0xffffffff).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = mix32((keys & np.uint64(0xffffffff)).astype(np.uint32) + lo)
        h = mix32(h ^ ((keys >> np.uint64(32)).astype(np.uint32) + hi))
        return mix32(h ^ (epoch * GOLD + np.uint32(0x85EBCA6B)))


def u24(h, k):
    with np.errstate(over="ignore"):
        return (mix32(h + np.uint32(k) * GOLD) >> np.uint32(8)).astype(np.int64)


def config_dict(cfg):
    """The fields of an ops.AugConfig as Python numbers (floats are the struct's fp32 values)."""
    d = {name: getattr(cfg, name) for name, _ in cfg._fields_ if name != "photo_thr"}
    d["photo_thr"] = [int(v) for v in cfg.photo_thr]
    return d


def draw_params(cfg, H, W, keys, epoch):
    """cfg: config_dict(...); H, W, keys, epoch: equal-length arrays (epoch may be a scalar).  Returns a dict of int64 arrays
    nh, nw, top, left, flip and float64 M [n,3,3], o [n,3]."""
    H, W = np.asarray(H, dtype=np.int64), np.asarray(W, dtype=np.int64)
    h = sample_hash(cfg["seed_lo"] | (cfg["seed_hi"] << 32), epoch, keys)
    S = cfg["crop_size"]
    r = cfg["ratio_lo1024"] + ((u24(h, 0) * (cfg["ratio_hi1024"] - cfg["ratio_lo1024"] + 1)) >> 24)
    t = (cfg["base_size"] * r + 512) >> 10
    s = np.minimum(H, W)
    nh = np.clip((2 * H * t + s) // (2 * s), 1, MAX_RESIZED)
    nw = np.clip((2 * W * t + s) // (2 * s), 1, MAX_RESIZED)
    top = (u24(h, 1) * (np.maximum(nh - S, 0) + 1)) >> 24
    left = (u24(h, 2) * (np.maximum(nw - S, 0) + 1)) >> 24
    flip = (u24(h, 3) < cfg["flip_thr"]).astype(np.int64)
    n = len(H)
    M = np.tile(np.eye(3), (n, 1, 1))
    o = np.zeros((n, 3))

    def uniform(k, lo, hi):
        return lo + (hi - lo) * (u24(h, k) / 16777216.0)

    def left_mul(A, on):
        M[on] = A[on] @ M[on]
        o[on] = np.einsum("nij,nj->ni", A[on], o[on])

    on = u24(h, 4) < cfg["photo_thr"][0]
    o[on] += uniform(5, -cfg["brightness_delta"], cfg["brightness_delta"])[on, None]
    on = u24(h, 6) < cfg["photo_thr"][1]
    c = uniform(7, cfg["contrast_lo"], cfg["contrast_hi"])
    M[on] *= c[on, None, None]
    o[on] *= c[on, None]
    left_mul(saturation_matrix(uniform(9, cfg["saturation_lo"], cfg["saturation_hi"])), u24(h, 8) < cfg["photo_thr"][2])
    left_mul(hue_matrix(uniform(11, -cfg["hue_delta"], cfg["hue_delta"])), u24(h, 10) < cfg["photo_thr"][3])
    return dict(nh=nh, nw=nw, top=top, left=left, flip=flip, M=M, o=o, ratio1024=r)


def saturation_matrix(s):
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    w = np.array([0.299, 0.587, 0.114])
    return s[:, None, None] * np.eye(3) + (1 - s)[:, None, None] * np.tile(w, (3, 1))


def hue_matrix(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    cs, sn = np.cos(a)[:, None, None], np.sin(a)[:, None, None]
    K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    return cs * np.eye(3) + (1 - cs) / 3.0 * np.ones((3, 3)) + sn / np.sqrt(3.0) * K


def param_rows(p):
    """The int32 [n, 20] table the kernel writes for draw_params' result (colour fields rounded to fp32)."""
    n = len(p["nh"])
    rows = np.zeros((n, P_WORDS), dtype=np.int32)
    for k, name in ((NH, "nh"), (NW, "nw"), (TOP, "top"), (LEFT, "left"), (FLIP, "flip")):
        rows[:, k] = p[name]
    rows[:, M0:M0 + 9] = p["M"].reshape(n, 9).astype(np.float32).view(np.int32)
    rows[:, O0:O0 + 3] = p["o"].astype(np.float32).view(np.int32)
    return rows


def apply_ref(img, lab, nh, nw, top, left, flip, M, o, S, L, mean, std, pad_label=0):
    """float64 restatement of lc2is_aug_apply for one sample: img uint8 [H,W,3], lab uint8 [H,W]; M [3,3], o [3] as the kernel reads
    them (fp32 values).  Returns (pixel_values float64 [3,S,S], label int64 [L,L])."""
    H, W = lab.shape
    nh, nw, top, left = int(nh), int(nw), int(top), int(left)
    i = np.arange(S, dtype=np.int64)
    yr = top + i
    xr = left + (S - 1 - i if flip else i)
    in_y, in_x = (yr >= 0) & (yr < nh), (xr >= 0) & (xr < nw)

    def taps(r, n_in, n_out):
        r = np.clip(r, 0, n_out - 1)
        num = np.clip((2 * r + 1) * n_in - n_out, 0, 2 * n_out * (n_in - 1))
        i0 = num // (2 * n_out)
        return i0, np.minimum(i0 + 1, n_in - 1), (num - i0 * 2 * n_out) / float(2 * n_out)

    y0, y1, fy = taps(yr, H, nh)
    x0, x1, fx = taps(xr, W, nw)
    px = img.astype(np.float64)
    fx_, fy_ = fx[None, :, None], fy[:, None, None]
    h0 = px[y0][:, x0] + fx_ * (px[y0][:, x1] - px[y0][:, x0])
    h1 = px[y1][:, x0] + fx_ * (px[y1][:, x1] - px[y1][:, x0])
    a = h0 + fy_ * (h1 - h0)                                                   # [S,S,3]
    v = np.clip(a @ np.asarray(M, dtype=np.float64).T + np.asarray(o, dtype=np.float64), 0.0, 255.0)
    out = (v * (1.0 / 255.0) - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    out = np.where((in_y[:, None] & in_x[None, :])[:, :, None], out, 0.0).transpose(2, 0, 1)
    q = S // L
    c = np.arange(L, dtype=np.int64) * q + q // 2
    ys = ((2 * np.clip(yr[c], 0, nh - 1) + 1) * H) // (2 * nh)
    xs = ((2 * np.clip(xr[c], 0, nw - 1) + 1) * W) // (2 * nw)
    labels = np.where(in_y[c][:, None] & in_x[c][None, :], lab[ys][:, xs].astype(np.int64), np.int64(pad_label))
    return out, labels
