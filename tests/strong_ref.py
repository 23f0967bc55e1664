"""Numpy restatement of the strong photometric views (include/lc2is_hip.h, lc2is_strong_params / lc2is_strong_apply), test-only,
written from the header: the draws with uint32 / int64 integers (switches and R bit for bit what the kernel computes; sigma as the
one-rounding fp32 number the header defines), the (M, o) composition and the taps in float64, and the apply definition in float64.
Shared by tests/test_strong_cpu.py and tests/test_gpu_strong.py; the RNG and the matrix builders are tests/augment_ref.py's."""
import numpy as np

from augment_ref import hue_matrix, sample_hash, saturation_matrix, u24

STREAM = np.uint32(0x53545231)
MAX_RADIUS, P_WORDS = 8, 32
FLAGS, R_WORD, SIGMA, M0, O0, W0 = 0, 1, 2, 3, 12, 15
COLOUR, GREY, BLUR = 1, 2, 4
GREY_W = np.array([0.299, 0.587, 0.114])


def strong_hash(seed, epoch, keys):
    """The strong view's stream: the sample hash of the augmentation XOR a constant of its own."""
    return sample_hash(seed, epoch, keys) ^ STREAM


def config_dict(cfg):
    """The fields of an ops.StrongConfig as Python numbers (floats are the struct's fp32 values)."""
    d = {name: getattr(cfg, name) for name, _ in cfg._fields_ if name not in ("mean", "std", "inv_std")}
    for name in ("mean", "std", "inv_std"):
        d[name] = [float(v) for v in getattr(cfg, name)]
    return d


def radius(sigma):
    """R = min(8, ceil(4 sigma)); 4 * sigma is exact for an fp32 sigma."""
    return np.minimum(MAX_RADIUS, np.ceil(4.0 * np.asarray(sigma, dtype=np.float64))).astype(np.int64)


def taps(sigma, R):
    """w[0 .. 8] in float64: exp(-k^2 / (2 sigma^2)) for k <= R, normalised so that w_0 + 2 sum_{k >= 1} w_k = 1; 0 past R."""
    k = np.arange(MAX_RADIUS + 1, dtype=np.float64)
    w = np.where(k <= R, np.exp(-k * k / (2.0 * float(sigma) ** 2)), 0.0)
    return w / (w[0] + 2.0 * w[1:].sum())


def draw_sigma(cfg, t):
    """fma(sigma_hi - sigma_lo, t, sigma_lo) in fp32: the difference is rounded to fp32, the product of two fp32 numbers and its sum
    with sigma_lo are exact in float64 here (at most 49 significant bits apart), and the one rounding is the cast."""
    span = np.float32(cfg["sigma_hi"]) - np.float32(cfg["sigma_lo"])
    return (np.float64(span) * np.asarray(t, dtype=np.float64) + np.float64(np.float32(cfg["sigma_lo"]))).astype(np.float32)


def draw_params(cfg, keys, epoch):
    """cfg: config_dict(...).  Returns int64 arrays jitter, grey, blur, flags, R, fp32 sigma and float64 M [n,3,3], o [n,3], w [n,9]."""
    h = strong_hash(cfg["seed_lo"] | (cfg["seed_hi"] << 32), epoch, keys)
    n = len(h)

    def uniform(k, lo, hi):
        return lo + (hi - lo) * (u24(h, k) / 16777216.0)

    jitter, grey, blur = u24(h, 0) < cfg["jitter_thr"], u24(h, 5) < cfg["gray_thr"], u24(h, 6) < cfg["blur_thr"]
    M = np.tile(np.eye(3), (n, 1, 1))
    o = np.zeros((n, 3))

    def left_mul(A, on):
        M[on] = A[on] @ M[on]
        o[on] = np.einsum("nij,nj->ni", A[on], o[on])

    o[jitter] += uniform(1, -cfg["brightness_delta"], cfg["brightness_delta"])[jitter, None]
    c = uniform(2, cfg["contrast_lo"], cfg["contrast_hi"])
    M[jitter] *= c[jitter, None, None]
    o[jitter] *= c[jitter, None]
    left_mul(saturation_matrix(uniform(3, cfg["saturation_lo"], cfg["saturation_hi"])), jitter)
    left_mul(hue_matrix(uniform(4, -cfg["hue_delta"], cfg["hue_delta"])), jitter)
    left_mul(np.tile(np.tile(GREY_W, (3, 1)), (n, 1, 1)), grey)
    sigma = draw_sigma(cfg, u24(h, 7) / 16777216.0)
    R = radius(sigma)
    w = np.stack([taps(s, r) for s, r in zip(sigma, R)]) if n else np.zeros((0, MAX_RADIUS + 1))
    flags = np.where(jitter | grey, COLOUR, 0) | np.where(grey, GREY, 0) | np.where(blur, BLUR, 0)
    return dict(jitter=jitter.astype(np.int64), grey=grey.astype(np.int64), blur=blur.astype(np.int64), flags=flags.astype(np.int64),
                R=R, sigma=sigma, M=M, o=o, w=w)


def param_rows(p):
    """The int32 [n, 32] table the kernel writes for draw_params' result (fp32 fields rounded from the float64 values)."""
    n = len(p["R"])
    rows = np.zeros((n, P_WORDS), dtype=np.int32)
    rows[:, FLAGS], rows[:, R_WORD] = p["flags"], p["R"]
    rows[:, SIGMA] = np.asarray(p["sigma"], dtype=np.float32).view(np.int32)
    rows[:, M0:M0 + 9] = p["M"].reshape(n, 9).astype(np.float32).view(np.int32)
    rows[:, O0:O0 + 3] = p["o"].astype(np.float32).view(np.int32)
    rows[:, W0:W0 + 9] = p["w"].astype(np.float32).view(np.int32)
    return rows


def make_row(flags, R=0, sigma=1.0, M=None, o=None, w=None):
    """One hand-written int32 row."""
    p = dict(flags=np.array([flags]), R=np.array([R]), sigma=np.array([sigma], np.float32),
             M=np.asarray(np.eye(3) if M is None else M, dtype=np.float64).reshape(1, 3, 3),
             o=np.asarray(np.zeros(3) if o is None else o, dtype=np.float64).reshape(1, 3),
             w=np.asarray(taps(sigma, R) if w is None else w, dtype=np.float64).reshape(1, 9))
    return param_rows(p)[0]


def reflect(i, S):
    """torch's "reflect": -i for i < 0, 2 (S - 1) - i for i >= S."""
    i = np.asarray(i, dtype=np.int64)
    i = np.where(i < 0, -i, i)
    return np.where(i >= S, 2 * (S - 1) - i, i)


def blur_ref(v, w, R):
    """float64 separable blur of v [..., S, S] with taps w[0 .. R], rows (along x) first, then columns, borders reflected."""
    v = np.asarray(v, dtype=np.float64)
    S = v.shape[-1]
    idx = np.arange(S)
    t = w[0] * v
    for k in range(1, int(R) + 1):
        t = t + w[k] * (v[..., :, reflect(idx - k, S)] + v[..., :, reflect(idx + k, S)])
    u = w[0] * t
    for k in range(1, int(R) + 1):
        u = u + w[k] * (t[..., reflect(idx - k, S), :] + t[..., reflect(idx + k, S), :])
    return u


def apply_ref(x, rows, mean, std, inv_std=None):
    """float64 restatement of lc2is_strong_apply: x fp32 [B,3,S,S]; rows int32 [B,32] as the kernel reads them (fp32 fields).  Returns
    float64 [B,3,S,S]; a sample that is copied holds exactly the fp32 input values (compare those bit for bit through fp32)."""
    x = np.asarray(x)
    rows = np.asarray(rows, dtype=np.int32)
    mean, std = np.asarray(mean, dtype=np.float64)[:, None, None], np.asarray(std, dtype=np.float64)[:, None, None]
    inv_std = 1.0 / std if inv_std is None else np.asarray(inv_std, dtype=np.float64)[:, None, None]
    out = x.astype(np.float64)
    for b in range(x.shape[0]):
        flags, R = int(rows[b, FLAGS]), int(rows[b, R_WORD])
        if flags & ~(COLOUR | GREY | BLUR) or not 0 <= R <= MAX_RADIUS or not flags & (COLOUR | BLUR):
            continue
        f = rows[b].view(np.float32).astype(np.float64)
        v = x[b].astype(np.float64)
        if flags & COLOUR:
            v = 255.0 * (v * std + mean)
            v = np.einsum("ij,jyx->iyx", f[M0:M0 + 9].reshape(3, 3), v) + f[O0:O0 + 3][:, None, None]
            v = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0))
        if flags & BLUR:
            v = blur_ref(v, f[W0:W0 + 9], R)
        if flags & COLOUR:
            v = (v * (1.0 / 255.0) - mean) * inv_std
        out[b] = v
    return out
