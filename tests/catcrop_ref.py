"""Numpy restatement of the class-ratio crop re-draw (include/lc2is_hip.h, lc2is_aug_crop_select), of the per-image label
histogram (lc2is_label_histogram) and of lc2is_amd.data.class_weights, test-only.  Integers only for the selection: bit for bit
what the kernel computes.  The candidates come from augment_ref's hash, and the cells that are counted are literally the labels
augment_ref.apply_ref writes, with -1 as the padding sentinel.  Shared by tests/test_catcrop_cpu.py and tests/test_gpu_catcrop.py."""
import numpy as np

import augment_ref as R

MAX_TRIES = 10


def make_label_map(H, W):
    """The test input of the issue: class 7 everywhere, 8 x 8 blocks of random classes 1..149 from column floor(0.55 W) on, class 0
    (the ignored one) in the rows above floor(H / 6)."""
    lab = np.full((H, W), 7, dtype=np.uint8)
    blocks = np.random.default_rng(5).integers(1, 150, (-(-H // 8), -(-W // 8)))
    full = np.kron(blocks, np.ones((8, 8), dtype=np.int64))[:H, :W]
    c0 = int(0.55 * W)
    lab[:, c0:] = full[:, c0:]
    lab[:H // 6] = 0
    return lab


def candidates(cfg, nh, nw, top0, left0, keys, epoch, tries=MAX_TRIES):
    """(top, left) int64 [n, tries + 1]: column 0 is the row's own draw, column t >= 1 uses draws 10 + 2t and 11 + 2t."""
    nh, nw = np.asarray(nh, dtype=np.int64), np.asarray(nw, dtype=np.int64)
    h = R.sample_hash(cfg["seed_lo"] | (cfg["seed_hi"] << 32), epoch, keys)
    S = cfg["crop_size"]
    top, left = [np.asarray(top0, dtype=np.int64)], [np.asarray(left0, dtype=np.int64)]
    for t in range(1, tries + 1):
        top.append((R.u24(h, 10 + 2 * t) * (np.maximum(nh - S, 0) + 1)) >> 24)
        left.append((R.u24(h, 11 + 2 * t) * (np.maximum(nw - S, 0) + 1)) >> 24)
    return np.stack(top, axis=1), np.stack(left, axis=1)


def label_tile(lab, nh, nw, top, left, flip, S, L):
    """The [L, L] labels aug_apply writes for this geometry, -1 where the cell is padding."""
    H, W = lab.shape
    img = np.zeros((H, W, 3), dtype=np.uint8)
    return R.apply_ref(img, lab, nh, nw, top, left, flip, np.eye(3), np.zeros(3), S, L, (0.0,) * 3, (1.0,) * 3, pad_label=-1)[1]


def cell_stats(tile, ignore_label):
    """(n, m, d) of a label tile: counted cells, the largest class count, the number of classes present."""
    v = tile[(tile >= 0) & (tile != ignore_label)]
    cnt = np.bincount(v, minlength=256)
    return int(cnt.sum()), int(cnt.max()), int((cnt > 0).sum())


def accepted(n, m, d, ratio1024):
    return d > 1 and m * 1024 < ratio1024 * n


def select_ref(labs, slots, rows, keys, epoch, cfg, L, ratio1024, ignore_label=-1, tries=MAX_TRIES):
    """labs: the pool's label maps; slots / keys: per sample; rows: int32 [B, 20] as aug_params writes them (every row valid).
    Returns (rows with top / left replaced, info int32 [B, 4] = t*, n, m, d)."""
    rows = np.asarray(rows, dtype=np.int32)
    out, info = rows.copy(), np.zeros((len(rows), 4), dtype=np.int32)
    S = cfg["crop_size"]
    top, left = candidates(cfg, rows[:, R.NH], rows[:, R.NW], rows[:, R.TOP], rows[:, R.LEFT], keys, epoch, tries)
    for b, slot in enumerate(slots):
        nh, nw, flip = int(rows[b, R.NH]), int(rows[b, R.NW]), int(rows[b, R.FLIP])
        pick, stats = tries, (0, 0, 0)
        for t in range(tries):
            n, m, d = cell_stats(label_tile(labs[slot], nh, nw, top[b, t], left[b, t], flip, S, L), ignore_label)
            if accepted(n, m, d, ratio1024):
                pick, stats = t, (n, m, d)
                break
        out[b, R.TOP], out[b, R.LEFT] = top[b, pick], left[b, pick]
        info[b] = (pick,) + stats
    return out, info


def class_counts_ref(labs):
    """int64 [n, 256]: pixels of every label value per image."""
    return np.stack([np.bincount(np.asarray(l, dtype=np.uint8).reshape(-1), minlength=256) for l in labs]).astype(np.int64)


def class_weights_ref(counts, n_classes=151, ignore_index=0, mode="median_freq"):
    """float64 [n_classes].  Valid classes: 0 .. n_classes - 1 without ignore_index; only their pixels count.
    median_freq (Eigen & Fergus): f_c = pixels of c / valid pixels of the images in which c occurs, w_c = median(f) / f_c, the
    median over the classes that occur (mean of the two middle values for an even number of them).
    enet (Paszke et al.): w_c = 1 / ln(1.02 + p_c), p_c = pixels of c / all valid pixels.  Weight 0 for a class that never occurs
    and for ignore_index."""
    c = np.asarray(counts, dtype=np.int64)[:, :n_classes].copy()
    if ignore_index is not None and 0 <= ignore_index < n_classes:
        c[:, ignore_index] = 0
    pix = c.sum(axis=0)
    occurs = pix > 0
    w = np.zeros(n_classes, dtype=np.float64)
    if not occurs.any():
        return w
    if mode == "median_freq":
        per_image = c.sum(axis=1)
        total = ((c > 0) * per_image[:, None]).sum(axis=0)
        f = pix[occurs].astype(np.float64) / total[occurs].astype(np.float64)
        s = np.sort(f)
        k = len(s)
        w[occurs] = 0.5 * (s[(k - 1) // 2] + s[k // 2]) / f
    elif mode == "enet":
        p = pix[occurs].astype(np.float64) / np.float64(pix.sum())
        w[occurs] = 1.0 / np.log(1.02 + p)
    else:
        raise ValueError(mode)
    return w
