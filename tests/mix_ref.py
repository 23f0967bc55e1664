"""Numpy restatement of the mixed-sample augmentation (include/lc2is_hip.h, lc2is_mix_select / lc2is_mix_apply), test-only: the plan
and info rows with uint32 / int64 integers, bit for bit what the kernels write, and the three selects.  Shared by
tests/test_mix_cpu.py and tests/test_gpu_mix.py; the RNG is tests/augment_ref.py's."""
import numpy as np

from augment_ref import sample_hash, u24

NONE, CLASSMIX, CUTMIX = 0, 1, 2
MODES = {"none": NONE, "classmix": CLASSMIX, "cutmix": CUTMIX}
MAX_CLASSES, P_WORDS, BITMAP, STREAM = 1024, 40, 8, np.uint32(0x4D495831)


def mix_hash(seed, epoch, keys):
    """The mixer's stream: the sample hash of the augmentation XOR a constant of its own."""
    return sample_hash(seed, epoch, keys) ^ STREAM


def present_classes(src_map, n_classes, ignore_index=-100, exclude_label=None):
    """The sorted class ids present in one source label map."""
    v = np.unique(np.asarray(src_map, dtype=np.int64))
    keep = (v >= 0) & (v < n_classes) & (v != ignore_index)
    if exclude_label is not None and exclude_label != -1:
        keep &= v != exclude_label
    return v[keep]


def chosen_classes(h, present):
    """The ceil(n / 2) present classes with the smallest (u24(h, 16 + c), c) pairs; h: one uint32 hash."""
    present = np.asarray(present, dtype=np.int64)
    if not present.size:
        return present
    draws = u24(np.uint32(h), (16 + present).astype(np.uint32))
    order = np.lexsort((present, draws))               # by draw, ties by class id
    return np.sort(present[order[:(present.size + 1) // 2]])


def cutmix_box(h, L, lo1024=256, hi1024=512):
    """(top, left, bh, bw, a) of one sample, Python integers only."""
    h = np.uint32(h)
    a = lo1024 + ((int(u24(h, 0)) * (hi1024 - lo1024 + 1)) >> 24)
    hmin = max(1, -(-a * L // 1024))
    bh = hmin + ((int(u24(h, 1)) * (L - hmin + 1)) >> 24)
    bw = min(max((2 * a * L * L + 1024 * bh) // (2 * 1024 * bh), 1), L)
    top = (int(u24(h, 2)) * (L - bh + 1)) >> 24
    left = (int(u24(h, 3)) * (L - bw + 1)) >> 24
    return top, left, bh, bw, a


def area1024(box_area):
    return tuple(int(round(float(v) * 1024)) for v in box_area)


def select_ref(src_lab, keys, epoch, mode, seed=0, n_classes=151, ignore_index=-100, exclude_label=None, box_area=(0.25, 0.5),
               src_index=None):
    """(plan int32 [B, 40], info int32 [B, 4], mask bool [B, L, L]) of lc2is_mix_select.  src_lab int64 [Bs, L, L]."""
    src_lab = np.asarray(src_lab, dtype=np.int64)
    Bs, L, _ = src_lab.shape
    keys = np.asarray(keys, dtype=np.int64)
    B = len(keys)
    src_index = np.arange(B) if src_index is None else np.asarray(src_index, dtype=np.int64)
    mode = MODES.get(mode, mode)
    lo, hi = area1024(box_area)
    plan, info, mask = np.zeros((B, P_WORDS), np.int32), np.zeros((B, 4), np.int32), np.zeros((B, L, L), bool)
    hs = mix_hash(seed, epoch, keys)
    for b in range(B):
        s = int(src_index[b])
        if not 0 <= s < Bs:
            info[b] = (-1, 0, 0, 0)
            continue
        plan[b, 0], plan[b, 1] = mode, s
        if mode == CUTMIX:
            top, left, bh, bw, _ = cutmix_box(hs[b], L, lo, hi)
            plan[b, 2:6] = (top, left, bh, bw)
            mask[b, top:top + bh, left:left + bw] = True
        elif mode == CLASSMIX:
            present = present_classes(src_lab[s], n_classes, ignore_index, exclude_label)
            chosen = chosen_classes(hs[b], present)
            plan[b, 6], plan[b, 7] = present.size, chosen.size
            words = np.zeros(MAX_CLASSES // 32, np.uint32)
            for c in chosen:
                words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
            plan[b, BITMAP:] = words.view(np.int32)
            mask[b] = np.isin(src_lab[s], chosen)
            info[b, :2] = (present.size, chosen.size)
        info[b, 2], info[b, 3] = mask[b].sum(), L * L
    return plan, info, mask


def apply_ref(dst, src, mask, src_index=None):
    """The three selects.  dst / src: (pixels fp32 [n,3,S,S], labels int64 [n,L,L], weights fp32 [n,L,L] or None); mask bool [B,L,L]
    (all False in a row whose source lies outside the batch).  Bit patterns are moved, never computed with."""
    dpx, dlab, dpw = dst
    spx, slab, spw = src
    B, S, L = dpx.shape[0], dpx.shape[2], dlab.shape[1]
    src_index = np.arange(B) if src_index is None else np.asarray(src_index, dtype=np.int64)
    rows = np.where((src_index >= 0) & (src_index < spx.shape[0]), src_index, 0)
    ones = lambda lab: np.ones(lab.shape, np.float32)
    dpw, spw = ones(dlab) if dpw is None else dpw, ones(slab) if spw is None else spw
    r = S // L
    big = np.repeat(np.repeat(mask, r, axis=1), r, axis=2)[:, None]                     # [B,1,S,S]
    px = np.where(big, spx[rows].view(np.uint32), dpx.view(np.uint32)).view(np.float32)
    return px, np.where(mask, slab[rows], dlab), np.where(mask, spw[rows].view(np.uint32), dpw.view(np.uint32)).view(np.float32)
