"""CPU checks of the class-ratio crop re-draw (lc2is_aug_crop_select) and of the class statistics: the numpy restatement
(tests/catcrop_ref.py) against a brute-force count written from the definition in include/lc2is_hip.h, the candidate draws, the
argument checks of TrainAugment, class_weights against a hand-computed case, and the bindings of the two new entry points."""
import re
from pathlib import Path

import numpy as np
import pytest

import augment_ref as R
import catcrop_ref as CR

ROOT = Path(__file__).resolve().parent.parent
SEED, BASE, EPOCH, RATIO1024, IGNORE = 1234, 64, 3, 768, 0
KEYS = np.arange(64)


def _cfg(S, L):
    from lc2is_amd.data import TrainAugment
    return R.config_dict(TrainAugment(crop_size=S, label_size=L, base_size=BASE, seed=SEED).config)


def _drawn(cfg, H, W):
    return R.draw_params(cfg, np.full(len(KEYS), H), np.full(len(KEYS), W), KEYS, EPOCH)


def _brute_stats(lab, nh, nw, top, left, flip, S, L, ignore_label):
    """(n, m, d) cell by cell from the definition: cell (i, j) looks at output pixel (i*q + q/2, j*q + q/2); yr = top + that row,
    xr = left + (flip ? S-1-column : column); outside [0, nh) x [0, nw): padding; ys = ((2 yr + 1) H) / (2 nh), xs likewise."""
    H, W = lab.shape
    q = S // L
    cnt = {}
    for ci in range(L):
        for cj in range(L):
            i, j = ci * q + q // 2, cj * q + q // 2
            yr, xr = top + i, left + (S - 1 - j if flip else j)
            if not (0 <= yr < nh and 0 <= xr < nw):
                continue
            v = int(lab[((2 * yr + 1) * H) // (2 * nh), ((2 * xr + 1) * W) // (2 * nw)])
            if v != ignore_label:
                cnt[v] = cnt.get(v, 0) + 1
    return sum(cnt.values()), max(cnt.values(), default=0), len(cnt)


@pytest.mark.parametrize("H,W", [(96, 160), (75, 131)])
def test_restatement_counts_what_apply_writes(H, W):
    """(S, L) = (32, 8), q = 4: for every sample and every candidate 0..10, flipped and unflipped, the restatement's (n, m, d) -
    a bincount over apply_ref's label tile - equals the cell-by-cell count from the definition, and a count over the tile's
    entries one by one.  The flip is part of the definition: at even q the mirrored cell centres fall on other columns, and for
    at least one candidate the verdict differs between the flipped and the unflipped crop."""
    S, L = 32, 8
    cfg, lab = _cfg(S, L), CR.make_label_map(H, W)
    p = _drawn(cfg, H, W)
    top, left = CR.candidates(cfg, p["nh"], p["nw"], p["top"], p["left"], KEYS, EPOCH)
    differ = 0
    for b in range(len(KEYS)):
        nh, nw = int(p["nh"][b]), int(p["nw"][b])
        for t in range(CR.MAX_TRIES + 1):
            verdicts = []
            for flip in (0, 1):
                tile = CR.label_tile(lab, nh, nw, top[b, t], left[b, t], flip, S, L)
                got = CR.cell_stats(tile, IGNORE)
                assert got == _brute_stats(lab, nh, nw, int(top[b, t]), int(left[b, t]), flip, S, L, IGNORE), (b, t, flip)
                one_by_one = {}
                for v in tile.reshape(-1).tolist():
                    if v >= 0 and v != IGNORE:
                        one_by_one[v] = one_by_one.get(v, 0) + 1
                assert got == (sum(one_by_one.values()), max(one_by_one.values(), default=0), len(one_by_one))
                verdicts.append(CR.accepted(*got, RATIO1024))
            differ += verdicts[0] != verdicts[1]
    assert differ >= 1


@pytest.mark.parametrize("S,L", [(32, 8), (64, 64)])
def test_candidate_zero_is_the_drawn_origin_and_selection_is_ordered(S, L):
    """Candidate 0 is draw_params' top / left; the later candidates use draws 12..31 (they differ from draws 1, 2 and lie in the
    free range); select_ref takes the first accepted candidate and leaves every other word of the row alone.  The spread of t*
    over the batch is the one the GPU test relies on: t* = 0, 1 <= t* <= 9 and (constant map) t* = tries all occur."""
    cfg = _cfg(S, L)
    for H, W in ((96, 160), (75, 131)):
        lab = CR.make_label_map(H, W)
        p = _drawn(cfg, H, W)
        rows = R.param_rows(p)
        top, left = CR.candidates(cfg, p["nh"], p["nw"], p["top"], p["left"], KEYS, EPOCH)
        assert np.array_equal(top[:, 0], p["top"]) and np.array_equal(left[:, 0], p["left"])
        assert (top >= 0).all() and (top <= np.maximum(p["nh"] - S, 0)[:, None]).all()
        assert (left >= 0).all() and (left <= np.maximum(p["nw"] - S, 0)[:, None]).all()
        free = p["nw"] - S > 8
        assert any((left[free, t] != left[free, 0]).any() for t in range(1, 11))
        out, info = CR.select_ref([lab], [0] * 64, rows, KEYS, EPOCH, cfg, L, RATIO1024, IGNORE)
        keep = [k for k in range(R.P_WORDS) if k not in (R.TOP, R.LEFT)]
        assert np.array_equal(out[:, keep], rows[:, keep])
        for b in range(64):
            t = info[b, 0]
            assert (out[b, R.TOP], out[b, R.LEFT]) == (top[b, t], left[b, t])
            for u in range(t):      # every earlier candidate was rejected
                st = CR.cell_stats(CR.label_tile(lab, p["nh"][b], p["nw"][b], top[b, u], left[b, u], p["flip"][b], S, L), IGNORE)
                assert not CR.accepted(*st, RATIO1024)
            if t < 10:
                assert info[b, 3] > 1 and info[b, 2] * 1024 < RATIO1024 * info[b, 1]
        hist = np.bincount(info[:, 0], minlength=11)
        assert hist[0] >= 20 and hist[1:10].sum() >= 10, hist
        assert np.array_equal(out[info[:, 0] == 0], rows[info[:, 0] == 0])
    const = np.full((40, 50), 9, dtype=np.uint8)
    p = _drawn(cfg, 40, 50)
    out, info = CR.select_ref([const], [0] * 64, R.param_rows(p), KEYS, EPOCH, cfg, L, RATIO1024, IGNORE)
    top, left = CR.candidates(cfg, p["nh"], p["nw"], p["top"], p["left"], KEYS, EPOCH)
    assert (info == np.array([10, 0, 0, 0])).all()
    assert np.array_equal(out[:, R.TOP], top[:, 10]) and np.array_equal(out[:, R.LEFT], left[:, 10])
    out3, info3 = CR.select_ref([const], [0] * 64, R.param_rows(p), KEYS, EPOCH, cfg, L, RATIO1024, IGNORE, tries=3)
    assert (info3[:, 0] == 3).all() and np.array_equal(out3[:, R.TOP], top[:, 3])


def test_train_augment_argument_errors():
    from lc2is_amd.data import TrainAugment
    for bad in (0.0, 1.0, -0.5, 1.5, 0.0001, 0.9999):
        with pytest.raises(ValueError, match="cat_max_ratio"):
            TrainAugment(cat_max_ratio=bad)
    for bad in (-1, 256, 1000):
        with pytest.raises(ValueError, match="cat_ignore_label"):
            TrainAugment(cat_max_ratio=0.75, cat_ignore_label=bad)
    with pytest.raises(ValueError, match="cat_ignore_label"):
        TrainAugment(cat_max_ratio=0.75, pad_label=-100)             # the default ignore label is pad_label
    for bad in (0, 11, -3):
        with pytest.raises(ValueError, match="cat_tries"):
            TrainAugment(cat_max_ratio=0.75, cat_tries=bad)
    a = TrainAugment(cat_max_ratio=0.75, pad_label=150)
    assert (a.cat_ratio1024, a.cat_ignore_label, a.cat_tries, a.last_crop_info) == (768, 150, 10, None)
    assert TrainAugment(cat_max_ratio=0.5, cat_ignore_label=None, cat_tries=1).cat_ignore_label == -1
    off = TrainAugment(pad_label=-100)                               # the rule is off: today's arguments stay valid
    assert off.cat_max_ratio is None and off.cat_ratio1024 is None


def test_class_weights_restatement_on_a_hand_computed_case():
    """Three classes + the ignored class 0, two images:
         image 0: class 1 x 60, class 2 x 20, ignored x 20      image 1: class 1 x 40, class 3 x 10, ignored x 50
    median_freq: f1 = 100 / (80 + 50), f2 = 20 / 80, f3 = 10 / 50; median = f2 = 0.25.
    enet: p = 100 / 130, 20 / 130, 10 / 130."""
    counts = np.zeros((2, 256), dtype=np.int64)
    counts[0, [0, 1, 2]] = (20, 60, 20)
    counts[1, [0, 1, 3]] = (50, 40, 10)
    w = CR.class_weights_ref(counts, n_classes=5, ignore_index=0, mode="median_freq")
    f = np.array([100 / 130, 20 / 80, 10 / 50])
    assert np.allclose(w, [0.0, 0.25 / f[0], 1.0, 0.25 / f[2], 0.0], rtol=1e-15, atol=0)
    w = CR.class_weights_ref(counts, n_classes=5, ignore_index=0, mode="enet")
    want = [0.0] + [1.0 / np.log(1.02 + v / 130) for v in (100, 20, 10)] + [0.0]
    assert np.allclose(w, want, rtol=1e-15, atol=0)
    # an even number of occurring classes: the mean of the two middle frequencies; no ignored class
    w = CR.class_weights_ref(counts, n_classes=4, ignore_index=None, mode="median_freq")
    f = np.array([70 / 200, 100 / 200, 20 / 100, 10 / 100])
    assert np.allclose(w, 0.5 * (0.2 + 0.35) / f, rtol=1e-15, atol=0)
    assert np.array_equal(CR.class_counts_ref([np.array([[1, 1], [3, 255]], dtype=np.uint8)])[0, [1, 3, 255]], [2, 1, 1])
    with pytest.raises(ValueError):
        CR.class_weights_ref(counts, mode="other")


def test_class_weights_torch_ops_match_the_restatement_on_the_host():
    """lc2is_amd.data.class_weights is torch arithmetic on the counts' device: on host tensors it gives the restatement's values."""
    import torch
    from lc2is_amd.data import class_weights
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 5000, (7, 256)) * (rng.random((7, 256)) < 0.3)
    counts[:, 17] = 0
    for mode in ("median_freq", "enet"):
        for n_classes, ignore in ((151, 0), (150, None), (256, 255)):
            got = class_weights(torch.from_numpy(counts), n_classes, ignore, mode)
            want = CR.class_weights_ref(counts, n_classes, ignore, mode)
            assert got.dtype == torch.float32 and got.shape == (n_classes,)
            assert np.allclose(got.numpy(), want, rtol=2e-7, atol=0)      # one fp32 rounding of the fp64 result
            assert got[17] == 0 and (ignore is None or got[ignore] == 0)
    assert (class_weights(torch.zeros(2, 256, dtype=torch.int64), 151) == 0).all()
    with pytest.raises(ValueError):
        class_weights(torch.from_numpy(counts), mode="other")


def test_bindings_and_header_declare_the_new_entry_points():
    """Both symbols are declared in the header, exported by the library and bound with as many argument types as the
    declaration has parameters."""
    from lc2is_amd import _lib, ops
    header = (ROOT / "include" / "lc2is_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("lc2is_aug_crop_select", "lc2is_label_histogram"):
        assert name in _lib.header_symbols()
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(ops._ARGTYPES[name]) == len(m.group(1).split(","))
        assert ops._fn(name).argtypes == ops._ARGTYPES[name]
    assert callable(ops.aug_crop_select) and callable(ops.label_histogram)
    assert "#define LC2IS_AUG_MAX_TRIES 10" in header and ops.AUG_MAX_TRIES == 10 and ops.LABEL_BINS == 256
    # refused before any device call
    f = ops._fn("lc2is_aug_crop_select")
    cfg = ops.AugConfig()
    cfg.crop_size = 32
    import ctypes
    c = ctypes.addressof(cfg)
    assert f(None, 0, None, 1, None, None, 1, None, c, None, 8, 768, 0, 10, None, None) == -2
    assert f(4, 0, 8, 1, 8, None, 1, 4, c, 4, 8, 1024, 0, 10, None, None) == -1      # ratio1024 out of range
    assert f(4, 0, 8, 1, 8, None, 1, 4, c, 4, 8, 768, 256, 10, None, None) == -1     # ignore_label
    assert f(4, 0, 8, 1, 8, None, 1, 4, c, 4, 8, 768, 0, 11, None, None) == -1       # tries
    assert f(4, 0, 8, 1, 8, None, 1, 4, c, 4, 5, 768, 0, 10, None, None) == -1       # S % L
    g = ops._fn("lc2is_label_histogram")
    assert g(None, 0, None, 1, None, 1, None, None) == -2
    assert g(4, 0, 8, 1, 8, 0, 4, None) == -1
