"""Mixed-sample augmentation (ClassMix / CutMix), the part that needs no GPU: the bindings and the library's refusals (host code,
before any launch), the argument checks of SampleMix and the ops wrappers, and the properties of the numpy restatement
tests/mix_ref.py that tests/test_gpu_mix.py holds the kernels to."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_ref as R
import mix_ref as MR

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("lc2is_mix_select", "lc2is_mix_apply")


def test_bindings_and_header_declare_the_entry_points():
    from lc2is_amd import _lib, ops
    header = (ROOT / "include" / "lc2is_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.header_symbols() and hasattr(lib, name)
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(ops._ARGTYPES[name]) == len(m.group(1).split(","))
        assert ops._fn(name).argtypes == ops._ARGTYPES[name]
    for c_name, value in (("LC2IS_MIX_NONE", ops.MIX_NONE), ("LC2IS_MIX_CLASSMIX", ops.MIX_CLASSMIX), ("LC2IS_MIX_CUTMIX", ops.MIX_CUTMIX),
                          ("LC2IS_MIX_MAX_CLASSES", ops.MIX_MAX_CLASSES), ("LC2IS_MIX_PLAN_WORDS", ops.MIX_PLAN_WORDS),
                          ("LC2IS_MIX_BITMAP", ops.MIX_BITMAP)):
        assert re.search(rf"#define {c_name} {value}\b", header), c_name
    assert f"#define LC2IS_MIX_STREAM 0x{ops.MIX_STREAM:08X}u" in header and int(MR.STREAM) == ops.MIX_STREAM
    assert (MR.MAX_CLASSES, MR.P_WORDS, MR.BITMAP) == (ops.MIX_MAX_CLASSES, ops.MIX_PLAN_WORDS, ops.MIX_BITMAP)
    assert ctypes.sizeof(ops.MixConfig) == 40 and ops.MixConfig.ignore_index.offset == 16 and ops.MixConfig.area_lo1024.offset == 32


def _cfg(mode=1, n_classes=151, lo=256, hi=512):
    from lc2is_amd import ops
    c = ops.MixConfig()
    c.mode, c.n_classes, c.ignore_index, c.exclude_label, c.area_lo1024, c.area_hi1024 = mode, n_classes, -100, -1, lo, hi
    return c


def test_the_library_refuses_null_then_shape_then_unsupported_before_any_launch():
    """Pointers are only tested, never followed: every call below returns from the checks."""
    from lc2is_amd import ops
    f, g = ops._fn("lc2is_mix_select"), ops._fn("lc2is_mix_apply")
    p = 0x1000

    def sel(cfg, src_lab=p, Bs=2, src_index=None, keys=p, B=3, epoch=p, L=8, plan=p, info=p):
        return f(src_lab, Bs, src_index, keys, B, epoch, ctypes.addressof(cfg) if cfg is not None else None, L, plan, info, None)

    for missing in ("src_lab", "keys", "epoch", "plan", "info"):
        assert sel(_cfg(mode=7, n_classes=0), **{missing: None}) == -2, missing       # NULL first, whatever else is wrong
    assert sel(None) == -2
    for kw in (dict(B=0), dict(Bs=0), dict(L=0), dict(L=4097), dict(plan=p + 2), dict(src_lab=p + 4), dict(src_index=p + 4)):
        assert sel(_cfg(mode=7), **kw) == -1, kw                                          # SHAPE before UNSUPPORTED
    for cfg in (_cfg(n_classes=0), _cfg(n_classes=1025), _cfg(lo=0), _cfg(lo=600, hi=512), _cfg(hi=1025)):
        cfg.mode = 7
        assert sel(cfg) == -1
    assert sel(_cfg(mode=7)) == -3 and sel(_cfg(mode=-1)) == -3

    def app(dst_px=p, dst_lab=p, dst_pw=None, src_px=2 * p, src_lab=2 * p, src_pw=None, Bs=2, plan=p, B=3, S=16, L=4,
            out_px=0x100000, out_lab=0x100000, out_pw=0x100000):
        return g(dst_px, dst_lab, dst_pw, src_px, src_lab, src_pw, Bs, plan, B, S, L, out_px, out_lab, out_pw, None)

    for missing in ("dst_px", "dst_lab", "src_px", "src_lab", "plan", "out_px", "out_lab", "out_pw"):
        assert app(S=7, **{missing: None}) == -2, missing
    for kw in (dict(B=0), dict(B=65536), dict(Bs=0), dict(S=0), dict(S=18), dict(S=4100), dict(L=0), dict(L=3), dict(dst_px=p + 8),
               dict(out_lab=0x100004), dict(src_pw=p + 2), dict(plan=p + 1)):
        assert app(**kw) == -1, kw
    # an output that overlaps an input (the destination's last byte, the source's first); the source may be the destination
    px_bytes, lab_bytes, pw_bytes = 3 * 3 * 16 * 16 * 4, 3 * 16 * 8, 3 * 16 * 4
    big = 0x40000000
    assert app(dst_px=big, out_px=big + px_bytes - 16) == -1 and app(dst_lab=big, out_lab=big + lab_bytes - 8) == -1
    assert app(src_px=big, out_px=big - px_bytes + 16) == -1 and app(dst_pw=big, out_pw=big + pw_bytes - 4) == -1
    assert app(src_pw=big, out_pw=big) == -1


def test_samplemix_refuses_bad_settings():
    from lc2is_amd.data import SampleMix
    for kw in (dict(mode="mixup"), dict(mode=None), dict(n_classes=0), dict(n_classes=1025), dict(box_area=(0.0, 0.5)),
               dict(box_area=(0.25, 1.5)), dict(box_area=(0.5, 0.25)), dict(box_area=(1e-5, 0.5))):
        with pytest.raises(ValueError):
            SampleMix(**kw)
    for kw in (dict(n_classes=151.0), dict(ignore_index=None), dict(exclude_label=0.0), dict(n_classes=True)):
        with pytest.raises(TypeError):
            SampleMix(**kw)
    m = SampleMix("cutmix", n_classes=1024, exclude_label=0, box_area=(0.25, 1.0), seed=2 ** 40 + 5)
    c = m.config
    assert (c.mode, c.n_classes, c.ignore_index, c.exclude_label, c.area_lo1024, c.area_hi1024) == (2, 1024, -100, 0, 256, 1024)
    assert (c.seed_lo, c.seed_hi) == (5, 256) and SampleMix().config.exclude_label == -1 and SampleMix().config.mode == 1
    assert SampleMix("none").config.mode == 0 and m.last_info is None


def _batch(n=2, S=16, L=4):
    return (torch.zeros(n, 3, S, S), torch.zeros(n, L, L, dtype=torch.int64), torch.ones(n, L, L))


def test_samplemix_and_the_wrappers_check_arguments_before_device_work():
    from lc2is_amd import ops
    from lc2is_amd.data import SampleMix
    mix = SampleMix()
    keys = torch.arange(2)
    px, lab, pw = _batch()
    with pytest.raises(ValueError, match="multiple of 4 and of L"):
        mix(_batch(S=16, L=3), _batch(S=16, L=3), keys, 0)                    # S % L != 0
    with pytest.raises(ValueError, match="multiple of 4 and of L"):
        mix(_batch(S=6, L=3), _batch(S=6, L=3), keys, 0)                      # S % 4 != 0
    with pytest.raises(ValueError):
        mix((px, lab, pw), _batch(S=32, L=4), keys, 0)                        # two sizes
    with pytest.raises(ValueError):
        mix((px, lab[:, :, :2], None), (px, lab, pw), keys, 0)
    for bad in ((px.double(), lab, pw), (px, lab.int(), pw), (px, lab, pw.half()), (px.numpy(), lab, pw), (px, lab)):
        with pytest.raises(TypeError):
            mix(bad, (px, lab, pw), keys, 0)
        with pytest.raises(TypeError):
            mix((px, lab, None), bad, keys, 0)
    # host tensors of the right types: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        mix((px, lab, pw), (px, lab, None), keys, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mix_select(lab, keys, torch.zeros(1, dtype=torch.int32), mix.config)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mix_apply((px, lab, pw), (px, lab, None), torch.zeros(2, ops.MIX_PLAN_WORDS, dtype=torch.int32))
    assert mix.last_info is None


def test_the_selftraining_recipe_names_the_mixer():
    from lc2is_amd import selftrain
    doc = selftrain.__doc__
    scope = doc[doc.index("Out of scope here"):]
    assert "ClassMix" not in scope and "SampleMix" in doc and "step.step(" in doc
    assert callable(selftrain.PseudoLabeler.mixed) and callable(selftrain.PseudoLabeler.combine)


# ---- properties of the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 7, 150, 1024])
def test_the_chosen_count_is_exactly_half_rounded_up(n):
    rng = np.random.default_rng(n)
    present = np.sort(rng.permutation(1024)[:n])
    for key in range(20):
        h = MR.mix_hash(3, 1, [key])[0]
        chosen = MR.chosen_classes(h, present)
        assert chosen.size == (n + 1) // 2 and np.isin(chosen, present).all() and np.unique(chosen).size == chosen.size
    # through a label map, with labels that never count mixed in
    if n:
        L = 32
        cells = np.resize(present, L * L).astype(np.int64)
        cells[::7] = -100
        plan, info, mask = MR.select_ref(cells.reshape(1, L, L), [5], 0, "classmix", n_classes=1024)
        n_here = np.unique(cells[cells >= 0]).size
        assert tuple(info[0, :2]) == (n_here, (n_here + 1) // 2) and info[0, 3] == L * L and info[0, 2] == mask.sum()
        assert sum(bin(int(w) & 0xffffffff).count("1") for w in plan[0, MR.BITMAP:]) == (n_here + 1) // 2


def test_every_class_is_chosen_half_of_the_time():
    """4000 keys, 6 classes present, 3 chosen each time: a class's count is Binomial(4000, 1/2) up to the fixed-size coupling,
    sd = sqrt(4000 / 4) = 31.6 draws; the bound 0.04 * 4000 = 160 draws is five of them."""
    present = np.array([2, 3, 11, 40, 97, 150])
    hs = MR.mix_hash(1234, 0, np.arange(4000))
    counts = {int(c): 0 for c in present}
    for h in hs:
        for c in MR.chosen_classes(h, present):
            counts[int(c)] += 1
    shares = np.array(list(counts.values())) / 4000.0
    assert sum(counts.values()) == 3 * 4000 and (np.abs(shares - 0.5) <= 0.04).all(), shares


def test_ties_of_the_draw_break_by_class_id(monkeypatch):
    monkeypatch.setattr(MR, "u24", lambda h, k: np.asarray(k, dtype=np.int64) * 0 + 7)
    assert MR.chosen_classes(np.uint32(1), np.array([9, 4, 30, 2, 17])).tolist() == [2, 4, 9]


@pytest.mark.parametrize("L", [1, 4, 8, 32, 128, 4096])
@pytest.mark.parametrize("area", [(0.25, 0.5), (1 / 1024, 1 / 1024), (1.0, 1.0), (0.01, 1.0)])
def test_every_cutmix_box_lies_inside_the_grid_and_has_the_drawn_area(L, area):
    lo, hi = MR.area1024(area)
    for h in MR.mix_hash(7, 2, np.arange(300)):
        top, left, bh, bw, a = MR.cutmix_box(h, L, lo, hi)
        assert lo <= a <= hi and 1 <= bh <= L and 1 <= bw <= L and 0 <= top <= L - bh and 0 <= left <= L - bw
        assert abs(bh * bw * 1024 - a * L * L) <= 512 * bh + 1024 * max(bh, bw), (L, a, bh, bw)


def test_the_epoch_the_key_and_the_stream_change_the_draw():
    L = 32
    lab = np.random.default_rng(0).integers(0, 40, (1, L, L))
    base = {m: MR.select_ref(lab, [11], 4, m, seed=9, n_classes=40)[0] for m in ("classmix", "cutmix")}
    for m in ("classmix", "cutmix"):
        assert not np.array_equal(base[m], MR.select_ref(lab, [11], 5, m, seed=9, n_classes=40)[0])
        assert not np.array_equal(base[m], MR.select_ref(lab, [12], 4, m, seed=9, n_classes=40)[0])
        assert not np.array_equal(base[m], MR.select_ref(lab, [11], 4, m, seed=10, n_classes=40)[0])
        assert np.array_equal(base[m], MR.select_ref(lab, [11], 4, m, seed=9, n_classes=40)[0])
    # a mixer and a TrainAugment with the same seed do not share draws
    assert MR.mix_hash(9, 4, [11])[0] != R.sample_hash(9, 4, [11])[0]
    assert MR.mix_hash(9, 4, [11])[0] == R.sample_hash(9, 4, [11])[0] ^ MR.STREAM


def test_the_restated_apply_is_a_select_of_bit_patterns():
    rng = np.random.default_rng(1)
    S, L = 8, 4
    dst = (rng.standard_normal((2, 3, S, S)).astype(np.float32), rng.integers(0, 5, (2, L, L)), None)
    src = (rng.standard_normal((1, 3, S, S)).astype(np.float32), rng.integers(5, 9, (1, L, L)), np.full((1, L, L), 0.5, np.float32))
    dst[0][0, :, :4, :4] = np.nan
    mask = np.zeros((2, L, L), bool)
    mask[0, :2, :2] = True
    px, lab, pw = MR.apply_ref(dst, src, mask, src_index=[0, 5])
    assert np.isfinite(px).all() and np.array_equal(px[0, :, :4, :4], src[0][0, :, :4, :4]) and np.array_equal(px[1], dst[0][1])
    assert np.array_equal(lab[0, :2, :2], src[1][0, :2, :2]) and np.array_equal(lab[1], dst[1][1])
    assert (pw[0, :2, :2] == 0.5).all() and pw.sum() == 2 * L * L - 2.0
