"""Strong photometric views (colour jitter, greyscale, Gaussian blur), the part that needs no GPU: the bindings and the library's
refusals (host code, before any launch), the argument checks of StrongAugment and the ops wrappers, and the properties of the numpy
restatement tests/strong_ref.py that tests/test_gpu_strong.py holds the kernels to."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R
import mix_ref as MR
import strong_ref as SR

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("lc2is_strong_params", "lc2is_strong_apply")


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
        comment = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "replaces:" in comment, name
    for c_name, value in (("LC2IS_STRONG_MAX_RADIUS", ops.STRONG_MAX_RADIUS), ("LC2IS_STRONG_PARAM_WORDS", ops.STRONG_PARAM_WORDS),
                          ("LC2IS_STRONG_FLAGS", ops.STRONG_FLAGS), ("LC2IS_STRONG_R", ops.STRONG_R), ("LC2IS_STRONG_SIGMA", ops.STRONG_SIGMA),
                          ("LC2IS_STRONG_M", ops.STRONG_M), ("LC2IS_STRONG_O", ops.STRONG_O), ("LC2IS_STRONG_W", ops.STRONG_W),
                          ("LC2IS_STRONG_COLOUR", ops.STRONG_COLOUR), ("LC2IS_STRONG_GREY", ops.STRONG_GREY),
                          ("LC2IS_STRONG_BLUR", ops.STRONG_BLUR)):
        assert re.search(rf"#define {c_name} {value}\b", header), c_name
    assert f"#define LC2IS_STRONG_STREAM 0x{ops.STRONG_STREAM:08X}u" in header and int(SR.STREAM) == ops.STRONG_STREAM
    assert (SR.MAX_RADIUS, SR.P_WORDS, SR.FLAGS, SR.R_WORD, SR.SIGMA, SR.M0, SR.O0, SR.W0) == \
        (ops.STRONG_MAX_RADIUS, ops.STRONG_PARAM_WORDS, ops.STRONG_FLAGS, ops.STRONG_R, ops.STRONG_SIGMA, ops.STRONG_M, ops.STRONG_O,
         ops.STRONG_W)
    assert (SR.COLOUR, SR.GREY, SR.BLUR) == (ops.STRONG_COLOUR, ops.STRONG_GREY, ops.STRONG_BLUR)
    assert ops.STRONG_W + ops.STRONG_MAX_RADIUS + 1 <= ops.STRONG_PARAM_WORDS
    # the struct: 5 uint32, 8 floats, 3 x 3 floats, no padding
    c = ops.StrongConfig
    assert ctypes.sizeof(c) == 88 and c.jitter_thr.offset == 8 and c.brightness_delta.offset == 20 and c.sigma_lo.offset == 44
    assert (c.mean.offset, c.std.offset, c.inv_std.offset) == (52, 64, 76)
    fields = re.search(r"typedef struct \{([^}]*)\} lc2is_strong_config;", code).group(1)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in c._fields_]


def test_the_stream_differs_from_the_mix_and_augment_streams():
    assert int(SR.STREAM) not in (0, int(MR.STREAM))
    for key in (0, 11, 2 ** 40 + 3):
        a, m, s = R.sample_hash(9, 4, [key])[0], MR.mix_hash(9, 4, [key])[0], SR.strong_hash(9, 4, [key])[0]
        assert len({int(a), int(m), int(s)}) == 3 and s == a ^ SR.STREAM


def _cfg(**kw):
    from lc2is_amd.data import StrongAugment
    return StrongAugment(**kw).config


def test_the_library_refuses_null_then_shape_before_any_launch():
    """Pointers are only tested, never followed: every call below returns from the checks."""
    from lc2is_amd import ops
    f, g = ops._fn("lc2is_strong_params"), ops._fn("lc2is_strong_apply")
    p = 0x1000
    good = _cfg()

    def par(cfg=good, keys=p, B=3, epoch=p, params=p):
        return f(keys, B, epoch, ctypes.addressof(cfg) if cfg is not None else None, params, None)

    bad_sigma = _cfg()
    bad_sigma.sigma_hi = 2.5
    for missing in ("keys", "epoch", "params"):
        assert par(cfg=bad_sigma, B=0, **{missing: None}) == -2, missing          # NULL first, whatever else is wrong
    assert par(cfg=None, B=0) == -2
    for kw in (dict(B=0), dict(B=-1), dict(keys=p + 4), dict(epoch=p + 2), dict(params=p + 1)):
        assert par(**kw) == -1, kw
    assert par(cfg=bad_sigma) == -1                                                # a sigma range past 2.0
    for name, value in (("sigma_lo", 0.0), ("sigma_lo", -1.0), ("sigma_lo", float("nan")), ("sigma_hi", 0.05), ("jitter_thr", (1 << 24) + 1),
                        ("gray_thr", (1 << 24) + 1), ("blur_thr", 1 << 25)):
        cfg = _cfg()
        setattr(cfg, name, value)
        assert par(cfg=cfg) == -1, (name, value)

    big = 0x40000000

    def app(inp=big, params=p, cfg=good, B=3, S=16, out=2 * big):
        return g(inp, params, ctypes.addressof(cfg) if cfg is not None else None, B, S, out, None)

    for missing in ("inp", "params", "out"):
        assert app(S=7, B=0, **{missing: None}) == -2, missing
    assert app(cfg=None, S=7) == -2
    for kw in (dict(B=0), dict(B=65536), dict(S=8), dict(S=0), dict(S=14), dict(S=18), dict(S=4100), dict(inp=big + 8), dict(out=2 * big + 4),
               dict(params=p + 2)):
        assert app(**kw) == -1, kw
    # in and out overlapping: in place, the input's last 16 bytes, the output's last 16 bytes
    nbytes = 3 * 3 * 16 * 16 * 4
    assert app(out=big) == -1 and app(out=big + nbytes - 16) == -1 and app(out=big - nbytes + 16) == -1


def test_strongaugment_refuses_bad_settings():
    from lc2is_amd.data import StrongAugment
    for kw in (dict(jitter_prob=1.5), dict(gray_prob=-0.1), dict(blur_prob=2), dict(sigma_range=(0.1, 2.5)), dict(sigma_range=(0.0, 1.0)),
               dict(sigma_range=(1.0, 0.5)), dict(contrast_range=(1.5, 0.5)), dict(saturation_range=(-0.5, 1.0)), dict(brightness_delta=-1.0),
               dict(hue_delta=float("nan")), dict(image_std=(0.2, 0.0, 0.2)), dict(image_mean=(0.5, 0.5))):
        with pytest.raises(ValueError):
            StrongAugment(**kw)
    for kw in (dict(jitter_prob="0.8"), dict(gray_prob=None), dict(blur_prob=True), dict(sigma_range=1.0), dict(contrast_range=(0.5,)),
               dict(brightness_delta="32"), dict(seed=1.5), dict(seed=None)):
        with pytest.raises(TypeError):
            StrongAugment(**kw)
    s = StrongAugment(jitter_prob=1.0, gray_prob=0.0, blur_prob=0.5, sigma_range=(0.25, 2.0), hue_delta=180.0, seed=2 ** 40 + 5)
    c = s.config
    assert (c.jitter_thr, c.gray_thr, c.blur_thr) == (1 << 24, 0, 1 << 23) and (c.seed_lo, c.seed_hi) == (5, 256)
    assert (c.sigma_lo, c.sigma_hi) == (0.25, 2.0) and abs(c.hue_delta - np.pi) < 1e-6 and s.last_params is None
    assert all(abs(c.std[i] * c.inv_std[i] - 1.0) < 1e-6 for i in range(3))
    d = StrongAugment().config
    assert (d.jitter_thr, d.gray_thr, d.blur_thr) == (round(0.8 * 2 ** 24), round(0.2 * 2 ** 24), 1 << 23)
    assert abs(d.sigma_lo - 0.1) < 1e-7 and d.sigma_hi == 2.0


def test_strongaugment_and_the_wrappers_check_arguments_before_device_work():
    from lc2is_amd import ops
    from lc2is_amd.data import StrongAugment
    strong = StrongAugment()
    keys = torch.arange(2)
    x = torch.zeros(2, 3, 16, 16)
    for bad in (x.double(), x.half(), x.numpy(), None):
        with pytest.raises(TypeError):
            strong(bad, keys, 0)
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 14, 14), torch.zeros(2, 1, 16, 16), torch.zeros(2, 3, 16, 20), torch.zeros(3, 16, 16),
                torch.zeros(0, 3, 16, 16)):
        with pytest.raises(ValueError):
            strong(bad, keys, 0)
    # host tensors of the right types: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        strong(x, keys, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        strong.view({"pixel_values": x, "label": None}, keys, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.strong_params(keys, torch.zeros(1, dtype=torch.int32), strong.config)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.strong_apply(x, torch.zeros(2, ops.STRONG_PARAM_WORDS, dtype=torch.int32), strong.config)
    assert strong.last_params is None


def test_the_selftraining_recipe_draws_its_views():
    from lc2is_amd import selftrain
    doc = selftrain.__doc__
    scope = doc[doc.index("Out of scope here"):]
    assert "views" not in scope and "strong / weak" not in scope
    recipe = doc[:doc.index("Out of scope here")]
    assert "StrongAugment" in recipe and "TrainAugment(photometric=False" in recipe and "strong.view(weak, keys, epoch)" in recipe
    assert recipe.index("photometric=False") < recipe.index("labeler(weak") < recipe.index("strong.view(weak")


# ---- properties of the restatement ------------------------------------------------------------------------------------------
def _torch_blur(v, w, Rr):
    """F.pad(mode="reflect") + F.conv2d in float64, rows then columns, one kernel for every plane."""
    t = torch.from_numpy(v)[None]                                               # [1, C, S, S]
    C_ = t.shape[1]
    k = torch.from_numpy(np.concatenate([w[Rr:0:-1], w[:Rr + 1]]))              # w_R .. w_1 w_0 w_1 .. w_R
    t = F.conv2d(F.pad(t, (Rr, Rr, 0, 0), mode="reflect"), k.view(1, 1, 1, -1).repeat(C_, 1, 1, 1), groups=C_)
    t = F.conv2d(F.pad(t, (0, 0, Rr, Rr), mode="reflect"), k.view(1, 1, -1, 1).repeat(C_, 1, 1, 1), groups=C_)
    return t[0].numpy()


@pytest.mark.parametrize("S,Rr,sigma", [(12, 8, 2.0), (20, 3, 0.75)])
def test_the_restated_blur_is_reflect_pad_plus_conv2d(S, Rr, sigma):
    assert SR.radius(sigma) == Rr
    w = SR.taps(sigma, Rr)
    v = np.random.default_rng(S).standard_normal((3, S, S))
    assert np.abs(SR.blur_ref(v, w, Rr) - _torch_blur(v, w, Rr)).max() <= 1e-12
    # through apply_ref, blur only: the same numbers on the fp32 input
    x = v.astype(np.float32)[None]
    row = SR.make_row(SR.BLUR, Rr, sigma)
    got = SR.apply_ref(x, row[None], (0.5,) * 3, (0.25,) * 3)[0]
    assert np.abs(got - _torch_blur(x[0].astype(np.float64), row.view(np.float32)[SR.W0:SR.W0 + 9].astype(np.float64), Rr)).max() <= 1e-12


def test_the_radius_and_the_taps():
    for sigma, want in ((0.1, 1), (0.25, 1), (0.2500001, 2), (2.0, 8), (0.5, 2), (1.0, 4), (1.9, 8)):
        assert SR.radius(np.float32(sigma)) == want, sigma
    for sigma in (0.1, 0.25, 0.2500001, 0.7, 1.3, 2.0):
        Rr = int(SR.radius(np.float32(sigma)))
        w = SR.taps(sigma, Rr)
        assert abs(w[0] + 2.0 * w[1:].sum() - 1.0) <= 1e-15 and (w[Rr + 1:] == 0).all() and (w[:Rr + 1] > 0).all()
        assert (np.diff(w[:Rr + 1]) < 0).all()
        assert abs(w[1] / w[0] - np.exp(-1.0 / (2.0 * sigma ** 2))) <= 1e-15


def test_the_on_rates_over_4000_keys():
    """4000 keys: an on-count is Binomial(4000, p), sd = sqrt(4000 p (1 - p)) = 25.3 (p = 0.8 and 0.2) and 31.6 (p = 0.5) draws; the
    bound is five of them: 0.0317 and 0.0396 as a share."""
    cfg = SR.config_dict(_cfg(seed=1234))
    p = SR.draw_params(cfg, np.arange(4000), 3)
    n = 4000.0
    for name, prob in (("jitter", 0.8), ("grey", 0.2), ("blur", 0.5)):
        bound = 5.0 * np.sqrt(prob * (1.0 - prob) / n)
        assert abs(p[name].mean() - prob) <= bound, (name, p[name].mean(), bound)
    assert ((p["flags"] & SR.COLOUR) > 0).sum() == (p["jitter"] | p["grey"]).sum()
    assert p["R"].min() >= 1 and p["R"].max() == 8 and (p["sigma"] >= np.float32(0.1)).all() and (p["sigma"] <= 2.0).all()


def test_the_restated_colour_and_rows():
    cfg = SR.config_dict(_cfg(jitter_prob=0.5, gray_prob=0.5, seed=7))
    p = SR.draw_params(cfg, np.arange(400), 0)
    grey, jit = p["grey"] == 1, p["jitter"] == 1
    assert (grey & jit).any() and (grey & ~jit).any() and (~grey & jit).any() and (~grey & ~jit).any()
    # a grey map has three equal rows; an untouched one is the identity; grey alone is exactly 1 w^T
    assert np.abs(p["M"][grey] - p["M"][grey][:, :1]).max() <= 1e-15 and np.abs(p["o"][grey] - p["o"][grey][:, :1]).max() <= 1e-12
    assert (p["M"][~grey & ~jit] == np.eye(3)).all() and (p["o"][~grey & ~jit] == 0).all()
    assert np.abs(p["M"][grey & ~jit] - np.tile(SR.GREY_W, (3, 1))).max() <= 1e-15
    # saturation and hue keep the grey axis: with them alone every row of M sums to the contrast
    assert np.abs(p["M"][~grey & jit].sum(axis=2) - p["M"][~grey & jit].sum(axis=2)[:, :1]).max() <= 1e-12
    rows = SR.param_rows(p)
    assert rows.shape == (400, SR.P_WORDS) and not rows[:, SR.W0 + 9:].any()
    assert (rows[:, SR.FLAGS] == p["flags"]).all() and set(np.unique(rows[:, SR.FLAGS] & 3).tolist()) == {0, 1, 3}
    # the epoch, the key and the seed change the draw
    base = SR.param_rows(SR.draw_params(cfg, [11], 4))
    assert not np.array_equal(base, SR.param_rows(SR.draw_params(cfg, [11], 5)))
    assert not np.array_equal(base, SR.param_rows(SR.draw_params(cfg, [12], 4)))
    assert np.array_equal(base, SR.param_rows(SR.draw_params(cfg, [11], 4)))


def test_the_restated_apply_copies_what_has_no_flag_and_bad_rows():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((4, 3, 12, 12)).astype(np.float32)
    rows = np.stack([SR.make_row(0), SR.make_row(SR.BLUR, 9), SR.make_row(8 | SR.BLUR, 2), SR.make_row(SR.COLOUR, 0, M=np.eye(3) * 0.5)])
    out = SR.apply_ref(x, rows, (0.5,) * 3, (0.25,) * 3)
    assert np.array_equal(out[:3].astype(np.float32), x[:3]) and not np.allclose(out[3], x[3])
    # colour alone: halving on the 0..255 scale, clamped, back to normalised units
    want = (np.clip(0.5 * 255.0 * (x[3].astype(np.float64) * 0.25 + 0.5), 0, 255) / 255.0 - 0.5) / 0.25
    assert np.abs(out[3] - want).max() <= 1e-12
