"""Refusals and output bits of the device data views, to compare two trees of this project line for line.

  python tools/view_path_digest.py --root TREE --validate   (no device)
      sweeps valid and invalid arguments through TrainAugment, SampleMix, StrongAugment and GeometricAugment (constructors and
      calls), through the ten ``ops`` wrappers of the family, and through the eleven ``lc2is_*`` entry points by ctypes with pointers
      that are never followed (every ctypes call carries a refusal: nothing is launched).  Records the exception class of each call
      (and its message where the suite matches on one) and the return code of each entry point.
  python tools/view_path_digest.py --root TREE              (one HIP device; a few seconds)
      runs the augmenter, the crop re-draw, the label histogram, the mixer, the strong view, the geometric view and the score warp
      on fixed seeds and hand-written parameter rows, at the smallest shapes that reach every branch of their kernels, and prints a
      sha256 of the raw bytes of every output.

``--root`` is the tree whose ``lc2is_amd`` is imported (default: the tree this file is in); set LC2IS_LIB to choose the built
library.  ``--out FILE`` writes the lines there; the last line of stdout is always "sha256 <hash> <n> lines".
"""
import argparse
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE / "tests"))      # the numpy restatements only build hand-written rows here
MATCHED = ("no CPU path", "overlap", "alias", "table", "multiple of 4 and of L", "cat_max_ratio", "cat_ignore_label", "cat_tries",
           "label shape", "3 channels", "4096", "multiple of label_size", "multiple of 4", "unknown photometric")


def raised(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except Exception as e:   # noqa: BLE001  (the sweep records whatever comes first)
        words = [w for w in MATCHED if w in str(e)]
        return type(e).__name__ + (f" [{', '.join(words)}]" if words else "")
    return "returned"


# ---- --validate ---------------------------------------------------------------------------------------------------------------
def validate(torch, emit):
    from lc2is_amd import ops
    from lc2is_amd.data import DeviceImagePool, GeometricAugment, SampleMix, StrongAugment, TrainAugment
    nan, inf = float("nan"), float("inf")

    # constructors: every setting, its bad values
    sweeps = {
        TrainAugment: dict(crop_size=[512, 2, 510, 8192], label_size=[128, 0, 100], base_size=[512, 0, 70000], ratio_range=[(0.5, 2.0), (2.0, 0.5), (0.0, 1.0)],
                           flip_prob=[0.5, -0.1, 1.5], photometric=[True, False, dict(prob=0.3), dict(bogus=1), dict(prob=(0.1, 0.2))],
                           image_mean=[(0.5, 0.5, 0.5), (0.5, 0.5)], image_std=[(0.2, 0.2, 0.2), (0.2, 0.0, 0.2)], seed=[0, -1, 2 ** 70, 1.5, "7", "x", None],
                           cat_max_ratio=[None, 0.75, 0.0, 1.0, 0.0001], cat_ignore_label=["pad_label", None, 255, 256, -1], cat_tries=[10, 0, 11],
                           pad_label=[0, 255, 300]),
        SampleMix: dict(mode=["classmix", "cutmix", "none", "bogus"], n_classes=[151, 0, 1025, 1.5, True], ignore_index=[-100, 1.5], exclude_label=[None, 0, "a"],
                        box_area=[(0.25, 0.5), (0.5, 0.25), (0.0, 0.5), (0.5, 1.5), ("0.25", "0.5"), (0.0001, 0.5), 0.5], seed=[0, -1, 1.5, "7", "x", True]),
        StrongAugment: dict(jitter_prob=[0.8, -0.1, 1.5, "a", nan, True], brightness_delta=[64.0, -1.0, inf], contrast_range=[(0.5, 1.5), (1.5, 0.5), (-0.5, 1.0), 0.5, (0.5,)],
                            saturation_range=[(0.5, 1.5), (-1.0, 1.0), ("a", 1.0)], hue_delta=[90.0, -1.0, None], gray_prob=[0.2, 2.0], blur_prob=[0.5, -1.0],
                            sigma_range=[(0.1, 2.0), (0.0, 1.0), (0.1, 2.5), (1.0, 0.5)], image_mean=[(0.5, 0.5, 0.5), (0.5, 0.5)], image_std=[(0.2, 0.2, 0.2), (0.2, -0.2, 0.2)],
                            seed=[0, -1, 2 ** 70, 1.5, "7", True]),
        GeometricAugment: dict(prob=[1.0, -0.5, "a"], rotate_deg=[20.0, 181.0, -1.0, nan], scale_range=[(0.8, 1.25), (0.2, 1.0), (1.0, 4.5), (1.25, 0.8), 1.0], shear_deg=[0.0, 46.0],
                               translate=[0.0, 0.6, -0.1], flip_prob=[0.0, 1.5], fill=[None, (0, 0, 0), (0, 0), (0, 0, 256), (0, "a", 0), 3], ignore_index=[-100, 2 ** 63, 1.5, True],
                               image_mean=[(0.5, 0.5, 0.5), (0.5,)], image_std=[(0.2, 0.2, 0.2), (0.0, 0.2, 0.2)], seed=[0, -1, 1.5, "7", True]),
    }
    for cls, settings in sweeps.items():
        for key, values in settings.items():
            for v in values:
                emit(f"{cls.__name__}({key}={v!r}) -> {raised(cls, **{key: v})}")

    # calls: host tensors of every kind (there is no device: a call that passes stage one stops at "no CPU path")
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    px = {name: torch.zeros(shape, dtype=dt) for name, shape, dt in (
        ("ok", (2, 3, 16, 16), f32), ("f64", (2, 3, 16, 16), torch.float64), ("rank3", (2, 3, 16), f32), ("c4", (2, 4, 16, 16), f32), ("rect", (2, 3, 16, 12), f32),
        ("S10", (2, 3, 10, 10), f32), ("S4", (2, 3, 4, 4), f32), ("S8", (2, 3, 8, 8), f32), ("S12", (2, 3, 12, 12), f32), ("B0", (0, 3, 16, 16), f32))}
    px["none"], px["list"] = None, [[0.0]]
    lab = {name: torch.zeros(shape, dtype=dt) for name, shape, dt in (
        ("ok", (2, 4, 4), i64), ("i32", (2, 4, 4), i32), ("rank2", (2, 4), i64), ("rect", (2, 4, 2), i64), ("L3", (2, 3, 3), i64), ("L5", (2, 5, 5), i64), ("B3", (3, 4, 4), i64),
        ("L16", (2, 16, 16), i64))}
    lab["none"] = None
    pw = {name: torch.zeros(shape, dtype=dt) for name, shape, dt in (("ok", (2, 4, 4), f32), ("f64", (2, 4, 4), torch.float64), ("L2", (2, 2, 2), f32), ("rank2", (2, 4), f32))}
    pw["none"] = None
    keys = dict(ok=[3, 5], three=[1, 2, 3], tensor=torch.tensor([3, 5]), none=None)
    strong, geo, mix = StrongAugment(seed=1), GeometricAugment(seed=1), SampleMix(seed=1)
    for p in px:
        emit(f"StrongAugment()(px={p}) -> {raised(strong, px[p], [3, 5], 0)}")
    for k in keys:
        emit(f"StrongAugment()(keys={k}) -> {raised(strong, px['ok'], keys[k], 0)}")
    emit(f"StrongAugment()(out=px) -> {raised(strong, px['ok'], [3, 5], 0, out=px['ok'])}")
    emit(f"StrongAugment().view(px=rank3) -> {raised(strong.view, dict(pixel_values=px['rank3']), [3, 5], 0)}")
    # one operand off at a time, the others valid
    for p, lb, w in [(p, "ok", "ok") for p in px] + [("ok", lb, "none") for lb in lab] + [("ok", "ok", w) for w in pw] + [("ok", "none", w) for w in pw]:
        emit(f"GeometricAugment()(px={p}, lab={lb}, pw={w}) -> {raised(geo, (px[p], lab[lb], pw[w]), [3, 5], 0)}")
        emit(f"SampleMix()(dst=({p}, {lb}, {w}), src=ok) -> {raised(mix, (px[p], lab[lb], pw[w]), (px['ok'], lab['ok'], None), [3, 5], 0)}")
        emit(f"SampleMix()(dst=ok, src=({p}, {lb}, {w})) -> {raised(mix, (px['ok'], lab['ok'], None), (px[p], lab[lb], pw[w]), [3, 5], 0)}")
    for batch in (None, (px["ok"],), [px["ok"], None, None], (px["ok"], lab["ok"], pw["ok"], None)):
        tag = "None" if batch is None else len(batch)
        emit(f"GeometricAugment()(batch of {tag}) -> {raised(geo, batch, [3, 5], 0)}")
        emit(f"SampleMix()(dst of {tag}) -> {raised(mix, batch, (px['ok'], lab['ok'], None), [3, 5], 0)}")
    emit(f"GeometricAugment()(out of 2) -> {raised(geo, (px['ok'], None, None), [3, 5], 0, out=(None, None))}")
    scores = {name: torch.zeros(shape, dtype=dt) for name, shape, dt in (
        ("ok", (2 * 4, 8), f32), ("f64", (8, 8), torch.float64), ("rank1", (8,), f32), ("rows7", (7, 8), f32), ("g-not-square", (2 * 3, 8), f32), ("ld6", (8, 6), f32),
        ("ld2", (8, 2), f32), ("ld1028", (8, 1028), f32))}
    scores["none"] = None
    table = {"ok": torch.zeros(2, 16, dtype=i32), "i64": torch.zeros(2, 16, dtype=i64), "words15": torch.zeros(2, 15, dtype=i32), "rank1": torch.zeros(32, dtype=i32),
             "B0": torch.zeros(0, 16, dtype=i32), "none": None}
    sizes = (("none", None), ("ok", None), ("ok", 4), ("ok", 8), ("L2", None), ("f64", None), ("rank2", None), ("none", 4), ("none", 3), ("none", 1.5), ("none", True),
             ("none", 0), ("none", 8192))
    for s, t, (tw, L) in [(s, "ok", sizes[0]) for s in scores] + [("ok", t, sizes[0]) for t in table] + [("ok", "ok", z) for z in sizes]:
        emit(f"GeometricAugment().warp_scores(scores={s}, params={t}, tw={tw}, label_size={L!r}) -> "
             f"{raised(geo.warp_scores, scores[s], pw[tw], L, params=table[t])}")
    maps = (("ok", "none", "none"), ("none", "none", "none"), ("none", "ok", "none"), ("none", "none", "ok"), ("ok", "L2", "none"), ("L16", "none", "ok"))
    for p, s, (lb, w, tw) in [(p, "ok", maps[0]) for p in ("ok", "none", "rank3", "B0")] + [("ok", s, maps[0]) for s in ("f64", "rows7", "none")] + \
            [("ok", "ok", m) for m in maps[1:]]:
        emit(f"GeometricAugment().view_distill(px={p}, scores={s}, lab={lb}, pw={w}, tw={tw}) -> "
             f"{raised(geo.view_distill, dict(pixel_values=px[p]), lab[lb], scores[s], [3, 5], 0, pw[w], pw[tw])}")
    aug = TrainAugment(crop_size=16, label_size=4, seed=1)
    u8 = np.zeros((5, 7, 3), np.uint8)
    for im, lb, tag in ((u8, u8[..., 0], "ok"), (u8.astype(np.float32), u8[..., 0], "float image"), (u8, u8[:4, :, 0], "label shape"), (u8[..., :2], u8[..., 0], "2 channels"),
                        (np.zeros((5000, 2, 3), np.uint8), np.zeros((5000, 2), np.uint8), "5000 rows"), (u8.tolist(), u8[..., 0], "a list")):
        emit(f"DeviceImagePool.check({tag}) -> {raised(DeviceImagePool.check, im, lb)}")
    emit(f"DeviceImagePool('cpu') -> {raised(DeviceImagePool, 'cpu')}")
    emit(f"TrainAugment()(indices=None) -> {raised(aug, None, None, 0)}")
    emit(f"TrainAugment()(images without labels) -> {raised(aug, images=[u8], indices=[0])}")
    emit(f"TrainAugment()(no images) -> {raised(aug, images=[], labels=[], indices=[])}")

    # the ten wrappers with host tensors: the first refusal of each
    cfgs = dict(aug=aug.config, mix=mix.config, strong=strong.config, geo=geo.config)
    desc, slots, epoch = torch.zeros(3, 3, dtype=i64), torch.zeros(2, dtype=i64), torch.zeros(1, dtype=i32)
    u8buf, kt = torch.zeros(64, dtype=torch.uint8), torch.tensor([3, 5])
    calls = [("aug_params", lambda: ops.aug_params(slots, epoch, desc, cfgs["aug"])),
             ("aug_apply", lambda: ops.aug_apply(u8buf, u8buf, desc, slots, torch.zeros(2, 20, dtype=i32), 16, 4, aug.norm)),
             ("aug_crop_select", lambda: ops.aug_crop_select(u8buf, desc, slots, epoch, cfgs["aug"], torch.zeros(2, 20, dtype=i32), 4, ratio1024=768)),
             ("label_histogram", lambda: ops.label_histogram(u8buf, desc, slots)),
             ("mix_select", lambda: ops.mix_select(lab["ok"], kt, epoch, cfgs["mix"])),
             ("mix_apply", lambda: ops.mix_apply((px["ok"], lab["ok"], None), (px["ok"], lab["ok"], None), torch.zeros(2, 40, dtype=i32))),
             ("strong_params", lambda: ops.strong_params(kt, epoch, cfgs["strong"])),
             ("strong_apply", lambda: ops.strong_apply(px["ok"], torch.zeros(2, 32, dtype=i32), cfgs["strong"])),
             ("geo_params", lambda: ops.geo_params(kt, epoch, cfgs["geo"])),
             ("geo_apply", lambda: ops.geo_apply((px["ok"], lab["ok"], pw["ok"]), table["ok"], cfgs["geo"])),
             ("geo_apply batch of 2", lambda: ops.geo_apply((px["ok"], None), table["ok"], cfgs["geo"])),
             ("geo_apply no pixels", lambda: ops.geo_apply((None, lab["ok"], None), table["ok"], cfgs["geo"])),
             ("geo_scores", lambda: ops.geo_scores(scores["ok"], table["ok"], 2, 2)),
             ("geo_scores B=1.5", lambda: ops.geo_scores(scores["ok"], table["ok"], 1.5, 2)),
             ("geo_scores g=True", lambda: ops.geo_scores(scores["ok"], table["ok"], 2, True)),
             ("geo_scores out of 3", lambda: ops.geo_scores(scores["ok"], table["ok"], 2, 2, out=(None, None, None))),
             ("geo_scores scores list", lambda: ops.geo_scores([1.0], table["ok"], 2, 2)),
             ("_geo_config rotate 4", lambda: ops._geo_config(ops.GeoConfig(rotate=4.0, scale_lo=1.0, scale_hi=1.0), "x")),
             ("_geo_config scale nan", lambda: ops._geo_config(ops.GeoConfig(scale_lo=nan, scale_hi=1.0), "x")),
             ("_geo_config thresholds", lambda: ops._geo_config(ops.GeoConfig(warp_thr=(1 << 24) + 1, scale_lo=1.0, scale_hi=1.0), "x")),
             ("_geo_config fine", lambda: ops._geo_config(ops.GeoConfig(scale_lo=1.0, scale_hi=1.0), "x"))]
    for name, fn in calls:
        emit(f"ops.{name} on host tensors -> {raised(fn)}")

    # the eleven entry points: pointers that are never followed; every call carries a refusal
    p, big = 0x1000, 0x40000000
    acfg, mcfg, scfg, gcfg = (C.addressof(cfgs[k]) for k in ("aug", "mix", "strong", "geo"))
    norm = C.addressof(aug.norm)

    def sweep(name, args, null, bad):
        """args: name -> valid value, in the entry point's order.  null: the arguments that may not be NULL; bad: overrides, each
        of which must be refused.  NULL is tried on top of a bad shape: NULL comes first."""
        f = ops._fn(name)
        first_bad = bad[0]
        for n in null:
            emit(f"{name}({n}=NULL, {first_bad}) -> {f(*{**args, **first_bad, n: None}.values())}")
        for b in bad:
            emit(f"{name}({b}) -> {f(*{**args, **b}.values())}")

    sweep("lc2is_aug_params", dict(slots=p, keys=p, B=2, epoch=p, desc=p, n_images=3, cfg=acfg, params=p, stream=None),
          ("slots", "epoch", "desc", "cfg", "params"), [dict(B=0), dict(B=-1), dict(n_images=0)])
    sweep("lc2is_aug_apply", dict(img=p, img_bytes=64, lab=p, lab_bytes=64, desc=big, n_images=3, slots=p, params=p, B=2, S=16, L=4, norm=norm, pad=0, out_img=2 * big,
                                  out_lab=3 * big, stream=None),
          ("img", "lab", "desc", "slots", "params", "norm", "out_img", "out_lab"),
          [dict(B=0), dict(B=65536), dict(n_images=0), dict(S=0), dict(S=8192), dict(S=18), dict(L=0), dict(L=5), dict(out_img=2 * big + 4), dict(out_lab=3 * big + 4),
           dict(params=p + 2), dict(desc=big + 4)])
    sweep("lc2is_aug_crop_select", dict(lab=p, lab_bytes=64, desc=big, n_images=3, slots=p, keys=p, B=2, epoch=p, cfg=acfg, params=p, L=4, ratio=768, ignore=0, tries=10, info=p,
                                        stream=None),
          ("lab", "desc", "slots", "epoch", "cfg", "params"),
          [dict(B=0), dict(n_images=0), dict(L=0), dict(L=5), dict(ratio=0), dict(ratio=1024), dict(ignore=-2), dict(ignore=256), dict(tries=0), dict(tries=11),
           dict(params=p + 2), dict(info=p + 2), dict(desc=big + 4)])
    sweep("lc2is_label_histogram", dict(lab=p, lab_bytes=64, desc=big, n_images=3, slots=p, B=2, counts=p, stream=None), ("lab", "desc", "slots", "counts"),
          [dict(B=0), dict(n_images=0), dict(counts=p + 2), dict(desc=big + 4)])
    sweep("lc2is_mix_select", dict(src_lab=big, Bs=2, src_index=p, keys=p, B=2, epoch=p, cfg=mcfg, L=4, plan=p, info=p, stream=None),
          ("src_lab", "keys", "epoch", "cfg", "plan", "info"),
          [dict(B=0), dict(Bs=0), dict(L=0), dict(L=4097), dict(src_lab=big + 4), dict(keys=p + 4), dict(src_index=p + 4), dict(plan=p + 2), dict(info=p + 2), dict(epoch=p + 2)])
    npx, nlab, npw = 2 * 3 * 16 * 16 * 4, 2 * 4 * 4 * 8, 2 * 4 * 4 * 4
    sweep("lc2is_mix_apply", dict(dst_px=big, dst_lab=2 * big, dst_pw=3 * big, src_px=4 * big, src_lab=5 * big, src_pw=6 * big, Bs=2, plan=p, B=2, S=16, L=4, out_px=7 * big,
                                  out_lab=8 * big, out_pw=9 * big, stream=None),
          ("dst_px", "dst_lab", "src_px", "src_lab", "plan", "out_px", "out_lab", "out_pw"),
          [dict(B=0), dict(B=65536), dict(Bs=0), dict(S=0), dict(S=18), dict(S=8192), dict(L=0), dict(L=5), dict(dst_px=big + 4), dict(src_lab=5 * big + 4), dict(out_pw=9 * big + 2),
           dict(plan=p + 2), dict(out_px=big), dict(out_px=big + npx - 16), dict(out_px=4 * big - npx + 16), dict(out_lab=2 * big), dict(out_lab=5 * big + nlab - 8),
           dict(out_pw=3 * big), dict(out_pw=6 * big - npw + 4)])
    sweep("lc2is_strong_params", dict(keys=p, B=2, epoch=p, cfg=scfg, params=p, stream=None), ("keys", "epoch", "cfg", "params"),
          [dict(B=0), dict(keys=p + 4), dict(epoch=p + 2), dict(params=p + 2)])
    sweep("lc2is_strong_apply", dict(inp=big, params=p, cfg=scfg, B=2, S=16, out=2 * big, stream=None), ("inp", "params", "cfg", "out"),
          [dict(B=0), dict(B=65536), dict(S=8), dict(S=18), dict(S=8192), dict(inp=big + 8), dict(out=2 * big + 4), dict(params=p + 2), dict(out=big), dict(out=big + npx - 16),
           dict(out=big - npx + 16)])
    sweep("lc2is_geo_params", dict(keys=p, B=2, epoch=p, cfg=gcfg, params=p, stream=None), ("keys", "epoch", "cfg", "params"),
          [dict(B=0), dict(keys=p + 4), dict(epoch=p + 2), dict(params=p + 2)])
    sweep("lc2is_geo_apply", dict(in_px=big, in_lab=2 * big, in_pw=3 * big, params=p, cfg=gcfg, B=2, S=16, L=4, out_px=4 * big, out_lab=5 * big, out_pw=6 * big, stream=None),
          ("in_px", "params", "cfg", "out_px", "out_lab", "out_pw"),
          [dict(B=0), dict(B=65536), dict(S=4), dict(S=18), dict(S=8192), dict(L=0), dict(L=5), dict(in_px=big + 8), dict(out_lab=5 * big + 4), dict(in_pw=3 * big + 2), dict(params=p + 2),
           dict(out_px=big), dict(out_px=big + npx - 16), dict(out_px=big - npx + 16), dict(out_lab=2 * big), dict(out_lab=2 * big + nlab - 8), dict(out_pw=3 * big),
           dict(out_pw=3 * big - npw + 4)])
    bad_geo = ops.GeoConfig(rotate=4.0, scale_lo=1.0, scale_hi=1.0)
    emit(f"lc2is_geo_params(cfg out of range) -> {ops._fn('lc2is_geo_params')(p, 2, p, C.addressof(bad_geo), p, None)}")
    emit(f"lc2is_geo_apply(cfg out of range) -> {ops._fn('lc2is_geo_apply')(big, None, None, p, C.addressof(bad_geo), 2, 16, 4, 4 * big, None, None, None)}")
    bad_mix = ops.MixConfig(mode=7, n_classes=151, area_lo1024=256, area_hi1024=512)
    emit(f"lc2is_mix_select(mode 7, B=0) -> {ops._fn('lc2is_mix_select')(big, 2, None, p, 0, p, C.addressof(bad_mix), 4, p, p, None)}")
    nsc = 2 * 4 * 4 * 16 * 4
    sweep("lc2is_geo_scores", dict(sc=big, tw=3 * big, params=p, B=2, g=4, ld=16, L=8, want=1, out_sc=2 * big, out_tw=4 * big, stream=None), ("sc", "params", "out_sc", "out_tw"),
          [dict(B=0), dict(B=65536), dict(g=0), dict(g=513), dict(ld=0), dict(ld=18), dict(ld=1028), dict(L=0), dict(L=6), dict(L=4100), dict(sc=big + 8), dict(out_sc=2 * big + 4),
           dict(tw=3 * big + 2), dict(params=p + 2), dict(out_sc=big), dict(out_sc=big + nsc - 16), dict(out_sc=big - nsc + 16), dict(out_tw=3 * big), dict(want=0, out_sc=big)])


# ---- digests on the device ----------------------------------------------------------------------------------------------------
def _sha(torch, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"<none>")
        else:
            h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:20]


def digest(torch, emit):
    import geo_ref as GR
    import strong_ref as SR
    from lc2is_amd import ops
    from lc2is_amd.data import DeviceImagePool, GeometricAugment, SampleMix, StrongAugment, TrainAugment
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    gen = torch.Generator().manual_seed(2024)

    def refused(what, fn):
        emit(f"{what} -> {raised(fn)}")

    # ---- augmenter, crop re-draw, label histogram ----
    shapes = [(5, 7), (37, 23), (64, 64)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    labels = [rng.integers(0, 6, (h, w), dtype=np.uint8) for h, w in shapes]
    labels[2][:, :40] = 3                                         # a dominant class: the re-draw has something to refuse
    pool = DeviceImagePool.from_arrays(images, labels, device=dev, chunk_bytes=4096)
    idx = torch.tensor([0, 1, 2, 7, 2, 1], dtype=torch.int64, device=dev)      # slot 7 is out of range
    epoch = torch.tensor([3], dtype=torch.int32, device=dev)
    emit(f"label_histogram | counts={_sha(torch, ops.label_histogram(pool.labels, pool.desc, idx))} class_counts={_sha(torch, pool.class_counts())}")
    for L in (4, 16):
        for ratio in ((0.25, 0.5), (1.0, 2.0)):                  # the resized image leaves padding rows / fills the crop
            for flip in (0.0, 1.0):
                aug = TrainAugment(crop_size=16, label_size=L, base_size=16, ratio_range=ratio, flip_prob=flip, seed=11)
                params = ops.aug_params(idx, epoch, pool.desc, aug.config)
                px, lb = ops.aug_apply(pool.images, pool.labels, pool.desc, idx, params, 16, L, aug.norm, pad_label=255)
                emit(f"augment L={L} ratio={ratio} flip={flip} | params={_sha(torch, params)} pixels={_sha(torch, px)} labels={_sha(torch, lb)}")
                for tries in (1, 10):
                    for ignore in (-1, 3):
                        p2 = params.clone()
                        info = ops.aug_crop_select(pool.labels, pool.desc, idx, epoch, aug.config, p2, L, ratio1024=512, ignore_label=ignore, tries=tries)
                        emit(f"crop_select L={L} ratio={ratio} flip={flip} tries={tries} ignore={ignore} | params={_sha(torch, p2)} info={_sha(torch, info)}")
    aug = TrainAugment(crop_size=16, label_size=4, base_size=24, seed=5, cat_max_ratio=0.75)
    out = aug(pool, [0, 1, 2, 1], 2)
    emit(f"TrainAugment pool form | pixels={_sha(torch, out['pixel_values'])} labels={_sha(torch, out['label'])} info={_sha(torch, aug.last_crop_info)}")
    out = aug(images=images, labels=labels, indices=[0, 1, 2], epoch=2)
    emit(f"TrainAugment streaming form | pixels={_sha(torch, out['pixel_values'])} labels={_sha(torch, out['label'])}")
    refused("aug_apply params of 19 words", lambda: ops.aug_apply(pool.images, pool.labels, pool.desc, idx, torch.zeros(6, 19, dtype=torch.int32, device=dev), 16, 4, aug.norm))
    refused("aug_apply S=18", lambda: ops.aug_apply(pool.images, pool.labels, pool.desc, idx, torch.zeros(6, 20, dtype=torch.int32, device=dev), 18, 6, aug.norm))
    refused("aug_params 5 keys for 6", lambda: ops.aug_params(idx, epoch, pool.desc, aug.config, keys=idx[:5]))
    refused("aug_params host epoch", lambda: ops.aug_params(idx, epoch.cpu(), pool.desc, aug.config))
    refused("aug_crop_select tries=11", lambda: ops.aug_crop_select(pool.labels, pool.desc, idx, epoch, aug.config, torch.zeros(6, 20, dtype=torch.int32, device=dev), 4,
                                                                     ratio1024=512, tries=11))
    refused("label_histogram out int64", lambda: ops.label_histogram(pool.labels, pool.desc, idx, out=torch.zeros(6, 256, dtype=torch.int64, device=dev)))

    # ---- mix ----
    def batch(n, S, L, with_pw, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(n, 3, S, S, generator=g).to(dev), torch.randint(-1, 8, (n, L, L), generator=g).to(dev),
                torch.rand(n, L, L, generator=g).to(dev) if with_pw else None)

    keys = torch.tensor([10, 11, 12], dtype=torch.int64, device=dev)
    for S, L in ((16, 4), (12, 4), (16, 16), (8, 8)):             # r = 4: the QUAD kernel; r = 3: quads straddle cells; L = S
        for mode in ("none", "classmix", "cutmix"):
            for dst_pw, src_pw in ((True, True), (False, True), (True, False)):
                dst, src = batch(3, S, L, dst_pw, 1), batch(2, S, L, src_pw, 2)      # Bs != B
                mix = SampleMix(mode, n_classes=7, ignore_index=-1, exclude_label=0, seed=9)
                src_index = torch.tensor([1, 5, 0], dtype=torch.int64, device=dev)       # row 5 lies outside the source
                plan, info = ops.mix_select(src[1], keys, epoch, mix.config, src_index=src_index)
                o = ops.mix_apply(dst, src, plan)
                emit(f"mix S={S} L={L} {mode} pw=({int(dst_pw)}, {int(src_pw)}) | plan={_sha(torch, plan)} info={_sha(torch, info)} pixels={_sha(torch, o[0])} "
                     f"labels={_sha(torch, o[1])} weights={_sha(torch, o[2])}")
        dst = batch(3, S, L, True, 1)
        o = SampleMix("classmix", n_classes=7, seed=9)(dst, dst, [4, 5, 6], 1, src_index=[1, 2, 0])
        emit(f"SampleMix within the batch S={S} L={L} | {_sha(torch, *o)}")
    dst, src = batch(3, 16, 4, True, 1), batch(2, 16, 4, True, 2)
    plan, _ = ops.mix_select(src[1], keys, epoch, SampleMix("cutmix", seed=9).config)
    refused("mix_apply out pixels = dst pixels", lambda: ops.mix_apply(dst, src, plan, out=(dst[0], torch.empty_like(dst[1]), torch.empty_like(dst[2]))))
    refused("mix_apply out weights = src weights' tail", lambda: ops.mix_apply(dst, (src[0], src[1], torch.zeros(5, 4, 4, device=dev)[3:]), plan,
                                                                              out=(torch.empty_like(dst[0]), torch.empty_like(dst[1]), torch.zeros(5, 4, 4, device=dev)[:3])))
    refused("mix_apply plan of 39 words", lambda: ops.mix_apply(dst, src, plan[:, :39].contiguous()))
    refused("mix_apply L mismatch", lambda: ops.mix_apply(dst, batch(2, 16, 8, True, 2), plan))
    refused("mix_apply strided pixels", lambda: ops.mix_apply((dst[0].transpose(2, 3), dst[1], dst[2]), src, plan))
    refused("mix_select 2 keys, 3 source rows", lambda: ops.mix_select(src[1], keys[:2], epoch, SampleMix(seed=9).config, src_index=torch.zeros(3, dtype=torch.int64, device=dev)))

    # ---- strong ----
    M = np.array([[0.9, 0.2, -0.1], [0.05, 1.1, 0.0], [-0.2, 0.1, 1.3]])
    rows = [SR.make_row(flags, R, 0.25 * R + 0.2, M if flags & 1 else None, (9.0, -14.0, 3.0) if flags & 1 else None) for flags in range(8) for R in range(9)]
    bad = SR.make_row(5, 8, 2.0, M)
    bad[0], bad[1] = 13, 9                                        # an unknown flag bit and R = 9: the row is a copy
    rows.append(bad)
    table = torch.from_numpy(np.stack(rows)).to(dev)
    strong = StrongAugment(seed=3)
    for S in (12, 68):                                            # 68: ragged tiles in both directions
        x = torch.randn(len(rows), 3, S, S, generator=gen).to(dev)
        y = ops.strong_apply(x, table, strong.config)
        emit(f"strong S={S} hand-written rows | out={_sha(torch, y)} per-row={' '.join(_sha(torch, r)[:8] for r in y)}")
        k = torch.arange(len(rows), dtype=torch.int64, device=dev)
        y = strong(x, k, epoch)
        emit(f"StrongAugment S={S} | params={_sha(torch, strong.last_params)} out={_sha(torch, y)}")
    x = torch.randn(2, 3, 12, 12, generator=gen).to(dev)
    refused("strong_apply in place", lambda: ops.strong_apply(x, table[:2].contiguous(), strong.config, out=x))
    refused("strong_apply S=8", lambda: ops.strong_apply(torch.zeros(2, 3, 8, 8, device=dev), table[:2].contiguous(), strong.config))
    refused("strong_apply S=14", lambda: ops.strong_apply(torch.zeros(2, 3, 14, 14, device=dev), table[:2].contiguous(), strong.config))
    refused("strong_apply params of 3 rows", lambda: ops.strong_apply(x, table[:3].contiguous(), strong.config))
    refused("strong_apply unaligned base", lambda: ops.strong_apply(torch.zeros(2 * 3 * 144 + 1, device=dev)[1:].view(2, 3, 12, 12), table[:2].contiguous(), strong.config))
    refused("strong_apply permuted", lambda: ops.strong_apply(x.permute(0, 1, 3, 2), table[:2].contiguous(), strong.config))
    refused("strong_params out of 31 words", lambda: ops.strong_params(keys, epoch, strong.config, out=torch.zeros(3, 31, dtype=torch.int32, device=dev)))
    refused("StrongAugment 2 keys for 3", lambda: strong(torch.zeros(3, 3, 12, 12, device=dev), [1, 2], 0))

    # ---- geo and the score warp ----
    out_of_range = GR.affine_row(10.0)
    out_of_range[GR.M0 + 1] = 2 ** 20                             # a matrix word out of range: the row is a copy
    grows = [GR.make_row(0), GR.make_row(GR.FLIP, (-GR.ONE, 0, 0, GR.ONE)), GR.affine_row(90.0), GR.affine_row(10.0), GR.affine_row(45.0, 0.8), GR.affine_row(0.0, 0.25),
             GR.affine_row(0.0, 1.0, 0.0, 0.5, -0.5), GR.affine_row(-33.0, 1.3, 12.0, 0.07, -0.11, flip=True), out_of_range]
    gtable = torch.from_numpy(np.stack(grows)).to(dev)
    n = len(grows)
    geo = GeometricAugment(rotate_deg=30.0, scale_range=(0.5, 2.0), shear_deg=10.0, translate=0.2, flip_prob=0.5, fill=(10, 20, 30), seed=4)
    for S in (8, 36, 68):
        x = torch.randn(n, 3, S, S, generator=gen).to(dev)
        for L in (S, S // 4, None):
            lb = None if L is None else torch.randint(0, 9, (n, L, L), generator=gen).to(dev)
            w = None if L is None else torch.rand(n, L, L, generator=gen).to(dev)
            for batch3 in ((x, lb, w), (x, lb, None), (x, None, w)) if L else ((x, None, None),):
                o = ops.geo_apply(batch3, gtable, geo.config)
                emit(f"geo S={S} L={L} maps=({int(batch3[1] is not None)}, {int(batch3[2] is not None)}) | pixels={_sha(torch, o[0])} labels={_sha(torch, o[1])} "
                     f"weights={_sha(torch, o[2])} per-row={' '.join(_sha(torch, r)[:8] for r in o[0])}")
        o = geo((x, None, None), list(range(n)), epoch)
        emit(f"GeometricAugment S={S} | params={_sha(torch, geo.last_params)} pixels={_sha(torch, o[0])}")
    for g in (1, 3, 8):
        for ld in (4, 12, 152):
            sc = torch.randn(n * g * g, ld, generator=gen).to(dev)
            for L in (g, 4 * g):
                tw = torch.rand(n, L, L, generator=gen).to(dev)
                a, b, c = ops.geo_scores(sc, gtable, n, g), ops.geo_scores(sc, gtable, n, g, label_size=L), ops.geo_scores(sc, gtable, n, g, teacher_weight=tw)
                emit(f"geo_scores g={g} ld={ld} L={L} | scores={_sha(torch, a[0])} none={a[1] is None} mask={_sha(torch, b[1])} weights={_sha(torch, c[1])} "
                     f"same scores={_sha(torch, a[0]) == _sha(torch, b[0]) == _sha(torch, c[0])}")
    x = torch.randn(3, 3, 16, 16, generator=gen).to(dev)
    lb, w = torch.zeros(3, 4, 4, dtype=torch.int64, device=dev), torch.zeros(3, 4, 4, device=dev)
    inputs_g, labels_g, pw_g, scores_g, tw_g = geo.view_distill(dict(pixel_values=x), lb, torch.randn(3 * 4, 8, generator=gen).to(dev), [7, 8, 9], epoch, pixel_weight=w)
    emit(f"GeometricAugment.view_distill | {_sha(torch, inputs_g['pixel_values'], labels_g, pw_g, scores_g, tw_g)}")
    t3 = gtable[:3].contiguous()
    refused("geo_apply in place", lambda: ops.geo_apply((x, lb, w), t3, geo.config, out=(x, None, None)))
    refused("geo_apply out labels = labels", lambda: ops.geo_apply((x, lb, w), t3, geo.config, out=(None, lb, None)))
    refused("geo_apply S=4", lambda: ops.geo_apply((torch.zeros(3, 3, 4, 4, device=dev), None, None), t3, geo.config))
    refused("geo_apply L=3", lambda: ops.geo_apply((x, torch.zeros(3, 3, 3, dtype=torch.int64, device=dev), None), t3, geo.config))
    refused("geo_apply labels and weights of two L", lambda: ops.geo_apply((x, lb, torch.zeros(3, 8, 8, device=dev)), t3, geo.config))
    refused("geo_apply strided labels", lambda: ops.geo_apply((x, lb.transpose(1, 2), None), t3, geo.config))
    refused("geo_apply params of 2 rows", lambda: ops.geo_apply((x, lb, w), gtable[:2].contiguous(), geo.config))
    refused("geo_apply params int64", lambda: ops.geo_apply((x, lb, w), t3.long(), geo.config))
    refused("geo_apply out pixels of another shape", lambda: ops.geo_apply((x, lb, w), t3, geo.config, out=(torch.zeros(3, 3, 16, 12, device=dev), None, None)))
    refused("geo_params host keys", lambda: ops.geo_params(keys.cpu(), epoch, geo.config))
    refused("geo_params two epochs", lambda: ops.geo_params(keys, torch.zeros(2, dtype=torch.int32, device=dev), geo.config))
    sc = torch.randn(3 * 4, 8, generator=gen).to(dev)
    refused("geo_scores in place", lambda: ops.geo_scores(sc, t3, 3, 2, out=(sc, None)))
    refused("geo_scores out weight = teacher_weight", lambda: ops.geo_scores(sc, t3, 3, 2, teacher_weight=w, out=(None, w)))
    refused("geo_scores out weight without a size", lambda: ops.geo_scores(sc, t3, 3, 2, out=(None, w)))
    refused("geo_scores L=3 for g=2", lambda: ops.geo_scores(sc, t3, 3, 2, label_size=3))
    refused("geo_scores label_size against teacher_weight", lambda: ops.geo_scores(sc, t3, 3, 2, teacher_weight=w, label_size=8))
    refused("geo_scores ld=6", lambda: ops.geo_scores(torch.zeros(12, 6, device=dev), t3, 3, 2))
    refused("geo_scores rows for another B", lambda: ops.geo_scores(sc, t3, 2, 2))
    refused("geo_scores host params", lambda: ops.geo_scores(sc, t3.cpu(), 3, 2))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--validate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.root).resolve()))
    import torch

    import lc2is_amd
    assert Path(lc2is_amd.__file__).resolve().is_relative_to(Path(a.root).resolve()), lc2is_amd.__file__
    out = open(a.out, "w") if a.out else None
    h, n = hashlib.sha256(), 0

    def emit(line):
        nonlocal n
        h.update(line.encode() + b"\n")
        n += 1
        print(line, file=out or sys.stdout)

    (validate if a.validate else digest)(torch, emit)
    if out:
        out.close()
    print(f"sha256 {h.hexdigest()} {n} lines")


if __name__ == "__main__":
    main()
