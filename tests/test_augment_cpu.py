"""Host side of the device augmentation (lc2is_amd/data/augment.py), no GPU: the numpy restatement the GPU tests compare the
kernels with (tests/augment_ref.py) is itself pinned to torch's fp64 F.interpolate + pad + crop + flip, the restated draw has
the statistics it should have, and the pool packing, argument checks and epoch permutation are host logic."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R

SEED = 20240229      # fixed: the restatement is deterministic, so the statistics below either hold for this seed or do not


def _cfg(**kw):
    from lc2is_amd.data import TrainAugment
    return R.config_dict(TrainAugment(**kw).config)


@pytest.mark.parametrize("case", range(12))
def test_restated_sampling_matches_torch_fp64(case):
    """bilinear align_corners=False resize to (nh, nw) + zero pad + crop + flip for the image (<= 1e-9), nearest-exact resize
    subsampled at [q//2::q] for the labels (equal), 12 random geometries: H, W in 20..60, S = 32, L = 8.
    One correction of the reference: torch evaluates nearest-exact's floor((x + 0.5) * n_in / n_out) with an fp32 scale also for
    fp64 data, so where that product is EXACTLY an integer (case 10: 58 -> 55 columns at x = 27 gives 29.0) it lands on
    28.999998 and takes the pixel before.  The definition here is the exact rational floor; torch's source index is taken from
    torch (resizing an arange) and replaced by the exact quotient at those ties only, and it is asserted that ties are the only
    places where the two differ."""
    rng = np.random.default_rng(100 + case)
    S, L = 32, 8
    q = S // L
    H, W = (int(v) for v in rng.integers(20, 61, 2))
    nh, nw = (int(v) for v in rng.integers(12, 97, 2))
    top, left = int(rng.integers(0, max(nh - S, 0) + 1)), int(rng.integers(0, max(nw - S, 0) + 1))
    flip = case % 2
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, 151, (H, W), dtype=np.uint8)
    out, labels = R.apply_ref(img, lab, nh, nw, top, left, flip, np.eye(3), np.zeros(3), S, L, (0, 0, 0), (1, 1, 1), pad_label=255)
    x = F.interpolate(torch.from_numpy(img).double().permute(2, 0, 1)[None], size=(nh, nw), mode="bilinear", align_corners=False)[0]
    x = F.pad(x, (0, max(left + S - nw, 0), 0, max(top + S - nh, 0)))[:, top:top + S, left:left + S] / 255.0
    src = []
    for n_in, n_out in ((H, nh), (W, nw)):
        t = F.interpolate(torch.arange(n_in).double().reshape(1, 1, 1, n_in), size=(1, n_out), mode="nearest-exact").reshape(-1).long()
        num = (2 * torch.arange(n_out) + 1) * n_in
        tie = num % (2 * n_out) == 0
        assert torch.equal(t[~tie], (num // (2 * n_out))[~tie])
        src.append(torch.where(tie, num // (2 * n_out), t))
    y = torch.from_numpy(lab).double()[src[0]][:, src[1]]
    y = F.pad(y, (0, max(left + S - nw, 0), 0, max(top + S - nh, 0)), value=255.0)[top:top + S, left:left + S]
    if flip:
        x, y = x.flip(-1), y.flip(-1)
    err = float((torch.from_numpy(out) - x).abs().max())
    print(f"case {case}: {H}x{W} -> {nh}x{nw} crop@({top},{left}) flip={flip}: max |restatement - torch fp64| = {err:.3e}")
    assert err <= 1e-9
    assert np.array_equal(labels, y[q // 2::q, q // 2::q].long().numpy())


@pytest.fixture(scope="module")
def draws():
    idx, ep = np.meshgrid(np.arange(4096, dtype=np.int64), np.arange(16, dtype=np.int64), indexing="ij")
    H, W = np.full(idx.size, 683), np.full(idx.size, 512)
    p = R.draw_params(_cfg(seed=SEED), H, W, idx.reshape(-1), ep.reshape(-1))
    return {k: v.reshape(4096, 16, *v.shape[1:]) for k, v in p.items()}


def test_restated_draw_statistics(draws):
    """65 536 (index, epoch) keys: flip rate 0.5 +- 4 sigma, the ratio uniform over its 1537 values (16 bins, each within 4 sigma
    of its share), top reaches both ends of its range."""
    n = 65536
    flips = draws["flip"].mean()
    print(f"flip rate {flips:.5f}")
    assert abs(flips - 0.5) <= 4 * 0.5 / np.sqrt(n)                          # 0.0078
    r = draws["ratio1024"].reshape(-1)
    assert r.min() >= 512 and r.max() <= 2048
    share = np.bincount((np.arange(1537) * 16) // 1537, minlength=16) / 1537.0
    got = np.bincount(((r - 512) * 16) // 1537, minlength=16)
    z = (got - n * share) / np.sqrt(n * share * (1 - share))
    print("ratio histogram z-scores:", np.round(z, 2))
    assert np.abs(z).max() <= 4.0
    nh, top = draws["nh"].reshape(-1), draws["top"].reshape(-1)
    assert ((top >= 0) & (top <= np.maximum(nh - 512, 0))).all()
    big = nh > 512 + 8
    assert (top[big] == 0).any() and (top[big] == (nh - 512)[big]).any()
    assert (draws["top"][draws["nh"] <= 512] == 0).all()


def test_restated_draws_are_uncorrelated_between_neighbouring_keys(draws):
    """Consecutive dataset indices and consecutive epochs: |correlation| < 0.02 for every drawn quantity (1/sqrt(61440) = 0.004)."""
    for name in ("ratio1024", "top", "left", "flip"):
        x = draws[name].astype(np.float64)
        for what, a, b in (("index", x[:-1], x[1:]), ("epoch", x[:, :-1], x[:, 1:])):
            c = np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]
            print(f"{name}: correlation between consecutive {what} values {c:+.4f}")
            assert abs(c) < 0.02, (name, what, c)
    hue = draws["M"][..., 0, 1]                                              # a colour field, across indices
    assert abs(np.corrcoef(hue[:-1].reshape(-1), hue[1:].reshape(-1))[0, 1]) < 0.02


def test_draw_depends_on_seed_epoch_and_the_high_word_of_the_index():
    H, W = np.full(64, 300), np.full(64, 400)
    k = np.arange(64, dtype=np.int64)
    base = R.param_rows(R.draw_params(_cfg(seed=1), H, W, k, 0))
    assert np.array_equal(base, R.param_rows(R.draw_params(_cfg(seed=1), H, W, k, 0)))
    for other in (R.draw_params(_cfg(seed=2), H, W, k, 0), R.draw_params(_cfg(seed=1 + (1 << 32)), H, W, k, 0),
                  R.draw_params(_cfg(seed=1), H, W, k, 1), R.draw_params(_cfg(seed=1), H, W, k + (1 << 32), 0)):
        assert (R.param_rows(other) != base).any(axis=1).mean() > 0.9
    ident = R.draw_params(_cfg(seed=1, photometric=False), H, W, k, 0)
    assert (ident["M"] == np.eye(3)).all() and (ident["o"] == 0).all()
    assert np.array_equal(ident["nh"], R.draw_params(_cfg(seed=1), H, W, k, 0)["nh"])   # the geometry does not depend on the colour


def test_pool_packing_offsets_and_alignment():
    from lc2is_amd.data.augment import ALIGN, pack_offsets
    shapes = [(17, 4096), (64, 64), (1, 1), (683, 512), (16, 16)]
    io, lo, img_end, lab_end = pack_offsets(shapes)
    assert ALIGN == 256 and io[0] == lo[0] == 0
    for k, (h, w) in enumerate(shapes):
        assert io[k] % ALIGN == 0 and lo[k] % ALIGN == 0
        nxt_i, nxt_l = (io[k + 1], lo[k + 1]) if k + 1 < len(shapes) else (img_end, lab_end)
        assert 0 <= nxt_i - (io[k] + 3 * h * w) < ALIGN and 0 <= nxt_l - (lo[k] + h * w) < ALIGN   # no overlap, no wasted block
    assert io[2] == io[1] + 64 * 64 * 3 and io[3] == io[2] + 256          # a multiple of 256 packs tight; 3 bytes take a block
    io2, lo2, _, _ = pack_offsets([(5, 5)], img_start=img_end, lab_start=lab_end)   # appending continues where the pool ends
    assert io2 == [img_end] and lo2 == [lab_end]
    assert pack_offsets([(5, 5)], img_start=3, lab_start=257)[:2] == ([256], [512])


def test_argument_errors():
    from lc2is_amd.data import AugmentedBatches, DeviceImagePool, TrainAugment
    img, lab = np.zeros((8, 12, 3), np.uint8), np.zeros((8, 12), np.uint8)
    assert DeviceImagePool.check(img, lab) == (8, 12)
    assert DeviceImagePool.check(torch.from_numpy(img), torch.from_numpy(lab)) == (8, 12)
    with pytest.raises(TypeError):
        DeviceImagePool.check(img.astype(np.float32), lab)
    with pytest.raises(TypeError):
        DeviceImagePool.check(img, lab.astype(np.int64))
    with pytest.raises(ValueError, match="label shape"):
        DeviceImagePool.check(img, np.zeros((8, 11), np.uint8))
    with pytest.raises(ValueError, match="3 channels"):
        DeviceImagePool.check(np.zeros((8, 12, 4), np.uint8), lab)
    with pytest.raises(ValueError, match="4096"):
        DeviceImagePool.check(np.zeros((1, 4097, 3), np.uint8), np.zeros((1, 4097), np.uint8))
    with pytest.raises(ValueError, match="multiple of label_size"):
        TrainAugment(crop_size=32, label_size=5)
    with pytest.raises(ValueError, match="multiple of 4"):
        TrainAugment(crop_size=30, label_size=5)
    with pytest.raises(ValueError):
        TrainAugment(flip_prob=1.5)
    with pytest.raises(ValueError, match="unknown photometric"):
        TrainAugment(photometric=dict(gamma=2.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceImagePool(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceImagePool.from_arrays([img], [lab], device="cpu")

    class HostPool:
        device = torch.device("cpu")

    with pytest.raises(RuntimeError, match="no CPU path"):
        AugmentedBatches(HostPool(), TrainAugment(), 2, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TrainAugment()(HostPool(), [0], 0)


def test_config_struct_holds_the_documented_defaults():
    c = _cfg(seed=(7 << 32) | 5)
    assert (c["seed_lo"], c["seed_hi"], c["crop_size"], c["base_size"], c["ratio_lo1024"], c["ratio_hi1024"]) == (5, 7, 512, 512, 512, 2048)
    assert c["flip_thr"] == 1 << 23 and c["photo_thr"] == [1 << 23] * 4
    assert c["brightness_delta"] == 32.0 and (c["contrast_lo"], c["contrast_hi"], c["saturation_lo"], c["saturation_hi"]) == (0.5, 1.5, 0.5, 1.5)
    assert abs(c["hue_delta"] - np.deg2rad(36.0)) < 1e-7
    assert _cfg(photometric=False)["photo_thr"] == [0] * 4
    assert _cfg(photometric=dict(prob=(1.0, 0.0, 0.25, 0.5)))["photo_thr"] == [1 << 24, 0, 1 << 22, 1 << 23]


def test_epoch_permutation():
    from lc2is_amd.data import AugmentedBatches
    n, world = 1000, 4
    parts = [AugmentedBatches.epoch_indices(n, 11, 3, r, world) for r in range(world)]
    assert all(p.dtype == torch.int64 and p.numel() == n // world for p in parts)
    assert torch.equal(torch.cat(parts).sort().values, torch.arange(n))                       # disjoint and covers the epoch
    assert all(torch.equal(p, AugmentedBatches.epoch_indices(n, 11, 3, r, world)) for r, p in enumerate(parts))   # reproducible
    assert not torch.equal(parts[0], AugmentedBatches.epoch_indices(n, 11, 4, 0, world))      # another epoch, another order
    assert not torch.equal(parts[0], AugmentedBatches.epoch_indices(n, 12, 3, 0, world))      # another seed
    assert not torch.equal(parts[0], torch.arange(n)[0::world])                               # shuffled at all
    # strided: rank r takes every world-th entry of the one permutation
    whole = AugmentedBatches.epoch_indices(n, 11, 3, 0, 1)
    assert all(torch.equal(p, whole[r::world]) for r, p in enumerate(parts))
    odd = torch.cat([AugmentedBatches.epoch_indices(1003, 11, 3, r, world) for r in range(world)])
    assert odd.numel() == 1000 and odd.unique().numel() == 1000                               # cut to a multiple of world
