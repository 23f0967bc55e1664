"""Device augmentation (lc2is_amd/csrc/augment.hip, lc2is_amd/data/augment.py) on the MI355X against its numpy restatement
(tests/augment_ref.py, pinned to torch's fp64 F.interpolate in tests/test_augment_cpu.py): the parameter draw, the fused
resize / crop / flip / colour / normalise launch, and the properties the loader relies on: a sample's bits do not depend on its
batch, everything is reproducible, the streaming form equals the pool form, the two launches replay from a graph, and
AugmentedBatches feeds TrainStep.step without a host synchronisation."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
# Image tolerance, absolute in normalised units.  The taps are the restatement's by construction (integer coordinates); the fp32
# weight rem * rcp(2n) is within 2.5 ulp of the quotient; about 12 fp32 operations (three lerps, the 3 x 3 colour product with
# its offset, the clamp's operands, the scale and the normalisation) act on magnitudes <= 1020, which is <= 3e-4 in pixel units,
# or 5e-6 after / 255 / 0.26; times a margin of 4.
IMAGE_TOL = 2e-5


def _noise(shapes, seed):
    rng = np.random.default_rng(seed)
    return ([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes],
            [rng.integers(0, 151, (h, w), dtype=np.uint8) for h, w in shapes])


def _pool(shapes, seed, dev):
    from lc2is_amd.data import DeviceImagePool
    imgs, labs = _noise(shapes, seed)
    return DeviceImagePool.from_arrays(imgs, labs, device=dev), imgs, labs


def _norm():
    from lc2is_amd.data import TrainAugment
    return TrainAugment().norm


def _ref_batch(imgs, labs, slots, rows, S, L, pad_label=0):
    """apply_ref for every row of an int32 [B, 20] table (numpy), colour fields read back as the fp32 the kernel reads."""
    px, lb = [], []
    for b, k in enumerate(slots):
        r = rows[b]
        M = r[R.M0:R.M0 + 9].view(np.float32).astype(np.float64).reshape(3, 3)
        o = r[R.O0:R.O0 + 3].view(np.float32).astype(np.float64)
        a, c = R.apply_ref(imgs[k], labs[k], r[R.NH], r[R.NW], r[R.TOP], r[R.LEFT], r[R.FLIP], M, o, S, L, MEAN, STD, pad_label)
        px.append(a); lb.append(c)
    return np.stack(px), np.stack(lb)


def test_params_match_the_restatement(dev):
    """4096 keys over 64 images of mixed sizes (portrait, landscape, square, sides 17..4096): integer fields equal, colour matrix
    and offset within 1e-5 * max(1, |x|) (fp32 sinf / cosf and three composed 3x3 products against fp64)."""
    from lc2is_amd import ops
    from lc2is_amd.data import TrainAugment
    from lc2is_amd.data.augment import _desc_rows, pack_offsets
    rng = np.random.default_rng(5)
    shapes = [(17, 4096), (4096, 17), (4096, 4096), (17, 17), (683, 512), (512, 683), (512, 512), (4096, 2048), (33, 4095)]
    shapes += [tuple(int(v) for v in rng.integers(17, 4097, 2)) for _ in range(64 - len(shapes))]
    io, lo, _, _ = pack_offsets(shapes)
    desc = _desc_rows(shapes, io, lo).to(dev)
    aug = TrainAugment(seed=0x1234567887654321)
    cfg = R.config_dict(aug.config)
    worst_m = worst_o = 0.0
    for epoch in (0, 1, 77, 2 ** 31 - 1):
        slots = rng.integers(0, 64, 1024)
        keys = np.where(rng.random(1024) < 0.5, rng.integers(0, 20210, 1024), rng.integers(0, 2 ** 62, 1024))
        got = ops.aug_params(torch.from_numpy(slots).to(dev), torch.tensor([epoch], dtype=torch.int32, device=dev), desc, aug.config,
                             keys=torch.from_numpy(keys).to(dev)).cpu().numpy()
        H, W = np.array([shapes[s][0] for s in slots]), np.array([shapes[s][1] for s in slots])
        ref = R.draw_params(cfg, H, W, keys, epoch)
        for word, name in ((R.NH, "nh"), (R.NW, "nw"), (R.TOP, "top"), (R.LEFT, "left"), (R.FLIP, "flip")):
            assert np.array_equal(got[:, word].astype(np.int64), ref[name]), name
        assert (got[:, 17:] == 0).all()
        M = got[:, R.M0:R.M0 + 9].view(np.float32).astype(np.float64).reshape(-1, 3, 3)
        o = got[:, R.O0:R.O0 + 3].view(np.float32).astype(np.float64)
        em = np.abs(M - ref["M"]) / np.maximum(1.0, np.abs(ref["M"]))
        eo = np.abs(o - ref["o"]) / np.maximum(1.0, np.abs(ref["o"]))
        worst_m, worst_o = max(worst_m, em.max()), max(worst_o, eo.max())
        assert 0.3 < (ref["flip"] == 1).mean() < 0.7 and (np.abs(ref["o"]).max(axis=1) > 0).mean() > 0.3   # the draw is not trivial
    print(f"aug_params: colour matrix error {worst_m:.3e}, offset error {worst_o:.3e} (scaled by max(1, |x|))")
    assert worst_m <= 1e-5 and worst_o <= 1e-5
    # slots default to the keys; a slot outside the table gives the all-zero row
    slots = torch.tensor([3, 64, -1, 5], dtype=torch.int64, device=dev)
    ep = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = ops.aug_params(slots, ep, desc, aug.config).cpu()
    assert torch.equal(rows[[0, 3]], ops.aug_params(slots[[0, 3]], ep, desc, aug.config, keys=slots[[0, 3]]).cpu())
    assert (rows[1] == 0).all() and (rows[2] == 0).all() and rows[0, 0] > 0


def _colour(c, b, s, h_deg):
    """(M, o) of contrast c after brightness b, then saturation s, then hue h: the kernel's order, in float64."""
    A = R.hue_matrix(np.deg2rad(h_deg))[0] @ R.saturation_matrix(s)[0]
    return c * A, A @ (c * b * np.ones(3))


IDENT = (np.eye(3), np.zeros(3))
BRIGHT, DARK = _colour(1.5, 32.0, 1.5, 36.0), _colour(0.5, -32.0, 0.5, -36.0)
SHAPES = [(40, 56), (97, 131), (64, 64), (17, 4096), (4096, 17), (200, 150)]
#        slot nh      nw      top     left   flip colour
CASES = [(0, 100, 140, 10, 30, 0, IDENT),            # upscaling
         (0, 100, 140, 36, 76, 1, BRIGHT),           # upscaling, flipped, crop at the bottom right border
         (1, 70, 95, 0, 0, 0, DARK),                 # downscaling, crop at the top left border
         (1, 70, 95, 6, 31, 1, IDENT),               # downscaling, crop at the bottom right border
         (1, 20, 160, 0, 50, 0, BRIGHT),             # resized image smaller than the crop in one axis
         (1, 150, 24, 40, 0, 1, DARK),               # ... in the other axis
         (2, 20, 24, 0, 0, 1, BRIGHT),               # ... in both
         (2, 64, 64, 0, 0, 0, IDENT),                # identity geometry
         (3, 512, 123362, 448, 60000, 0, BRIGHT),    # the 17 x 4096 image at base_size * 1.0
         (3, 1024, 246723, 960, 246659, 1, DARK),    # ... at * 2.0, crop at the far corner (the largest integers)
         (4, 246723, 1024, 0, 0, 0, IDENT),          # the 4096 x 17 image
         (4, 9, 1, 0, 0, 1, BRIGHT),                 # shrunk to one column
         (5, 37, 28, 0, 0, 0, DARK),                 # strong downscaling (every tap pair far apart)
         (5, 200, 150, 100, 43, 1, IDENT)]


def _case_rows(S):
    p = dict(nh=[], nw=[], top=[], left=[], flip=[], M=[], o=[])
    for _, nh, nw, top, left, flip, (M, o) in CASES:
        top, left = min(top, max(nh - S, 0)), min(left, max(nw - S, 0))      # the borders of the S = 64 list, moved for another S
        for k, v in zip(p, (nh, nw, top, left, flip, M, o)):
            p[k].append(v)
    return R.param_rows({k: np.array(v) for k, v in p.items()})


@pytest.mark.parametrize("S,L", [(64, 16), (64, 64), (32, 8)])
def test_apply_matches_the_fp64_restatement(dev, S, L):
    """Hand-made parameter tables, and tables read back from aug_params, on uniform-noise images (the worst case for
    interpolation): image within IMAGE_TOL of the float64 restatement, labels bit-exact.  (64, 64) places the bottom right crops
    of the S = 64 list flush with the border; for S = 32 the same origins lie inside.)"""
    from lc2is_amd import ops
    from lc2is_amd.data import TrainAugment
    pool, imgs, labs = _pool(SHAPES, 11, dev)
    worst = 0.0
    aug = TrainAugment(crop_size=S, label_size=L, base_size=48, seed=9)
    drawn_slots = [0, 1, 2, 5, 5, 1, 0, 2] * 2
    drawn = aug.params(pool, drawn_slots, 4).cpu().numpy()
    for name, slots, rows in (("hand-made", [c[0] for c in CASES], _case_rows(S)), ("drawn", drawn_slots, drawn)):
        px, lb = ops.aug_apply(pool.images, pool.labels, pool.desc, torch.tensor(slots, dtype=torch.int64, device=dev),
                               torch.from_numpy(rows).to(dev), S, L, _norm(), pad_label=150)
        ref_px, ref_lb = _ref_batch(imgs, labs, slots, rows, S, L, pad_label=150)
        err = np.abs(px.cpu().numpy().astype(np.float64) - ref_px).reshape(len(slots), -1).max(axis=1)
        print(f"aug_apply S={S} L={L} {name}: max |kernel - fp64| per sample = {np.array2string(err, precision=2)}")
        worst = max(worst, err.max())
        assert np.array_equal(lb.cpu().numpy(), ref_lb), name
        assert (ref_lb != 150).any() and np.abs(ref_px).max() > 1.5
    print(f"aug_apply S={S} L={L}: max |kernel - fp64| = {worst:.3e} (bound {IMAGE_TOL:.0e})")
    assert worst <= IMAGE_TOL


def test_identity_parameters_give_the_normalised_source_crop(dev):
    """nh = H, nw = W, no flip, identity colour: the output is (u8 * (1/255) - mean) / std of the source crop to 1e-6."""
    from lc2is_amd import ops
    pool, imgs, labs = _pool([(80, 100), (64, 64)], 3, dev)
    S, L = 64, 64
    rows = R.param_rows(dict(nh=np.array([80, 64]), nw=np.array([100, 64]), top=np.array([9, 0]), left=np.array([21, 0]),
                             flip=np.array([0, 0]), M=np.stack([np.eye(3)] * 2), o=np.zeros((2, 3))))
    px, lb = ops.aug_apply(pool.images, pool.labels, pool.desc, torch.tensor([0, 1], device=dev), torch.from_numpy(rows).to(dev),
                           S, L, _norm())
    for b, (top, left) in enumerate(((9, 21), (0, 0))):
        crop = imgs[b][top:top + S, left:left + S].astype(np.float64)
        want = ((crop * (1.0 / 255.0) - np.array(MEAN)) / np.array(STD)).transpose(2, 0, 1)
        err = np.abs(px[b].cpu().numpy() - want).max()
        print(f"identity sample {b}: max error {err:.3e}")
        assert err <= 1e-6
        assert np.array_equal(lb[b].cpu().numpy(), labs[b][top:top + S, left:left + S].astype(np.int64))


def test_out_of_range_tables_are_rendered_as_padding(dev):
    """A slot outside the pool, a zero row or sizes beyond the supported range read nothing: zeros and pad_label."""
    from lc2is_amd import ops
    pool, imgs, labs = _pool([(40, 56)], 2, dev)
    rows = _case_rows(32)[:4].copy()
    rows[2] = 0
    rows[3, R.NW] = R.MAX_RESIZED + 1
    slots = torch.tensor([0, 7, 0, 0], dtype=torch.int64, device=dev)
    px, lb = ops.aug_apply(pool.images, pool.labels, pool.desc, slots, torch.from_numpy(rows).to(dev), 32, 8, _norm(), pad_label=9)
    assert px[0].abs().max() > 0 and (lb[0] != 9).any()
    assert (px[1:] == 0).all() and (lb[1:] == 9).all()


@pytest.fixture()
def small(dev):
    from lc2is_amd.data import TrainAugment
    shapes = [(50, 70), (90, 60), (64, 64), (33, 120), (128, 40), (75, 75)]
    pool, imgs, labs = _pool(shapes, 21, dev)
    return pool, imgs, labs, TrainAugment(crop_size=64, label_size=16, base_size=64, seed=77)


def _same(a, b):
    return torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["label"], b["label"])


def test_a_sample_does_not_depend_on_its_batch(dev, small):
    pool, _, _, aug = small
    whole = aug(pool, [0, 1, 2, 3, 4, 5], 3)
    assert whole["pixel_values"].shape == (6, 3, 64, 64) and whole["pixel_values"].dtype == torch.float32
    assert whole["label"].shape == (6, 16, 16) and whole["label"].dtype == torch.int64
    assert _same(whole, aug(pool, torch.arange(6, device=dev), torch.tensor([3], dtype=torch.int32, device=dev)))   # run to run
    order = [4, 0, 5, 5, 2]
    mixed = aug(pool, order, 3)
    for pos, k in enumerate(order):
        alone = aug(pool, [k], 3)
        for key in ("pixel_values", "label"):
            assert torch.equal(alone[key][0], whole[key][k]) and torch.equal(mixed[key][pos], whole[key][k]), (key, k)


def test_epoch_and_seed_change_the_augmentation(dev, small):
    from lc2is_amd.data import TrainAugment
    pool, _, _, aug = small
    a = aug(pool, [0, 1, 2, 3, 4, 5], 3)
    b = aug(pool, [0, 1, 2, 3, 4, 5], 4)
    c = TrainAugment(crop_size=64, label_size=16, base_size=64, seed=78)(pool, [0, 1, 2, 3, 4, 5], 3)
    for other in (b, c):
        assert all(not torch.equal(a["pixel_values"][k], other["pixel_values"][k]) for k in range(6))
    plain = TrainAugment(crop_size=64, label_size=16, base_size=64, seed=77, photometric=False, flip_prob=0.0, ratio_range=(1.0, 1.0))
    rows = plain.params(pool, [2], 3).cpu()
    assert rows[0, :5].tolist() == [64, 64, 0, 0, 0]
    assert torch.equal(rows[0, 5:17].view(torch.float32), torch.tensor([1., 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]))


def test_streaming_form_equals_the_pool_form(dev, small):
    """Host arrays with their dataset indices through the pinned staging buffer: the bits of the pool form, twice in a row (the
    staging buffer is reused)."""
    pool, imgs, labs, aug = small
    for order, epoch in (([5, 1, 3], 2), ([0, 2], 9)):
        got = aug(images=[imgs[k] for k in order], labels=[labs[k] for k in order], indices=order, epoch=epoch)
        assert _same(got, aug(pool, order, epoch))


def test_params_and_apply_replay_from_a_graph(dev, small):
    """params + apply captured as one linear chain; new indices and a new epoch copied into the static tensors; the replay has
    the bits of the eager call."""
    pool, _, _, aug = small
    idx = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device=dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {"pixel_values": torch.empty(4, 3, 64, 64, device=dev), "label": torch.empty(4, 16, 16, dtype=torch.int64, device=dev)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.apply(pool, idx, aug.params(pool, idx, epoch), out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug.apply(pool, idx, aug.params(pool, idx, epoch), out)
    for order, e in (([5, 4, 0, 2], 6), ([1, 1, 3, 5], 11)):
        idx.copy_(torch.tensor(order, device=dev))
        epoch.fill_(e)
        graph.replay()
        assert _same(out, aug(pool, order, e)), (order, e)


def test_augmented_batches_feed_the_train_step(dev):
    """Three TrainStep.step calls on a tiny BaseModelWithText fed by AugmentedBatches (one batch per epoch, three epochs): finite,
    decreasing loss, and no host synchronisation inside the loader (torch's sync debug mode raises on one).
    The batch is built so that "decreasing" is a statement about the step and not about the draw: two flat-colour images whose
    label maps (and the padding label) are one class, so every augmentation asks for the same answer.  With uniform-noise images
    the loss of a randomly initialised model differs more from one augmented batch to the next (6.8 / 7.0 / 7.9 before any
    update, on the CPU oracle) than three small SGD steps move it.  Parity of the pixels is the business of the tests above."""
    import lc2is_amd.nn as N
    from lc2is_amd.data import AugmentedBatches, DeviceImagePool, TrainAugment
    from lc2is_amd.step import TrainStep
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64).to(dev).train()
    shapes = [(80, 100), (90, 70)]
    imgs = [np.broadcast_to(np.array(c, np.uint8), (h, w, 3)).copy() for (h, w), c in zip(shapes, ((200, 120, 40), (60, 90, 180)))]
    labs = [np.full(s, 3, np.uint8) for s in shapes]
    pool = DeviceImagePool.from_arrays(imgs, labs, device=dev)
    assert len(pool) == 2 and pool.nbytes == 24064 + 8192 + 18944 + 6400
    ids = torch.randint(1, 500, (2, 8), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, -1] = 510, 511
    extra = {"input_ids": ids.to(dev), "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    loader = AugmentedBatches(pool, TrainAugment(crop_size=64, label_size=16, base_size=64, pad_label=3, seed=5), 2, shuffle_seed=1,
                              extra_inputs=extra)
    assert len(loader) == 1
    ts = TrainStep(m, optimizer="sgd", lr=1e-3)
    losses, seen = [], []
    for epoch in range(3):
        loader.set_epoch(epoch)
        it = iter(loader)
        torch.cuda.set_sync_debug_mode("error")
        try:
            inputs, metas = next(it)
            assert next(it, None) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert set(inputs) == {"pixel_values", "label", "input_ids", "attention_mask"}
        assert sorted(d["index"] for d in metas) == [0, 1] and all(d["epoch"] == epoch for d in metas)
        seen.append(inputs["pixel_values"].clone())
        losses.append(ts.step(inputs, inputs.pop("label")))
    losses = [float(v) for v in losses]
    print("losses of three steps fed by AugmentedBatches:", losses)
    assert all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2]
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
