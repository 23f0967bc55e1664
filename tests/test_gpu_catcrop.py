"""Class-ratio crop re-draw (lc2is_aug_crop_select) and the class statistics (lc2is_label_histogram, DeviceImagePool.class_counts,
data.class_weights) on the MI355X against tests/catcrop_ref.py.  The selection is integer arithmetic: every comparison of rows,
info and labels is bitwise.  The label maps are the piecewise-constant ones of catcrop_ref.make_label_map (pinned against a
brute-force count in tests/test_catcrop_cpu.py): over 64 keys they spread t* over several candidates, and the constant map
exhausts every sample."""
import functools

import numpy as np
import pytest
import torch

import augment_ref as R
import catcrop_ref as CR

pytestmark = pytest.mark.gpu

SEED, BASE, EPOCH, RATIO, RATIO1024, IGNORE = 1234, 64, 3, 0.75, 768, 0
SIZES = [(96, 160), (75, 131)]


@functools.lru_cache(maxsize=None)
def _labels():
    """Slots 0, 1: the two test maps; 2: the constant map; 3..5: variants, so that a pool form with keys = slots has a spread too."""
    a, b = (CR.make_label_map(h, w) for h, w in SIZES)
    return [a, b, np.full((40, 50), 9, np.uint8), b.T.copy(), a[::-1].copy(), CR.make_label_map(33, 120)]


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(8)
    return [rng.integers(0, 256, l.shape + (3,), dtype=np.uint8) for l in _labels()]


@pytest.fixture(scope="module")
def pool(dev):
    from lc2is_amd.data import DeviceImagePool
    return DeviceImagePool.from_arrays(_images(), _labels(), device=dev)


def _aug(S, L, **kw):
    from lc2is_amd.data import TrainAugment
    kw.setdefault("cat_max_ratio", RATIO)
    return TrainAugment(crop_size=S, label_size=L, base_size=BASE, seed=SEED, **kw)


def _t(a, dev, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def _select(pool, aug, slots, keys, epoch, dev, **kw):
    """(raw rows, selected rows, info) as numpy, through ops.aug_params + ops.aug_crop_select."""
    from lc2is_amd import ops
    s, k, e = _t(slots, dev), None if keys is None else _t(keys, dev), _t([epoch], dev, torch.int32)
    raw = ops.aug_params(s, e, pool.desc, aug.config, keys=k)
    rows = raw.clone()
    info = ops.aug_crop_select(pool.labels, pool.desc, s, e, aug.config, rows, aug.label_size, ratio1024=RATIO1024, keys=k, **kw)
    return raw.cpu().numpy(), rows.cpu().numpy(), info.cpu().numpy()


def _same(a, b):
    return torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["label"], b["label"])


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("S,L", [(32, 8), (64, 64)])
def test_select_matches_the_restatement(dev, pool, S, L, slot):
    """64 keys on one of the two maps plus 8 on the constant map, keys different from the slots: all 20 words of every row and the
    info rows equal the restatement's, with ignore_label 0, with none, and with tries = 3.  (64, 64) has q = 1 and windows larger
    than the resized image: padding is in play.  The batch holds a sample taken at once, one re-drawn and one that exhausts."""
    aug = _aug(S, L)
    cfg = R.config_dict(aug.config)
    slots = [slot] * 64 + [2] * 8
    keys = list(range(64)) + list(range(100, 108))
    for kw in (dict(ignore_label=IGNORE), dict(ignore_label=-1), dict(ignore_label=IGNORE, tries=3)):
        raw, rows, info = _select(pool, aug, slots, keys, EPOCH, dev, **kw)
        want_rows, want_info = CR.select_ref(_labels(), slots, raw, keys, EPOCH, cfg, L, RATIO1024, **kw)
        hist = np.bincount(want_info[:, 0], minlength=11)
        print(f"S={S} L={L} slot={slot} {kw}: t* histogram {hist.tolist()}")
        assert np.array_equal(info, want_info), kw
        assert np.array_equal(rows, want_rows), kw
        tries = kw.get("tries", 10)
        assert hist[0] >= 1 and hist[1:tries].sum() >= 1 and hist[tries] >= 8
        assert np.array_equal(rows[info[:, 0] == 0], raw[info[:, 0] == 0])        # taken at once: the row of the plain draw
        assert (rows[info[:, 0] > 0][:, [R.TOP, R.LEFT]] != raw[info[:, 0] > 0][:, [R.TOP, R.LEFT]]).any()
    # keys default to the slots, and info is optional storage of the caller's
    raw, rows, info = _select(pool, aug, [0, 1, 2, 3, 4, 5], None, 0, dev, ignore_label=IGNORE)
    want_rows, want_info = CR.select_ref(_labels(), range(6), raw, range(6), 0, cfg, L, RATIO1024, IGNORE)
    assert np.array_equal(rows, want_rows) and np.array_equal(info, want_info)


def test_off_is_the_parent_path_and_on_cuts_the_selected_rows(dev, pool):
    """cat_max_ratio=None: no third launch, the bits of params + apply.  With the rule on, the batch is apply on the selected
    rows, and its labels are the restatement's tiles."""
    from lc2is_amd import ops
    S, L = 32, 8
    off, on = _aug(S, L, cat_max_ratio=None), _aug(S, L)
    idx = _t([0, 1, 2, 3, 4, 5, 0, 1], dev)
    ep = _t([EPOCH], dev, torch.int32)
    raw = ops.aug_params(idx, ep, pool.desc, off.config)
    px, lb = ops.aug_apply(pool.images, pool.labels, pool.desc, idx, raw, S, L, off.norm, pad_label=0)
    got = off(pool, idx, ep)
    assert torch.equal(got["pixel_values"], px) and torch.equal(got["label"], lb) and off.last_crop_info is None
    assert torch.equal(off.params(pool, idx, ep), raw) and torch.equal(on.params(pool, idx, ep), raw)      # params(): the raw draw
    got = on(pool, idx, ep)
    info = on.last_crop_info
    assert info.is_cuda and info.dtype == torch.int32 and tuple(info.shape) == (8, 4)
    rows = raw.clone()
    info2 = ops.aug_crop_select(pool.labels, pool.desc, idx, ep, on.config, rows, L, ratio1024=RATIO1024, ignore_label=0)
    assert torch.equal(info, info2) and not torch.equal(rows, raw)
    px2, lb2 = ops.aug_apply(pool.images, pool.labels, pool.desc, idx, rows, S, L, on.norm, pad_label=0)
    assert torch.equal(got["pixel_values"], px2) and torch.equal(got["label"], lb2)
    r = rows.cpu().numpy()
    for b, k in enumerate(idx.tolist()):
        tile = CR.label_tile(_labels()[k], r[b, R.NH], r[b, R.NW], r[b, R.TOP], r[b, R.LEFT], r[b, R.FLIP], S, L)
        assert np.array_equal(np.where(tile < 0, 0, tile), got["label"][b].cpu().numpy())
        if info[b, 0] == 0:
            assert torch.equal(rows[b], raw[b]) and torch.equal(got["label"][b], lb[b])


def test_a_sample_does_not_depend_on_its_batch_and_streaming_equals_pool(dev, pool):
    S, L = 32, 8
    aug = _aug(S, L)
    seen = set()
    for epoch in (0, 3):
        whole = aug(pool, [0, 1, 2, 3, 4, 5], epoch)
        info = aug.last_crop_info.clone()
        seen |= set(info[:, 0].tolist())
        order = [4, 0, 5, 5, 2, 3]
        mixed = aug(pool, order, epoch)
        assert torch.equal(aug.last_crop_info, info[order])
        for pos, k in enumerate(order):
            alone = aug(pool, [k], epoch)
            assert torch.equal(aug.last_crop_info[0], info[k])
            for key in ("pixel_values", "label"):
                assert torch.equal(alone[key][0], whole[key][k]) and torch.equal(mixed[key][pos], whole[key][k]), (key, k)
        stream = aug(images=[_images()[k] for k in order], labels=[_labels()[k] for k in order], indices=order, epoch=epoch)
        assert _same(stream, mixed) and torch.equal(aug.last_crop_info, info[order])
    assert 0 in seen and 10 in seen and seen & set(range(1, 10))


def test_bad_tables_are_left_untouched(dev, pool):
    """A slot out of range, a row with nh = 0 and a descriptor whose lab_off lies past the label buffer: range-checked inputs.  The
    rows stay as they were, info is {-1, 0, 0, 0}, and the rows next to them are the restatement's."""
    from lc2is_amd import ops
    S, L = 32, 8
    aug = _aug(S, L)
    cfg = R.config_dict(aug.config)
    desc = torch.cat([pool.desc, pool.desc[1:2].clone()])
    desc[6, 1] = pool.labels.numel() - 100                  # 75 x 131 labels do not fit behind this offset
    slots = [0, 99, 1, 0, 6, 1, -1]
    keys = [5, 6, 7, 8, 9, 10, 11]
    s, k, e = _t(slots, dev), _t(keys, dev), _t([EPOCH], dev, torch.int32)
    raw = ops.aug_params(s, e, desc, aug.config, keys=k)
    raw[3, R.NH] = 0
    assert (raw[1] == 0).all() and (raw[6] == 0).all() and raw[4, R.NH] > 0
    rows = raw.clone()
    info = ops.aug_crop_select(pool.labels, desc, s, e, aug.config, rows, L, ratio1024=RATIO1024, ignore_label=IGNORE, keys=k)
    bad, good = [1, 3, 4, 6], [0, 2, 5]
    assert torch.equal(rows[bad], raw[bad])
    assert info[bad].cpu().tolist() == [[-1, 0, 0, 0]] * 4
    want_rows, want_info = CR.select_ref(_labels(), [slots[b] for b in good], raw[good].cpu().numpy(), [keys[b] for b in good], EPOCH,
                                         cfg, L, RATIO1024, IGNORE)
    assert np.array_equal(rows[good].cpu().numpy(), want_rows) and np.array_equal(info[good].cpu().numpy(), want_info)
    # the histogram takes the same checks: zeros for the bad rows
    counts = ops.label_histogram(pool.labels, desc, s)
    assert (counts[[1, 4, 6]] == 0).all() and int(counts[0].sum()) == 96 * 160


def test_three_launches_replay_from_a_graph_and_runs_are_bitwise_equal(dev, pool):
    """params + select + apply captured as one chain; new indices and a new epoch in the static tensors; the replay has the bits
    of the eager call, which has the bits of its own repetition."""
    S, L = 32, 8
    aug = _aug(S, L)
    idx = _t([0, 1, 2, 3], dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {"pixel_values": torch.empty(4, 3, S, S, device=dev), "label": torch.empty(4, L, L, dtype=torch.int64, device=dev)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(pool, idx, epoch, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug(pool, idx, epoch, out=out)
    static_info = aug.last_crop_info
    eager = _aug(S, L)
    seen = set()
    for order, e in (([5, 4, 0, 2], 0), ([1, 1, 3, 5], 3)):
        idx.copy_(torch.tensor(order, device=dev))
        epoch.fill_(e)
        graph.replay()
        first = eager(pool, order, e)
        info = eager.last_crop_info.clone()
        assert _same(out, first) and torch.equal(static_info, info), (order, e)
        again = eager(pool, order, e)
        assert _same(first, again) and torch.equal(eager.last_crop_info, info)
        seen |= set(info[:, 0].tolist())
    assert 0 in seen and seen & set(range(1, 10))


def test_cat_max_ratio_batches_feed_the_train_step(dev):
    """TrainAugment(cat_max_ratio=0.75) through AugmentedBatches into one TrainStep.step of the tiny BaseModelWithText: a finite
    loss.  Two classes, left and right half of every image; every label counts."""
    import lc2is_amd.nn as N
    from lc2is_amd.data import AugmentedBatches, DeviceImagePool, TrainAugment
    from lc2is_amd.step import TrainStep
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64).to(dev).train()
    shapes = [(80, 100), (90, 70)]
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    labs = [np.repeat((np.arange(w) >= w // 2).astype(np.uint8)[None], h, axis=0) for h, w in shapes]
    pool = DeviceImagePool.from_arrays(imgs, labs, device=dev)
    ids = torch.randint(1, 500, (2, 8), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, -1] = 510, 511
    extra = {"input_ids": ids.to(dev), "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    aug = TrainAugment(crop_size=64, label_size=16, base_size=64, pad_label=0, seed=5, cat_max_ratio=0.75, cat_ignore_label=None)
    loader = AugmentedBatches(pool, aug, 2, shuffle_seed=1, extra_inputs=extra)
    ts = TrainStep(m, optimizer="sgd", lr=1e-3)
    inputs, metas = next(iter(loader))
    assert tuple(aug.last_crop_info.shape) == (2, 4) and sorted(d["index"] for d in metas) == [0, 1]
    loss = float(ts.step(inputs, inputs.pop("label")))
    print("loss of one step fed by cat_max_ratio batches:", loss, "info:", aug.last_crop_info.cpu().tolist())
    assert np.isfinite(loss)
    assert (aug.last_crop_info[:, 0] >= 0).all()


@functools.lru_cache(maxsize=None)
def _hist_labels():
    rng = np.random.default_rng(12)
    noise = np.stack([rng.permutation(256)[:64] for _ in range(48)]).astype(np.uint8)          # every 64 neighbours differ
    big = np.kron(rng.integers(0, 256, (64, 32)), np.ones((16, 32), dtype=np.int64)).astype(np.uint8)   # 1024 x 1024, piecewise
    assert big.shape == (1024, 1024) and all(len(set(r.tolist())) == 64 for r in noise)
    return [np.array([[201]], np.uint8), CR.make_label_map(75, 131), noise, big]


def test_label_histogram_and_class_weights(dev):
    """ops.label_histogram / DeviceImagePool.class_counts against np.bincount, exact: a 1 x 1 image, a 75 x 131 map, a noise image
    in which the 64 lanes of a wave all hold different labels, and one 1024 x 1024 image (more than one round of the block-stride
    loop).  class_weights (fp64 torch ops on the device) against the fp64 restatement at rtol 1e-12: both sides are fp64 and only
    the order of the sums differs.  The fp32 result is taken by CrossEntropyLoss(weight=): the weighted mean over 128 pixels in
    fp32 (log-sum-exp over 151 logits, two sums of 128 terms: about 300 roundings of 6e-8, 2e-5 relative at the worst) against
    torch's in fp64 within 1e-4."""
    from lc2is_amd import ops
    from lc2is_amd.data import DeviceImagePool, class_weights
    from lc2is_amd.nn import CrossEntropyLoss
    labs = _hist_labels()
    pool = DeviceImagePool.from_arrays([np.zeros(l.shape + (3,), np.uint8) for l in labs], labs, device=dev)
    want = CR.class_counts_ref(labs)
    order = [3, 0, 2, 1, 0]
    got = ops.label_histogram(pool.labels, pool.desc, _t(order, dev))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want[order])
    assert torch.equal(got, ops.label_histogram(pool.labels, pool.desc, _t(order, dev)))
    counts = pool.class_counts()
    assert counts.dtype == torch.int64 and counts.is_cuda and np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(pool.class_counts(chunk=3).cpu().numpy(), want)
    assert np.array_equal(pool.class_counts([2, 1]).cpu().numpy(), want[[2, 1]])
    for mode in ("median_freq", "enet"):
        for n_classes, ignore in ((151, 0), (256, 255), (150, None)):
            w64 = class_weights(counts, n_classes, ignore, mode, dtype=torch.float64)
            ref = CR.class_weights_ref(want, n_classes, ignore, mode)
            assert w64.is_cuda and w64.dtype == torch.float64
            np.testing.assert_allclose(w64.cpu().numpy(), ref, rtol=1e-12, atol=0)
            assert (ref > 0).sum() > 100
            w = class_weights(counts, n_classes, ignore, mode)
            assert w.dtype == torch.float32 and torch.equal(w, w64.float())
    w = class_weights(counts)
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(2, 151, 8, 8, generator=g).to(dev)
    target = torch.randint(0, 151, (2, 8, 8), generator=g).to(dev)
    loss = CrossEntropyLoss(weight=w, ignore_index=0)(logits, target)
    ref = torch.nn.functional.cross_entropy(logits.double().cpu(), target.cpu(), weight=w.double().cpu(), ignore_index=0)
    print("weighted CE with pool class weights:", float(loss), "torch fp64:", float(ref))
    assert np.isfinite(float(loss)) and abs(float(loss) - float(ref)) <= 1e-4 * abs(float(ref))
