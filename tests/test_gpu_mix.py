"""ClassMix / CutMix on the MI355X (lc2is_mix_select, lc2is_mix_apply, data.SampleMix) against tests/mix_ref.py.  The plan is integer
arithmetic and every output is a select, so every comparison is bitwise: plan and info with torch.equal, pixels and weights through
their int32 views (a NaN equals itself there)."""
import functools

import numpy as np
import pytest
import torch

import mix_ref as MR

pytestmark = pytest.mark.gpu

SEED, EPOCH, IGNORE, EXCLUDE = 1234, 3, -100, 1
MODES = ("classmix", "cutmix")


def _mix(mode, n_classes=9, **kw):
    from lc2is_amd.data import SampleMix
    kw.setdefault("seed", SEED)
    kw.setdefault("ignore_index", IGNORE)
    return SampleMix(mode, n_classes=n_classes, **kw)


def _ref_kw(mix):
    return dict(seed=mix.seed, n_classes=mix.n_classes, ignore_index=mix.ignore_index, exclude_label=mix.exclude_label,
                box_area=mix.box_area)


def _t(a, dev, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def _to(batch, dev):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in batch)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, dev):
    """got: device tensors; want: numpy arrays; bitwise."""
    return all(torch.equal(_bits(g), _bits(torch.from_numpy(np.ascontiguousarray(w)).to(dev))) for g, w in zip(got, want))


def _select(mix, src_lab, keys, epoch, dev, src_index=None):
    from lc2is_amd import ops
    return ops.mix_select(_t(src_lab, dev), _t(keys, dev), _t([epoch], dev, torch.int32), mix.config,
                          src_index=None if src_index is None else _t(src_index, dev))


@functools.lru_cache(maxsize=None)
def _tie_key():
    """A key under which two of the 1024 classes draw the same 24-bit number (about 3 % of the keys)."""
    cls = np.arange(16, 16 + 1024, dtype=np.uint32)
    for key in range(2000):
        if np.unique(MR.u24(MR.mix_hash(SEED, EPOCH, [key])[0], cls)).size < 1024:
            return key
    raise AssertionError("no key with a tie")


def _source_maps(K, L):
    """The source label maps of the select test: all ignore; one class; two classes; seven classes (five where K = 5) with EXCLUDE
    among them; classes with -2, K and K + 2 mixed in; uniform labels over 1024 classes; every one of 1024 classes (32 x 32 only:
    with _tie_key a tie of the draw among present classes)."""
    rng = np.random.default_rng(100 * K + L)
    two = np.zeros((L, L), np.int64)
    two[:, L // 2:] = K - 1
    some = np.concatenate([[EXCLUDE], rng.permutation(np.setdiff1d(np.arange(K), [EXCLUDE]))[:min(7, K) - 1]])
    stray = rng.integers(0, K, (L, L))
    stray.reshape(-1)[::3] = rng.choice([-2, K, K + 2, IGNORE], size=stray.reshape(-1)[::3].size)
    maps = [np.full((L, L), IGNORE), np.full((L, L), K - 1), two, rng.choice(some, size=(L, L)), stray, rng.integers(0, 1024, (L, L)),
            np.resize(rng.permutation(1024), (L, L))]
    return np.stack(maps).astype(np.int64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [4, 8, 32])
@pytest.mark.parametrize("K", [5, 151, 1024])
def test_select_matches_the_restatement(dev, K, L, mode):
    mix = _mix(mode, K, exclude_label=EXCLUDE)
    maps = _source_maps(K, L)
    present = set()
    for rows, keys in (([0, 1, 2], [5, 6, 7]), ([3, 4, 5], [2 ** 40 + 1, 0, -3]), ([6, 6, 3], [_tie_key(), 8, 5])):   # B = 3
        plan, info = _select(mix, maps, keys, EPOCH, dev, rows)
        want_plan, want_info, mask = MR.select_ref(maps, keys, EPOCH, mode, src_index=rows, **_ref_kw(mix))
        assert _same((plan, info), (want_plan, want_info), dev), (rows, plan.cpu().numpy()[:, :8], want_plan[:, :8], info.cpu(), want_info)
        assert (want_info[:, 2] == mask.sum((1, 2))).all() and (want_info[:, 3] == L * L).all()
        present |= set(want_info[:, 0].tolist())
    if mode == "classmix":
        assert {0, 1, 2} <= present                          # the empty, the one-class and the two-class map
        if K == 1024 and L == 32:
            assert 1023 in present and max(present - {1023}) > 300      # every class but EXCLUDE; the uniform map's hundreds


CASES = [(8, 8), (8, 4), (16, 4), (24, 4)]                  # r = 1, 2, 4, 6


@functools.lru_cache(maxsize=None)
def _batches(S, L, B=3, Bs=2):
    rng = np.random.default_rng(S * 10 + L)
    dst = (rng.standard_normal((B, 3, S, S)).astype(np.float32), rng.integers(0, 9, (B, L, L)), rng.random((B, L, L)).astype(np.float32))
    src = (rng.standard_normal((Bs, 3, S, S)).astype(np.float32), rng.integers(0, 9, (Bs, L, L)), rng.random((Bs, L, L)).astype(np.float32))
    dst[1][0, 0, 0], src[1][0, 0, 1] = IGNORE, IGNORE
    return dst, src


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,L", CASES)
def test_apply_matches_the_restatement_with_and_without_weights(dev, S, L, mode):
    dst, src = _batches(S, L)
    keys, rows = [10, 11, 12], [1, 0, 1]
    mix = _mix(mode, exclude_label=EXCLUDE)
    _, info, mask = MR.select_ref(src[1], keys, EPOCH, mode, src_index=rows, **_ref_kw(mix))
    assert 0 < mask.sum() < mask.size
    for dw, sw in ((True, True), (False, True), (True, False), (False, False)):
        d, s = (dst[0], dst[1], dst[2] if dw else None), (src[0], src[1], src[2] if sw else None)
        px, lab, pw, got_info = mix(_to(d, dev), _to(s, dev), keys, EPOCH, src_index=rows)
        assert _same((px, lab, pw, got_info), MR.apply_ref(d, s, mask, rows) + (info,), dev), (dw, sw)
        assert mix.last_info is got_info


@pytest.mark.parametrize("S,L", [(16, 4), (24, 4)])
def test_non_finite_values_on_the_side_not_chosen_do_not_reach_the_output(dev, S, L):
    """NaN, +inf and -inf in dst_px under the mask and in src_px outside it: the output is bitwise the select, and finite."""
    dst, src = _batches(S, L)
    keys, rows = [10, 11, 12], [1, 0, 1]
    mix = _mix("classmix", exclude_label=EXCLUDE)
    _, info, mask = MR.select_ref(src[1], keys, EPOCH, "classmix", src_index=rows, **_ref_kw(mix))
    r = S // L
    big = np.repeat(np.repeat(mask, r, axis=1), r, axis=2)[:, None].repeat(3, axis=1)
    bad = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), big.shape)
    dpx = np.where(big, bad, dst[0])
    spx = src[0].copy()
    for s_row in range(spx.shape[0]):
        used = np.zeros(big.shape[1:], bool)
        for b, row in enumerate(rows):
            if row == s_row:
                used |= big[b]
        spx[s_row] = np.where(used, spx[s_row], bad[0])
    d, s = (dpx, dst[1], dst[2]), (spx, src[1], None)
    want = MR.apply_ref(d, s, mask, rows)
    assert np.isfinite(want[0]).all() and not np.isfinite(dpx).all() and not np.isfinite(spx).all()
    px, lab, pw, _ = mix(_to(d, dev), _to(s, dev), keys, EPOCH, src_index=rows)
    assert _same((px, lab, pw), want, dev) and bool(torch.isfinite(px).all())


@pytest.mark.parametrize("mode", MODES)
def test_mixing_within_a_batch_and_refusing_aliased_outputs(dev, mode):
    S, L = 16, 4
    dst, _ = _batches(S, L)
    keys, roll = [4, 5, 6], [1, 2, 0]
    mix = _mix(mode)
    _, info, mask = MR.select_ref(dst[1], keys, EPOCH, mode, src_index=roll, **_ref_kw(mix))
    batch = _to(dst, dev)
    before = tuple(t.clone() for t in batch)
    got = mix(batch, batch, keys, EPOCH, src_index=roll)
    assert _same(got, MR.apply_ref(dst, dst, mask, roll) + (info,), dev)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(batch, before))
    fresh = lambda: (torch.empty_like(batch[0]), torch.empty_like(batch[1]), torch.empty_like(batch[2]))
    for k in range(3):
        out = list(fresh())
        out[k] = batch[k]
        with pytest.raises(RuntimeError, match="alias"):
            mix(batch, batch, keys, EPOCH, src_index=roll, out=tuple(out))
    out = fresh()
    again = mix(batch, batch, keys, EPOCH, src_index=roll, out=out)
    assert all(a is b for a, b in zip(again[:3], out)) and _same(out, MR.apply_ref(dst, dst, mask, roll), dev)


@pytest.mark.parametrize("mode", MODES)
def test_a_source_row_outside_the_batch_keeps_the_destination(dev, mode):
    S, L = 16, 4
    dst, src = _batches(S, L)
    keys, rows = [10, 11, 12], [-1, 2, 0]                       # Bs = 2
    mix = _mix(mode)
    plan_want, info, mask = MR.select_ref(src[1], keys, EPOCH, mode, src_index=rows, **_ref_kw(mix))
    assert info[:2].tolist() == [[-1, 0, 0, 0]] * 2 and not mask[:2].any() and mask[2].any()
    px, lab, pw, got_info = mix(_to(dst, dev), _to(src, dev), keys, EPOCH, src_index=rows)
    assert _same((px, lab, pw, got_info), MR.apply_ref(dst, src, mask, rows) + (info,), dev)
    assert _same((px[:2], lab[:2], pw[:2]), (dst[0][:2], dst[1][:2], dst[2][:2]), dev)
    plan, _ = _select(mix, src[1], keys, EPOCH, dev, rows)
    assert _same((plan,), (plan_want,), dev) and not plan[:2].any()
    # the apply launch on its own, and on rows no select wrote: an unknown mode or a source row outside the batch is the destination
    from lc2is_amd import ops
    assert _same(ops.mix_apply(_to(dst, dev), _to(src, dev), plan), MR.apply_ref(dst, src, mask, rows), dev)
    odd = plan.clone()
    odd[2, 0] = 7
    odd[1] = plan[2]
    odd[1, 1] = 2
    odd[0] = plan[2]
    odd[0, 1] = -5
    assert _same(ops.mix_apply(_to(dst, dev), _to(src, dev), odd), dst, dev)
    # src_index = None is row b: the third sample of three has no source row in a batch of two
    _, _, _, info_none = mix(_to(dst, dev), _to(src, dev), keys, EPOCH)
    assert info_none[2].tolist() == [-1, 0, 0, 0] and (info_none[:2, 0] >= 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_a_sample_does_not_depend_on_its_batch(dev, mode):
    L = 8
    maps = _source_maps(151, L)
    mix = _mix(mode, 151)
    small, _ = _select(mix, maps, [21, 22, 23], EPOCH, dev, [3, 4, 3])
    large, _ = _select(mix, maps, [9, 9, 22, 7, 21], EPOCH, dev, [4, 4, 4, 0, 3])
    assert torch.equal(small[0], large[4]) and torch.equal(small[1], large[2])
    # the same map at another row of another source batch: everything but the source-row word
    moved, _ = _select(mix, maps[[4, 3]], [22, 21], EPOCH, dev, [0, 1])
    keep = [w for w in range(MR.P_WORDS) if w != 1]
    assert torch.equal(moved[0, keep], small[1, keep]) and torch.equal(moved[1, keep], small[0, keep])
    assert moved[:, 1].tolist() == [0, 1] and small[:, 1].tolist() == [3, 4, 3]
    assert not torch.equal(small[0, keep], small[2, keep])      # another key, the same map: another draw


@pytest.mark.parametrize("mode", MODES)
def test_the_two_launches_replay_from_a_graph(dev, mode):
    """The device epoch tensor is incremented between replays: each replay equals the restatement for its epoch, and a replay has
    the bits of the eager call."""
    S, L = 16, 4
    dst, src = _batches(S, L)
    keys_np, rows_np = [10, 11, 12], [1, 0, 1]
    mix = _mix(mode)
    d, s = _to(dst, dev), _to(src, dev)
    keys, rows = _t(keys_np, dev), _t(rows_np, dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = (torch.empty_like(d[0]), torch.empty_like(d[1]), torch.empty_like(d[2]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mix(d, s, keys, epoch, src_index=rows, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mix(d, s, keys, epoch, src_index=rows, out=out)
    static_info = mix.last_info
    eager = _mix(mode)
    masks = []
    for e in (0, 1, 2):
        graph.replay()
        _, info, mask = MR.select_ref(src[1], keys_np, e, mode, src_index=rows_np, **_ref_kw(mix))
        assert _same(out + (static_info,), MR.apply_ref(dst, src, mask, rows_np) + (info,), dev), e
        first = tuple(t.clone() for t in out + (static_info,))
        graph.replay()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, out + (static_info,)))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, eager(d, s, keys, epoch, src_index=rows)))
        masks.append(mask)
        epoch += 1
    assert not (np.array_equal(masks[0], masks[1]) and np.array_equal(masks[1], masks[2]))


def test_mixed_batches_feed_the_train_step(dev):
    """PseudoLabeler.mixed: a labelled batch pasted into a pseudo-labelled one by ClassMix, into one TrainStep.step(inputs, labels,
    pixel_weight) of the tiny BaseModelWithText: a finite loss."""
    import lc2is_amd.nn as N
    from lc2is_amd.selftrain import PseudoLabeler
    from lc2is_amd.step import TrainStep
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64).to(dev).train()
    ids = torch.randint(1, 500, (2, 8), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, -1] = 510, 511
    text = {"input_ids": ids.to(dev), "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    g = torch.Generator().manual_seed(3)
    halves = (torch.arange(16) >= 8).to(torch.int64)
    labels = torch.stack([halves[None].expand(16, 16), halves[:, None].expand(16, 16)]).contiguous().to(dev)
    labels_u = torch.full((2, 16, 16), -100, dtype=torch.int64)
    labels_u[:, 4:12] = 0
    inputs = {**text, "pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev)}
    inputs_u = {**text, "pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev)}
    pw_u = torch.full((2, 16, 16), 0.5, device=dev)
    mix = _mix("classmix", 2)
    both, labels_m, pw_m = PseudoLabeler.mixed((inputs, labels), (inputs_u, labels_u.to(dev), pw_u), mix, [0, 1], 0)
    assert mix.last_info[:, :2].tolist() == [[2, 1], [2, 1]] and (mix.last_info[:, 2] == 128).all()
    assert set(both) == set(inputs) and both["input_ids"] is text["input_ids"] and both["pixel_values"] is not inputs_u["pixel_values"]
    assert set(pw_m.unique().tolist()) == {0.5, 1.0} and int((pw_m == 1.0).sum()) == 256
    loss = float(TrainStep(m, optimizer="sgd", lr=1e-3).step(both, labels_m, pw_m))
    print("loss of one step fed by a ClassMix batch:", loss, "info:", mix.last_info.cpu().tolist())
    assert np.isfinite(loss)
