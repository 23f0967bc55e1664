"""Strong photometric views on the MI355X (lc2is_strong_params, lc2is_strong_apply, data.StrongAugment) against tests/strong_ref.py:
switches, radius and copies bit for bit; colour fields, taps and the blurred image within bounds derived from the fp32 roundings."""
import functools

import numpy as np
import pytest
import torch

import augment_ref as AR
import strong_ref as SR

pytestmark = pytest.mark.gpu

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
SEED = 1234


def image_tol(R):
    """Absolute, in normalised units.  Every tap the kernel uses is the restatement's by construction (integer indices), so the
    difference is fp32 rounding alone: the two blur passes are 2 (2R + 1) multiply-adds per output, the de-normalisation, the 3 x 3
    colour product with its offset and the re-normalisation about 16 more operations; each rounds by at most 2^-24 of a magnitude
    <= 255 on the pixel scale (the taps sum to 1, so the blur does not grow it), and the result is divided by 255 * std_c, std_c >=
    0.261.  Times the margin of 4 that test_gpu_augment.py's IMAGE_TOL takes (it also covers the saturating inputs, whose operands in
    front of the clamp reach about 2.2 * 255).  R = 8: 4.6e-5; R = 0: 1.6e-5.  Without colour the blur acts on |x| <= 6 directly and
    its error is far below this.  A wrong tap, weight or reflection is off by more than 1e-3 on the inputs below (asserted there)."""
    return 4.0 * (2 * (2 * R + 1) + 16) * 2.0 ** -24 * 255.0 * (1.0 / min(STD)) / 255.0


def _strong(**kw):
    from lc2is_amd.data import StrongAugment
    kw.setdefault("seed", SEED)
    return StrongAugment(image_mean=MEAN, image_std=STD, **kw)


def _norm(cfg):
    return [float(v) for v in cfg.mean], [float(v) for v in cfg.std], [float(v) for v in cfg.inv_std]


def _t(a, dev, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- params ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _keys():
    rng = np.random.default_rng(5)
    return np.concatenate([np.arange(2048), rng.integers(0, 2 ** 62, 2046), [2 ** 62, 2 ** 62 - 1]]).astype(np.int64)


@pytest.mark.parametrize("epoch", [0, 1, 77, 2 ** 31 - 1])
def test_params_match_the_restatement(dev, epoch):
    """4096 keys (small ones and keys up to 2^62): flags and R equal, sigma equal (one rounding, restated exactly), trailing words 0;
    M, o, sigma and w within 1e-5 * max(1, |x|), the bound test_gpu_augment.py uses for fp32 sinf / cosf and composed 3x3 products
    (expf and the normalising division of the taps are a few ulp of numbers <= 1)."""
    from lc2is_amd import ops
    strong = _strong()
    keys = _keys()
    got = ops.strong_params(_t(keys, dev), _t([epoch], dev, torch.int32), strong.config).cpu().numpy()
    ref = SR.draw_params(SR.config_dict(strong.config), keys, epoch)
    assert got.shape == (4096, SR.P_WORDS) and (got[:, SR.W0 + 9:] == 0).all()
    assert np.array_equal(got[:, SR.FLAGS], ref["flags"]) and np.array_equal(got[:, SR.R_WORD], ref["R"])
    f = got.view(np.float32).astype(np.float64)
    worst = {}
    for name, lo, n in (("M", SR.M0, 9), ("o", SR.O0, 3), ("w", SR.W0, 9), ("sigma", SR.SIGMA, 1)):
        want = np.asarray(ref[name], dtype=np.float64).reshape(4096, n)
        worst[name] = (np.abs(f[:, lo:lo + n] - want) / np.maximum(1.0, np.abs(want))).max()
    print(f"strong_params epoch {epoch}: scaled errors {worst}; sigma bit-equal: {np.array_equal(got[:, SR.SIGMA], ref['sigma'].view(np.int32))}")
    assert all(v <= 1e-5 for v in worst.values()), worst
    w = f[:, SR.W0:SR.W0 + 9]
    assert all((w[ref["R"] == r, r + 1:] == 0).all() for r in range(1, 9)) and np.abs(w[:, 0] + 2 * w[:, 1:].sum(1) - 1).max() <= 1e-6
    # the draw is not trivial: every radius, every flag combination the probabilities allow
    assert set(ref["R"].tolist()) == set(range(1, 9)) and set(ref["flags"].tolist()) == {0, 1, 3, 4, 5, 7}
    assert 0.7 < ref["jitter"].mean() < 0.9 and 0.1 < ref["grey"].mean() < 0.3 and 0.4 < ref["blur"].mean() < 0.6


def test_the_class_draws_nothing_or_everything(dev):
    """Probabilities 0 / 0 / 0: the input bits; 1 / 1 / 1: every row has all three flags."""
    x = torch.randn(4, 3, 20, 20, generator=torch.Generator().manual_seed(0)).to(dev)
    x[0, 0, 0, 0], x[1, 2, 3, 4] = float("nan"), float("inf")
    none = _strong(jitter_prob=0.0, gray_prob=0.0, blur_prob=0.0)
    out = none(x, [1, 2, 3, 4], 0)
    assert out is not x and _same_bits(out, x) and (none.last_params[:, SR.FLAGS] == 0).all()
    every = _strong(jitter_prob=1.0, gray_prob=1.0, blur_prob=1.0)
    out = every(x, [1, 2, 3, 4], 0)
    assert (every.last_params[:, SR.FLAGS] == 7).all() and not _same_bits(out[2:], x[2:])
    assert (out[2:, 0] - out[2:, 1] * (STD[1] / STD[0]) - (MEAN[1] - MEAN[0]) / STD[0]).abs().max() < 1e-4      # grey: r = g on the pixel scale


# ---- apply ----------------------------------------------------------------------------------------------------------------------
def _jitter_map():
    """A hand-made jitter: brightness +20, contrast 1.3, saturation 1.4, hue 0.6 rad, composed as the header says."""
    M, o = 1.3 * np.eye(3), 1.3 * np.full(3, 20.0)
    for A in (AR.saturation_matrix(1.4)[0], AR.hue_matrix(0.6)[0]):
        M, o = A @ M, A @ o
    return M, o


@functools.lru_cache(maxsize=None)
def _hand_rows():
    """30 rows: every R in 0 .. 8 with blur alone, with jitter and with jitter + grey (taps of sigma = R / 4, and 0.5 in the entries
    past R, which must not be read); jitter alone and grey alone without blur (the streaming path), and the row with no flag."""
    M, o = _jitter_map()
    G = np.tile(SR.GREY_W, (3, 1))
    rows = []
    for R in range(9):
        sigma = max(R, 1) / 4.0
        w = SR.taps(sigma, R)
        w[R + 1:] = 0.5
        rows += [SR.make_row(SR.BLUR, R, sigma, w=w), SR.make_row(SR.BLUR | SR.COLOUR, R, sigma, M, o, w),
                 SR.make_row(SR.BLUR | SR.COLOUR | SR.GREY, R, sigma, G @ M, G @ o, w)]
    rows += [SR.make_row(SR.COLOUR, 5, 1.0, M, o), SR.make_row(SR.COLOUR | SR.GREY, 0, 1.0, G @ M, G @ o), SR.make_row(0, 3)]
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _inputs(S):
    """[3 kinds][B = 3, 3, S, S]: random normal; saturating (|x| up to 6: the clamp acts on both sides); one channel constant."""
    rng = np.random.default_rng(S)
    normal = rng.standard_normal((3, 3, S, S)).astype(np.float32)
    sat = rng.uniform(-6.0, 6.0, (3, 3, S, S)).astype(np.float32)
    const = rng.standard_normal((3, 3, S, S)).astype(np.float32)
    const[:, 1] = 0.75
    return normal, sat, const


def _repeat_edge_blur(v, w, R):
    """A wrong reflection (the edge repeated: "symmetric"), to show what the tolerance tells apart."""
    S = v.shape[-1]
    idx = np.arange(S)
    sym = lambda i: np.where(i < 0, -i - 1, np.where(i >= S, 2 * S - 1 - i, i))
    t = w[0] * v + sum(w[k] * (v[..., :, sym(idx - k)] + v[..., :, sym(idx + k)]) for k in range(1, R + 1))
    return w[0] * t + sum(w[k] * (t[..., sym(idx - k), :] + t[..., sym(idx + k), :]) for k in range(1, R + 1))


@pytest.mark.parametrize("S", [12, 20, 68, 132])
def test_apply_matches_the_fp64_restatement(dev, S):
    """Hand-written rows, three different ones per launch (B = 3), on the three kinds of input: within image_tol(R) of the float64
    restatement per sample; rows without blur or colour bit for bit.  S = 12: the reflection reaches 8 deep into a 12-wide image;
    68 and 132 are no multiples of the 32 x 64 tile and cross tile seams on both axes."""
    from lc2is_amd import ops
    strong = _strong()
    mean, std, inv_std = _norm(strong.config)
    rows = _hand_rows()
    worst = {}
    for kind, x in zip(("normal", "saturating", "constant channel"), _inputs(S)):
        xd = torch.from_numpy(x).to(dev)
        for j in range(10):
            pick = rows[[j, j + 10, j + 20]]
            got = ops.strong_apply(xd, torch.from_numpy(pick).to(dev), strong.config).cpu().numpy()
            ref = SR.apply_ref(x, pick, mean, std, inv_std)
            for b in range(3):
                flags, R = int(pick[b, SR.FLAGS]), int(pick[b, SR.R_WORD])
                if not flags & (SR.COLOUR | SR.BLUR):
                    assert np.array_equal(got[b].view(np.int32), x[b].view(np.int32))
                    continue
                Rb = R if flags & SR.BLUR else 0
                err = np.abs(got[b].astype(np.float64) - ref[b]).max()
                worst[(kind, flags, Rb)] = err
                assert err <= image_tol(Rb), (kind, flags, R, err, image_tol(Rb))
    print(f"strong_apply S={S}: max |kernel - fp64| by radius:",
          {R: f"{max(v for (_, _, r), v in worst.items() if r == R):.2e} (bound {image_tol(R):.1e})" for R in range(9)})
    # what the bound tells apart: the edge-repeating reflection on the same input is off by more than 1e-3, at every radius
    x = _inputs(S)[0][0].astype(np.float64)
    for R in range(1, 9):
        w = SR.taps(R / 4.0, R)
        assert np.abs(SR.blur_ref(x, w, R) - _repeat_edge_blur(x, w, R)).max() > 1e-3
    sat = SR.apply_ref(_inputs(S)[1], rows[[1, 1, 1]], mean, std, inv_std)
    lo, hi = (0.0 - np.array(mean)) / np.array(std), (1.0 - np.array(mean)) / np.array(std)
    assert np.isclose(sat.min(axis=(0, 2, 3)), lo).all() and np.isclose(sat.max(axis=(0, 2, 3)), hi).all()      # the clamp acted on both sides


@pytest.mark.parametrize("S", [12, 20, 68, 132])
def test_the_class_matches_the_restatement_given_its_device_table(dev, S):
    """The launch pair through StrongAugment; the table is read back (here, not by the class) as the fp32 the kernel reads."""
    strong = _strong(jitter_prob=0.7, gray_prob=0.3, blur_prob=0.7)
    mean, std, inv_std = _norm(strong.config)
    x = np.concatenate(_inputs(S)[:2])                                          # B = 6
    keys = [3, 2 ** 50 + 1, 9, 10, 11, 12]
    got = strong(torch.from_numpy(x).to(dev), keys, 5)
    rows = strong.last_params.cpu().numpy()
    ref_rows = SR.draw_params(SR.config_dict(strong.config), keys, 5)
    assert np.array_equal(rows[:, SR.FLAGS], ref_rows["flags"]) and np.array_equal(rows[:, SR.R_WORD], ref_rows["R"])
    ref = SR.apply_ref(x, rows, mean, std, inv_std)
    for b in range(6):
        R = int(rows[b, SR.R_WORD]) if rows[b, SR.FLAGS] & SR.BLUR else 0
        err = np.abs(got[b].cpu().numpy().astype(np.float64) - ref[b]).max()
        assert err <= image_tol(R), (b, rows[b, :2], err)
    assert len(set(rows[:, SR.FLAGS].tolist())) >= 3


def _plant(x):
    x = x.clone()
    x[0, 0, 0, 0], x[0, 1, 5, 7], x[0, 2, -1, -1] = float("nan"), float("inf"), float("-inf")
    x.view(torch.int32)[0, 0, 1, 1] = 0x7FC12345                                # a NaN with a payload
    x.view(torch.int32)[0, 1, 2, 2] = -4194303                                  # 0xFFC00001: a negative NaN with a payload
    return x


@pytest.mark.parametrize("S", [12, 68])
def test_no_flag_and_bad_rows_copy_the_bits(dev, S):
    from lc2is_amd import ops
    strong = _strong()
    x = _plant(torch.from_numpy(_inputs(S)[0]).to(dev))[:1].contiguous()
    M, o = _jitter_map()
    bad = [SR.make_row(0, 0), SR.make_row(0, 8), SR.make_row(SR.BLUR | SR.COLOUR, 9, 2.0, M, o), SR.make_row(SR.BLUR, -1, 1.0, w=np.full(9, 0.1)),
           SR.make_row(8 | SR.BLUR | SR.COLOUR, 2, 0.5, M, o), SR.make_row(SR.GREY, 2, 0.5, M, o), np.full(SR.P_WORDS, -1, np.int32),
           SR.make_row(1 << 30, 0), SR.make_row(SR.BLUR, 2 ** 31 - 1, 1.0)]
    for row in bad:
        out = ops.strong_apply(x, torch.from_numpy(row[None].copy()).to(dev), strong.config)
        assert _same_bits(out, x), row[:2]


def test_the_same_call_twice_gives_the_same_bytes_and_a_sample_does_not_depend_on_its_batch(dev):
    from lc2is_amd import ops
    S = 68
    strong = _strong()
    rows = _hand_rows()
    x5 = torch.from_numpy(np.concatenate(_inputs(S)[:2])[:5]).to(dev)
    for pick in ([25, 1, 26, 14, 27], [4, 28, 22, 9, 0]):                       # row 2: R = 8 jitter + grey; R = 7 jitter
        table = torch.from_numpy(rows[pick]).to(dev)
        a = ops.strong_apply(x5, table, strong.config)
        b = ops.strong_apply(x5, table, strong.config)
        assert _same_bits(a, b)
        one = ops.strong_apply(x5[2:3], table[2:3].contiguous(), strong.config)  # B = 1 against row 2 of B = 5
        assert _same_bits(one[0], a[2])
    keys = [7, 8, 9, 10, 11]
    full = strong(x5, keys, 2)
    alone = strong(x5[2:3], keys[2:3], 2)
    assert _same_bits(alone[0], full[2])


def test_out_and_views(dev):
    """A preallocated out is written and returned; an overlapping out is refused; a batch slice (contiguous, offset, 16-byte base) is
    HANDLED; a strided, permuted or misaligned view is REFUSED (RuntimeError), never copied silently."""
    from lc2is_amd import ops
    S = 20
    strong = _strong(jitter_prob=1.0, blur_prob=1.0)
    big = torch.from_numpy(np.concatenate(_inputs(S))).to(dev)                  # [9, 3, S, S]
    keys = list(range(9))
    want = strong(big, keys, 1)
    out = torch.empty_like(big)
    assert strong(big, keys, 1, out=out) is out and _same_bits(out, want)
    assert strong.view({"pixel_values": big, "input_ids": keys}, keys, 1)["input_ids"] is keys
    part = strong(big[3:7], keys[3:7], 1)                                       # an offset view of the batch
    assert _same_bits(part, want[3:7])
    n = big.numel()
    buf = torch.zeros(2 * n, device=dev)
    x_in = buf[:n].view_as(big).copy_(big)
    for bad_out in (x_in, buf[n // 2:n // 2 + n].view_as(big), buf[n - 4:2 * n - 4].view_as(big)):      # in place; half; the last 16 bytes
        with pytest.raises(RuntimeError, match="overlap"):
            strong(x_in, keys, 1, out=bad_out)
    assert strong(x_in, keys, 1, out=buf[n:].view_as(big)) is not None and _same_bits(buf[n:].view_as(big), want)      # adjacent: fine
    wide = torch.zeros(2, 3, S, S + 4, device=dev)
    flat = torch.zeros(2 * 3 * S * S + 1, device=dev)
    for view in (wide[..., :S], torch.zeros(2, S, S, 3, device=dev).permute(0, 3, 1, 2), big[::2], flat[1:].view(2, 3, S, S)):
        with pytest.raises(RuntimeError):
            strong(view, keys[:view.shape[0]], 1)
    with pytest.raises(RuntimeError):
        strong(big, keys, 1, out=torch.empty(9, 3, S, S + 4, device=dev)[..., :S])


def test_the_pair_replays_from_a_graph(dev):
    """Capture both launches; write a new value into the device epoch tensor; the replay equals the restatement for the new epoch."""
    S = 20
    strong = _strong(jitter_prob=0.7, gray_prob=0.3, blur_prob=0.7)
    mean, std, inv_std = _norm(strong.config)
    x_np = np.concatenate(_inputs(S)[:2])
    x = torch.from_numpy(x_np).to(dev)
    keys_np = [21, 22, 23, 24, 25, 26]
    keys = _t(keys_np, dev)
    epoch = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        strong(x, keys, epoch, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        strong(x, keys, epoch, out=out)
    table = strong.last_params
    seen = []
    for e in (0, 3, 77):
        epoch.fill_(e)
        graph.replay()
        rows = table.cpu().numpy()
        want = SR.draw_params(SR.config_dict(strong.config), keys_np, e)
        assert np.array_equal(rows[:, SR.FLAGS], want["flags"]) and np.array_equal(rows[:, SR.R_WORD], want["R"]), e
        assert np.array_equal(rows[:, SR.SIGMA], want["sigma"].view(np.int32))
        ref = SR.apply_ref(x_np, rows, mean, std, inv_std)
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref).reshape(6, -1).max(axis=1)
        assert (err <= image_tol(8)).all(), (e, err)
        assert _same_bits(out, _strong(jitter_prob=0.7, gray_prob=0.3, blur_prob=0.7)(x, keys, epoch))      # the eager call's bits
        seen.append(rows[:, :2].tolist())
    assert seen[0] != seen[1] and seen[1] != seen[2]


def test_strong_views_feed_the_mixed_train_step(dev):
    """The recipe: a TrainAugment(photometric=False) batch as the weak view, its strong view, ClassMix with a labelled batch through
    PseudoLabeler.mixed, one TrainStep.step of the tiny BaseModelWithText: a finite loss."""
    import lc2is_amd.nn as N
    from lc2is_amd.data import DeviceImagePool, SampleMix, TrainAugment
    from lc2is_amd.selftrain import PseudoLabeler
    from lc2is_amd.step import TrainStep
    torch.manual_seed(7)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64).to(dev).train()
    ids = torch.randint(1, 500, (2, 8), generator=torch.Generator().manual_seed(1))
    ids[:, 0], ids[:, -1] = 510, 511
    text = {"input_ids": ids.to(dev), "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}
    rng = np.random.default_rng(3)
    pool = DeviceImagePool.from_arrays([rng.integers(0, 256, (80, 96, 3), dtype=np.uint8) for _ in range(2)],
                                       [rng.integers(0, 2, (80, 96), dtype=np.uint8) for _ in range(2)], device=dev)
    keys, epoch = [0, 1], 4
    batch_u = TrainAugment(crop_size=64, label_size=16, base_size=64, photometric=False, image_mean=MEAN, image_std=STD, seed=SEED)(pool, keys, epoch)
    weak = {**text, "pixel_values": batch_u["pixel_values"]}
    strong = _strong(jitter_prob=1.0, gray_prob=0.0, blur_prob=1.0)
    view = strong.view(weak, keys, epoch)
    assert set(view) == set(weak) and view["input_ids"] is text["input_ids"] and view["pixel_values"].shape == (2, 3, 64, 64)
    assert (strong.last_params[:, SR.FLAGS] == 5).all() and not _same_bits(view["pixel_values"], weak["pixel_values"])
    halves = (torch.arange(16) >= 8).to(torch.int64)
    labels = torch.stack([halves[None].expand(16, 16), halves[:, None].expand(16, 16)]).contiguous().to(dev)
    labels_u = torch.full((2, 16, 16), -100, dtype=torch.int64)
    labels_u[:, 4:12] = 0
    inputs = {**text, "pixel_values": torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)}
    pw_u = torch.full((2, 16, 16), 0.5, device=dev)
    mix = SampleMix("classmix", n_classes=2, seed=SEED)
    both, labels_m, pw_m = PseudoLabeler.mixed((inputs, labels), (view, labels_u.to(dev), pw_u), mix, keys, epoch)
    after = strong.view(both, keys, epoch)                                      # DACS / DAFormer: the strong view after the mix
    assert after["pixel_values"].shape == both["pixel_values"].shape
    loss = float(TrainStep(m, optimizer="sgd", lr=1e-3).step(both, labels_m, pw_m))
    print("loss of one step fed by a strong view through ClassMix:", loss)
    assert np.isfinite(loss)
