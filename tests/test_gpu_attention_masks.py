"""GPU: the fused attention kernels under holed key masks, finite key biases, single visible keys and empty rows, row by row
against fp64 (tests/attn_ref.py; the reference runs on the CPU).

The contract under test (include/lc2is_hip.h, attention section): kbias is any finite additive bias or -inf per key; a query
row with no visible key gives O = 0, lse2 = -inf, dQ = 0 and nothing to dK / dV; the K / V rows of masked keys may hold any
FINITE values and do not matter.  NaN / Inf in masked K / V rows are outside the contract (0 * NaN is NaN in torch as well).

Per-row bound (a): for every row (b, h, q) of O and dQ and every row (b, h, key) of dK and dV
    ||got - ref|| <= 3 * floor_rel * ||ref|| + a
floor_rel = the largest per-row relative error of attention_rounded (fp64 with the kernels' documented bf16 roundings) against
attention_ref, for that tensor of that case, computed at test time; a = attn_ref.abs_slack (fp32 roundoff of a D-term product
chain, derived there).  The whole-tensor bounds of tests/test_gpu_attention.py hold next to it, unchanged.

Observed ratio (kernel's worst row / floor; the bound is 3) on an MI355X, largest over the packed and unpacked runs of a case
(they agree to the digit shown); "pX" = with dropout.  0.00 with floor 0 marks a tensor whose exact value is 0 (one visible
key) and whose rows all lie within the slack.  Where the dQ floor is large (softmax nearly one-hot on some row, see
attn_ref.floor_rel) the per-row dQ bound of that case is correspondingly loose; its whole-tensor dQ bound (1.5e-2) and the dK /
dV rows still bind, and the one-hot case itself is pinned exactly by test_single_visible_key_is_exact.  A ratio of 1.00 means
the kernel's worst row is the emulation's worst row with the same error: the kernels round where the header says they do.
RATIO_TABLE_BEGIN
case                                  O     dQ    dK    dV    floors: O / dQ / dK / dV
2x2x193x193x64/holes30                1.12  1.01  1.05  1.00    2.9e-03 / 4.4e-03 / 3.4e-03 / 3.7e-03
2x2x193x193x64/holes70                1.12  1.00  0.97  1.00    3.2e-03 / 4.4e-03 / 3.7e-03 / 3.2e-03
2x2x193x193x64/sparse                 1.19  0.76  1.09  1.00    3.5e-03 / 2.3e-02 / 3.1e-03 / 2.7e-03
2x2x193x193x64/tiles                  1.02  1.00  1.02  1.00    3.2e-03 / 1.3e-02 / 3.9e-03 / 3.1e-03
2x2x193x193x64/finite                 1.23  0.97  1.08  1.00    3.3e-03 / 1.7e-01 / 3.7e-03 / 3.1e-03
2x2x193x193x64/finite_holes           1.59  1.00  1.10  1.00    2.8e-03 / 3.1e-01 / 5.8e-03 / 3.5e-03
2x2x193x193x64/soft                   1.36  1.00  0.96  1.00    2.9e-03 / 2.4e-02 / 3.5e-03 / 3.0e-03
2x2x193x193x64/single                 0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 1.6e-03
1x2x130x321x96/holes30                1.02  0.89  1.00  1.00    2.9e-03 / 3.6e-03 / 3.3e-03 / 3.7e-03
1x2x130x321x96/holes70                1.08  1.01  1.03  1.00    2.9e-03 / 4.1e-03 / 4.0e-03 / 3.0e-03
1x2x130x321x96/sparse                 1.23  1.03  0.89  1.00    2.9e-03 / 5.8e-03 / 3.6e-03 / 2.9e-03
1x2x130x321x96/tiles                  1.12  1.15  1.13  1.00    2.7e-03 / 3.0e-03 / 3.2e-03 / 3.3e-03
1x2x130x321x96/finite                 1.37  0.97  0.87  1.00    2.6e-03 / 9.3e-03 / 3.5e-03 / 2.7e-03
1x2x130x321x96/finite_holes           1.29  0.68  1.14  1.00    2.8e-03 / 1.5e-02 / 3.2e-03 / 3.0e-03
1x2x130x321x96/soft                   1.36  0.96  0.94  1.00    2.7e-03 / 8.2e-03 / 3.3e-03 / 2.8e-03
1x2x130x321x96/single                 0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 1.6e-03
1x1x257x257x128/holes30               1.07  0.99  1.02  1.00    2.8e-03 / 3.7e-03 / 3.0e-03 / 3.0e-03
1x1x257x257x128/holes70               1.18  0.97  0.94  1.00    2.6e-03 / 3.6e-03 / 3.0e-03 / 2.9e-03
1x1x257x257x128/sparse                1.24  1.40  1.04  1.00    2.6e-03 / 8.5e-03 / 3.0e-03 / 2.9e-03
1x1x257x257x128/tiles                 1.17  0.97  0.99  1.00    2.6e-03 / 3.2e-03 / 2.9e-03 / 2.9e-03
1x1x257x257x128/finite                1.34  1.40  1.12  1.00    2.7e-03 / 5.6e-03 / 2.8e-03 / 2.8e-03
1x1x257x257x128/finite_holes          1.38  1.05  1.04  1.00    2.6e-03 / 2.6e-02 / 3.1e-03 / 2.7e-03
1x1x257x257x128/soft                  1.25  1.00  1.06  1.00    2.7e-03 / 7.2e-03 / 3.1e-03 / 2.6e-03
1x1x257x257x128/single                0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 1.8e-03
2x2x200x200x64c/holes30               1.19  1.00  1.09  1.00    3.2e-03 / 8.5e-02 / 4.3e-03 / 3.6e-03
2x2x200x200x64c/holes70               1.20  1.00  0.89  1.00    3.0e-03 / 2.8e-02 / 4.1e-03 / 3.4e-03
2x2x200x200x64c/sparse                1.34  1.00  1.09  1.00    2.9e-03 / 1.7e+00 / 4.3e-03 / 3.8e-03
2x2x200x200x64c/tiles                 1.45  1.00  0.71  1.00    2.9e-03 / 1.8e-02 / 6.3e-03 / 3.5e-03
2x2x200x200x64c/finite                1.43  1.00  1.00  1.00    3.1e-03 / 2.8e-01 / 1.9e-02 / 4.0e-03
2x2x200x200x64c/finite_holes          1.30  1.00  1.00  1.00    2.9e-03 / 7.9e-02 / 5.5e-03 / 3.5e-03
2x2x200x200x64c/soft                  1.37  1.00  1.00  1.00    3.0e-03 / 1.7e+00 / 7.9e-03 / 3.3e-03
2x2x200x200x64c/single                0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 1.8e-03
1x3x65x449x64/holes30                 1.00  0.98  1.00  1.00    2.8e-03 / 3.8e-03 / 3.9e-03 / 3.7e-03
1x3x65x449x64/holes70                 1.25  0.97  1.00  1.00    2.9e-03 / 3.8e-03 / 3.6e-03 / 3.9e-03
1x3x65x449x64/sparse                  1.31  1.02  1.26  1.00    2.7e-03 / 5.9e-03 / 3.7e-03 / 3.5e-03
1x3x65x449x64/tiles                   1.35  1.00  0.92  1.00    2.7e-03 / 3.3e-03 / 3.3e-03 / 3.6e-03
1x3x65x449x64/finite                  1.53  1.01  1.09  1.00    2.7e-03 / 2.1e-02 / 4.2e-03 / 3.4e-03
1x3x65x449x64/finite_holes            1.18  1.00  0.99  1.00    3.0e-03 / 2.4e-02 / 3.5e-03 / 3.1e-03
1x3x65x449x64/soft                    1.47  0.63  1.11  1.00    2.8e-03 / 9.3e-03 / 3.3e-03 / 3.4e-03
1x3x65x449x64/single                  0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 1.9e-03
2x8x256x16x96/holes30                 1.00  1.00  0.98  1.00    3.0e-03 / 4.9e-02 / 3.7e-03 / 2.8e-03
2x8x256x16x96/holes70                 1.00  1.00  1.00  1.00    3.0e-03 / 9.1e-02 / 3.8e-03 / 2.7e-03
2x8x256x16x96/sparse                  1.00  1.00  1.00  1.00    2.7e-03 / 9.0e+01 / 4.9e-03 / 2.6e-03
2x8x256x16x96/tiles                   0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 2.0e-03
2x8x256x16x96/finite                  1.00  1.00  1.00  1.00    2.8e-03 / 1.4e+01 / 5.6e-02 / 3.4e-03
2x8x256x16x96/finite_holes            1.00  1.00  1.00  1.00    2.9e-03 / 2.6e-01 / 4.6e-03 / 3.0e-03
2x8x256x16x96/soft                    1.00  1.00  1.00  1.00    2.9e-03 / 2.1e+00 / 5.5e-03 / 2.8e-03
2x8x256x16x96/single                  0.00  0.00  0.00  1.00    0.0e+00 / 0.0e+00 / 0.0e+00 / 1.9e-03
2x2x193x193x64/empty_batch1           1.27  1.00  0.96  1.00    2.8e-03 / 3.8e-03 / 3.9e-03 / 3.8e-03
2x8x256x16x96/empty_batch0            1.00  1.00  1.00  1.00    2.9e-03 / 4.7e-02 / 3.5e-03 / 2.6e-03
2x2x200x200x64c/lead5                 1.19  1.00  1.00  1.00    2.9e-03 / 1.1e-02 / 5.6e-03 / 3.7e-03
2x2x200x200x64c/lead64                1.18  1.00  1.22  1.00    3.0e-03 / 2.1e-02 / 3.9e-03 / 3.4e-03
2x2x200x200x64c/lead70                1.06  1.00  0.99  1.00    3.1e-03 / 9.4e-03 / 4.5e-03 / 3.4e-03
2x2x193x193x64/empty_batch1 p0.2      1.03  0.98  1.07  1.00    3.1e-03 / 3.8e-03 / 3.3e-03 / 3.3e-03
2x2x193x193x64/holes30 p0.2           1.07  0.98  1.03  1.00    3.3e-03 / 4.1e-03 / 3.5e-03 / 3.5e-03
2x2x193x193x64/finite_holes p0.2      1.30  1.00  1.02  1.00    3.4e-03 / 2.3e-01 / 4.9e-03 / 3.6e-03
largest ratio of the run: 1.59
RATIO_TABLE_END
"""
import functools
import math
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import attn_ref as R  # noqa: E402

G = HERE / "golden"
LN2 = math.log(2.0)
INF = float("inf")

SHAPES = [
    # B, H, Sq, Sk, D, causal
    (2, 2, 193, 193, 64, False),    # 3-deep ring, two query blocks, ragged 1-key last tile
    (1, 2, 130, 321, 96, False),    # D = 96, Sq != Sk, 6 tiles of which the last holds one key
    (1, 1, 257, 257, 128, False),   # two-stage ring
    (2, 2, 200, 200, 64, True),     # diagonal tiles and bias together
    (1, 3, 65, 449, 64, False),     # 8 tiles: unrolled triple, rolled tail, ragged key
    (2, 8, 256, 16, 96, False),     # class-memory cross attention, Sk smaller than a tile
]
PATTERNS = ["holes30", "holes70", "sparse", "tiles", "finite", "finite_holes", "soft", "single"]


def _bias(pattern, B, Sq, Sk, causal, seed):
    if pattern == "holes30":
        return R.holes(B, Sk, 0.3, seed, causal)
    if pattern == "holes70":
        return R.holes(B, Sk, 0.7, seed, causal)
    if pattern == "sparse":
        return R.sparse(B, Sk, seed, causal)
    if pattern == "tiles":
        return R.tiles(B, Sk, seed, causal)
    if pattern == "finite":
        return R.finite(B, Sk, seed)
    if pattern == "finite_holes":
        return R.finite_holes(B, Sk, seed, causal)
    if pattern == "soft":
        return R.soft(B, Sk, seed)
    if pattern == "single":
        return R.single(B, Sk, 0 if causal else Sk - 1, 0.75)
    if pattern.startswith("lead"):
        return R.lead(B, Sk, int(pattern[4:]))
    if pattern.startswith("empty_batch"):
        return R.empty_batch(B, Sk, seed, which=int(pattern[11:]))
    raise KeyError(pattern)


@functools.lru_cache(maxsize=None)
def _case(shape, pattern):
    """Inputs, bias, exact reference, rounded emulation and slack of a case: computed once, shared by every test that uses the
    case, never modified."""
    B, H, Sq, Sk, D, causal = shape
    seed = 1000 * Sq + Sk + D + sum(map(ord, pattern))
    q, k, v, do = R.make_inputs(B, H, Sq, Sk, D, seed)
    kb = _bias(pattern, B, Sq, Sk, causal, seed)
    scale = D ** -0.5
    args = (B, H, Sq, Sk, D, scale, causal, kb)
    return dict(q=q, k=k, v=v, do=do, kb=kb, scale=scale, ref=R.attention_ref_grads(q, k, v, do, *args),
                rounded=R.attention_rounded(q, k, v, do, *args), slack=R.abs_slack(D, scale, do, k, v))


def _run(dev, shape, q, k, v, do, kb, scale, packed=False, p=0.0, seed=0, bwd=True):
    """Forward and backward on the device; CPU tensors o, lse2, lse (natural units), dq, dk, dv.  packed: Q, K, V (and dQ, dK,
    dV) are column slices of one [B*S, 3*H*D] buffer where Sq == Sk, else K, V share a [B*Sk, 2*H*D] buffer."""
    from lc2is_amd import ops
    B, H, Sq, Sk, D, causal = shape
    C = H * D
    if packed and Sq == Sk:
        buf = torch.cat([q, k, v], dim=1).to(dev)
        qd, kd, vd = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]
        gb = torch.zeros_like(buf)
        dq, dk, dv = gb[:, :C], gb[:, C:2 * C], gb[:, 2 * C:]
    elif packed:
        buf = torch.cat([k, v], dim=1).to(dev)
        qd, kd, vd = q.to(dev), buf[:, :C], buf[:, C:]
        gb = torch.zeros_like(buf)
        dq, dk, dv = torch.zeros_like(qd), gb[:, :C], gb[:, C:]
    else:
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        dq = dk = dv = None
    kbd = None if kb is None else kb.to(dev)
    o, lse2 = ops.attention_fwd(qd, kd, vd, B, H, Sq, Sk, D, scale, causal=causal, kbias=kbd, dropout_p=p, seed=seed)
    out = dict(o=o.cpu(), lse2=lse2.cpu(), lse=lse2.double().cpu() * LN2)
    if bwd:
        dq, dk, dv = ops.attention_bwd(qd, kd, vd, o, do.to(dev), lse2, B, H, Sq, Sk, D, scale, causal=causal, kbias=kbd,
                                       dq=dq, dk=dk, dv=dv, dropout_p=p, seed=seed)
        out.update(dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
    return out


def _note(name, res):
    """Print a case's observed ratios (worst row / floor): `pytest -s` shows them, the docstring table is filled from that."""
    print("RATIO", name, " ".join(f"{n}={r[1]:.2f}(floor {r[2]:.2e})" for n, r in res.items()))


def _check_parity(name, got, c, shape, lse_tol=2e-3):
    """(a): no NaN, empty rows exact, whole-tensor bounds as in tests/test_gpu_attention.py, per-row bound."""
    B, H, Sq, Sk, D, causal = shape
    ref = c["ref"]
    for n in ("o", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n].float()).all()), (name, n)
    empty = torch.isinf(ref["lse"])                                              # [B,H,Sq]
    assert torch.equal(torch.isinf(got["lse2"]), empty) and bool((got["lse2"][empty] == -INF).all()), name
    if bool(empty.any()):
        er = empty.transpose(1, 2)
        assert bool((got["o"].reshape(B, Sq, H, D)[er] == 0).all()) and bool((got["dq"].reshape(B, Sq, H, D)[er] == 0).all()), name
    lse_err = float((got["lse"][~empty] - ref["lse"][~empty]).abs().max())
    res = R.compare_rows(got, ref, c["rounded"], c["slack"], B, H, Sq, Sk, D)
    _note(name, res)
    assert lse_err < lse_tol, (name, lse_err)
    # (an exact gradient whose norm is below what the slack allows its rows in total is zero: `single`, dQ and dK)
    zero = {n: c["slack"][n] * math.sqrt(got[n].shape[0] * H) for n in ("dq", "dk", "dv")}
    bad = R.whole_tensor_failures(got, ref, zero)
    print("WHOLE", name, "o_abs=%.2e o_rel=%.2e" % (float((got["o"].double() - ref["o"]).abs().max()),
                                                     float((got["o"].double() - ref["o"]).norm() / ref["o"].norm().clamp_min(1e-30))))
    assert not bad, (name, bad)
    assert all(ok for ok, _, _ in res.values()), (name, {n: (r[1], r[2]) for n, r in res.items()})


# ---- (a) fp64 parity, per row ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:5])) + ("c" if s[5] else ""))
def test_masked_attention_per_row(dev, shape, pattern, packed):
    c = _case(shape, pattern)
    B, H, Sq, Sk, D, causal = shape
    assert R.count_empty_rows(c["kb"], B, H, Sq, Sk, causal) == 0
    got = _run(dev, shape, c["q"], c["k"], c["v"], c["do"], c["kb"], c["scale"], packed=packed)
    _check_parity(f"{'x'.join(map(str, shape[:5]))}{'c' if causal else ''}/{pattern}/{'packed' if packed else 'unpacked'}",
                  got, c, shape)


# ---- (b) one visible key: exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("biased", [False, True], ids=["bias0", "biased"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sk", [129, 193])
def test_single_visible_key_is_exact(dev, Sk, D, biased):
    """Softmax over one element is exactly 1: O rows equal V[j] bitwise, lse2 = log2(e) (scale q.k_j + kbias_j); every other
    key's dK / dV row is exactly 0, dV[j] = sum_q dO to one bf16 rounding, and dQ, dK[j] (exactly 0) are within the slack.
    j = first / last key of a half tile, of a tile, and the key of the ragged last tile."""
    B, H, Sq = 2, 2, 70
    shape = (B, H, Sq, Sk, D, False)
    scale = D ** -0.5
    q, k, v, do = R.make_inputs(B, H, Sq, Sk, D, 7 * Sk + D)
    slack = R.abs_slack(D, scale, do, k, v)
    q4, k4, v4, g4 = (t.double().reshape(B, S, H, D) for t, S in ((q, Sq), (k, Sk), (v, Sk), (do, Sq)))
    for j in (0, 31, 32, 63, 64, Sk - 1):
        bj = (1.75 if j % 2 else -2.5) if biased else 0.0
        got = _run(dev, shape, q, k, v, do, R.single(B, Sk, j, bj), scale)
        want_o = v.reshape(B, Sk, H, D)[:, j:j + 1].expand(B, Sq, H, D)
        assert torch.equal(got["o"].reshape(B, Sq, H, D), want_o), j
        want_lse = (q4 * k4[:, j:j + 1]).sum(-1).transpose(1, 2) * scale + bj          # [B,H,Sq], natural units
        assert float((got["lse"] - want_lse).abs().max()) < 2e-3, j
        others = torch.ones(Sk, dtype=torch.bool)
        others[j] = False
        for n in ("dk", "dv"):
            assert bool((got[n].reshape(B, Sk, H, D)[:, others] == 0).all()), (n, j)
        want_dv = g4.sum(1)                                                            # [B,H,D]
        err = (got["dv"].double().reshape(B, Sk, H, D)[:, j] - want_dv).abs()
        # one bf16 rounding (half an ulp <= 2^-9 relative, so 2^-8 bounds it with the ulp's own granularity) of an fp32 sum of Sq terms
        assert bool((err <= 2.0 ** -8 * want_dv.abs() + Sq * 2.0 ** -24 * g4.abs().sum(1)).all()), j
        assert float(R.row_norms(got["dq"], B, Sq, H, D).max()) <= slack["dq"], j
        assert float(got["dk"].double().reshape(B, Sk, H, D)[:, j].norm(dim=-1).max()) <= slack["dk"], j


# ---- (c) the content of masked keys does not matter --------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["holes30", "tiles"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s[:5])))
def test_masked_key_content_is_ignored(dev, shape, pattern):
    """K and V rows of masked keys replaced by large finite values (randn * 2^10): O, lse2, dQ and the dK / dV rows of visible
    keys are bitwise unchanged, the dK / dV rows of masked keys are exactly 0 in both runs.  (Finite only: see the header.)"""
    c = _case(shape, pattern)
    B, H, Sq, Sk, D, causal = shape
    masked = torch.isinf(c["kb"])                                                      # [B,Sk]
    assert bool(masked.any())
    g = torch.Generator().manual_seed(99)
    rows = masked.reshape(B * Sk, 1)
    k2 = torch.where(rows, (torch.randn(B * Sk, H * D, generator=g) * 1024.0).bfloat16(), c["k"])
    v2 = torch.where(rows, (torch.randn(B * Sk, H * D, generator=g) * 1024.0).bfloat16(), c["v"])
    a = _run(dev, shape, c["q"], c["k"], c["v"], c["do"], c["kb"], c["scale"])
    b = _run(dev, shape, c["q"], k2, v2, c["do"], c["kb"], c["scale"])
    for n in ("o", "lse2", "dq"):
        assert torch.equal(a[n], b[n]), n
    for n in ("dk", "dv"):
        a4, b4 = a[n].reshape(B, Sk, H, D), b[n].reshape(B, Sk, H, D)
        assert torch.equal(a4[~masked], b4[~masked]), n
        assert bool((a4[masked] == 0).all()) and bool((b4[masked] == 0).all()), n


# ---- (d) empty rows ----------------------------------------------------------------------------------------------------
def _mult(dev, B, H, Sq, Sk, p, seed):
    from lc2is_amd import ops
    peff = round(p * 65536) / 65536.0                # the kernels quantise p to 16 bits (tests/test_gpu_dropout.py)
    return (ops.dropout_mask(B * H * Sq, Sk, p, seed, dev).double().cpu() / (1.0 - peff)).reshape(B, H, Sq, Sk)


def _case_dropout(dev, shape, pattern, p, seed):
    c = dict(_case(shape, pattern))
    B, H, Sq, Sk, D, causal = shape
    mult = _mult(dev, B, H, Sq, Sk, p, seed)
    args = (B, H, Sq, Sk, D, c["scale"], causal, c["kb"], mult)
    c["ref"] = R.attention_ref_grads(c["q"], c["k"], c["v"], c["do"], *args)
    c["rounded"] = R.attention_rounded(c["q"], c["k"], c["v"], c["do"], *args)
    return c


EMPTY_CASES = [(SHAPES[0], "empty_batch1", 0.0), (SHAPES[5], "empty_batch0", 0.0), (SHAPES[3], "lead5", 0.0),
               (SHAPES[3], "lead64", 0.0), (SHAPES[3], "lead70", 0.0), (SHAPES[0], "empty_batch1", 0.2)]
# (The dropout case is the masked batch element, not lead(j): under lead(j) query j sees key j alone, and with dropout its
#  O = v_j / (1 - p) is no bf16 number, so delta = rowsum(dO . O) carries O's rounding at full size against an exact dQ of 0 —
#  the rounded emulation itself leaves the per-row form there, as any flash-style backward does.  Without dropout O = v_j exactly.)


@pytest.mark.parametrize("shape,pattern,p", EMPTY_CASES,
                         ids=[f"{'x'.join(map(str, s[:5]))}-{pt}-p{p}" for s, pt, p in EMPTY_CASES])
def test_empty_rows(dev, shape, pattern, p):
    """A fully masked batch element, and causal rows whose leading keys are masked (empty and non-empty rows in one 32-row group
    and one 64-row tile): O rows exactly 0, lse2 exactly -inf, dQ rows exactly 0, everything else finite and within the
    bounds of (a) against the reference."""
    B, H, Sq, Sk, D, causal = shape
    seed = 0xC0FFEE1234 + Sq
    c = _case(shape, pattern) if p == 0.0 else _case_dropout(dev, shape, pattern, p, seed)
    n_empty = H * Sq if pattern.startswith("empty_batch") else B * H * int(pattern[4:])
    assert int(torch.isinf(c["ref"]["lse"]).sum()) == n_empty
    got = _run(dev, shape, c["q"], c["k"], c["v"], c["do"], c["kb"], c["scale"], p=p, seed=seed)
    _check_parity(f"{'x'.join(map(str, shape[:5]))}{'c' if causal else ''}/{pattern}/p{p}", got, c, shape)
    if p > 0.0:
        _check_dropout_whole(got, c["ref"])


# ---- (e) dropout with holes --------------------------------------------------------------------------------------------
def _check_dropout_whole(got, ref):
    """The whole-tensor bounds of tests/test_gpu_dropout.py::test_attention_probability_dropout_fwd_bwd, next to those of (a),
    which _check_parity applies to the dropout cases unchanged (O max-abs 2e-2, O rel 6e-3, gradients rel 1.5e-2)."""
    def rel(a, b):
        return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))
    assert rel(got["o"], ref["o"]) < 8e-3
    for n in ("dq", "dk", "dv"):
        assert rel(got[n], ref[n]) < 1.5e-2, n


@pytest.mark.parametrize("pattern", ["holes30", "finite_holes"])
def test_dropout_with_holes(dev, pattern):
    """p = 0.2 with the exported decisions: the normaliser (lse2) comes from the UNDROPPED probabilities, everything else as (a)
    against the reference run with the same keep / (1 - p) multipliers."""
    shape = SHAPES[0]
    B, H, Sq, Sk, D, causal = shape
    p, seed = 0.2, 0x1234567890ABCDEF + len(pattern)
    c = _case_dropout(dev, shape, pattern, p, seed)
    assert torch.equal(c["ref"]["lse"], _case(shape, pattern)["ref"]["lse"])
    got = _run(dev, shape, c["q"], c["k"], c["v"], c["do"], c["kb"], c["scale"], p=p, seed=seed)
    _check_parity(f"{'x'.join(map(str, shape[:5]))}/{pattern}/p{p}", got, c, shape)
    _check_dropout_whole(got, c["ref"])
    plain = _run(dev, shape, c["q"], c["k"], c["v"], c["do"], c["kb"], c["scale"], bwd=False)
    assert not torch.equal(plain["o"], got["o"])


# ---- (f) reproducibility -----------------------------------------------------------------------------------------------
def test_masked_backward_is_bitwise_reproducible(dev):
    shape = SHAPES[0]
    c = _case(shape, "finite_holes")
    runs = [_run(dev, shape, c["q"], c["k"], c["v"], c["do"], c["kb"], c["scale"]) for _ in range(3)]
    for r in runs[1:]:
        for n in ("o", "lse2", "dq", "dk", "dv"):
            assert torch.equal(runs[0][n], r[n]), n


# ---- (g) module level --------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_decoder_block_scattered_memory_mask_vs_oracle(dev):
    """DecoderBlock with the weights of tests/golden/decoder_d96.pt and a memory_key_padding_mask that is a subset, not a
    suffix (which class embeddings an image has), against the CPU oracle; the bounds of test_decoder_block_d96_vs_reference."""
    import lc2is_amd.nn as N
    from oracle import ref_cpu as O
    fx = torch.load(G / "decoder_d96.pt", weights_only=True)
    Bm, Sm = fx["kpm"].shape
    base = torch.tensor([[True, False, True, False, False, True, False], [False, True, True, True, True, True, True]])
    kpm = torch.stack([base[i % 2].repeat((Sm + 6) // 7)[:Sm] for i in range(Bm)])
    assert bool((~kpm).any(dim=1).all()) and bool(kpm[:, :-1].any()) and not torch.equal(kpm, fx["kpm"])
    blk = N.DecoderBlock(N.DecoderLayer(192, 128, 2, dim_feedforward=128, dropout=0, batch_first=True, norm_first=True), 2)
    blk.load_state_dict(fx["state_dict"], strict=True)
    blk = blk.to(dev)
    tgt = fx["tgt"].to(dev).requires_grad_(True)
    mem = fx["memory"].to(dev).requires_grad_(True)
    out = blk(tgt=tgt, memory=mem, memory_key_padding_mask=kpm.to(dev))
    out.backward(fx["dout"].to(dev))
    sd = {k: v.clone().requires_grad_(True) for k, v in fx["state_dict"].items()}
    tr, mr = fx["tgt"].clone().requires_grad_(True), fx["memory"].clone().requires_grad_(True)
    ref = O.decoder_block(sd, "", tr, mr, nhead=2, num_layers=2, norm_first=True, memory_key_padding_mask=kpm)
    ref.backward(fx["dout"])
    suffix = O.decoder_block(fx["state_dict"], "", fx["tgt"], fx["memory"], nhead=2, num_layers=2, norm_first=True,
                             memory_key_padding_mask=fx["kpm"])
    assert _rel(suffix, ref.detach()) > 3e-2                     # the scattered mask is another function than the fixture's
    assert _rel(out, ref.detach()) < 1e-2
    assert _rel(tgt.grad, tr.grad) < 3e-2 and _rel(mem.grad, mr.grad) < 3e-2
    # memory rows of masked keys receive no gradient through the cross attention of any layer
    assert bool((mem.grad[kpm.to(dev)] == 0).all()) and bool((mr.grad[kpm] == 0).all())
    named = dict(blk.named_parameters())
    for k in fx["grads"]:
        r = _rel(named[k].grad, sd[k].grad)
        assert r < 8e-2, (k, r)
