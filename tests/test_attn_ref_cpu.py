"""CPU: the attention reference of tests/attn_ref.py is right, its pattern generators keep their guarantees, and the per-row
comparison that tests/test_gpu_attention_masks.py applies to the kernels can fail."""
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attn_ref as R

INF = float("inf")


def _sdpa(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kbias):
    """torch's scaled_dot_product_attention in fp64 with a float attn_mask; dict(o, lse, dq, dk, dv)."""
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    q4, k4, v4 = (t.reshape(B, S, H, D).transpose(1, 2) for t, S in ((qd, Sq), (kd, Sk), (vd, Sk)))
    mask = kbias.double()[:, None, None, :].expand(B, 1, Sq, Sk).clone()
    if causal:
        mask = mask.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), -INF)
    o = F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask, scale=scale).transpose(1, 2).reshape(B * Sq, H * D)
    o.backward(do.double())
    lse = torch.logsumexp(q4.detach() @ k4.detach().transpose(-1, -2) * scale + mask, -1)
    return dict(o=o.detach(), lse=lse, dq=qd.grad, dk=kd.grad, dv=vd.grad)


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-11, atol=1e-12 * max(1.0, float(b.abs().max())))


@pytest.mark.parametrize("pattern", ["holes", "sparse", "tiles", "finite", "finite_holes", "soft", "single"])
@pytest.mark.parametrize("B,H,Sq,Sk,D,causal", [(2, 2, 70, 193, 64, False), (2, 3, 97, 97, 32, True)])
def test_reference_matches_torch_sdpa(pattern, B, H, Sq, Sk, D, causal):
    """Rows with a visible key: output, lse and the three gradients equal torch's fp64 sdpa with a float mask."""
    kb = {"holes": lambda: R.holes(B, Sk, 0.5, 1, causal), "sparse": lambda: R.sparse(B, Sk, 2, causal),
          "tiles": lambda: R.tiles(B, Sk, 0, causal), "finite": lambda: R.finite(B, Sk, 3),
          "finite_holes": lambda: R.finite_holes(B, Sk, 4, causal), "soft": lambda: R.soft(B, Sk, 5),
          "single": lambda: R.single(B, Sk, 0 if causal else Sk - 1, 1.5)}[pattern]()
    assert R.count_empty_rows(kb, B, H, Sq, Sk, causal) == 0
    q, k, v, do = R.make_inputs(B, H, Sq, Sk, D, 17)
    scale = D ** -0.5
    ref = R.attention_ref_grads(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kb)
    want = _sdpa(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kb)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert _close(ref[n], want[n]), n


@pytest.mark.parametrize("case", ["empty_batch", "lead5", "lead70"])
def test_reference_empty_row_convention(case):
    """Empty rows: O = 0, lse = -inf, dQ = 0, nothing reaches dK / dV from them.  The other rows equal torch's sdpa on a problem
    in which the empty rows are opened (bias 0 on their keys would change other rows, so instead their upstream gradient is
    zeroed and the rows are compared only where both are defined)."""
    if case == "empty_batch":
        B, H, Sq, Sk, D, causal = 2, 2, 40, 130, 64, False
        kb = R.empty_batch(B, Sk, 6, which=1)
        n_empty = H * Sq
    else:
        j = int(case[4:])
        B, H, Sq, Sk, D, causal = 2, 2, 100, 100, 64, True
        kb = R.lead(B, Sk, j)
        n_empty = B * H * j
    assert R.count_empty_rows(kb, B, H, Sq, Sk, causal) == n_empty
    q, k, v, do = R.make_inputs(B, H, Sq, Sk, D, 23)
    scale = D ** -0.5
    ref = R.attention_ref_grads(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kb)
    empty = torch.isinf(ref["lse"])                                   # [B,H,Sq]
    assert int(empty.sum()) == n_empty and bool((ref["lse"][empty] == -INF).all())
    er = empty.transpose(1, 2)                                        # [B,Sq,H]
    for n in ("o", "dq"):
        assert bool((ref[n].reshape(B, Sq, H, D)[er] == 0).all()), n
    for n in ("o", "dq", "dk", "dv"):
        assert bool(torch.isfinite(ref[n]).all()), n
    # the same problem without the empty rows' queries: drop them by zeroing their dO and giving them one visible key through a
    # per-row mask — torch then has no NaN, and those rows touch nothing else
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    q4, k4, v4 = (t.reshape(B, S, H, D).transpose(1, 2) for t, S in ((qd, Sq), (kd, Sk), (vd, Sk)))
    mask = kb.double()[:, None, None, :].expand(B, H, Sq, Sk).clone()
    if causal:
        mask = mask.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), -INF)
    mask[..., 0] = torch.where(empty, torch.zeros(()).double(), mask[..., 0])
    do2 = do.double().reshape(B, Sq, H, D).clone()
    do2[er] = 0
    o = F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask, scale=scale).transpose(1, 2).reshape(B * Sq, H * D)
    o.backward(do2.reshape(B * Sq, H * D))
    keep = ~er
    assert _close(ref["o"].reshape(B, Sq, H, D)[keep], o.detach().reshape(B, Sq, H, D)[keep])
    assert _close(ref["dq"].reshape(B, Sq, H, D)[keep], qd.grad.reshape(B, Sq, H, D)[keep])
    assert _close(ref["dk"], kd.grad) and _close(ref["dv"], vd.grad)
    # the rounded emulation follows the same convention
    rd = R.attention_rounded(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kb)
    assert bool((rd["o"].reshape(B, Sq, H, D)[er] == 0).all()) and bool((rd["dq"].reshape(B, Sq, H, D)[er] == 0).all())
    assert all(bool(torch.isfinite(rd[n]).all()) for n in ("o", "dq", "dk", "dv"))


def test_dropout_multiplier_and_normaliser():
    """mult scales the probabilities after normalisation: lse is that of the undropped scores, and the result equals the
    explicit softmax -> multiply -> P.V."""
    B, H, Sq, Sk, D = 1, 2, 33, 70, 64
    q, k, v, do = R.make_inputs(B, H, Sq, Sk, D, 5)
    kb = R.finite_holes(B, Sk, 8)
    mult = (torch.rand(B, H, Sq, Sk, generator=torch.Generator().manual_seed(1)) >= 0.2).double() / 0.8
    ref = R.attention_ref_grads(q, k, v, do, B, H, Sq, Sk, D, 0.125, False, kb, mult)
    plain = R.attention_ref_grads(q, k, v, do, B, H, Sq, Sk, D, 0.125, False, kb)
    assert torch.equal(ref["lse"], plain["lse"]) and not _close(ref["o"], plain["o"])
    qd, kd, vd = (t.double().reshape(B, S, H, D).transpose(1, 2).requires_grad_(True) for t, S in ((q, Sq), (k, Sk), (v, Sk)))
    s = qd @ kd.transpose(-1, -2) * 0.125 + kb.double()[:, None, None, :]
    o = ((torch.softmax(s, -1) * mult) @ vd).transpose(1, 2).reshape(B * Sq, H * D)
    o.backward(do.double())
    assert _close(ref["o"], o.detach())
    for n, g, S in (("dq", qd.grad, Sq), ("dk", kd.grad, Sk), ("dv", vd.grad, Sk)):
        assert _close(ref[n], g.transpose(1, 2).reshape(B * S, H * D)), n


def test_generators_keep_their_guarantees():
    for B, H, Sq, Sk, causal in [(2, 2, 193, 193, False), (1, 2, 130, 321, False), (2, 2, 200, 200, True), (2, 8, 256, 16, False),
                                 (1, 3, 65, 449, False), (3, 1, 5, 3, False)]:
        for seed in range(4):
            pats = dict(holes3=R.holes(B, Sk, 0.3, seed, causal), holes7=R.holes(B, Sk, 0.7, seed, causal),
                        sparse=R.sparse(B, Sk, seed, causal), tiles=R.tiles(B, Sk, seed, causal),
                        finite=R.finite(B, Sk, seed), finite_holes=R.finite_holes(B, Sk, seed, causal), soft=R.soft(B, Sk, seed),
                        single=R.single(B, Sk, 0 if causal else Sk - 1))
            for name, kb in pats.items():
                assert kb.shape == (B, Sk) and kb.dtype == torch.float32, name
                assert not bool(torch.isnan(kb).any()) and not bool((kb == INF).any()), name
                assert R.count_empty_rows(kb, B, H, Sq, Sk, causal) == 0, (name, B, Sk, causal, seed)
            assert bool(torch.isfinite(pats["finite"]).all()) and bool(torch.isfinite(pats["soft"]).all())
            assert float(pats["soft"].abs().max()) <= 20.0
            assert int((~torch.isinf(pats["single"])).sum()) == B
            if not causal:
                assert R.count_empty_rows(R.empty_batch(B, Sk, seed, which=B - 1), B, H, Sq, Sk, False) == H * Sq
    # the patterns do what their names say at a size with room for it
    B, Sk = 2, 449
    assert 0.25 < float(torch.isinf(R.holes(B, Sk, 0.3, 0)).float().mean()) < 0.35
    assert 0.90 < float(torch.isinf(R.sparse(B, Sk, 0)).float().mean()) < 0.99
    t = torch.isinf(R.tiles(B, Sk, 0))
    assert bool(t[:, :64].all()) and bool(t[0, 128:192].all()) and bool(t[1, 192:256].all())      # whole tiles, tile 0 among them
    assert bool(t[0, 64:96].all()) and not bool(t[0, 96:128].any()) and bool(t[1, 96:128].all()) and not bool(t[1, 64:96].any())
    assert 0.2 < float(torch.isinf(R.finite_holes(B, Sk, 0)).float().mean()) < 0.4
    for j in (5, 64, 70):
        assert R.count_empty_rows(R.lead(2, 200, j), 2, 2, 200, 200, True) == 2 * 2 * j


# ---- the check can fail ------------------------------------------------------------------------------------------------
_B, _H, _S, _D = 2, 2, 193, 64          # ragged 1-key last tile
_SCALE = _D ** -0.5


def _family(name):
    causal = name.startswith("lead")
    S = 200 if causal else _S
    kb = {"holes": lambda: R.holes(_B, S, 0.5, 11), "sparse": lambda: R.sparse(_B, S, 12), "tiles": lambda: R.tiles(_B, S, 0),
          "finite": lambda: R.finite(_B, S, 13), "finite_holes": lambda: R.finite_holes(_B, S, 14), "soft": lambda: R.soft(_B, S, 15),
          "single": lambda: R.single(_B, S, S - 1, 0.75),
          "empty_batch": lambda: R.empty_batch(_B, S, 16, which=1), "lead": lambda: R.lead(_B, S, 70)}[name]()
    return kb, S, causal


def _plant(fault, kb, q, k, v, do, S, causal, weighty):
    """The rounded emulation, broken the way a kernel could be; None where the pattern has no place for the fault.
    weighty [B,S,H]: keys whose exact dV row stands well above the absolute slack."""
    args = (_B, _H, S, S, _D, _SCALE, causal)
    kbh = kb[:, None, :].expand(_B, _H, S).clone()                  # per-head bias: the fault hits one (b, h)
    b, h = 1, 1
    if fault == "masked_key_visible":
        js = torch.nonzero(torch.isinf(kb[b])).flatten()
        if len(js) == 0 or bool(torch.isinf(kb[b]).all()):
            return None
        kbh[b, h, js[len(js) // 2]] = 0.0
    elif fault == "finite_bias_dropped":
        # a key that carries weight in this (b, h) — one whose bias lies far below the row's largest is as good as masked, and
        # no check can see its bias — and whose bias is not nearly zero already
        js = torch.nonzero((kb[b].abs() >= 0.5) & ~torch.isinf(kb[b]) & weighty[b, :, h]).flatten()
        if int((~torch.isinf(kb[b])).sum()) < 2:     # one visible key: softmax is shift-invariant, its bias shows in lse alone
            return None
        if len(js) == 0:
            return None
        kbh[b, h, js[0]] = 0.0
    elif fault == "ragged_key_left_out":
        bs = [i for i in range(_B) if bool(weighty[i, S - 1, h]) and int((~torch.isinf(kb[i])).sum()) > 1]   # (not alone, and it matters)
        if not bs or S % 64 != 1:
            return None
        kbh[bs[-1], h, S - 1] = -INF
    elif fault == "empty_row_uniform":
        out = R.attention_rounded(q, k, v, do, *args, kb)
        empty = torch.isinf(out["lse"]).transpose(1, 2)             # [B,S,H]
        if not bool(empty.any()):
            return None
        o4, dv4 = out["o"].reshape(_B, S, _H, _D).clone(), out["dv"].reshape(_B, S, _H, _D).clone()
        v4, g4 = v.double().reshape(_B, S, _H, _D), do.double().reshape(_B, S, _H, _D)
        o4 = torch.where(empty[..., None], R.bf16r(v4.mean(1, keepdim=True)).expand_as(o4), o4)
        dv4 = dv4 + R.bf16r((g4 * empty[..., None]).sum(1, keepdim=True) / S)
        out["o"], out["dv"] = o4.reshape(_B * S, -1), dv4.reshape(_B * S, -1)
        return out
    return R.attention_rounded(q, k, v, do, *args, kbh)


FAULTS = ["masked_key_visible", "finite_bias_dropped", "ragged_key_left_out", "empty_row_uniform"]
FAMILIES = ["holes", "sparse", "tiles", "finite", "finite_holes", "soft", "single", "empty_batch", "lead"]
# which (family, fault) pairs the whole-tensor bounds of tests/test_gpu_attention.py ACCEPT (recorded from this test; it
# asserts the record)
WHOLE_TENSOR_ACCEPTS = {
    ("finite", "finite_bias_dropped"),          # per-row: dK row 301x, dV row 343x the floor; whole-tensor: every bound met
    ("finite_holes", "masked_key_visible"),     # per-row: dK / dV rows of the key are nonzero where the exact ones are 0
}


@pytest.fixture(scope="module")
def planted():
    out = {}
    for fam in FAMILIES:
        kb, S, causal = _family(fam)
        q, k, v, do = R.make_inputs(_B, _H, S, S, _D, 31)
        args = (_B, _H, S, S, _D, _SCALE, causal, kb)
        ref = R.attention_ref_grads(q, k, v, do, *args)
        rounded = R.attention_rounded(q, k, v, do, *args)
        slack = R.abs_slack(_D, _SCALE, do, k, v)
        out[fam] = (kb, S, causal, (q, k, v, do), ref, rounded, slack)
    return out


def test_rounding_floor_is_the_expected_size(planted):
    """bf16 keeps 8 bits: a row of O summed from P rounded to 2^-9 relative and rounded once more lies 2e-3 .. 4e-3 from
    the exact one; the emulation itself passes the per-row bound (ratio 1 by construction) and the whole-tensor bounds."""
    for fam, (kb, S, causal, _, ref, rounded, slack) in planted.items():
        res = R.compare_rows(rounded, ref, rounded, slack, _B, _H, S, S, _D)
        assert all(ok for ok, _, _ in res.values()), fam
        assert all(ratio <= 1.0 + 1e-12 for _, ratio, _ in res.values()), fam
        if fam == "single":      # one visible key: P = 1 and O = V[j] are bf16 numbers, nothing is rounded
            assert res["o"][2] == 0.0
        else:
            assert 1.5e-3 < res["o"][2] < 6e-3, (fam, res["o"][2])
        assert R.whole_tensor_failures(rounded, ref) == [], fam


def test_per_row_check_rejects_planted_faults(planted):
    """Every applicable (pattern family, fault) pair is rejected by the per-row bound; every family meets at least one fault
    and every fault at least one family.

    What the whole-tensor bounds of tests/test_gpu_attention.py (O abs 2e-2 / rel 6e-3, lse 2e-3, gradients rel 1.5e-2)
    would have ACCEPTED of the same faults is recorded in WHOLE_TENSOR_ACCEPTS above and asserted here.  At this small shape
    (4 (b, h) pairs of 193 keys, so one key of one pair is 1/800 of the problem) they accept two of the fourteen outright:
    finite / finite_bias_dropped and finite_holes / masked_key_visible.  Two more pass every bound on O and on the gradients and
    are caught by the log-sum-exp alone, narrowly: soft / finite_bias_dropped (lse off by 3.9e-3 against 2e-3) and
    finite_holes / finite_bias_dropped (lse 1.1e-2; O max-abs 2.7e-2 against 2e-2).  The existing GPU cases are 5 to 100 times
    larger in (b, h, key) count, which dilutes one key's share of a whole-tensor norm by as much; the per-row bound does not
    dilute (the faulty key's dK / dV rows are 60 to 340 times the floor, or nonzero against an exact 0)."""
    hit_fam, hit_fault, accepted = set(), set(), set()
    for fam, (kb, S, causal, (q, k, v, do), ref, rounded, slack) in planted.items():
        for fault in FAULTS:
            weighty = R.row_norms(ref["dv"], _B, S, _H, _D) > 100.0 * slack["dv"]
            broken = _plant(fault, kb, q, k, v, do, S, causal, weighty)
            if broken is None:
                continue
            hit_fam.add(fam); hit_fault.add(fault)
            res = R.compare_rows(broken, ref, rounded, slack, _B, _H, S, S, _D)
            assert not all(ok for ok, _, _ in res.values()), (fam, fault, res)
            wt = R.whole_tensor_failures(broken, ref)
            print(fam, fault, "per-row ratios", {n: round(r[1], 1) for n, r in res.items()}, "whole-tensor failures", wt)
            if not wt:
                accepted.add((fam, fault))
    assert hit_fam == set(FAMILIES) and hit_fault == set(FAULTS)
    assert accepted == set(WHOLE_TENSOR_ACCEPTS), sorted(accepted)
