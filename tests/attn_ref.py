"""Softmax attention with an additive key bias restated in plain fp64 torch, on the token-major 2-D views the ops use
(q [B*Sq, H*D], k / v [B*Sk, H*D]), the same computation with the kernels' documented bf16 rounding points, the per-row
comparison the GPU tests apply, and seeded key-bias patterns.  No GPU code, nothing from lc2is_amd.

Contract restated here (include/lc2is_hip.h, attention section): kbias is fp32 [B,Sk], any finite value or -inf per key.  A
query row with no visible key (every key -inf, the causal mask included) has P = 0, O = 0, lse = -inf, receives no gradient
and gives none.  softmax is written exp(s - m) / sum with guarded `where`, so autograd carries that convention."""
import math

import torch

NEG_INF = float("-inf")


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and return in x's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def _heads(x, B, S, H, D):
    return x.double().reshape(B, S, H, D).transpose(1, 2)          # [B,H,S,D]


def _flat(x4, B, S, H, D):
    return x4.transpose(1, 2).reshape(B * S, H * D)


def _scores(q4, k4, Sq, Sk, scale, causal, kbias):
    s = q4 @ k4.transpose(-1, -2) * scale
    if kbias is not None:      # [B,Sk]; a [B,H,Sk] bias (one head differs) is taken too: the planted faults of the CPU tests use it
        kb = kbias.double().to(s.device)
        s = s + (kb[:, None, None, :] if kb.dim() == 2 else kb[:, :, None, :])
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).triu(1), NEG_INF)
    return s


def _softmax_parts(s):
    """m (0 on empty rows), e = exp(s - m), l = sum e, p = e / l (0 on empty rows), lse (-inf on empty rows)."""
    vis = torch.isfinite(s) | (s == float("inf"))
    m = s.detach().amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(vis, torch.exp(torch.where(vis, s, torch.zeros_like(s)) - m), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    some = l > 0
    l1 = torch.where(some, l, torch.ones_like(l))
    p = e / l1
    lse = torch.where(some, m + torch.log(l1), torch.full_like(l, NEG_INF)).squeeze(-1)
    return e, l1, p, lse


def attention_ref(q, k, v, B, H, Sq, Sk, D, scale, causal, kbias, mult=None):
    """fp64.  Returns (o [B*Sq, H*D], lse [B,H,Sq] in natural units); differentiable in q, k, v.  mult: optional [B,H,Sq,Sk]
    keep / (1 - p) multiplier on the probabilities (the normaliser comes from the undropped ones)."""
    q4, k4, v4 = _heads(q, B, Sq, H, D), _heads(k, B, Sk, H, D), _heads(v, B, Sk, H, D)
    s = _scores(q4, k4, Sq, Sk, scale, causal, kbias)
    _, _, p, lse = _softmax_parts(s)
    pd = p if mult is None else p * mult.double().to(p.device)
    return _flat(pd @ v4, B, Sq, H, D), lse


def attention_ref_grads(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kbias, mult=None):
    """attention_ref and its autograd backward for the upstream gradient `do`: dict(o, lse, dq, dk, dv), all fp64."""
    qd, kd, vd = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    o, lse = attention_ref(qd, kd, vd, B, H, Sq, Sk, D, scale, causal, kbias, mult)
    o.backward(do.double())
    return dict(o=o.detach(), lse=lse.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)


def attention_rounded(q, k, v, do, B, H, Sq, Sk, D, scale, causal, kbias, mult=None):
    """The same computation in fp64 with the kernels' documented roundings: exp(s - m) (times the dropout multiplier) to bf16
    before P.V; O to bf16; delta = rowsum(dO . O) from that O; dS = P (dP - delta) to bf16 before the dQ / dK products; P to bf16
    before dV; dQ, dK, dV to bf16.  Returns the same dict as attention_ref_grads.  Its per-row error against attention_ref is
    the rounding floor of a case."""
    q4, k4, v4 = _heads(q, B, Sq, H, D), _heads(k, B, Sk, H, D), _heads(v, B, Sk, H, D)
    g4 = _heads(do, B, Sq, H, D)
    mu = None if mult is None else mult.double()
    s = _scores(q4, k4, Sq, Sk, scale, causal, kbias)
    e, l1, p, lse = _softmax_parts(s)
    ed = e if mu is None else e * mu
    o4 = bf16r(bf16r(ed) @ v4 / l1)
    delta = (g4 * o4).sum(-1, keepdim=True)
    dp = g4 @ v4.transpose(-1, -2)
    if mu is not None:
        dp = dp * mu
    ds = bf16r(p * (dp - delta))
    dq4 = bf16r(ds @ k4 * scale)
    dk4 = bf16r(ds.transpose(-1, -2) @ q4 * scale)
    dv4 = bf16r(bf16r(p if mu is None else p * mu).transpose(-1, -2) @ g4)
    return dict(o=_flat(o4, B, Sq, H, D), lse=lse, dq=_flat(dq4, B, Sq, H, D), dk=_flat(dk4, B, Sk, H, D),
                dv=_flat(dv4, B, Sk, H, D))


# ---- the per-row comparison ------------------------------------------------------------------------------------------
FACTOR = 3.0     # the kernel's rounding is another realisation of the noise the emulation samples once


def row_norms(x, B, S, H, D):
    """[B*S, H*D] -> the D-vector norm of every (b, s, h) row, fp64 [B,S,H]."""
    return x.double().cpu().reshape(B, S, H, D).norm(dim=-1)


def abs_slack(D, scale, do, k, v):
    """Allowance for rows whose exact value is zero or nearly so, derived: fp32 roundoff of a D-term product chain
    (D * 2^-24) with a factor 4 of slack on the magnitudes the chain multiplies.  One bf16 ulp of that quantity (2^-8 of it)
    is added.  `dq` / `dk` carry scale * dO * V * K (the issue's quantity); O carries only V and dV only dO."""
    mo, mk, mv = (float(t.double().abs().max()) for t in (do, k, v))
    u = D * 2.0 ** -22 * (1.0 + 2.0 ** -8)
    g = u * scale * mo * mk * mv
    return dict(o=u * mv, dq=g, dk=g, dv=u * mo)


def floor_rel(rounded, ref, slack, B, S, H, D):
    """Largest per-row relative error of the rounded emulation against the exact reference: max over the rows with a nonzero
    exact norm of (||rounded - ref|| - slack)+ / ||ref||, i.e. the smallest floor with which the emulation itself meets
    ||err|| <= floor * ||ref|| + slack on every row (a row whose exact value is zero or nearly so is the slack's business; taking
    the slack off can only lower the floor).  Note what this says about a case: where softmax is nearly one-hot, the exact dQ row
    is tiny while delta = rowsum(dO . O) carries the 2^-9 rounding of O at full size, so the dQ floor of such a case is large —
    that is the documented arithmetic, and test (b) pins the exactly one-hot case instead."""
    rn = row_norms(ref, B, S, H, D)
    en = row_norms(rounded.double().cpu() - ref.double().cpu(), B, S, H, D)
    nz = rn > 0
    return float(((en[nz] - slack).clamp_min(0.0) / rn[nz]).max()) if bool(nz.any()) else 0.0


def row_check(got, ref, rounded, slack, B, S, H, D):
    """Per-row bound  ||got - ref|| <= FACTOR * floor_rel * ||ref|| + slack.  Returns (ok, ratio, floor): ratio is the worst
    row's (||got - ref|| - slack)+ / (floor_rel * ||ref||), i.e. the observed multiple of the floor (<= FACTOR iff ok)."""
    fl = floor_rel(rounded, ref, slack, B, S, H, D)
    rn = row_norms(ref, B, S, H, D)
    en = row_norms(got.double().cpu() - ref.double().cpu(), B, S, H, D)
    if not bool(torch.isfinite(en).all()):
        return False, float("inf"), fl
    ok = bool((en <= FACTOR * fl * rn + slack).all())
    excess = (en - slack).clamp_min(0.0)
    den = fl * rn
    ratio = torch.where(excess > 0, excess / den.clamp_min(1e-300), torch.zeros_like(excess))
    return ok, float(ratio.max()), fl


def compare_rows(got: dict, ref: dict, rounded: dict, slack: dict, B, H, Sq, Sk, D):
    """row_check of o, dq (rows (b, q, h)) and dk, dv (rows (b, key, h)): dict name -> (ok, ratio, floor)."""
    out = {}
    for name in ("o", "dq", "dk", "dv"):
        if name in got:
            S = Sq if name in ("o", "dq") else Sk
            out[name] = row_check(got[name], ref[name], rounded[name], slack[name], B, S, H, D)
    return out


def whole_tensor_failures(got: dict, ref: dict, zero_below: dict | None = None):
    """The whole-tensor bounds of tests/test_gpu_attention.py, unchanged: O max-abs 2e-2 and relative L2 6e-3, lse 2e-3 (natural
    units, over the non-empty rows), gradients relative L2 1.5e-2.  Returns the list of (name, figure) that exceed them.
    zero_below: per gradient, the norm at or below which the EXACT tensor counts as zero (one visible key: dQ = dK = 0 exactly,
    and no implementation is relatively close to 0); such a tensor is left to the per-row bound, whose slack is absolute."""
    bad = []

    def rel(a, b):
        return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30))

    err = float((got["o"].double().cpu() - ref["o"].cpu()).abs().max())
    if not err < 2e-2:
        bad.append(("o_abs", err))
    r = rel(got["o"], ref["o"])
    if not r < 6e-3:
        bad.append(("o_rel", r))
    if "lse" in got:
        gl, rl = got["lse"].double().cpu(), ref["lse"].cpu()
        fin = torch.isfinite(rl)
        e = float((gl[fin] - rl[fin]).abs().max()) if bool(fin.any()) else 0.0
        if not e < 2e-3:
            bad.append(("lse", e))
    for n in ("dq", "dk", "dv"):
        if n in got and not (zero_below and float(ref[n].norm()) <= zero_below[n]):
            r = rel(got[n], ref[n])
            if not r < 1.5e-2:
                bad.append((n + "_rel", r))
    return bad


# ---- key-bias patterns ([B,Sk] fp32 from a seeded CPU generator) --------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def _ensure_visible(kb, causal, fill=0.0):
    """At least one visible key per query row: with a causal mask row 0 sees key 0 only, so key 0; otherwise any key (the
    last one is opened where a batch element has none).  Consequence for the causal shape: key 0 is always visible, so no
    pattern that goes through here masks the whole first tile under a causal mask; a row whose first frame is formed late
    TOGETHER with the diagonal is reached by lead(64) / lead(70) instead, whose first 64 / 70 rows are empty by design."""
    if causal:
        kb[:, 0] = torch.where(torch.isinf(kb[:, 0]), torch.full_like(kb[:, 0], fill), kb[:, 0])
    else:
        none = torch.isinf(kb).all(dim=1)
        kb[none, -1] = fill
    return kb


def holes(B, Sk, p, seed, causal=False):
    """Bernoulli(p) of the keys masked."""
    kb = torch.zeros(B, Sk)
    kb[torch.rand(B, Sk, generator=_gen(seed)) < p] = NEG_INF
    return _ensure_visible(kb, causal)


def sparse(B, Sk, seed, causal=False):
    """About 5 % of the keys visible."""
    return holes(B, Sk, 0.95, seed, causal)


def tiles(B, Sk, seed=0, causal=False):
    """Whole 64-key tiles masked — tile 0 (a row's first frame is formed late) and tile 2 or 3 — and one 32-key half of
    tile 1; batch element b (plus seed) picks which.  Slices past Sk are empty."""
    kb = torch.zeros(B, Sk)
    for b in range(B):
        o = (b + seed) % 2
        for t in (0, 2 + o):
            kb[b, 64 * t:64 * t + 64] = NEG_INF
        kb[b, 64 + 32 * o:96 + 32 * o] = NEG_INF
    return _ensure_visible(kb, causal)


def finite(B, Sk, seed, causal=False):
    return (torch.randn(B, Sk, generator=_gen(seed)) * 3.0).float()


def finite_holes(B, Sk, seed, causal=False):
    g = _gen(seed)
    kb = (torch.randn(B, Sk, generator=g) * 3.0).float()
    kb[torch.rand(B, Sk, generator=g) < 0.3] = NEG_INF
    return _ensure_visible(kb, causal)


def soft(B, Sk, seed, causal=False):
    """Finite values in +-20 (e^-40 between the extremes: keys that are all but masked, none exactly)."""
    return ((torch.rand(B, Sk, generator=_gen(seed)) * 2.0 - 1.0) * 20.0).float()


def single(B, Sk, j, value=0.0):
    """Only key j visible (with bias `value`)."""
    kb = torch.full((B, Sk), NEG_INF)
    kb[:, j] = value
    return kb


def empty_batch(B, Sk, seed, which=0):
    """Batch element `which` fully masked (H * Sq empty rows), Bernoulli(0.3) holes elsewhere."""
    kb = holes(B, Sk, 0.3, seed)
    kb[which] = NEG_INF
    return kb


def lead(B, Sk, j):
    """Keys < j masked.  With the causal mask, queries 0 .. j-1 of every (b, h) see nothing: exactly j empty rows."""
    kb = torch.zeros(B, Sk)
    kb[:, :j] = NEG_INF
    return kb


def count_empty_rows(kbias, B, H, Sq, Sk, causal):
    """Number of (b, h, q) rows with no visible key."""
    vis = ~torch.isinf(kbias)[:, None, :].expand(B, Sq, Sk)
    if causal:
        vis = vis & ~torch.ones(Sq, Sk, dtype=torch.bool).triu(1)
    return int((~vis.any(-1)).sum()) * H


def make_inputs(B, H, Sq, Sk, D, seed, do_scale=1.0):
    """bf16 q, k, v, do on the CPU from one seeded generator."""
    g = _gen(seed)
    q = torch.randn(B * Sq, H * D, generator=g).bfloat16()
    k = torch.randn(B * Sk, H * D, generator=g).bfloat16()
    v = torch.randn(B * Sk, H * D, generator=g).bfloat16()
    do = (torch.randn(B * Sq, H * D, generator=g) * do_scale).bfloat16()
    return q, k, v, do


LOG2E = 1.0 / math.log(2.0)
