"""The fp64 references of tests/glue_ref.py checked against independent torch formulations, and the case lists of
tests/test_gpu_glue_edges.py shown to be able to fail — all without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G

BILINEAR_ATOL = 1e-5   # what the GPU test allows an fp32 bilinear output on N(0,1) data


def _tokens(B, h, w, C, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(B * h * w, C, generator=g, dtype=torch.float64)


def _nchw(x, B, h, w):
    return x.reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


def _tok(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


@pytest.mark.parametrize("case", G.BILINEAR_CASES + [(1, 6, 10, 4, 2)])   # (the big case's formula at a size a CPU likes)
def test_bilinear_reference_is_interpolate(case):
    B, h, w, C, S = case
    x = _tokens(B, h, w, C, 1)
    xn = _nchw(x, B, h, w).requires_grad_(True)
    ref = F.interpolate(xn, scale_factor=S, mode="bilinear", align_corners=False)
    mine = G.bilinear_up(x, B, h, w, S)
    assert mine.shape == (B * h * S * w * S, C)
    assert (mine - _tok(ref)).abs().max().item() < 1e-12
    dout = _tokens(B, h * S, w * S, C, 2)
    ref.backward(_nchw(dout, B, h * S, w * S))
    adj = G.bilinear_up_adjoint(dout, B, h, w, S)
    assert adj.shape == x.shape
    assert (adj - _tok(xn.grad)).abs().max().item() < 1e-12
    # <A x, g> == <x, A^T g>: the adjoint is the transpose of the forward, whatever autograd says
    assert abs((mine * dout).sum().item() - (x * adj).sum().item()) < 1e-9


def test_bilinear_big_case_exceeds_one_round_both_ways():
    B, h, w, C, S = G.BILINEAR_BIG
    assert B * h * w * (C // 4) > G.SP_GRID_ITEMS and B * h * S * w * S * (C // 4) > G.SP_GRID_ITEMS


@pytest.mark.parametrize("case", [c for c in G.BILINEAR_CASES if G.is_rectangular(c)])
def test_rectangular_bilinear_cases_notice_exchanged_h_w(case):
    """A kernel that exchanged h and w computes bilinear_up(x, B, w, h, S) on the same flat rows: the result has to be far
    outside what the GPU test tolerates, forward and backward, or the case could not catch the exchange."""
    B, h, w, C, S = case
    x = _tokens(B, h, w, C, 3)
    good, bad = G.bilinear_up(x, B, h, w, S), G.bilinear_up(x, B, w, h, S)
    assert good.shape == bad.shape   # flat token rows: only the values can tell
    if S == 1:   # the identity copies the flat rows whatever the grid is called: this one case cannot see the exchange, by nature
        assert torch.equal(good, x) and torch.equal(bad, x)
        return
    assert (good - bad).abs().max().item() > 100 * BILINEAR_ATOL
    dout = _tokens(B, h * S, w * S, C, 4)
    ga, ba = G.bilinear_up_adjoint(dout, B, h, w, S), G.bilinear_up_adjoint(dout, B, w, h, S)
    assert ((ga - ba).norm() / ga.norm()).item() > 100 * 1e-5


def test_bilinear_case_list_has_the_shapes_it_promises():
    rect = [c for c in G.BILINEAR_CASES if G.is_rectangular(c)]
    assert any(w > h for _, h, w, _, _ in rect) and any(h > w for _, h, w, _, _ in rect)
    assert any(h == 1 and w > 1 for _, h, w, _, _ in rect) and any(w == 1 and h > 1 for _, h, w, _, _ in rect)
    assert any(S == 1 for *_, S in G.BILINEAR_CASES) and any(S == 3 for *_, S in G.BILINEAR_CASES)


@pytest.mark.parametrize("B,h,w,C", G.SR_CASES[:3] + [(2, 6, 4, 8)])
def test_sr_gather_is_the_im2col_of_a_stride2_conv(B, h, w, C):
    g = torch.Generator(device="cpu").manual_seed(5)
    x = _tokens(B, h, w, C, 5)
    wt = torch.randn(C, C, 2, 2, generator=g, dtype=torch.float64)
    conv = F.conv2d(_nchw(x, B, h, w), wt, stride=2)
    wp = wt.permute(0, 2, 3, 1).reshape(C, 4 * C)   # [co][(2i+j)*C + ci]
    gth = G.sr_gather(x, B, h, w)
    assert gth.shape == (B * h * w // 4, 4 * C)
    mine = (gth @ wp.T).reshape(B, h // 2, w // 2, C).permute(0, 3, 1, 2)
    assert (mine - conv).abs().max().item() < 1e-12
    assert torch.equal(G.sr_scatter(gth, B, h, w), x)
    if h != w:   # the exchanged index map is another permutation
        assert not torch.equal(G.sr_gather(x, B, w, h), gth)


def test_sr_big_case_exceeds_one_round():
    B, h, w, C = G.SR_CASES[-1]
    assert B * h * w * C // 8 > G.SP_GRID_ITEMS


@pytest.mark.parametrize("B,H,ps,kpad", [c for c in G.PATCHIFY_CASES if c[1] <= 128])
def test_patchify_is_the_im2col_of_the_patch_conv(B, H, ps, kpad):
    g = torch.Generator(device="cpu").manual_seed(6)
    pix = torch.randn(B, 3, H, H, generator=g, dtype=torch.float64)
    wt = torch.randn(5, 3, ps, ps, generator=g, dtype=torch.float64)
    cols = G.patchify(pix, ps, kpad)
    k = 3 * ps * ps
    assert cols.shape == (B * (H // ps) ** 2, kpad or ((k + 63) // 64) * 64)
    assert cols[:, k:].abs().sum().item() == 0
    conv = F.conv2d(pix, wt, stride=ps).flatten(2).transpose(1, 2).reshape(-1, 5)
    assert (cols[:, :k] @ wt.reshape(5, k).T - conv).abs().max().item() < 1e-11


def test_grid_stride_cases_exceed_one_round():
    B, H, ps, _ = G.PATCHIFY_CASES[-1]
    assert ps % 8 == 0 and H % 8 == 0 and B * 3 * H * H // 8 > G.EW_GRID_ITEMS
    B, P, C = G.VIT_CASES[-1]
    assert B * (P + 1) * C // 4 > G.EW_GRID_ITEMS
    B, H, ps, _ = G.PATCHIFY_CASES[0]
    assert ps % 8 == 0 and H % 8 != 0 and H % ps != 0   # the scalar kernel on a vector-shaped patch, ragged image edge


def test_l2norm_reference_and_planted_rows():
    eps = 1e-6
    kinds = G.l2norm_kinds(eps)
    assert set(kinds) == {"zero", "half_eps", "two_eps", "huge", "norm_1e-7", "norm_1e-5"}
    assert set(G.l2norm_kinds(1e-12)) == {"zero", "half_eps", "two_eps", "huge"}
    x, where = G.l2norm_input(301, 260, eps, kinds, 7)
    assert where["zero"] == 0 and where["norm_1e-5"] == 300 and len(set(where.values())) == len(kinds)
    n = x.double().norm(dim=1)
    assert n[where["zero"]] == 0 and torch.isfinite(x).all()
    for kind, want in (("half_eps", 0.5 * eps), ("two_eps", 2 * eps), ("norm_1e-7", 1e-7), ("norm_1e-5", 1e-5)):
        assert abs(n[where[kind]].item() / want - 1) < 1e-6
    assert 1e15 <= x[where["huge"]].abs().min() and x[where["huge"]].abs().max() <= 1.25e15
    assert (x[where["huge"]].float() ** 2).sum().isfinite()
    xd = x.double().requires_grad_(True)
    y = G.l2norm(xd, eps)
    assert (y - F.normalize(x.double(), dim=1, eps=eps)).abs().max().item() < 1e-15
    dy = torch.randn(301, 260, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    y.backward(dy)
    for kind in ("zero", "half_eps", "norm_1e-7"):   # rows the clamp holds: the gradient is dy / eps
        assert torch.allclose(xd.grad[where[kind]], dy[where[kind]] / eps, rtol=1e-13, atol=0)
    r = where["two_eps"]
    yh = x[r].double() / n[r]
    assert torch.allclose(xd.grad[r], (dy[r] - yh * (dy[r] * yh).sum()) / n[r], rtol=1e-9, atol=1e-3)
    # M = 5 with four kinds leaves a random row, and the planted rows include the first and the last
    _, w5 = G.l2norm_input(5, 4, 1e-12, G.l2norm_kinds(1e-12), 9)
    assert sorted(w5.values()) == [0, 1, 2, 4]


def test_vit_embed_references():
    g = torch.Generator(device="cpu").manual_seed(10)
    B, P, C = 3, 5, 8
    patch, cls, pos = torch.randn(B * P, C, generator=g), torch.randn(C, generator=g), torch.randn(P + 1, C, generator=g)
    pd, cd, qd = (t.double().requires_grad_(True) for t in (patch, cls, pos))
    x = G.vit_embed_fwd(pd, cd, qd, B, P)
    assert x.dtype == torch.float64 and x.shape == (B * (P + 1), C)
    assert torch.equal(x.reshape(B, P + 1, C)[1, 0], cd + qd[0]) and torch.equal(x.reshape(B, P + 1, C)[2, 3], pd[2 * P + 2] + qd[3])
    assert G.vit_embed_fwd(patch, cls, pos, B, P, torch.float32).dtype == torch.float32
    dx = torch.randn(B * (P + 1), C, generator=g)
    x.backward(dx.double())
    dpos, dcls, dpatch = G.vit_embed_bwd(dx, B, P)
    assert torch.allclose(dpos, qd.grad, atol=1e-14) and torch.allclose(dcls, cd.grad, atol=1e-14)
    assert torch.equal(dpatch.double(), pd.grad)
    dpos0, dcls0 = torch.randn(P + 1, C, generator=g), torch.randn(C, generator=g)
    sp, sc = G.vit_embed_bwd_sequential(dx, B, P, dpos0, dcls0)
    assert sp.dtype == torch.float32
    assert (sp.double() - (dpos + dpos0)).abs().max().item() < 1e-5 and (sc.double() - (dcls + dcls0)).abs().max().item() < 1e-5
    # d cls must not contain the previous d pos[0]: with it the sum would be off by a whole N(0,1) value
    assert ((sc.double() - (dcls + dcls0 + dpos0[0])).abs().max().item()) > 0.1
    fp, fc = G.vit_embed_bwd_sequential(dx, B, P)
    assert torch.equal(fp[0], fc)


@pytest.mark.parametrize("B,L,V,C", G.TEXT_CASES)
def test_text_cases_repeat_ids_and_stay_inside_the_dtok_bound(B, L, V, C):
    ids = G.text_ids(B, L, V, 11)
    assert ids.shape == (B, L) and ids.min() >= 0 and ids.max() < V and L <= G.TEXT_POS_ROWS
    flat = ids.reshape(-1).tolist()
    R = B * L
    assert len(set(ids[:, 0].tolist())) == 1
    # A case can only show what its row count allows: every case with three rows or more has an id in three or more rows, every
    # case that reaches row 256 has a row at or above 256 that repeats an earlier id (test_text_case_list_can_fail holds the
    # list to having such cases).
    if R >= 3:
        assert max(flat.count(i) for i in set(flat)) >= 3
    if R > 256:
        assert any(flat[r] in flat[:r] for r in range(256, R))
    if V > 3:
        assert V // 2 not in flat   # a row of dtok that must keep its bits
    if L > 1:
        assert (ids[:, -1] == V - 1).any() and (ids[:, -2:] == V - 1).all(1).any()   # a padding tail of two or more
    g = torch.Generator(device="cpu").manual_seed(12)
    dx = torch.randn(R, C, generator=g)
    fresh, dpos = G.text_embed_bwd(ids, dx, V)
    assert torch.allclose(dpos, dx.double().reshape(B, L, C).sum(0), atol=1e-14)
    # the running gradient of the bound check: half the exact fresh one (see test_gpu_glue_edges: the bound has no term for it)
    dtok0 = (0.5 * fresh).float()
    seq = G.text_embed_dtok_sequential(ids, dx, dtok0)
    exact = dtok0.double() + fresh
    bound = G.dtok_bound(ids, dx, V)
    assert ((seq.double() - exact).abs() <= bound).all()
    # a random running gradient: unused ids keep their bits, used ones move
    dtok1 = torch.randn(V, C, generator=g)
    seq1 = G.text_embed_dtok_sequential(ids, dx, dtok1)
    used = torch.zeros(V, dtype=torch.bool)
    used[ids.reshape(-1)] = True
    assert torch.equal(seq1[~used], dtok1[~used]) and (seq1[used] != dtok1[used]).any()
    assert (seq1.double() - (dtok1.double() + fresh)).abs().max().item() < 1e-4
    # ascending row order matters to the bits somewhere, or "in row order" would be unobservable
    if R > 256:
        rev = G.text_embed_dtok_sequential(ids.flip(0, 1), dx.flip(0), dtok1)
        assert not torch.equal(rev, seq1) and torch.allclose(rev, seq1, atol=1e-4)


def test_text_case_list_can_fail():
    rows = [B * L for B, L, _, _ in G.TEXT_CASES]
    assert any(r > 256 for r in rows) and any(C > 256 and C % 256 for *_, C in G.TEXT_CASES) and 1 in rows


def test_text_embed_fwd_reference_clamps_ids():
    g = torch.Generator(device="cpu").manual_seed(13)
    V, C = 5, 4
    tok, pos = torch.randn(V, C, generator=g), torch.randn(G.TEXT_POS_ROWS, C, generator=g)
    ids = torch.tensor([[0, -1, V, 2 ** 40, 3]])
    x = G.text_embed_fwd(ids, tok, pos, torch.float32)
    want = tok[torch.tensor([0, 0, V - 1, V - 1, 3])] + pos[:5]
    assert torch.equal(x, want)
    dtok, _ = G.text_embed_bwd(ids, torch.ones(5, C), V)
    assert dtok[:, 0].tolist() == [2.0, 0.0, 0.0, 1.0, 2.0]


def test_rows_copy_and_add_n_references():
    g = torch.Generator(device="cpu").manual_seed(14)
    B, C = 2, 4
    src = torch.randn(B * 19, C, generator=g)
    dst = torch.full((B * 23, C), -7.0)
    out = G.rows_copy(src, 19, 2, dst, 23, 5, B, 11)
    o3 = out.view(B, 23, C)
    assert torch.equal(o3[:, 5:16], src.view(B, 19, C)[:, 2:13]) and (o3[:, :5] == -7).all() and (o3[:, 16:] == -7).all()
    assert (dst == -7).all()   # the input is left alone
    outb = G.rows_copy(src, 19, 2, dst.bfloat16(), 23, 5, B, 11)
    assert outb.dtype == torch.bfloat16 and torch.equal(outb.view(B, 23, C)[:, 5:16], src.view(B, 19, C)[:, 2:13].bfloat16())
    a, b, c, d = (torch.randn(64, generator=g) for _ in range(4))
    assert torch.equal(G.add_n([a, b, c, d], torch.float32), ((a + b) + c) + d)
    assert G.add_n([a, b, c]).dtype == torch.float64
