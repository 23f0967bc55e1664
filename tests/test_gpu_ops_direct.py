"""Direct op-level checks of the launchers that the module tests only reach at one tiny golden shape: the score-tail batched
GEMM and transpose, the transposed upsample, the contrastive / n-pair losses, the mIoU counts, the spatial-reduction scatter,
the Swin bias-table gradient and the uint8 preprocessing gathers.  Every kernel is compared with a plain float64 (or exact
integer / bitwise) torch restatement of the same operation on the same inputs, at production shapes and at the edges where
such kernels go wrong: grid-stride loops past the grid caps, tile-plan switches, batch strides, clamped borders, ties.
Seeds are fixed and every batch / image gets different data, so a kernel that reads batch 0 for every batch fails."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(dev, seed, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=_gen(dev, seed), device=dev).to(dtype)


# ---- gemm_nt_batched: out[b] = a[b] @ w[b].T (score tail, nn/score.py) ------------------------------------------------
def _gemm_ref(a, w):
    return torch.bmm(a.double(), w.double().transpose(1, 2))


def _tol32(K):
    return 2e-6 * K ** 0.5 + 1e-6


@pytest.mark.parametrize("B,M,N,K", [
    (32, 1024, 192, 512),     # score tail forward, 32 x 32 map: class scores against KPAD = 192 padded embeddings
    (32, 16384, 192, 512),    # ... 128 x 128 map
    (32, 1024, 512, 192),     # backward form: d(visual) = dS [P, KPAD] . text^T [C, KPAD]
    (32, 16384, 512, 192),
    (1, 1000, 192, 512),      # batch = 1: a single-row grid (no blockIdx.y offset)
    (3, 1, 192, 512),         # one row per image
    (5, 1000, 192, 64),       # ragged M, one K step
    (4, 3968, 128, 256),      # 124 tiles of 128 x 128: the 64 x 64 plan
    (4, 4000, 128, 256),      # 128 tiles of 128 x 128: the 128 x 128 plan
])
def test_gemm_nt_batched_vs_fp64(dev, B, M, N, K):
    from lc2is_amd import ops
    s = B * 7919 + M * 31 + N * 7 + K
    a = _randn(dev, s, B, M, K, dtype=torch.bfloat16)
    w = (_randn(dev, s + 1, B, N, K) * K ** -0.5).bfloat16()
    ob, of = ops.gemm_nt_batched(a, w)
    assert ob is None and of.shape == (B, M, N)
    ref = _gemm_ref(a, w)
    assert _rel(of, ref) < _tol32(K)
    for b in (0, B - 1):   # every image on its own (a batch-offset slip shows per image)
        assert _rel(of[b], ref[b]) < _tol32(K), b


@pytest.mark.parametrize("B,M,N,K", [(2, 1000, 192, 512), (32, 1024, 192, 512)])
def test_gemm_nt_batched_both_outputs(dev, B, M, N, K):
    from lc2is_amd import ops
    a = _randn(dev, 11 + M, B, M, K, dtype=torch.bfloat16)
    w = (_randn(dev, 12 + M, B, N, K) * K ** -0.5).bfloat16()
    ob, of = ops.gemm_nt_batched(a, w, out_bf16=True, out_f32=True)
    ref = _gemm_ref(a, w)
    assert _rel(of, ref) < _tol32(K)
    assert _rel(ob.float(), ref) < 4e-3
    _, of_only = ops.gemm_nt_batched(a, w)
    assert torch.equal(of, of_only)


@pytest.mark.parametrize("B,M,N,K", [(3, 700, 192, 512), (16, 1024, 192, 512)])
def test_gemm_nt_batched_strided_views(dev, B, M, N, K):
    """Inputs as views: row stride > K, batch stride != M * lda (every other matrix of a larger tensor), a column offset; the
    fp32 output is a view with ld > N whose pad columns must stay untouched."""
    from lc2is_amd import ops
    abig = _randn(dev, 21, 2 * B, M, K + 64, dtype=torch.bfloat16)
    wbig = (_randn(dev, 22, 2 * B + 1, N + 8, K + 96) * K ** -0.5).bfloat16()
    a = abig[::2, :, :K]
    w = wbig[1::2, 3:3 + N, 32:32 + K]
    assert a.stride(1) > K and a.stride(0) != M * a.stride(1) and w.stride(0) != N * w.stride(1)
    obig = torch.full((B, M, N + 4), float("nan"), device=dev)
    out = obig[:, :, :N]
    _, of = ops.gemm_nt_batched(a, w, out_f32=out)
    assert of.data_ptr() == out.data_ptr()
    ref = _gemm_ref(a, w)
    assert _rel(out, ref) < _tol32(K)
    assert torch.isnan(obig[:, :, N:]).all()
    _, dense = ops.gemm_nt_batched(a.contiguous(), w.contiguous())
    assert torch.equal(dense, out)


@pytest.mark.parametrize("B,M,N,K", [(32, 1024, 192, 512), (3, 1000, 192, 64)])
def test_gemm_nt_batched_is_bitwise_reproducible(dev, B, M, N, K):
    from lc2is_amd import ops
    a = _randn(dev, 31, B, M, K, dtype=torch.bfloat16)
    w = _randn(dev, 32, B, N, K, dtype=torch.bfloat16)
    r1 = ops.gemm_nt_batched(a, w, out_bf16=True)
    r2 = ops.gemm_nt_batched(a, w, out_bf16=True)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


# ---- transpose_bf16_batched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,C", [(32, 192, 512), (3, 70, 131), (1, 1, 65), (2, 129, 1)])
def test_transpose_bf16_batched_bitwise(dev, B, R, C):
    from lc2is_amd import ops
    x = _randn(dev, R * 1000 + C, B, R, C, dtype=torch.bfloat16)
    y = ops.transpose_bf16_batched(x)
    assert y.shape == (B, C, R) and y.is_contiguous()
    assert torch.equal(y, x.transpose(1, 2))


def test_transpose_bf16_batched_strided_view(dev):
    from lc2is_amd import ops
    big = _randn(dev, 41, 6, 80, 140, dtype=torch.bfloat16)
    x = big[::2, 5:75, 7:138]                                   # [3, 70, 131]: row stride 140, batch stride 2 * 80 * 140
    assert torch.equal(ops.transpose_bf16_batched(x), x.transpose(1, 2))


# ---- upsample_bwd_nchw: the adjoint of bicubic / bilinear xS (align_corners=False) ---------------------------------------------
@pytest.mark.parametrize("mode,B,h,w,K,S,ld", [
    ("bicubic", 32, 32, 32, 151, 4, 192),    # mIoU / eval head shape
    ("bilinear", 4, 32, 32, 151, 4, 192),    # score tail (nn/score.py) x4
    ("bilinear", 2, 16, 16, 151, 8, 192),
    ("bilinear", 2, 16, 16, 151, 16, 192),
    ("bicubic", 3, 1, 1, 5, 4, 64),          # one low-res pixel: every tap clamps to it
    ("bilinear", 3, 1, 1, 5, 8, 64),
    ("bicubic", 2, 2, 2, 7, 4, 8),
    ("bilinear", 2, 2, 2, 7, 16, 8),
    ("bicubic", 2, 5, 9, 150, 4, 192),       # w != h
    ("bicubic", 2, 11, 3, 64, 8, 64),
    ("bilinear", 2, 7, 13, 33, 4, 40),
])
def test_upsample_bwd_nchw_is_the_adjoint(dev, mode, B, h, w, K, S, ld):
    from lc2is_amd import ops
    dhi = _randn(dev, B * 100 + h * 10 + w + S, B, K, h * S, w * S)
    dlo = ops.upsample_bwd_nchw(dhi, B, h, w, K, S, ops.INTERP_BICUBIC if mode == "bicubic" else ops.INTERP_BILINEAR, ld)
    assert dlo.shape == (B * h * w, ld)
    x = torch.zeros(B, K, h, w, dtype=torch.float64, device=dev, requires_grad=True)
    F.interpolate(x, scale_factor=S, mode=mode, align_corners=False).backward(dhi.double())
    ref = x.grad.permute(0, 2, 3, 1).reshape(B * h * w, K)
    assert _rel(dlo[:, :K], ref) < 1e-5
    for b in range(B):
        assert _rel(dlo[b * h * w:(b + 1) * h * w, :K], ref[b * h * w:(b + 1) * h * w]) < 1e-5, b
    assert torch.equal(dlo[:, K:], torch.zeros_like(dlo[:, K:]))


# ---- rows_ce / cols_ce: the two terms of ContrastiveLoss (model/loss.py:39-64) ---------------------------------------------
def _rows_ref(x, lab, gscale):
    """softmax-CE per row in fp64; a row whose label lies outside [0, K) adds nothing."""
    xd = x.double()
    K = xd.shape[1]
    ok = (lab >= 0) & (lab < K)
    safe = torch.where(ok, lab, torch.zeros_like(lab))
    lse = torch.logsumexp(xd, 1)
    loss = ((lse - xd.gather(1, safe[:, None])[:, 0]) * ok).sum()
    dx = gscale * (torch.softmax(xd, 1) - F.one_hot(safe, K).double()) * ok[:, None]
    return loss, lse, dx


def _cols_ref(x, lab, B, H, W, K, gscale):
    """nn.CrossEntropyLoss on the [B,H,W,K] view with one-hot float targets (class axis = H), summed, in fp64; a label
    outside [0, K) matches no class."""
    xd = x.double().view(B, H, W, K)
    oh = (lab.view(B, H, W, 1) == torch.arange(K, device=x.device)).double()
    loss = (oh * (torch.logsumexp(xd, 1, keepdim=True) - xd)).sum()
    dx = gscale * (torch.softmax(xd, 1) * oh.sum(1, keepdim=True) - oh)
    return loss, dx.view(B * H * W, K)


@pytest.mark.parametrize("M,K", [(1000, 7), (1000, 151), (1000, 200), (40000, 151), (17, 151)])
def test_rows_ce_vs_fp64(dev, M, K):
    """M = 40000 > 4096 blocks x 4 rows: the grid-stride loop runs three rounds."""
    from lc2is_amd import ops
    x = _randn(dev, M + K, M, K) * 3
    lab = torch.randint(0, K, (M,), generator=_gen(dev, M + K + 1), device=dev)
    loss = torch.zeros(1, device=dev)
    dx = torch.empty_like(x)
    lse = ops.rows_ce(x, lab, loss_sum=loss, dx=dx, grad_scale=0.37, want_lse=True)
    rl, rlse, rdx = _rows_ref(x, lab, 0.37)
    assert abs(loss.item() - rl.item()) < 2e-5 * abs(rl.item())
    assert _rel(lse, rlse) < 2e-6
    assert _rel(dx, rdx) < 1e-5


def test_rows_ce_accumulates_dx_and_lse_only(dev):
    from lc2is_amd import ops
    M, K = 5000, 151
    x = _randn(dev, 51, M, K) * 2
    lab = torch.randint(0, K, (M,), generator=_gen(dev, 52), device=dev)
    dx0 = _randn(dev, 53, M, K)
    dx = dx0.clone()
    loss = torch.full((1,), 3.5, device=dev)                    # loss_sum is accumulated onto, too
    ops.rows_ce(x, lab, loss_sum=loss, dx=dx, grad_scale=-1.5, accumulate_dx=True)
    rl, rlse, rdx = _rows_ref(x, lab, -1.5)
    assert abs(loss.item() - (rl.item() + 3.5)) < 2e-5 * abs(rl.item())
    assert _rel(dx - dx0, rdx) < 1e-5
    assert _rel(dx, dx0.double() + rdx) < 1e-5
    lse = ops.rows_ce(x, lab, want_lse=True)                    # lse alone: no loss, no dx
    assert _rel(lse, rlse) < 2e-6


def test_rows_ce_ignores_labels_outside_the_class_range(dev):
    """-100 (row 0: before the start of the buffer), K, 255 and a label past int32: no loss and no dx (written as 0,
    left as is when accumulating), like ce_nchw's uncounted pixels."""
    from lc2is_amd import ops
    M, K = 20000, 151
    x = _randn(dev, 61, M, K)
    lab = torch.randint(0, K, (M,), generator=_gen(dev, 62), device=dev)
    bad = torch.randperm(M, generator=torch.Generator().manual_seed(63))[:2000].to(dev)
    lab[bad] = torch.tensor([-100, K, 255, -1, (1 << 32) + 3], device=dev).repeat(400)
    lab[0], lab[M - 1] = -100, K
    loss = torch.zeros(1, device=dev)
    dx = torch.full_like(x, 7.0)
    ops.rows_ce(x, lab, loss_sum=loss, dx=dx, grad_scale=0.25)
    rl, _, rdx = _rows_ref(x, lab, 0.25)
    assert abs(loss.item() - rl.item()) < 2e-5 * abs(rl.item())
    assert _rel(dx, rdx) < 1e-5
    assert torch.equal(dx[bad], torch.zeros_like(dx[bad]))
    dacc = torch.full_like(x, 7.0)
    ops.rows_ce(x, lab, dx=dacc, grad_scale=0.25, accumulate_dx=True)
    assert torch.equal(dacc[bad], torch.full_like(dacc[bad], 7.0))
    assert _rel(dacc - 7.0, rdx) < 1e-5


@pytest.mark.parametrize("B,H,W,K", [
    (2, 16, 16, 7), (2, 16, 16, 151), (2, 16, 16, 200), (3, 32, 32, 151),
    (8, 8, 2048, 151),    # B * W * K = 2.47 M columns > 8192 blocks x 256 threads: the grid-stride loop runs twice
])
def test_cols_ce_vs_fp64(dev, B, H, W, K):
    from lc2is_amd import ops
    x = _randn(dev, B * H * W + K, B * H * W, K) * 2
    lab = torch.randint(0, K, (B * H * W,), generator=_gen(dev, B + H + W + K), device=dev)
    lab[::97] = -1                                              # out of range: matches no class, reads nothing out of bounds
    lab[5::89] = K
    dx0 = _randn(dev, 71, B * H * W, K)
    dx = dx0.clone()                                            # cols_ce always accumulates into dx (after rows_ce wrote it)
    loss = torch.zeros(1, device=dev)
    ops.cols_ce(x, lab, B, H, W, K, loss, dx=dx, grad_scale=0.7)
    rl, rdx = _cols_ref(x, lab, B, H, W, K, 0.7)
    assert abs(loss.item() - rl.item()) < 2e-5 * abs(rl.item())
    assert _rel(dx - dx0, rdx) < 1e-5
    loss2 = torch.zeros(1, device=dev)
    ops.cols_ce(x, lab, B, H, W, K, loss2)                      # loss only
    assert abs(loss2.item() - rl.item()) < 2e-5 * abs(rl.item())


def test_contrastive_loss_module_vs_fp64_reference(dev):
    """ContrastiveLoss at [4, 16384, 151] (128 x 128 maps) against the reference's own formula (rearranges, F.one_hot,
    nn.CrossEntropyLoss with one-hot float targets) evaluated in fp64: the three losses and the gradient."""
    import lc2is_amd.nn as N
    B, H, K = 4, 128, 151
    out = (_randn(dev, 81, B, H * H, K) * 2).requires_grad_(True)
    labels = torch.randint(0, K, (B, H, H), generator=_gen(dev, 82), device=dev)
    total, lv, lt = N.ContrastiveLoss()(out, labels)
    (3 * total).backward()
    xd = out.detach().double().requires_grad_(True)
    rt = F.cross_entropy(xd.view(B, H, H, K), F.one_hot(labels, 151).double())
    rv = F.cross_entropy(xd.transpose(-2, -1).reshape(B, K, H, H), labels)
    rtot = (rt + rv) / 2
    (3 * rtot).backward()
    for got, ref in ((total, rtot), (lv, rv), (lt, rt)):
        assert abs(got.item() - ref.item()) < 2e-5 * abs(ref.item()), (got.item(), ref.item())
    assert _rel(out.grad, xd.grad) < 1e-5


# ---- npair / npair_bwd (model/loss.py:30-36) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,npos,nneg,d", [
    (6, 1, 1, 16), (100, 3, 17, 100), (1000, 17, 3, 512), (257, 17, 17, 100), (1000, 1, 1, 512), (33, 3, 3, 16),
])
def test_npair_fwd_bwd_vs_fp64_autograd(dev, n, npos, nneg, d):
    from lc2is_amd import ops
    s = n * 1000 + npos * 100 + nneg * 10 + d
    # positive entries keep pos + neg away from 0 (the formula has no guard there, in the reference either); x_pos carries its
    # mass in the first half of the features and x_neg in the second, so the two terms of dx do not cancel each other
    x, xp, xn = (torch.rand(m, d, generator=_gen(dev, s + i), device=dev) + 0.05 for i, m in enumerate((n, npos, nneg)))
    xp[:, d // 2:] *= 0.1
    xn[:, :d // 2] *= 0.1
    dres = torch.rand(n, generator=_gen(dev, s + 9), device=dev) + 0.5
    res = ops.npair(x, xp, xn)
    xd, xpd, xnd = (t.double().requires_grad_(True) for t in (x, xp, xn))
    pos = xd @ xpd.T
    neg = (xd @ xnd.T).sum(-1, keepdim=True)
    ref = (pos / (pos + neg)).sum(-1)
    ref.backward(dres.double())
    assert _rel(res, ref) < 1e-5
    dx, dxp, dxn = ops.npair_bwd(x, xp, xn, dres)
    assert _rel(dx, xd.grad) < 2e-5
    assert _rel(dxp, xpd.grad) < 2e-5
    assert _rel(dxn, xnd.grad) < 2e-5
    again = ops.npair_bwd(x, xp, xn, dres)
    for a, b in zip((dx, dxp, dxn), again):
        assert torch.equal(a, b)


# ---- miou_counts (metrics.py): exact integer counts -------------------------------------------------------------------------
def _miou_ref(hi, lab_lo, S):
    """[B, 3, K] int64: intersection, prediction and label counts per class.  The prediction is the FIRST maximal class
    (torch.argmax's rule), stated here without relying on argmax's tie handling; labels outside [0, K) count toward the
    predictions only."""
    B, K, H, W = hi.shape
    ks = torch.arange(K, device=hi.device).view(1, K, 1, 1)
    pred = torch.where(hi == hi.amax(1, keepdim=True), ks, K).amin(1)
    lab = lab_lo.repeat_interleave(S, 1).repeat_interleave(S, 2)
    out = torch.zeros(B, 3, K, dtype=torch.int64, device=hi.device)
    for b in range(B):
        p, lb = pred[b].flatten(), lab[b].flatten()
        ok = (lb >= 0) & (lb < K)
        out[b, 0] = torch.bincount(lb[ok & (lb == p)], minlength=K)
        out[b, 1] = torch.bincount(p, minlength=K)
        out[b, 2] = torch.bincount(lb[ok], minlength=K)
    return out


def _plant_labels(lab, K, seed):
    g = torch.Generator().manual_seed(seed)
    flat = lab.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:max(3, flat.numel() // 20)].to(lab.device)
    flat[idx] = torch.tensor([-1, K, 255], device=lab.device).repeat(idx.numel() // 3 + 1)[:idx.numel()]
    return lab


@pytest.mark.parametrize("K", [150, 151])
def test_miou_counts_eval_shapes_with_planted_ties(dev, K):
    """N = 4 images, 32 x 32 score maps upsampled x4 (bicubic, as metrics.per_image_mIOU does), labels at 32 x 32 incl.
    -1 / K / 255; at a tenth of the pixels two classes tie for the maximum."""
    from lc2is_amd import ops
    B, h, S = 4, 32, 4
    lo = _randn(dev, 90 + K, B, K, h, h)
    hi = F.interpolate(lo, scale_factor=S, mode="bicubic", align_corners=False).contiguous()
    g = _gen(dev, 91 + K)
    mask = torch.rand(B, 1, h * S, h * S, generator=g, device=dev) < 0.1
    c1 = torch.randint(0, K - 1, (B, 1, h * S, h * S), generator=g, device=dev)
    c2 = c1 + 1 + torch.randint(0, K - 1, c1.shape, generator=g, device=dev) % (K - 1 - c1)
    top = hi.amax(1, keepdim=True) + 1.0
    hi.scatter_(1, c1, torch.where(mask, top, hi.gather(1, c1)))
    hi.scatter_(1, c2, torch.where(mask, top, hi.gather(1, c2)))
    labels = torch.randint(0, K, (B, h, h), generator=g, device=dev)
    _plant_labels(labels, K, 92 + K)
    counts = ops.miou_counts(hi, labels, S)
    assert counts.dtype == torch.int32 and counts.shape == (B, 3, K)
    ref = _miou_ref(hi, labels, S)
    assert torch.equal(counts.long(), ref)
    assert (ref[:, 1].sum(1) == (h * S) ** 2).all()              # every pixel predicts exactly one class


def test_miou_counts_all_ties(dev):
    """Scores quantised to 4 levels: nearly every pixel has a tie at the top; the first maximal class must win."""
    from lc2is_amd import ops
    B, K, h, S = 3, 151, 16, 4
    hi = torch.randint(0, 4, (B, K, h * S, h * S), generator=_gen(dev, 95), device=dev).float()
    labels = torch.randint(0, K, (B, h, h), generator=_gen(dev, 96), device=dev)
    _plant_labels(labels, K, 97)
    assert torch.equal(ops.miou_counts(hi, labels, S).long(), _miou_ref(hi, labels, S))


def test_miou_counts_grid_stride_loop(dev):
    """3 x 1024 x 1024 pixels > 8192 blocks x 256 threads, K = 5 (cheap), heavy ties."""
    from lc2is_amd import ops
    B, K, H, S = 3, 5, 1024, 4
    hi = torch.randint(0, 3, (B, K, H, H), generator=_gen(dev, 98), device=dev).float()
    labels = torch.randint(0, K, (B, H // S, H // S), generator=_gen(dev, 99), device=dev)
    _plant_labels(labels, K, 100)
    assert torch.equal(ops.miou_counts(hi, labels, S).long(), _miou_ref(hi, labels, S))


# ---- sr_scatter_add: the adjoint of sr_gather's 2 x 2 space-to-channel permutation -----------------------------------------
@pytest.mark.parametrize("B,h,w,C", [(2, 8, 12, 64), (3, 2, 2, 4), (1, 6, 2, 12), (4, 64, 64, 1024)])
def test_sr_scatter_add_bitwise(dev, B, h, w, C):
    """dst[(b, 2y+i, 2x+j)][c] += src[(b, y, x)][(2i+j)*C + c]; (4, 64, 64, 1024) runs the grid-stride loop."""
    from lc2is_amd import ops
    src = _randn(dev, B + h + w + C, B * h * w // 4, 4 * C, dtype=torch.bfloat16)
    dst = _randn(dev, B + h + w + C + 1, B * h * w, C)
    fine = src.view(B, h // 2, w // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, C)
    ref = dst + fine.float()
    ops.sr_scatter_add(src, dst, B, h, w)
    assert torch.equal(dst, ref)


@pytest.mark.parametrize("B,h,w,C", [(2, 8, 12, 64), (3, 16, 16, 8), (2, 32, 32, 320)])
def test_sr_scatter_add_inverts_sr_gather(dev, B, h, w, C):
    from lc2is_amd import ops
    x16 = _randn(dev, 110 + C, B * h * w, C, dtype=torch.bfloat16)
    z = torch.zeros(B * h * w, C, device=dev)
    ops.sr_scatter_add(ops.sr_gather(x16, B, h, w), z, B, h, w)
    assert torch.equal(z, x16.float())


# ---- swin_bias_table_grad: sum of dbias over the pairs of each relative offset (nn/swin.py CSR) ------------------------------
@pytest.mark.parametrize("ws,nH", [(7, 3), (7, 6), (7, 24), (12, 4), (12, 12), (12, 32)])
def test_swin_bias_table_grad_vs_index_add(dev, ws, nH):
    from lc2is_amd import ops
    from lc2is_amd.nn.swin import relative_position_csr, relative_position_index
    S, T = ws * ws, (2 * ws - 1) ** 2
    offs, pos = (t.to(dev) for t in relative_position_csr(ws))
    dbias = _randn(dev, ws * 100 + nH, nH, S, S)
    idx = relative_position_index(ws).to(dev)
    ref = torch.zeros(T, nH, dtype=torch.float64, device=dev).index_add_(0, idx, dbias.double().permute(1, 2, 0).reshape(S * S, nH))
    got = ops.swin_bias_table_grad(dbias, offs, pos, torch.full((T, nH), float("nan"), device=dev))
    assert _rel(got, ref) < 1e-6
    base = _randn(dev, ws * 100 + nH + 1, T, nH)
    acc = ops.swin_bias_table_grad(dbias, offs, pos, base.clone(), accumulate=True)
    assert _rel(acc, base.double() + ref) < 1e-6
    assert torch.equal(ops.swin_bias_table_grad(dbias, offs, pos, torch.empty(T, nH, device=dev)), got)


# ---- preprocessing: gather2d_u8 (nearest resize) and crop_lut (crop + lookup) -----------------------------------------------
@pytest.mark.parametrize("H,W,C,oh,ow", [(37, 53, 3, 29, 71), (5, 300, 1, 9, 4), (480, 640, 3, 1000, 1000), (1, 1, 3, 3, 2)])
def test_gather2d_u8_bitwise(dev, H, W, C, oh, ow):
    """(480, 640) -> (1000, 1000) x 3 channels = 3 M bytes: past the 8192-block grid cap."""
    from lc2is_amd import ops
    g = _gen(dev, H * W + oh)
    src = torch.randint(0, 256, (H, W, C), generator=g, device=dev, dtype=torch.uint8)
    yi = torch.randint(0, H, (oh,), generator=g, device=dev, dtype=torch.int32)
    xi = torch.randint(0, W, (ow,), generator=g, device=dev, dtype=torch.int32)
    yi[0], xi[-1] = H - 1, W - 1
    out = ops.gather2d_u8(src, yi, xi)
    assert torch.equal(out, src[yi.long()][:, xi.long()])


@pytest.mark.parametrize("H,W,C,top,left,S", [(37, 53, 3, 5, 11, 31), (100, 64, 1, 36, 0, 64), (1100, 1300, 3, 37, 200, 1024),
                                             (9, 9, 3, 8, 8, 1)])
def test_crop_lut_bitwise(dev, H, W, C, top, left, S):
    from lc2is_amd import ops
    g = _gen(dev, H * W + top + left)
    src = torch.randint(0, 256, (H, W, C), generator=g, device=dev, dtype=torch.uint8)
    lut_f = torch.randn(C, 256, generator=g, device=dev)
    lut_i = torch.randint(-5, 200, (256,), generator=g, device=dev)
    crop = src[top:top + S, left:left + S].long()
    ref_f = torch.stack([lut_f[c][crop[..., c]] for c in range(C)])
    ref_i = lut_i[crop[..., 0]]
    out_f, out_i = ops.crop_lut(src, top, left, S, lut_f32=lut_f, lut_i64=lut_i)
    assert torch.equal(out_f, ref_f) and torch.equal(out_i, ref_i)
    batch = torch.full((2, C, S, S), float("nan"), device=dev)   # into a slot of a batch tensor, as data/preprocess.py does
    ops.crop_lut(src, top, left, S, lut_f32=lut_f, out_f32=batch[1])
    assert torch.equal(batch[1], ref_f) and torch.isnan(batch[0]).all()


# ---- ln_defer_flush: the deferred LayerNorm dgamma / dbeta reductions leave at the flush ------------------------------------
def test_ln_defer_flush_direct(dev):
    from lc2is_amd import ops
    M, C = 3000, 768
    x = _randn(dev, 120, M, C)
    gamma = _randn(dev, 121, C)
    _, _, mean, rstd = ops.layernorm_fwd(x, gamma, torch.zeros(C, device=dev))
    dy = _randn(dev, 122, M, C, dtype=torch.bfloat16)
    g0, b0 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma=g0, dbeta=b0)
    torch.cuda.synchronize()
    prev = ops.ln_defer_begin()
    try:
        deferred = ops._ln_defer is not None                    # LC2IS_LN_DEFER=0 switches the scope off
        g1, b1 = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma=g1, dbeta=b1)
        if deferred:
            assert len(ops._ln_defer) == 1
            torch.cuda.synchronize()
            assert torch.isnan(g1).all() and torch.isnan(b1).all()   # nothing reduced before the flush
        ops.ln_defer_flush()
        assert not ops._ln_defer
    finally:
        ops.ln_defer_end(prev)
    assert torch.equal(g1, g0) and torch.equal(b1, b0)
    xhat = (x.double() - x.double().mean(1, keepdim=True)) / (x.double().var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    assert _rel(g1, (dy.double() * xhat).sum(0)) < 1e-5
    assert _rel(b1, dy.double().sum(0)) < 1e-5
