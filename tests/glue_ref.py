"""Plain-torch references of the row-streaming glue kernels (lc2is_amd/csrc/misc.hip, spatial.hip), test-only: float64 unless a
dtype is asked for, no project kernels, any device.  The ``*_sequential`` functions restate the fp32 sums in the order the kernels
document; those kernels only add, so the match is bitwise.  The case lists live here so that tests/test_glue_ref_cpu.py (which
shows that every case can fail) and tests/test_gpu_glue_edges.py (which runs them) read the same ones."""
import torch
import torch.nn.functional as F

# (B, h, w, C, S) of bilinear_up_fwd / bilinear_up_bwd
BILINEAR_CASES = [
    (2, 4, 16, 8, 2),     # the FTN grid after one repeat: the height stays, the width grows 4x
    (1, 8, 128, 4, 2),
    (1, 16, 4, 12, 2),    # a tall grid
    (1, 1, 5, 4, 2),      # one row: both vertical taps fall on one index
    (2, 3, 1, 4, 4),      # one column
    (1, 1, 1, 4, 2),
    (2, 5, 7, 8, 3),      # 1/S is inexact in fp32
    (1, 3, 5, 4, 1),      # the identity
]
BILINEAR_BIG = (4, 48, 48, 1024, 2)   # 4*48*48*256 = 2 359 296 float4 items backward: above 8192 blocks x 256 in both directions
SP_GRID_ITEMS = 8192 * 256            # one round of an sp_grid launch
EW_GRID_ITEMS = 4096 * 256            # one round of an ew_grid launch

# (B, h, w, C) of sr_gather; the last one has 3*64*64*2048/8 = 3 145 728 sixteen-byte items
SR_CASES = [(2, 4, 12, 8), (1, 2, 2, 8), (1, 6, 2, 16), (3, 64, 64, 2048)]

# (B, L, V, C) of text_embed_fwd / text_embed_bwd
TEXT_CASES = [
    (4, 77, 50, 8),     # R = 308 rows: the scan for an earlier occurrence takes a second trip of 256
    (2, 16, 6, 516),    # C > 256 and C % 256 != 0: the column loop takes a ragged third trip
    (1, 1, 1, 4),
]
TEXT_POS_ROWS = 77

# (B, P, C) of vit_embed_fwd / vit_embed_bwd; the last one has 5*1025*256 = 1 312 000 float4 items forward
VIT_CASES = [(1, 1, 4), (3, 49, 64), (5, 1024, 1024)]

# (B, H, ps, kpad) of patchify; the last one has 3*3*1024*1024/8 = 1 179 648 eight-pixel items
PATCHIFY_CASES = [(1, 70, 16, None), (2, 28, 14, 640), (1, 8, 8, None), (3, 1024, 16, None)]

L2NORM_M = [1, 5, 301]
L2NORM_C = [4, 64, 252, 260, 1024]   # one active lane, 16 lanes, 63 lanes, 65 items (a second trip of one lane), four full trips


def is_rectangular(case):
    return case[1] != case[2]


# ------------------------------------------------------------------------------------------------------------------------------
# bilinear upsample of channels-last tokens [B*h*w, C] -> [B*h*S*w*S, C] (align_corners=False), and its adjoint
# ------------------------------------------------------------------------------------------------------------------------------
def bilinear_taps(n_in, S, device=None):
    """Per output index: (i0, i1, w0, w1) with src = (dst + 0.5) / S - 0.5 clamped at 0 and i1 = min(i0 + 1, n_in - 1)."""
    dst = torch.arange(n_in * S, dtype=torch.float64, device=device)
    src = ((dst + 0.5) / S - 0.5).clamp_min(0.0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp_max(n_in - 1)
    w1 = src - i0.double()
    return i0, i1, 1.0 - w1, w1


def bilinear_up(x, B, h, w, S):
    xd = x.double().reshape(B, h, w, -1)
    y0, y1, wy0, wy1 = bilinear_taps(h, S, x.device)
    x0, x1, wx0, wx1 = bilinear_taps(w, S, x.device)
    rows = wy0[None, :, None, None] * xd[:, y0] + wy1[None, :, None, None] * xd[:, y1]            # [B, H, w, C]
    out = wx0[None, None, :, None] * rows[:, :, x0] + wx1[None, None, :, None] * rows[:, :, x1]   # [B, H, W, C]
    return out.reshape(B * h * S * w * S, -1)


def bilinear_up_adjoint(dout, B, h, w, S):
    """The transpose of bilinear_up: every output pixel scatters its gradient to its four taps."""
    H, W = h * S, w * S
    g = dout.double().reshape(B, H, W, -1)
    y0, y1, wy0, wy1 = bilinear_taps(h, S, dout.device)
    x0, x1, wx0, wx1 = bilinear_taps(w, S, dout.device)
    cols = torch.zeros(B, H, w, g.shape[-1], dtype=torch.float64, device=dout.device)
    cols.index_add_(2, x0, g * wx0[None, None, :, None])
    cols.index_add_(2, x1, g * wx1[None, None, :, None])
    din = torch.zeros(B, h, w, g.shape[-1], dtype=torch.float64, device=dout.device)
    din.index_add_(1, y0, cols * wy0[None, :, None, None])
    din.index_add_(1, y1, cols * wy1[None, :, None, None])
    return din.reshape(B * h * w, -1)


# ------------------------------------------------------------------------------------------------------------------------------
# 2x2 stride-2 im2col of channels-last tokens: out[(b, y, x)][q*C + c] = in[(b, 2y+i, 2x+j)][c], q = 2i + j  (a permutation)
# ------------------------------------------------------------------------------------------------------------------------------
def sr_gather(x, B, h, w):
    C = x.shape[1]
    return x.reshape(B, h // 2, 2, w // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (h // 2) * (w // 2), 4 * C)


def sr_scatter(g, B, h, w):
    C = g.shape[1] // 4
    return g.reshape(B, h // 2, w // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, C)


# ------------------------------------------------------------------------------------------------------------------------------
# L2 normalisation over the last dimension; its backward is autograd through this expression
# ------------------------------------------------------------------------------------------------------------------------------
def l2norm(x, eps):
    xd = x if x.dtype == torch.float64 else x.double()
    return xd / xd.norm(dim=1, keepdim=True).clamp_min(eps)


L2NORM_KINDS = ("zero", "half_eps", "two_eps", "huge")


def l2norm_kinds(eps):
    """The planted rows of a case; eps = 1e-6 adds rows of norm 1e-7 and 1e-5."""
    return L2NORM_KINDS + (("norm_1e-7", "norm_1e-5") if eps == 1e-6 else ())


def l2norm_planted_row(kind, C, eps, gen):
    u = torch.randn(C, generator=gen, dtype=torch.float64)
    u = u / u.norm()
    if kind == "zero":
        return torch.zeros(C)
    if kind == "huge":   # entries near 1e15: the squares (1e30) and their sum stay finite in fp32
        return (1e15 * (1.0 + 0.25 * torch.rand(C, generator=gen, dtype=torch.float64)) * torch.sign(u)).float()
    norm = {"half_eps": 0.5 * eps, "two_eps": 2.0 * eps, "norm_1e-7": 1e-7, "norm_1e-5": 1e-5}[kind]
    return (u * norm).float()


def l2norm_input(M, C, eps, kinds, seed):
    """fp32 [M, C] of N(0,1) rows with one planted row per kind, spread from the first row to the last; -> (x, {kind: row})."""
    assert len(kinds) <= M
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(M, C, generator=gen)
    where = {}
    for i, kind in enumerate(kinds):
        r = 0 if len(kinds) == 1 else (i * (M - 1)) // (len(kinds) - 1)
        x[r] = l2norm_planted_row(kind, C, eps, gen)
        where[kind] = r
    return x, where


def add_n(tensors, dtype=torch.float64):
    """((a + b) + c) + d in ``dtype``."""
    s = tensors[0].to(dtype)
    for t in tensors[1:]:
        s = s + t.to(dtype)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# ViT patch gather and token assembly
# ------------------------------------------------------------------------------------------------------------------------------
def patchify(pix, ps, kpad=None):
    """[B,3,H,W] -> [B*G*G, kpad]: column c*ps*ps + i*ps + j of patch (gy, gx), zero pad columns; values unchanged (pix's dtype)."""
    B = pix.shape[0]
    k = 3 * ps * ps
    kpad = kpad or ((k + 63) // 64) * 64
    cols = F.unfold(pix, kernel_size=ps, stride=ps).transpose(1, 2).reshape(-1, k)   # (image edge beyond the last whole patch dropped)
    out = torch.zeros(cols.shape[0], kpad, dtype=pix.dtype, device=pix.device)
    out[:, :k] = cols
    assert out.shape[0] == B * (pix.shape[2] // ps) * (pix.shape[3] // ps)
    return out


def vit_embed_fwd(patch, cls, pos, B, P, dtype=torch.float64):
    C = patch.shape[1]
    x = torch.cat([cls.to(dtype).expand(B, 1, C), patch.to(dtype).reshape(B, P, C)], 1) + pos[:P + 1].to(dtype)
    return x.reshape(B * (P + 1), C)


def vit_embed_bwd(dx, B, P):
    """-> (dpos [P+1, C] fp64, dcls [C] fp64, dpatch [B*P, C] in dx's dtype)."""
    d3 = dx.reshape(B, P + 1, -1)
    return d3.double().sum(0), d3[:, 0].double().sum(0), d3[:, 1:].reshape(B * P, -1)


def vit_embed_bwd_sequential(dx, B, P, dpos0=None, dcls0=None):
    """fp32 sums over b = 0..B-1 from a zero accumulator, then ONE add of the previous value; dcls never sees the previous dpos[0]."""
    d3 = dx.float().reshape(B, P + 1, -1)
    acc = torch.zeros_like(d3[0])
    for b in range(B):
        acc = acc + d3[b]
    dpos = acc if dpos0 is None else acc + dpos0[:P + 1]
    dcls = acc[0].clone() if dcls0 is None else acc[0] + dcls0
    return dpos, dcls


# ------------------------------------------------------------------------------------------------------------------------------
# CLIP text token + position embedding
# ------------------------------------------------------------------------------------------------------------------------------
def clamp_ids(ids, V):
    return ids.clamp(0, V - 1)


def text_ids(B, L, V, seed):
    """Prompt-shaped ids: column 0 holds one id (start of text) in every row, every row ends in a padding tail of one id from a
    random position on, the rest are drawn from V.  Where V > 3 the id V // 2 is withheld (re-drawn as its neighbour) so that a row
    of dtok no id touches always exists."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, V, (B, L), generator=gen)
    if V > 3:
        ids[ids == V // 2] = V // 2 + 1
    ids[:, 0] = max(V - 2, 0)
    for b in range(B):
        start = int(torch.randint(1, L + 1, (1,), generator=gen))   # (start == L: no tail)
        ids[b, start:] = V - 1
    return ids


def text_embed_fwd(ids, tok, pos, dtype=torch.float64):
    B, L = ids.shape
    x = tok.to(dtype)[clamp_ids(ids, tok.shape[0])] + pos[:L].to(dtype)
    return x.reshape(B * L, -1)


def text_embed_bwd(ids, dx, V):
    """-> (dtok [V, C], dpos [L, C]) fresh gradients in fp64; dtok by index_add_."""
    B, L = ids.shape
    dxd = dx.double()
    dtok = torch.zeros(V, dx.shape[1], dtype=torch.float64, device=dx.device).index_add_(0, clamp_ids(ids, V).reshape(-1), dxd)
    return dtok, dxd.reshape(B, L, -1).sum(0)


def text_embed_dtok_sequential(ids, dx, dtok0):
    """The fp32 sum the kernel documents: for each id the rows that carry it are added in ascending row order to an fp32
    accumulator that starts at zero; the accumulator is then added once to dtok0.  Rows of ids nobody carries keep their bits."""
    V = dtok0.shape[0]
    flat = clamp_ids(ids, V).reshape(-1).tolist()
    dxf = dx.float()
    out = dtok0.float().clone()
    acc = {}
    for r, i in enumerate(flat):
        acc[i] = (acc[i] if i in acc else torch.zeros_like(dxf[0])) + dxf[r]
    for i, a in acc.items():
        out[i] = out[i] + a
    return out


def text_embed_dpos_sequential(dx, B, L, dpos0=None):
    """fp32 sums over b = 0..B-1 from a zero accumulator; rows L.. of dpos0 are not touched."""
    d3 = dx.float().reshape(B, L, -1)
    acc = torch.zeros_like(d3[0])
    for b in range(B):
        acc = acc + d3[b]
    if dpos0 is None:
        return acc
    out = dpos0.float().clone()
    out[:L] = out[:L] + acc
    return out


def dtok_bound(ids, dx, V):
    """Elementwise bound between a sequential fp32 sum and the exact one: R * 2^-23 * sum_rows |dx| (R = B*L rows; n - 1 adds of
    relative error 2^-24 each, plus the add onto the running gradient, stay below it with room to spare)."""
    R = ids.numel()
    mag = torch.zeros(V, dx.shape[1], dtype=torch.float64, device=dx.device).index_add_(0, clamp_ids(ids, V).reshape(-1),
                                                                                       dx.double().abs())
    return R * 2.0 ** -23 * mag


def rows_copy(src, S_src, src_off, dst, S_dst, dst_off, B, n):
    """dst[b][dst_off + s] = src[b][src_off + s] for s < n, converted to dst's dtype; every other row of dst unchanged."""
    C = src.shape[1]
    out = dst.clone()
    out.view(B, S_dst, C)[:, dst_off:dst_off + n] = src.view(B, S_src, C)[:, src_off:src_off + n].to(dst.dtype)
    return out
