"""The Swin index maps (SwinTransformer._window_maps / _merge_maps) against an independent formulation.

The module builds every re-layout of the backbone (pad + cyclic shift + window partition, its inverse, the 2x2 patch
merge) as int32 row maps from index arithmetic.  Here the same layouts come from the tensor operations of the reference's
modeling code: ``F.pad`` with a -1 sentinel, ``torch.roll(-shift)`` and the window partition by ``view`` / ``permute``
(modeling_swin.py:546-550), and the strided 2x2 concat of the patch merge (:318-321).  An ``arange`` token grid is
gathered through both.  CPU only: the maps are host-built index tensors."""
import pytest
import torch
import torch.nn.functional as F

from lc2is_amd.nn.swin import SwinArch, SwinTransformer


def _module(ws):
    return SwinTransformer(SwinArch(32, (2, 2, 2, 2), (1, 2, 4, 8), ws), drop_path_rate=0.0)


def _ref_window(B, H, W, ws, shift):
    tok = torch.arange(B * H * W).view(B, H, W)
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    t = F.pad(tok, (0, Wp - W, 0, Hp - H), value=-1)
    if shift > 0:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    return t.view(B, Hp // ws, ws, Wp // ws, ws).permute(0, 1, 3, 2, 4).reshape(-1), Hp, Wp


def _ref_merge(B, H, W):
    tok = torch.arange(B * H * W).view(B, H, W, 1)
    t = F.pad(tok, (0, 0, 0, W % 2, 0, H % 2), value=-1)
    return torch.cat([t[:, r::2, c::2, :] for c in range(2) for r in range(2)], dim=-1).reshape(-1)


def _check_bijection(fwd, inv, ntok):
    """fwd's non-negative rows hit every token exactly once; inv is their inverse, -1 exactly where no row maps."""
    fwd, inv = fwd.long(), inv.long()
    assert inv.shape == (ntok,)
    ok = fwd >= 0
    assert torch.equal(torch.sort(fwd[ok]).values, torch.arange(ntok))
    assert bool((fwd[~ok] == -1).all())
    rows = torch.nonzero(ok).view(-1)
    assert torch.equal(inv[fwd[ok]], rows)
    want = torch.full((ntok,), -1, dtype=torch.long)
    want[fwd[ok]] = rows
    assert torch.equal(inv, want)


GRIDS = (128, 64, 32, 112, 56, 28, 110, 55, 44, 11)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ws,shifted", [(7, False), (7, True), (5, False), (5, True)])
@pytest.mark.parametrize("H", GRIDS)
def test_window_maps_match_pad_roll_partition(H, ws, shifted, B):
    shift = ws // 2 if shifted else 0
    m = _module(ws)._window_maps(B, H, H, shift, "cpu")
    ref, Hp, Wp = _ref_window(B, H, H, ws, shift)
    assert (m["Hp"], m["Wp"], m["nwx"]) == (Hp, Wp, Wp // ws)
    assert m["per_img"] == (Hp // ws) * (Wp // ws) and m["nwin"] == B * m["per_img"]
    assert m["fwd"].dtype == torch.int32 and m["inv"].dtype == torch.int32
    assert m["fwd"].numel() == m["nwin"] * ws * ws
    assert torch.equal(m["fwd"].long(), ref)
    _check_bijection(m["fwd"], m["inv"], B * H * H)


@pytest.mark.parametrize("H,W,ws,shift", [(55, 28, 7, 3), (28, 55, 7, 3), (44, 11, 5, 2), (12, 30, 5, 0)])
def test_window_maps_non_square(H, W, ws, shift):
    m = _module(ws)._window_maps(2, H, W, shift, "cpu")
    ref, Hp, Wp = _ref_window(2, H, W, ws, shift)
    assert (m["Hp"], m["Wp"], m["nwx"], m["per_img"]) == (Hp, Wp, Wp // ws, (Hp // ws) * (Wp // ws))
    assert torch.equal(m["fwd"].long(), ref)
    _check_bijection(m["fwd"], m["inv"], 2 * H * W)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", GRIDS + (7,))
def test_merge_maps_match_strided_concat(H, B):
    for W in (H, H + 1):
        m = _module(7)._merge_maps(B, H, W, "cpu")
        assert (m["H2"], m["W2"]) == (-(-H // 2), -(-W // 2))
        assert m["fwd"].dtype == torch.int32 and m["fwd"].numel() == B * m["H2"] * m["W2"] * 4
        assert torch.equal(m["fwd"].long(), _ref_merge(B, H, W))
        _check_bijection(m["fwd"], m["inv"], B * H * W)
