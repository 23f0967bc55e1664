"""The OHEM selection rule restated in torch (any float dtype; the tests use it in fp64 and on given fp32 values), and the literal
p-space formulation it is checked against (mmseg's OHEMPixelSampler with a threshold / HRNet's OhemCrossEntropy).

Rule (loss space): a pixel is valid iff label != ignore_index and 0 <= label < C; k = min(K, n_valid - 1); L = the valid loss of
rank k (0-based) in descending order; tau = fp32(-log(thresh)) formed in fp64; L_eff = min(L, tau); kept iff valid and loss > L_eff
(strict).  Nothing valid: k = -1, L = +inf."""
import math

import torch


def tau32(thresh: float) -> torch.Tensor:
    return torch.tensor(-math.log(thresh), dtype=torch.float64).to(torch.float32)


def valid_mask(labels: torch.Tensor, C: int, ignore_index: int) -> torch.Tensor:
    return (labels != ignore_index) & (labels >= 0) & (labels < C)


def ohem_rule(loss: torch.Tensor, labels: torch.Tensor, C: int, ignore_index: int, thresh: float, min_kept_total: int) -> dict:
    """Returns dict(labels_out, kept, n_valid, k, L, L_eff); L and L_eff are 0-d tensors of loss's dtype."""
    valid = valid_mask(labels, C, ignore_index)
    n_valid = int(valid.sum())
    tau = tau32(thresh).to(loss.dtype)
    if n_valid == 0:
        k, L = -1, torch.tensor(float("inf"), dtype=loss.dtype)
    else:
        k = min(int(min_kept_total), n_valid - 1)
        L = torch.sort(loss[valid], descending=True).values[k]
    L_eff = tau if bool(torch.isnan(L)) else torch.minimum(L, tau)   # fminf
    kept = valid & (loss > L_eff)
    out = torch.where(kept, labels, torch.full_like(labels, ignore_index))
    return dict(labels_out=out, kept=kept, n_valid=n_valid, k=k, L=L, L_eff=L_eff)


def ohem_pspace(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int, thresh: float, min_kept_total: int) -> torch.Tensor:
    """The original: logits [N, C], labels [N] -> kept mask.  softmax, gather the label's probability, sort ascending,
    threshold = max(sorted[min(K, n - 1)], thresh), kept iff p < threshold."""
    C = logits.shape[1]
    valid = valid_mask(labels, C, ignore_index)
    kept = torch.zeros_like(valid)
    if not bool(valid.any()):
        return kept
    p = torch.softmax(logits[valid], dim=1).gather(1, labels[valid].unsqueeze(1)).squeeze(1)
    ps = torch.sort(p).values
    threshold = max(float(ps[min(int(min_kept_total), ps.numel() - 1)]), thresh)
    kept[valid] = p < threshold
    return kept


def plain_ce(logits: torch.Tensor, labels: torch.Tensor, C: int, ignore_index: int) -> torch.Tensor:
    """Per-pixel lse - z_y for logits [N, C] (0 where the pixel is not valid), in logits' dtype."""
    valid = valid_mask(labels, C, ignore_index)
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    l = torch.logsumexp(logits, dim=1) - logits.gather(1, safe.unsqueeze(1)).squeeze(1)
    return torch.where(valid, l, torch.zeros_like(l))
