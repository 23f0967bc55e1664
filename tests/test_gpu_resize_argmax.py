"""The original-size prediction and mIoU (lc2is_resize_argmax / ops.resize_argmax, metrics.compute_gt_mIOU,
metrics.original_size_predictions, segmentation_metrics / Evaluator with gt) against torch's own bicubic operator in fp64 on the
CPU, a host recount of the counts and a test-local fp64 restatement of the reference's compute_gt_mIOU (metrics.py:61-79)."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from lc2is_amd import evalloop, metrics, ops

pytestmark = pytest.mark.gpu

K, h, w = 151, 128, 128


def logits(n, seed, k=K, hh=h, ww=w):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, hh, ww, generator=g)


def ref_argmax(x, size, chunk=16):
    """fp64 CPU F.interpolate(x [1,K,h,w], size, bicubic, align_corners=False): (argmax [H,W] (first maximum), top-1 minus
    top-2 margin [H,W]), over channel chunks with a running top-2 (the [K,H,W] map at 2048 x 1536 would be 3.8 GB in fp64)."""
    v1 = v2 = i1 = None
    for c0 in range(0, x.shape[1], chunk):
        y = F.interpolate(x[:, c0:c0 + chunk].double(), size=size, mode="bicubic", align_corners=False)[0]
        top = y.topk(2, dim=0).values
        m, s, a = top[0], top[1], y.argmax(0) + c0
        if v1 is None:
            v1, v2, i1 = m, s, a
        else:
            up = m > v1
            v2 = torch.where(up, torch.maximum(v1, s), torch.maximum(v2, m))
            i1 = torch.where(up, a, i1)
            v1 = torch.where(up, m, v1)
    return i1, v1 - v2


def recount(pred, gt, k=K):
    """{intersection, predicted, labelled} [3, k] from a class map and a gt map (labelled: 0 <= gt < k)."""
    p, g = pred.reshape(-1).long().cpu(), gt.reshape(-1).long().cpu()
    lab = (g >= 0) & (g < k)
    return torch.stack([torch.bincount(p[lab & (p == g)], minlength=k), torch.bincount(p, minlength=k),
                        torch.bincount(g[lab], minlength=k)]).int()


def ref_gt_miou(x, gt_list, sizes, ignore_index=0):
    """compute_gt_mIOU restated in fp64: F.interpolate + argmax + bincount in place of JaccardIndex (torchmetrics not needed)."""
    out = []
    for i, (g, size) in enumerate(zip(gt_list, sizes)):
        pred, _ = ref_argmax(x[i:i + 1], tuple(size))
        c = recount(pred, g, x.shape[1]).double()
        iou = c[0] / (c[1] + c[2] - c[0]).clamp_min(1)
        classes = g.unique()
        classes = classes[classes != ignore_index].long()
        out.append(iou[classes].mean().item() if classes.numel() else float("nan"))
    return torch.tensor(out, dtype=torch.float64)


def test_identity_size_is_the_exact_argmax_with_lowest_index_ties(dev):
    x = logits(2, 1, hh=40, ww=56)
    x[:, 77] = x[:, 12]                                  # exact ties everywhere between 12 and 77
    x[0, 5, :10] = 50.0; x[0, 9, :10] = 50.0; x[0, 140, :10] = 50.0      # planted three-way ties: 5 wins
    preds, _ = ops.resize_argmax(x.to(dev), [(40, 56), (40, 56)])
    want = x.argmax(1)
    for i in range(2):
        assert preds[i].dtype == torch.uint8 and preds[i].shape == (40, 56)
        assert torch.equal(preds[i].cpu().long(), want[i])
    assert (preds[0][:10] == 5).all()
    assert not (torch.cat([p.reshape(-1) for p in preds]) == 77).any()


@pytest.mark.parametrize("size", [(683, 512), (512, 683), (97, 1031), (100, 90), (1, 777), (1, 1), (2048, 1536)])
def test_matches_torch_bicubic_argmax_in_fp64(dev, size):
    x = logits(1, 2)
    preds, _ = ops.resize_argmax(x.to(dev), [size])
    ref, margin = ref_argmax(x, size)
    sure = margin > 5e-5 * x.abs().max().item()
    got = preds[0].cpu().long()
    assert got.shape == size
    bad = int(((got != ref) & sure).sum())
    assert bad == 0, f"{bad} pixels differ from fp64 torch outside the near-tie margin at {size}"
    assert (~sure).float().mean().item() <= 5e-3


def test_planted_ties_after_a_resize_go_to_the_lower_index(dev):
    x = logits(2, 3)
    x[:, 40] += 4.0
    x[:, 100] = x[:, 40]                                 # bitwise copy: every interpolated value ties with channel 40
    preds, _ = ops.resize_argmax(x.to(dev), [(683, 512), (300, 97)])
    for p in preds:
        assert not (p == 100).any()
        assert (p == 40).float().mean().item() > 0.5


def _gt_maps(sizes, seed, k=K):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, s, generator=g) for s in sizes]


def test_counts_match_a_host_recount_and_ignore_out_of_range_gt(dev):
    sizes = [(683, 512), (100, 90), (1, 777)]
    x = logits(3, 4)
    gt64 = _gt_maps(sizes, 5)
    gt64[0][:3, :] = -1; gt64[0][3:6, :] = K; gt64[0][6:9, :] = 255; gt64[1][0, :50] = -1
    gt8 = [torch.where(g < 0, torch.full_like(g, 255), g).to(torch.uint8) for g in gt64]
    preds, c64 = ops.resize_argmax(x.to(dev), sizes, gt=gt64)
    _, c8 = ops.resize_argmax(x.to(dev), sizes, gt=[g.to(dev) for g in gt8], want_pred=False)
    _, c32 = ops.resize_argmax(x.to(dev), sizes, gt=[g.int() for g in gt64], want_pred=False)
    assert c64.shape == (3, 3, K) and c64.dtype == torch.int32
    assert torch.equal(c64, c8) and torch.equal(c64, c32)
    for i, (p, g) in enumerate(zip(preds, gt64)):
        assert torch.equal(c64[i].cpu(), recount(p, g))
        assert int(c64[i, 1].sum()) == sizes[i][0] * sizes[i][1]                  # every pixel is predicted
        assert int(c64[i, 2].sum()) == int(((g >= 0) & (g < K)).sum())
    assert int(c64[0, 2].sum()) == (683 - 9) * 512 and int(c64[1, 2].sum()) == 100 * 90 - 50     # planted -1 / K / 255 rows


def test_per_image_gt_miou_matches_an_fp64_restatement(dev):
    sizes = [(683, 512), (300, 400), (64, 80)]
    x = logits(3, 6)
    x[:, 3] += 2.5; x[:, 7] += 2.0                       # a few dominant classes, so that intersections are not empty
    gt = _gt_maps(sizes, 7, k=10)
    gt[2].zero_()                                        # nothing but ignore_index: NaN on both sides
    got = metrics.per_image_gt_mIOU(x.to(dev), gt, sizes).cpu()
    want = ref_gt_miou(x, gt, sizes)
    assert got.dtype == torch.float64 and got.shape == (3,)
    assert math.isnan(got[2]) and math.isnan(want[2])
    assert (got[:2] - want[:2]).abs().max().item() <= 1e-3
    assert torch.allclose(metrics.per_image_gt_mIOU(x.to(dev), gt, None).cpu(), got, equal_nan=True, rtol=0, atol=0)
    d = metrics.compute_gt_mIOU(x.to(dev), gt, torch.tensor(sizes))
    assert list(d) == ["mIOU_gt"] and math.isnan(d["mIOU_gt"])


def test_batched_call_equals_single_image_calls_bitwise_and_repeats(dev):
    sizes = [(683, 512), (100, 90), (1, 777), (257, 129), (16, 16)]
    x = logits(5, 8).to(dev)
    gt = [g.to(dev) for g in _gt_maps(sizes, 9)]
    preds, counts = ops.resize_argmax(x, sizes, gt=gt)
    preds2, counts2 = ops.resize_argmax(x, sizes, gt=gt)
    assert torch.equal(counts, counts2) and all(torch.equal(a, b) for a, b in zip(preds, preds2))
    for i, s in enumerate(sizes):
        p1, c1 = ops.resize_argmax(x[i:i + 1], [s], gt=[gt[i]])
        assert torch.equal(p1[0], preds[i]) and torch.equal(c1[0], counts[i])
    op = metrics.original_size_predictions(x, sizes)
    assert all(torch.equal(a, b) for a, b in zip(op, preds))


def test_peak_memory_is_a_fraction_of_the_score_map(dev):
    H, W = 2048, 1536
    x = logits(1, 10).to(dev)
    gt = _gt_maps([(H, W)], 11)[0].to(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    v = metrics.per_image_gt_mIOU(x, [gt], [(H, W)])
    preds, _ = ops.resize_argmax(x, [(H, W)])
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - base
    assert grown < K * H * W * 4 / 8, f"peak growth {grown / 2**20:.0f} MiB"
    assert v.shape == (1,) and preds[0].shape == (H, W)


class _Passthrough(nn.Module):
    def forward(self, inputs):
        return {"outputs": inputs["x"]}


def _loader(n_batches=3, per=2, hh=32, ww=32):
    g = torch.Generator().manual_seed(12)
    batches, sizes = [], [(70, 90), (45, 33), (128, 128), (31, 200), (90, 70), (64, 64)]
    for b in range(n_batches):
        x = torch.randn(per, K, hh, ww, generator=g)
        lab = torch.randint(0, K, (per, hh, ww), generator=g)
        metas = [{"gt": torch.randint(0, 20, sizes[b * per + j], generator=g).to(torch.uint8)} for j in range(per)]
        batches.append(({"x": x, "label": lab}, metas))
    return batches


def test_segmentation_metrics_and_evaluator_report_miou_gt(dev):
    batches = _loader()
    outputs = torch.cat([b[0]["x"] for b in batches]).to(dev)
    labels = torch.cat([b[0]["label"] for b in batches]).to(dev)
    gt = [m["gt"] for b in batches for m in b[1]]
    plain = evalloop.segmentation_metrics(outputs, labels)
    full = evalloop.segmentation_metrics(outputs, labels, gt_list=gt, sizes=torch.tensor([tuple(g.shape) for g in gt]))
    assert set(plain) == {"mIOU_label"} and set(full) == {"mIOU_label", "mIOU_gt"}
    assert full["mIOU_label"] == plain["mIOU_label"]
    want = metrics.compute_gt_mIOU(outputs, gt, None)["mIOU_gt"]
    assert full["mIOU_gt"] == want

    crit = lambda o, l: o.float().mean()
    hook = lambda metas: [m["gt"] for m in metas]
    base = evalloop.Evaluator(_Passthrough(), batches, crit, device=dev).evaluate()
    assert set(base) == {"eval_loss", "eval_mIOU_label"}
    ev = evalloop.Evaluator(_Passthrough(), batches, crit, device=dev, gt_from_metas=hook).evaluate()
    assert set(ev) == {"eval_loss", "eval_mIOU_label", "eval_mIOU_gt"}
    assert ev["eval_mIOU_gt"] == want and ev["eval_mIOU_label"] == base["eval_mIOU_label"]
    kept = evalloop.Evaluator(_Passthrough(), batches, crit, device=dev, gt_from_metas=hook, keep_outputs=True).evaluate()
    assert set(kept) == set(ev) and kept["eval_mIOU_gt"] == want

    seen = {}

    def reference_style(outputs, labels, gt_list, sizes, n_clas=151, ignore_index=0):
        seen.update(n=len(gt_list), sizes=sizes.tolist())
        return metrics.compute_gt_mIOU(outputs, gt_list, sizes)

    custom = evalloop.Evaluator(_Passthrough(), batches, crit, device=dev, compute_metrics=reference_style,
                                gt_from_metas=hook).evaluate()
    assert custom["eval_mIOU_gt"] == want and seen["n"] == 6 and seen["sizes"] == [list(g.shape) for g in gt]
