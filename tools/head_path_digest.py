"""Digests of every path through the fused head's criteria, to compare two trees of this project line for line.

  python tools/head_path_digest.py --root TREE --validate   (no device)
      sweeps the cross product of the criterion keywords, invalid values included, through BaseModelWithText.forward_loss,
      ScoreMapTail(4).loss, ScoreMapTail(8).loss and PromptFTN.forward_loss, and records what each call raises first
      ("type: message"; a call that passes every refusal stops at the first thing that needs the inputs or the device).
  python tools/head_path_digest.py --root TREE              (one HIP device)
      runs the model site, the tail site, TrainStep and the NCHW criteria for fixed seeds and prints a sha256 of the raw bytes of
      each loss, gradient and published statistic (raw bytes: NaN-safe).
  python tools/head_path_digest.py --root TREE --nchw       (one HIP device)
      the NCHW criteria alone, at more shapes: one block, ragged blocks, past the grid caps, C = 1, C = 192.

``--root`` is the tree whose ``lc2is_amd`` is imported (default: the tree this file is in); set LC2IS_LIB to share one built
library between trees.  ``--out FILE`` writes the lines there; the last line of stdout is always "sha256 <hash> <n> lines".
"""
import argparse
import hashlib
import itertools
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
IGN = -100
TINY = dict(vision=(128, 2, 2, 256), text=(64, 1, 2, 128))


def _tiny(N, torch, K):
    fx = torch.load(HERE / "tests" / "golden" / "base_tiny.pt", weights_only=True)
    sd = dict(fx["state_dict"])
    protos = None
    if K != sd["class_prototypes"].shape[0]:
        protos = torch.randn(K, sd.pop("class_prototypes").shape[1], generator=torch.Generator().manual_seed(5))
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(*TINY["vision"]),
                            text_arch=N.ClipArch(*TINY["text"], vocab=512, eos_token_id=511), nhead=2, dim_feedforward=128,
                            out_dim=64, **({} if protos is None else {"prototypes": protos}))
    m.load_state_dict(sd, strict=protos is None)
    return m


# ---- --validate ---------------------------------------------------------------------------------------------------------------
class _Towers(Exception):
    pass


def validate(N, torch, emit):
    def raised(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except Exception as e:   # noqa: BLE001  (the sweep records whatever comes first)
            return f"{type(e).__name__}: {e}"
        return "returned"

    class _Ftn:
        tail = N.ScoreMapTail(4)

        def _embeddings(self, inputs):
            raise _Towers("towers")

    accum_block = torch.zeros(4, dtype=torch.float64)
    for K in (151, 193):
        model = _tiny(N, torch, K)
        values = dict(
            weight=[("none", None), ("given", torch.ones(K))],
            label_smoothing=[("0", 0.0), ("0.1", 0.1), ("1.5", 1.5)],
            reduction=[(r, r) for r in ("mean", "sum", "none", "bad")],
            ohem=[("none", None), ("valid", (0.7, 8)), ("thresh1.5", (1.5, 8))],
            dice=[("none", None), ("valid", (1.0, 1.0, 1.0, True)), ("w00", (0.0, 0.0, 1.0, True))],
            focal=[("none", None), ("valid", (2.0, 0.0)), ("gamma-1", (-1.0, 0.0))],
            sigmoid=[("none", None), ("valid", (2.0, 0.25, "elements")), ("alpha2", (2.0, 2.0, "elements"))],
            accum=[("none", None), ("given", accum_block)],
            seg_counts=[("none", None), ("right", torch.zeros(3, K, dtype=torch.int64)), ("wrong", torch.zeros(3, K + 1, dtype=torch.int64))])
        tails = {S: (N.ScoreMapTail(S), (torch.zeros(1, 4, 64), torch.zeros(1, K, 64), torch.zeros(1, 2 * S, 2 * S, dtype=torch.long)))
                 for S in (4, 8)}
        labels = torch.zeros(1, 16, 16, dtype=torch.long)
        for combo in itertools.product(*values.values()):
            tag = f"K={K} " + " ".join(f"{k}={name}" for k, (name, _) in zip(values, combo))
            kw = {k: v for k, (_, v) in zip(values, combo)}
            emit(f"model {tag} -> {raised(model.forward_loss, {}, labels, **kw)}")
            for S, (tail, args) in tails.items():
                emit(f"tail{S} {tag} -> {raised(tail.loss, *args, **kw)}")
            if kw["ohem"] is None and kw["dice"] is None:   # PromptFTN.forward_loss has neither keyword
                ftn_kw = {k: v for k, v in kw.items() if k not in ("ohem", "dice")}
                emit(f"ftn {tag} -> {raised(N.PromptFTN.forward_loss, _Ftn(), {}, labels, **ftn_kw)}")


# ---- digests on the device ----------------------------------------------------------------------------------------------------
def _sha(torch, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"<none>")
        elif isinstance(t, torch.Tensor):
            h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
        else:
            h.update(repr(t).encode())
    return h.hexdigest()[:20]


def _labels(torch, B, H, W, K, seed, all_ignored=False):
    """As tests/head_cases.py draws them: some >= K, every fifth row ignored."""
    labels = torch.randint(0, K + 3, (B, H, W), generator=torch.Generator().manual_seed(seed))
    labels[:, 1::5] = IGN
    return torch.full_like(labels, IGN) if all_ignored else labels


def _criteria(torch, K, dev):
    w = (0.5 + torch.rand(K, generator=torch.Generator().manual_seed(3))).to(dev)
    return [("default", {}), ("weight", dict(weight=w)), ("smoothing", dict(label_smoothing=0.1)), ("sum", dict(reduction="sum")),
            ("ohem", dict(ohem=(0.7, 8))), ("dice", dict(dice=(1.0, 1.0, 1.0, True))),
            ("focal+weight", dict(focal=(2.0, 0.0), weight=w)), ("focal+ohem", dict(focal=(2.0, 1.0), ohem=(0.7, 8))),
            ("sigmoid-elements-mean", dict(sigmoid=(2.0, 0.25, "elements"))),
            ("sigmoid-pixels-sum", dict(sigmoid=(0.0, None, "pixels"), reduction="sum"))]


def _site_cases(torch, K, dev):
    """(name, keywords, accum?, seg_counts?, all labels ignored?) of one site."""
    crit = _criteria(torch, K, dev)
    if K > 192:
        w = crit[1][1]["weight"]
        return [("default", {}, False, False, False), ("weight+sum", dict(weight=w, reduction="sum"), False, False, False),
                ("accum", {}, True, False, False), ("seg_counts", {}, False, True, False)]
    cases = [(name, kw, accum, seg, False) for name, kw in crit for accum in (False, True) for seg in (False, True)
             if not (accum and "dice" in kw)]
    return cases + [("default all-ignored", {}, False, False, True), ("weight all-ignored", crit[1][1], False, False, True)]


def _run_site(torch, emit, site, K, dev, loss_fn, owner, grads):
    """``loss_fn(labels, **kw)`` -> loss; ``grads()`` -> the tensors whose gradients are digested (cleared before each case)."""
    for name, kw, accum, seg, ignored in _site_cases(torch, K, dev):
        extra = {}
        if accum:
            extra["accum"] = torch.zeros(4, dtype=torch.float64, device=dev)
        if seg:
            extra["seg_counts"] = torch.zeros(3, K, dtype=torch.int64, device=dev)
        for t in grads():
            t.grad = None
        owner.last_dice = owner.last_ohem = None
        loss = loss_fn(_labels(torch, 2, 16, 16, K, 11, ignored).to(dev), **kw, **extra)
        loss.backward()
        emit(f"{site} K={K} {name} accum={int(accum)} seg={int(seg)} | loss={_sha(torch, loss)} "
             f"grads={_sha(torch, *[t.grad for t in grads()])} last_dice={_sha(torch, *(owner.last_dice or (None,)))} "
             f"last_ohem={_sha(torch, *(owner.last_ohem or (None,)))} seg_counts={_sha(torch, extra.get('seg_counts'))} "
             f"accum_block={_sha(torch, extra.get('accum'))}")


def _inputs(torch, dev):
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(1, 500, (2, 8), generator=g)
    ids[:, 0], ids[:, -1] = 510, 511
    return {"pixel_values": torch.randn(2, 3, 64, 64, generator=g).to(dev), "input_ids": ids.to(dev),
            "attention_mask": torch.ones(2, 8, dtype=torch.long).to(dev)}


def digest(N, torch, emit):
    from lc2is_amd.step import TrainStep
    dev = torch.device("cuda", 0)
    inputs = _inputs(torch, dev)
    for K in (151, 193):
        model = _tiny(N, torch, K).to(dev).train()
        params = [p for p in model.parameters() if p.requires_grad]
        _run_site(torch, emit, "model", K, dev, lambda labels, **kw: model.forward_loss(inputs, labels, **kw), model, lambda: params)
        if K == 151:
            for p in params:
                p.grad = None
            logits = model(inputs)["outputs"]
            gout = torch.randn(logits.shape, generator=torch.Generator().manual_seed(13)).to(dev)
            logits.backward(gout)
            emit(f"model K={K} forward | logits={_sha(torch, logits)} grads={_sha(torch, *[p.grad for p in params])}")
        emit(f"model K={K} predict | pred={_sha(torch, model.predict(inputs))}")
        tail = N.ScoreMapTail(4)
        g = torch.Generator().manual_seed(17)
        visual = torch.randn(2, 16, 64, generator=g).to(dev).requires_grad_(True)
        text = torch.randn(2, K, 64, generator=g).to(dev).requires_grad_(True)
        _run_site(torch, emit, "tail", K, dev, lambda labels, **kw: tail.loss(visual, text, labels, **kw), tail, lambda: [visual, text])
    K = 151
    w = (0.5 + torch.rand(K, generator=torch.Generator().manual_seed(3)))
    labels = _labels(torch, 2, 16, 16, K, 11).to(dev)
    steps = [("none", None, {}), ("CrossEntropyLoss(weight, smoothing)", N.CrossEntropyLoss(weight=w, label_smoothing=0.1), {}),
             ("OhemCrossEntropyLoss", N.OhemCrossEntropyLoss(0.7, 8), {}), ("DiceCrossEntropyLoss", N.DiceCrossEntropyLoss(), {}),
             ("FocalLoss(weight)", N.FocalLoss(2.0, weight=w), {}), ("SigmoidFocalLoss(sum)", N.SigmoidFocalLoss(reduction="sum"), {}),
             ("FocalLoss accumulate=2 seg_metrics", N.FocalLoss(2.0, 1.0), dict(accumulate=2, seg_metrics=True))]
    for name, crit, extra in steps:
        model = _tiny(N, torch, K).to(dev).train()
        ts = TrainStep(model, optimizer="sgd", lr=1e-3, criterion=None if crit is None else crit.to(dev), **extra)
        losses = [ts.step(inputs, labels) for _ in range(extra.get("accumulate", 1))]
        pub = [getattr(crit, a, None) for a in ("last_labels", "last_info")] + list(getattr(crit, "last_stats", None) or ())
        emit(f"TrainStep {name} | loss={_sha(torch, *losses)} arena={_sha(torch, ts.arena.flat)} published={_sha(torch, *pub)} "
             f"seg_counts={_sha(torch, ts.seg_counts if extra else None)}")
    digest_nchw(N, torch, emit)


# one block; several ragged blocks; past the grid cap of the per-pixel kernels (8192 blocks) and of the Dice statistics (2048); C = 1;
# the Dice class limit (Dice only)
NCHW_SHAPES = ((2, 10, 12, 9), (2, 151, 24, 20), (1, 2, 1449, 1449), (1, 3, 725, 725), (1, 1, 5, 7), (1, 192, 9, 7))


def digest_nchw(N, torch, emit):
    """The criteria on materialised NCHW logits: every module and reduction, then each ``ops.*_nchw_bwd`` called directly with a
    device scalar (0.25) times a host scale (2.0)."""
    from lc2is_amd import ops
    dev = torch.device("cuda", 0)
    for B, C, H, W in NCHW_SHAPES:
        g = torch.Generator().manual_seed(19)
        z = (torch.randn(B, C, H, W, generator=g) * 3).to(dev)
        lab = _labels(torch, B, H, W, C, 23).to(dev)
        wc = (0.5 + torch.rand(C, generator=g)).to(dev)
        gpx = torch.randn(B, H, W, generator=g).to(dev)
        shape = f"{B}x{C}x{H}x{W}"
        modules = (("CrossEntropyLoss", lambda r: N.CrossEntropyLoss(reduction=r)),
                   ("CrossEntropyLoss(weight, smoothing)", lambda r: N.CrossEntropyLoss(weight=wc, label_smoothing=0.1, reduction=r)),
                   ("FocalLoss(weight)", lambda r: N.FocalLoss(2.0, 1.0, weight=wc, reduction=r)),
                   ("SigmoidFocalLoss(weight)", lambda r: N.SigmoidFocalLoss(2.0, 0.25, weight=wc, reduction=r)),
                   ("SigmoidFocalLoss(pixels)", lambda r: N.SigmoidFocalLoss(0.0, None, normalize="pixels", reduction=r)),
                   ("OhemCrossEntropyLoss(weight)", lambda r: N.OhemCrossEntropyLoss(0.7, 8, weight=wc, reduction=r)),
                   ("DiceCrossEntropyLoss", lambda r: N.DiceCrossEntropyLoss(reduction=r)))
        for name, make in modules[6 if C == 192 else 0:]:
            for reduction in ("mean", "sum", "none"):
                if (name.startswith("Dice") and reduction != "mean") or (name.startswith("Ohem") and reduction == "none"):
                    continue
                for ignored in (False, True):
                    x = z.clone().requires_grad_(True)
                    target = torch.full_like(lab, IGN) if ignored else lab
                    loss = make(reduction)(x, target)
                    loss.backward(gpx if reduction == "none" else None)
                    emit(f"nchw {shape} {name} {reduction} all-ignored={int(ignored)} | loss={_sha(torch, loss)} "
                         f"dlogits={_sha(torch, x.grad)}")
        quarter = torch.full((1,), 0.25, device=dev)
        loss4, stats, lse, coef = ops.ce_dice_nchw_fwd(z, lab, IGN)
        direct = [("ce_dice", (loss4, stats, coef), ops.ce_dice_nchw_bwd(z, lab, lse, coef, quarter, 2.0, IGN))]
        if C != 192:
            kw = dict(class_weight=wc, label_smoothing=0.1)
            loss2, lse = ops.ce_nchw_fwd(z, lab, IGN)
            direct.append(("ce", (loss2, lse), ops.ce_nchw_bwd(z, lab, lse, quarter, 2.0, IGN)))
            loss2, lse = ops.ce_nchw_fwd(z, lab, IGN, **kw)
            direct.append(("ce(weight, smoothing)", (loss2, lse), ops.ce_nchw_bwd(z, lab, lse, quarter, 2.0, IGN, **kw)))
            kw = dict(class_weight=wc, gamma=2.0, poly_eps=1.0)
            loss2, lse = ops.focal_nchw_fwd(z, lab, IGN, **kw)
            direct.append(("focal", (loss2, lse), ops.focal_nchw_bwd(z, lab, lse, quarter, 2.0, IGN, grad_px=gpx, **kw)))
            kw = dict(class_weight=wc, gamma=2.0, alpha=0.25, class_scale=1.0 / C)
            loss2 = ops.sigmoid_focal_nchw_fwd(z, lab, IGN, **kw)
            direct.append(("sigmoid_focal", (loss2,), ops.sigmoid_focal_nchw_bwd(z, lab, quarter, 2.0, IGN, **kw)))
        for name, fwd, d in direct:
            emit(f"nchw {shape} ops.{name}_nchw fwd+bwd scale=0.25*2.0 | fwd={_sha(torch, *fwd)} dlogits={_sha(torch, d)}")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--validate", action="store_true")
    ap.add_argument("--nchw", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.root).resolve()))
    import torch

    import lc2is_amd.nn as N
    assert Path(N.__file__).resolve().is_relative_to(Path(a.root).resolve()), N.__file__
    out = open(a.out, "w") if a.out else None
    h, n = hashlib.sha256(), 0

    def emit(line):
        nonlocal n
        h.update(line.encode() + b"\n")
        n += 1
        print(line, file=out or sys.stdout)

    (validate if a.validate else digest_nchw if a.nchw else digest)(N, torch, emit)
    if out:
        out.close()
    print(f"sha256 {h.hexdigest()} {n} lines")


if __name__ == "__main__":
    main()
