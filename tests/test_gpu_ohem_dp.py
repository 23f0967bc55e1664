"""The OHEM criterion under a GradReducer: a 1-rank RCCL group on the one GPU of the test box (a sum over one rank is the identity),
against the same steps without a reducer.  Each rank selects over its own batch; no collective is added by the selection."""
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
G = ROOT / "tests" / "golden"
IGN = -100


def _build(dev):
    import lc2is_amd.nn as N
    fx = torch.load(G / "base_tiny.pt", weights_only=True)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    m.load_state_dict(fx["state_dict"], strict=True)
    return m.to(dev).train(), fx


def _worker(port, out_path):
    """Fresh process: the 1-rank RCCL group is created BEFORE any other GPU call (as test_gpu_dp.py's worker does)."""
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    opts = dist.ProcessGroupNCCL.Options()
    opts.is_high_priority_stream = True
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, pg_options=opts)
    torch.cuda.set_device(dev)
    import lc2is_amd.nn as N
    from lc2is_amd.dp import GradReducer
    from lc2is_amd.step import TrainStep
    m_dp, fx = _build(dev)
    m_1, _ = _build(dev)
    red = GradReducer(bucket_elems=100_000)
    mk = lambda: N.OhemCrossEntropyLoss(1e-6, 64, label_smoothing=0.1).to(dev)   # rank-binding: the 2 * 64 hardest pixels
    ts_dp = TrainStep(m_dp, optimizer="sgd", lr=0.05, reducer=red, criterion=mk())
    red.broadcast_params(ts_dp.arena.flat, src=0)
    ts_1 = TrainStep(m_1, optimizer="sgd", lr=0.05, criterion=mk())
    inputs = {k: fx[k].to(dev) for k in ("pixel_values", "input_ids", "attention_mask")}
    labels = fx["labels"].to(dev)
    out = {"losses_dp": [], "losses_1": [], "kept_dp": [], "kept_1": []}
    for _ in range(2):
        out["losses_dp"].append(float(ts_dp.step(inputs, labels).item()))
        out["losses_1"].append(float(ts_1.step(inputs, labels).item()))
        out["kept_dp"].append(ts_dp.ohem_labels.cpu())
        out["kept_1"].append(ts_1.ohem_labels.cpu())
    torch.cuda.synchronize()
    out.update(flat_dp=ts_dp.arena.flat.cpu(), flat_1=ts_1.arena.flat.cpu(), n_labels=int(labels.numel()))
    torch.save(out, out_path)
    dist.barrier()
    dist.destroy_process_group()


def test_ohem_step_under_a_one_rank_reducer(dev, tmp_path):
    ctx = mp.get_context("spawn")
    port = 29900 + os.getpid() % 90
    outp = tmp_path / "ohem_rccl1.pt"
    p = ctx.Process(target=_worker, args=(port, str(outp)))
    p.start()
    p.join(timeout=300)
    if p.is_alive():
        p.terminate(); p.join(30)
        if p.is_alive():
            p.kill(); p.join()
        pytest.fail("the 1-rank RCCL worker did not finish within 300 s")
    assert p.exitcode == 0, p.exitcode
    r = torch.load(outp, weights_only=True)
    assert r["losses_dp"] == pytest.approx(r["losses_1"], abs=1e-5)
    assert torch.equal(r["kept_dp"][0], r["kept_1"][0])              # the same parameters: the same selection
    assert int((r["kept_dp"][0] != IGN).sum()) == 128 < r["n_labels"]
    assert (r["flat_dp"] - r["flat_1"]).abs().max().item() < 1e-6
