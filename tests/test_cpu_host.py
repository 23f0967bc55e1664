"""CPU-only checks of the host side: the C-ABI library loads and exports every declared symbol, the drop-in
modules keep the reference's state_dict keys and refuse to run without a GPU, and the arena/step plumbing."""
import ctypes
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
G = ROOT / "tests" / "golden"


def test_library_exports_every_declared_symbol():
    from lc2is_amd import _lib, ops
    if not _lib.lib_path().exists():
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    syms = _lib.header_symbols()
    assert len(syms) >= 25 and "lc2is_gemm_nt_bf16" in syms and "lc2is_attention_bwd" in syms
    for s in syms:
        assert isinstance(getattr(lib, s), ctypes._CFuncPtr), s
    assert _lib.version().startswith("lc2is_hip") and "gfx950" in _lib.version()
    # every entry point has explicit argtypes in the binding
    assert set(syms) - {"lc2is_version"} <= set(ops._ARGTYPES)


def test_workspace_size_queries_are_pure_host_functions():
    from lc2is_amd import ops
    assert ops._fn("lc2is_gemm_tn_workspace_bytes")(32800, 3072, 768) == 7 * 3072 * 769 * 4
    assert ops._fn("lc2is_gemm_tn_workspace_bytes")(64, 64, 64) == 0
    assert ops._fn("lc2is_colsum_workspace_bytes")(100, 64) == 25 * 64 * 4
    assert ops._fn("lc2is_layernorm_bwd_workspace_bytes")(10, 64) == 3 * 2 * 64 * 4


def test_grouped_weight_gradient_planner_on_the_host():
    """The grouped-launch planner is host code: its slab workspace tells which plan it chose.
    One ViT-B layer (108 tiles): every problem split in two.  The whole tower (72 problems, 1296 tiles = 5 rounds + 16):
    full-length blocks for the bulk, only two 9-tile problems split 14-way to fill the last round (+ the descriptor table).
    A group off the 256 grid (Swin block) takes the 128x128 plan."""
    from lc2is_amd import ops
    M, C, F = 32800, 768, 3072
    layer = [(C, C)] * 4 + [(F, C), (C, F)]           # q, k, v, o, fc1, fc2 as (N, K)

    def ws_bytes(shapes):
        arr = (ops.TnProblem * len(shapes))()
        for i, (N, K) in enumerate(shapes):
            arr[i] = ops.TnProblem(0x1000, 0x1000, 0x1000, 0x1000, N, K, K, M, N, K, 0)   # pointers are not dereferenced
        return ops._fn("lc2is_gemm_tn_grouped_workspace_bytes")(arr, len(shapes))

    slab = lambda sp, N, K: sp * N * (K + 1) * 4
    assert ws_bytes(layer) == sum(slab(2, N, K) for N, K in layer)
    tower = ws_bytes(layer * 12)
    table = tower - 2 * slab(14, C, C)
    assert 0 < table <= 32768 and table % 256 == 0
    swin = [(384, 384)] * 4 + [(1536, 384), (384, 1536)]
    assert ws_bytes(swin) > 0 and ws_bytes(swin) % 4 == 0
    assert ws_bytes([(100, 100)]) == 0                # N % 8 != 0: refused


def test_launchers_refuse_bad_arguments_without_touching_a_gpu():
    """Argument validation happens before any HIP call: NULL pointers / bad shapes return negative codes."""
    from lc2is_amd import _lib, ops
    f = ops._fn("lc2is_gemm_nt_bf16")
    assert f(None, 64, None, 64, None, None, 0, None, 0, None, 0, None, 0, None, 0, 8, 8, 64, 0, 0, None) == -2
    assert f(1, 64, 1, 64, None, None, 0, None, 0, 1, 8, None, 0, None, 0, 8, 8, 63, 0, 0, None) == -1
    with pytest.raises(RuntimeError, match="refused"):
        _lib.check(-1, "x")


def test_state_dict_keys_match_reference_fixture():
    import lc2is_amd.nn as N
    fx = torch.load(G / "base_tiny.pt", weights_only=True)
    m = N.BaseModelWithText(16, 64, 16, vision_arch=N.ClipArch(128, 2, 2, 256),
                            text_arch=N.ClipArch(64, 1, 2, 128, vocab=512, eos_token_id=511), nhead=2,
                            dim_feedforward=128, out_dim=64)
    assert set(m.state_dict().keys()) == set(fx["state_dict"].keys())
    m.load_state_dict(fx["state_dict"], strict=True)
    # legacy transformers<5 prefix (enc.vision_model.* / enc.text_model.*) also loads
    legacy = {}
    for k, v in fx["state_dict"].items():
        k = k.replace("vision_encoder.enc.", "vision_encoder.enc.vision_model.").replace(
            "text_encoder.enc.", "text_encoder.enc.text_model.")
        legacy[k] = v
    m.load_state_dict(legacy, strict=True)
    blk = N.DecoderBlock(N.DecoderLayer(192, 128, 2, dim_feedforward=128, batch_first=True, norm_first=True), 2)
    dfx = torch.load(G / "decoder_d96.pt", weights_only=True)
    assert set(blk.state_dict().keys()) == set(dfx["state_dict"].keys())
    biased = N.DecoderLayer(192, 128, 2, dim_feedforward=128, batch_first=True, norm_first=True, bias=True)
    assert "self_attn.in_proj_bias" in biased.state_dict() and "norm1.bias" in biased.state_dict()


def test_full_size_parameter_count_matches_survey():
    import lc2is_amd.nn as N
    m = N.BaseModelWithText(16, 512, 128)
    n = sum(p.numel() for p in m.parameters())
    # SURVEY.md §8e probed 157.09 M with a 128x128 position table (65 rows); at 512x512 the table has 1025 rows
    # (+0.737 M): 157.81 M, which is the all-reduce payload of BASELINE configs 2/3
    assert abs(n - (157.09e6 + (1025 - 65) * 768)) < 0.03e6, n


def test_product_has_no_cpu_path_and_never_imports_the_oracle():
    import lc2is_amd.nn as N
    enc = N.ImageEncoderCLIP(64, 16, arch=N.ClipArch(128, 2, 1, 256))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(1, 3, 64, 64))
    for f in (ROOT / "lc2is_amd").rglob("*.py"):
        text = f.read_text()
        assert "import oracle" not in text and "from oracle" not in text, f


def test_pos_embedding_interpolation_matches_reference_vector():
    """ImageEncoderCLIP.pos_emebedding_interpolate (model/encoder.py:32-44) and the load-time resize of a 224x224 table."""
    import lc2is_amd.nn as N
    fx = torch.load(G / "ops.pt", weights_only=True)
    enc = N.ImageEncoderCLIP(128, 16, arch=N.ClipArch(32, 1, 1, 64))
    out = enc.pos_emebedding_interpolate(8, weight=fx["posint_in"])
    assert torch.allclose(out, fx["posint_out"], atol=1e-5)
    sd = enc.state_dict()
    sd["enc.embeddings.position_embedding.weight"] = fx["posint_in"]          # 197 rows, as in a hub checkpoint
    enc.load_state_dict(sd, strict=True)
    assert torch.allclose(enc.enc.embeddings.position_embedding.weight, fx["posint_out"], atol=1e-5)


def test_prompt_aliases_exist():
    import lc2is_amd.nn as N
    layer = N.PromptLayer(d_model=128, d_kv=256, nhead=2, batch_first=True)
    assert layer.dropout_p == 0.1 and isinstance(N.PromptDecoder(layer, 2), N.DecoderBlock)


def test_evaluator_host_logic_matches_engine_eval_loop():
    """lc2is_amd.evalloop.Evaluator mirrors Engine.eval_loop (engine.py:134-168): label popped from the batch dict, loss =
    mean over batches of the per-batch criterion, aux loss x 0.4 when the model returns low_score_map, metric keys
    prefixed eval_.  (Host logic only: a toy CPU module and torch's CE stand in for the HIP model.)"""
    import torch
    from torch import nn
    from lc2is_amd.evalloop import Evaluator

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.randn(5, 3))

        def forward(self, inputs):
            assert "label" not in inputs and not self.training
            x = inputs["pixel_values"]                                  # [B,3,h,w]
            out = torch.einsum("kc,bchw->bkhw", self.w, x)
            return dict(outputs=out, low_score_map=out[:, :, ::2, ::2])

    class Aux(nn.Module):
        def forward(self, low, labels):
            return nn.functional.cross_entropy(low, labels[:, ::2, ::2])

    g = torch.Generator().manual_seed(0)
    batches = [(dict(pixel_values=torch.randn(b, 3, 4, 4, generator=g), label=torch.randint(0, 5, (b, 4, 4), generator=g)), None)
               for b in (1, 3, 2)]
    toy = Toy().train()
    seen = {}

    def metric(outputs, labels):
        seen["shapes"] = (tuple(outputs.shape), tuple(labels.shape))
        return dict(mIOU_label=0.25)

    ev = Evaluator(toy, batches, nn.CrossEntropyLoss(), aux_criterion=Aux(), compute_metrics=metric, device="cpu")
    got = ev.evaluate()
    with torch.no_grad():
        per = [float(nn.functional.cross_entropy(toy(dict(pixel_values=b[0]["pixel_values"]))["outputs"], b[0]["label"]))
               for b in batches]
    assert abs(got["eval_loss"] - sum(per) / 3) < 1e-6                  # mean over BATCHES (engine.py:165), not over pixels
    assert set(got) == {"eval_loss", "eval_aux_loss", "eval_mIOU_label"} and got["eval_mIOU_label"] == 0.25
    assert seen["shapes"] == ((6, 5, 4, 4), (6, 4, 4))
    assert "label" in batches[0][0]                                     # the caller's batch dict is left intact


def test_product_path_has_no_library_math():
    """PyTorch is plumbing (memory, streams, autograd between modules), never the math of the path: no matmul-family call
    may appear under lc2is_amd/ except the init-time (host, load-time) position-table resize of model/encoder.py:32-44."""
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent / "lc2is_amd"
    pat = re.compile(r"torch\.(mm|matmul|bmm|addmm|baddbmm|einsum|tensordot)\b|F\.(linear|conv2d|scaled_dot_product_attention)\b"
                     r"|nn\.functional\.(linear|conv2d|scaled_dot_product_attention)\b")
    hits = []
    for f in sorted(root.rglob("*.py")):
        for n, line in enumerate(f.read_text().splitlines(), 1):
            code = line.split("#", 1)[0]
            if pat.search(code):
                hits.append((str(f.relative_to(root)), code.strip()))
    # the one allowed use: pos_emebedding_interpolate's separable bicubic resize of the 14x14 position table at load time
    assert len(hits) == 1 and hits[0][0] == "nn/clip.py" and "yi,ijc,xj->yxc" in hits[0][1], hits


def test_swin_relative_position_csr_inverts_the_index():
    """The CSR index swin_bias_table_grad sums in: row t lists exactly the (query, key) pairs whose relative_position_index
    is t, in ascending order, and every pair appears once."""
    from lc2is_amd.nn.swin import relative_position_csr, relative_position_index
    for ws in (2, 7, 12):
        idx = relative_position_index(ws)
        offs, ids = relative_position_csr(ws)
        T = (2 * ws - 1) ** 2
        assert offs.dtype == ids.dtype == torch.int32 and offs.shape == (T + 1,) and ids.shape == (ws ** 4,)
        assert offs[0] == 0 and offs[-1] == ws ** 4 and bool((offs[1:] >= offs[:-1]).all())
        assert torch.equal(ids.sort().values, torch.arange(ws ** 4, dtype=torch.int32))
        for t in range(T):
            row = ids[offs[t]:offs[t + 1]].long()
            assert torch.equal(row, torch.nonzero(idx == t).flatten()), (ws, t)
