"""Every public launcher of lc2is_amd/ops.py (a function that calls ``_fn("lc2is_...")``) is called directly, as
``ops.<name>(``, by some GPU test — or is listed in EXEMPT with the reason.  A launcher reached only through module tests at
one golden shape is how grid-stride loops, tile-plan switches and batch strides went untested; this keeps that gap closed."""
import ast
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
OPS = ROOT / "lc2is_amd" / "ops.py"

EXEMPT = {
    "release_captured_tables": "host bookkeeping of captured descriptor tables: frees host memory, launches no kernel",
    "captured_tables_mark": "host bookkeeping of captured descriptor tables: returns a counter, launches no kernel",
    "release_captured_tables_range": "host bookkeeping of captured descriptor tables: frees host memory, launches no kernel",
}


def launchers(src: str) -> list[str]:
    """Public top-level functions of ops.py whose body calls _fn with an "lc2is_..." symbol name."""
    out = []
    for f in ast.parse(src).body:
        if not isinstance(f, ast.FunctionDef) or f.name.startswith("_"):
            continue
        for node in ast.walk(f):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_fn" and any(
                    isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("lc2is_")
                    for a in node.args for c in ast.walk(a)):
                out.append(f.name)
                break
    return out


def gpu_test_sources() -> dict[str, str]:
    return {p.name: p.read_text() for p in sorted((ROOT / "tests").glob("test_gpu_*.py"))}


def uncovered(names, sources) -> list[str]:
    return [n for n in names if n not in EXEMPT and not any(re.search(rf"\bops\.{n}\(", s) for s in sources.values())]


def test_launcher_list_is_found():
    names = launchers(OPS.read_text())
    # spot checks that the parser sees what it should: plain, conditional (rows_copy) and multi-symbol launchers
    for n in ("gemm_nt", "gemm_nt_batched", "rows_copy", "layernorm_bwd", "miou_counts", "crop_lut", "ln_defer_flush"):
        assert n in names, n
    assert "gemm_nt_ln_ok" not in names and "workspace" not in names   # pure host helpers
    assert len(names) >= 50


def test_every_launcher_is_called_directly_by_a_gpu_test():
    missing = uncovered(launchers(OPS.read_text()), gpu_test_sources())
    assert not missing, f"launchers of lc2is_amd/ops.py no GPU test calls as ops.<name>(: {missing} (test them, or add to EXEMPT)"


def test_exemptions_are_current():
    names = set(launchers(OPS.read_text()))
    stale = [n for n in EXEMPT if n not in names]
    assert not stale, f"EXEMPT lists names that are no longer launchers of ops.py: {stale}"
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in EXEMPT.values())


@pytest.mark.parametrize("name", ["gemm_nt_batched", "transpose_bf16_batched", "upsample_bwd_nchw", "rows_ce", "cols_ce", "npair",
                                  "npair_bwd", "miou_counts", "sr_scatter_add", "swin_bias_table_grad", "gather2d_u8", "crop_lut",
                                  "ln_defer_flush"])
def test_check_notices_a_deleted_call(name):
    """Removing every direct call of one of the launchers the direct tests were added for makes the check fail."""
    sources = gpu_test_sources()
    assert not uncovered([name], sources)
    stripped = {k: re.sub(rf"\bops\.{name}\(", "ops.removed(", v) for k, v in sources.items()}
    assert uncovered([name], stripped) == [name]
