"""Read-modify-write atomics (``atomicAdd``, ``unsafeAtomicAdd``, ``__hip_atomic_fetch_add``) in lc2is_amd/csrc are listed
in ALLOWED, per enclosing kernel or function, with the reason they cannot cost the training step its run-to-run bits: an
integer sum is exact in any order, and a float sum is allowed only off the step path.  A float atomic put back into one of the
step's reductions (head slabs, token-embedding gradient, split-K reduce, LayerNorm partials) makes the loss and the
gradients differ in their last bits from run to run; tolerance-based tests do not notice, this scan does.  Atomic loads and
stores (the GEMM + LayerNorm statistics exchange) are not read-modify-write and are not flagged."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lc2is_amd" / "csrc"

ALLOWED = {
    "lds_add": "float LDS add of the atomic head path (head_ce_kernel, S not in 4/8/16): off the step path, which runs S = 4",
    "head_ce_kernel": "float loss / count / gradient adds of the atomic head path (S not in 4/8/16): off the step path (S = 4)",
    "ce_nchw_fwd_kernel": "float loss sums of the workspace-less lc2is_ce_nchw_fwd / _opts C entry points, kept for the ABI: "
                          "off the step path, and ops.ce_nchw_fwd takes the ordered entry point",
    "rows_ce_kernel": "float loss sum of the contrastive rows CE (ContrastiveLoss): off the BaseModelWithText step path",
    "cols_ce_kernel": "float loss sum of the contrastive columns CE (ContrastiveLoss): off the BaseModelWithText step path",
    "miou_counts_kernel": "integer, exact in any order: per-class prediction / label / intersection pixel counts",
}

RMW = re.compile(r"\b(atomicAdd|unsafeAtomicAdd|__hip_atomic_fetch_add)\s*\(")
NOT_A_NAME = {"__launch_bounds__", "__attribute__", "alignas", "decltype", "sizeof", "operator", "if", "for", "while"}


def _blank(m):
    return re.sub(r"[^\n]", " ", m.group(0))


def strip_code(src: str) -> str:
    """Comments and string / character literals replaced by spaces (line numbers kept)."""
    return re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", _blank, src, flags=re.S)


def functions(src: str, kernels_only: bool = False) -> list[tuple[str, int, int]]:
    """(name, start, end) character spans of the function bodies of `src` (comments stripped) that are not nested in another
    function: namespaces and extern "C" blocks are looked through, struct bodies searched for member functions.
    kernels_only: the __global__ functions only."""
    code = strip_code(src)
    code = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", _blank, code, flags=re.M)   # preprocessor lines, continuations included
    out, stack, boundary = [], [], 0   # stack: (kind, name, start) per open brace
    for i, ch in enumerate(code):
        if ch == "{":
            in_fn = any(k in ("fn", "skip") for k, _, _ in stack)
            if in_fn:
                stack.append(("blk", None, i))
            else:
                head = code[boundary:i]
                names = [n for n in re.findall(r"\b([A-Za-z_]\w*)\s*\(", head) if n not in NOT_A_NAME]
                if re.match(r"\s*(namespace\b|extern\s*$)", head) or not names:
                    stack.append(("scope", None, i))
                else:
                    stack.append(("fn" if not kernels_only or "__global__" in head else "skip", names[0], i))
            boundary = i + 1
        elif ch == "}":
            kind, name, start = stack.pop()
            if kind == "fn":
                out.append((name, start, i + 1))
            boundary = i + 1
        elif ch == ";":
            boundary = i + 1
    assert not stack, "unbalanced braces"
    return out


def rmw_sites(src: str, fname: str = "<src>") -> list[tuple[str, int, str, str]]:
    """(file, line, enclosing function or '<top level>', atomic) for every read-modify-write atomic call in `src`."""
    code = strip_code(src)
    spans = functions(src)
    sites = []
    for m in RMW.finditer(code):
        owner = [n for n, a, b in spans if a <= m.start() < b]
        sites.append((fname, code.count("\n", 0, m.start()) + 1, owner[0] if owner else "<top level>", m.group(1)))
    return sites


def sources() -> dict[str, str]:
    files = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h"))
    assert files
    return {p.name: p.read_text() for p in files}


def all_sites():
    return [s for name, src in sources().items() for s in rmw_sites(src, name)]


def test_scan_sees_todays_sites():
    """The scan maps each known atomic to its kernel, and the GEMM + LayerNorm exchange's atomic loads / stores are not flagged."""
    by_fn = {}
    for f, line, fn, op in all_sites():
        by_fn.setdefault(fn, set()).add((f, op))
    assert by_fn.get("lds_add") == {("head.hip", "__hip_atomic_fetch_add")}
    assert by_fn.get("head_ce_kernel") == {("head.hip", "atomicAdd")}
    assert by_fn.get("miou_counts_kernel") == {("losses.hip", "atomicAdd")}
    assert "<top level>" not in by_fn
    assert not any(f.startswith("gemm_nt") for f, _, _, _ in all_sites())
    assert "__hip_atomic_store" in sources()["gemm_nt.hip"] and "__hip_atomic_load" in sources()["gemm_nt.hip"]


def test_no_read_modify_write_atomic_outside_allowed():
    bad = [s for s in all_sites() if s[2] not in ALLOWED]
    assert not bad, ("read-modify-write atomics outside ALLOWED (a float sum in any order is not reproducible; make the "
                     f"reduction ordered, or add the kernel with its reason): {bad}")


def test_allowed_entries_are_current():
    found = {s[2] for s in all_sites()}
    stale = [n for n in ALLOWED if n not in found]
    assert not stale, f"ALLOWED lists functions that hold no read-modify-write atomic any more: {stale}"
    for name, why in ALLOWED.items():
        assert why.strip() and "\n" not in why, name
        assert "integer, exact in any order" in why or "off the step path" in why or "off the BaseModelWithText step path" in why, name


def test_allowed_helpers_are_called_only_by_allowed_functions():
    """An allowed device helper (lds_add) carries its atomic into every caller: each caller must be allowed too."""
    kernels = {n for src in sources().values() for n, _, _ in functions(src, kernels_only=True)}
    helpers = [n for n in ALLOWED if n not in kernels]
    assert "lds_add" in helpers and "head_ce_kernel" in kernels
    for fname, src in sources().items():
        code = strip_code(src)
        for fn, a, b in functions(src):
            for h in helpers:
                if fn != h and re.search(rf"\b{h}\s*\(", code[a:b]):
                    assert fn in ALLOWED, f"{fname}: {fn} calls the atomic helper {h} but is not in ALLOWED"


def test_python_takes_the_ordered_ce_entry_point():
    """ce_nchw_fwd_kernel keeps its atomic variant only for the workspace-less C entry points: no Python code calls them."""
    for p in sorted((ROOT / "lc2is_amd").rglob("*.py")):
        src = p.read_text()
        for legacy in ("lc2is_ce_nchw_fwd", "lc2is_ce_nchw_fwd_opts"):
            assert not re.search(rf"_fn\(\s*[\"']{legacy}[\"']\s*\)", src), f"{p.name} calls {legacy}"
    assert '_fn("lc2is_ce_nchw_fwd_ordered")' in (ROOT / "lc2is_amd" / "ops.py").read_text()


STEP_KERNELS = [("head.hip", "head_finish_kernel"), ("misc.hip", "text_embed_dtok_kernel"),
                ("head.hip", "head_ce_grp_kernel")]


def _insert_in_body(src: str, fn: str, stmt: str) -> str:
    spans = [(a, b) for n, a, b in functions(src) if n == fn]
    assert spans, fn
    a = spans[0][0]
    return src[:a + 1] + "\n  " + stmt + "\n" + src[a + 1:]


@pytest.mark.parametrize("fname,fn", STEP_KERNELS)
@pytest.mark.parametrize("op", ["atomicAdd", "unsafeAtomicAdd", "__hip_atomic_fetch_add"])
def test_scan_notices_an_inserted_atomic(fname, fn, op):
    """An atomic add inserted into a copy of a step kernel's text is found and attributed to that kernel."""
    src = sources()[fname]
    assert not [s for s in rmw_sites(src, fname) if s[2] == fn]
    args = "(float*)0, 1.f" if op != "__hip_atomic_fetch_add" else "(float*)0, 1.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT"
    mutated = _insert_in_body(src, fn, f"{op}({args});")
    new = [s for s in rmw_sites(mutated, fname) if s[2] == fn]
    assert [s[3] for s in new] == [op]
    assert fn not in ALLOWED


@pytest.mark.parametrize("stmt", ["__hip_atomic_load((float*)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);",
                                  "// atomicAdd(p, v) in a comment", "const char* s = \"atomicAdd(\";"])
def test_scan_ignores_loads_comments_and_strings(stmt):
    src = sources()["head.hip"]
    mutated = _insert_in_body(src, "head_finish_kernel", stmt)
    assert not [s for s in rmw_sites(mutated, "head.hip") if s[2] == "head_finish_kernel"]
