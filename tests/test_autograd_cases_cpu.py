"""Keeps the autograd-contract table (tests/autograd_cases.py) complete, and shows on the CPU — with the oracle alone — that its
reference side can fail: the fp64 oracle under torch autograd returns None gradients exactly for the frozen names, and the sum of
the two inputs' gradients under accumulation.  Runs without a GPU (the modules are only constructed, never called)."""
import ast
import inspect
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import autograd_cases as AC  # noqa: E402

ROOT = HERE.parent
NN = ROOT / "lc2is_amd" / "nn"
CHEAP = [i for i in AC.CASE_IDS if i.startswith(("vision", "text", "decoder", "block"))]     # an fp64 pass of a few milliseconds
_ORACLES = {}


def function_names() -> set:
    """Names of the torch.autograd.Function subclasses defined in lc2is_amd/nn/*.py."""
    out = set()
    for f in sorted(NN.glob("*.py")):
        for node in ast.walk(ast.parse(f.read_text())):
            if isinstance(node, ast.ClassDef) and any(ast.unparse(b).endswith("autograd.Function") for b in node.bases):
                out.add(node.name)
    return out


def exported_classes() -> dict:
    """{name: class} of what lc2is_amd.nn exports (``ftn.X`` for the public classes of the ftn submodule)."""
    import lc2is_amd.nn as N
    out = {n: getattr(N, n) for n in N.__all__ if inspect.isclass(getattr(N, n))}
    out.update({f"ftn.{n}": c for n, c in vars(N.ftn).items()
                if inspect.isclass(c) and not n.startswith("_") and c.__module__ == N.ftn.__name__})
    return out


_OWNERS = {}


def owners(classes: dict, fns: set) -> list:
    """The classes whose own code, or that of a base class inside the package, calls ``<Function>.apply(``."""
    key = (tuple(classes), tuple(sorted(fns)))
    if key in _OWNERS:
        return list(_OWNERS[key])
    out = []
    for name, cls in classes.items():
        src = "".join(inspect.getsource(k) for k in cls.__mro__ if k.__module__.startswith("lc2is_amd."))
        if any(f"{fn}.apply(" in src for fn in fns):
            out.append(name)
    _OWNERS[key] = tuple(out)
    return out


def uncovered(names, table: set, exempt: dict) -> list:
    return [n for n in names if n not in table and n not in exempt]


def table_classes() -> set:
    return {k for c in AC.cases() for k in c.classes}


def test_owner_list_is_found():
    fns = function_names()
    for fn in ("_VisionFn", "_TextFn", "_DecoderFn", "_PyramidFn", "_BlockFn", "_TransformerFn", "_SwinFn", "_HeadFn", "_LinearFn"):
        assert fn in fns, fn
    own = owners(exported_classes(), fns)
    for n in ("ImageEncoderCLIP", "ImageEncoderCLIPFull", "TextEncoderCLIPPooler", "DecoderBlock", "PromptDecoder", "HierarchicalCrossA",
              "CrossABlock", "FTNDecoder", "ftn.Transformer", "ftn.Decoder", "SwinTransformer", "BaseModelWithText", "TextToPatch"):
        assert n in own, n
    assert "DecoderLayer" not in own and "ClipArch" not in own and "ParamArena" not in own     # parameter holders, plain classes


def test_every_module_with_a_hand_written_backward_is_in_the_table():
    missing = uncovered(owners(exported_classes(), function_names()), table_classes(), AC.EXEMPT)
    assert not missing, f"classes of lc2is_amd.nn with a torch.autograd.Function backward and no autograd-contract case: {missing} " \
                        "(add a case to tests/autograd_cases.py, or an EXEMPT entry with the reason)"


def test_exemptions_are_current():
    own = set(owners(exported_classes(), function_names()))
    stale = [n for n in AC.EXEMPT if n not in own or n in table_classes()]
    assert not stale, f"EXEMPT lists names that own no Function backward any more, or that the table covers: {stale}"
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in AC.EXEMPT.values())


@pytest.mark.parametrize("name", ["ImageEncoderCLIPFull", "TextEncoderCLIPPooler", "DecoderBlock", "HierarchicalSelfA", "CrossABlock", "FTNBlock", "FTNDecoder",
                                  "ftn.Transformer", "SwinTransformer", "BaseModelWithText"])
def test_check_notices_a_removed_entry(name):
    """Taking a class out of the table (and it is not exempt) makes the completeness check fail."""
    own = owners(exported_classes(), function_names())
    assert not uncovered([name], table_classes(), AC.EXEMPT)
    assert uncovered(own, table_classes() - {name}, AC.EXEMPT) == [name]


def test_case_ids_match_the_table():
    assert [c.id for c in AC.cases()] == AC.CASE_IDS
    for c in AC.cases():
        assert c.bounds.src.startswith("tests/test_gpu_"), c.id      # every baseline bound quotes the line it is taken from


# ---- the reference side can fail ------------------------------------------------------------------------------------------
def oracle(cid) -> AC.Oracle:
    if cid not in _ORACLES:
        c = AC.case(cid)
        _ORACLES[cid] = AC.Oracle(c, c.build())
    return _ORACLES[cid]


def _grad_names(grads):
    return {n for n, g in grads.items() if g is not None}


def _patterns(cid, names):
    """(b), (c), (d): every parameter for the cases whose fp64 pass takes milliseconds; for the larger ones the two halves and
    leave-one / only-one at the first, a middle and the last parameter, and at every parameter of the reduction conv and its norm
    (the ones a spatial-reduction ratio of 1 leaves unreached)."""
    ks = range(len(names)) if cid in CHEAP else sorted({0, len(names) // 2, len(names) - 1}
                                                        | {k for k, n in enumerate(names) if n.startswith(("sr.", "norm."))})
    out = [AC.pattern_leave_one(names, k) for k in ks] + [AC.pattern_only_one(names, k) for k in ks]
    return out + [AC.pattern_half(names, 0), AC.pattern_half(names, 1)]


def _close(a, b, scale):
    """fp64 tensors equal up to the order of a few additions (a leaf used twice receives its contributions one by one)."""
    return float((a - b).abs().max()) <= 1e-12 * max(float(scale), 1e-300)


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_oracle_gradients_are_none_exactly_for_frozen_names(cid):
    """Patterns (b), (c), (d) with requires_grad set literally on the fp64 leaves, for every table entry: torch returns None for
    every frozen name and a gradient for every trainable name the graph reaches — which is also what Oracle.grad_set derives
    without another pass; and a gradient that exists equals the all-trainable one (freezing a leaf changes no other leaf's
    gradient)."""
    o = oracle(cid)
    names = list(o.params)
    _, g_all, _ = o.run()
    reach = _grad_names(g_all)
    assert reach == o.reachable() and reach
    if cid == "ftn_transformer_sr1":
        assert {n for n in names if n.startswith(("sr.", "norm."))} == set(names) - reach       # unused when sr_ratio == 1
    if cid == "ftn_transformer_sr2":
        assert reach == set(names)                                                               # sr.* and norm.* are reached
    for trainable in _patterns(cid, names):
        _, g, _ = o.run(trainable)
        got = _grad_names(g)
        assert got == reach & trainable == o.grad_set(trainable)
        assert not got & (set(names) - trainable)
        for n in got:
            assert _close(g[n], g_all[n], g_all[n].abs().max()), n


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_oracle_accumulates_the_sum(cid):
    """Two backward passes on the same fp64 leaves add, for every table entry: g_A + g_B; a grad set to None in between restarts
    at g_B."""
    o = oracle(cid)
    names = list(o.params)
    gA, gB = o.run(which="A")[1], o.run(which="B")[1]
    assert any(not torch.equal(gA[n], gB[n]) for n in names if gA[n] is not None)            # A and B are different inputs
    acc = o.run_accumulate()
    dropped = set(names[0::2])

    def drop(sd):
        for n in dropped:
            sd[n].grad = None

    acc_drop = o.run_accumulate(between=drop)
    differs = 0
    for n in names:
        if gA[n] is None:
            assert gB[n] is None and acc[n] is None and acc_drop[n] is None
            continue
        scale = gA[n].abs().max() + gB[n].abs().max()
        assert _close(acc[n], gA[n] + gB[n], scale), n
        assert _close(acc_drop[n], gB[n] if n in dropped else gA[n] + gB[n], scale), n
        differs += not _close(acc[n], gB[n], 1e6 * scale)       # the sum is not g_B: the first pass did count
    assert differs >= len(_grad_names(gA)) - 8, differs           # (all but the mathematically zero key-bias gradients)


@pytest.mark.parametrize("cid", [i for i in AC.CASE_IDS if i.startswith(("decoder", "hier", "block", "ftn"))])
def test_oracle_input_gradients_follow_the_flags(cid):
    """Pattern (f) on the oracle: an input gradient exists exactly where the flag is set, with the parameters trainable or frozen."""
    o = oracle(cid)
    for trainable in (None, set()):
        for flags in AC.input_flag_sets(o.inputs["A"].floats):
            _, pg, ig = o.run(trainable, flags)
            assert {k for k, g in ig.items() if g is not None} == {k for k, f in flags.items() if f}
            assert bool(_grad_names(pg)) == (trainable is None)
