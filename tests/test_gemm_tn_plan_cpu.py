"""The weight-gradient (TN GEMM) dispatch seen from the host (no GPU): the plans lc2is_gemm_tn_bf16 and lc2is_gemm_tn_grouped run.

The M-split count of a plan fixes the ORDER of the fp32 partial sums, so a planner regression changes result bits and not only
speed.  ``ops.gemm_tn_plan`` / ``ops.gemm_tn_grouped_plan`` return the plan without launching; the tables below pin it for the
shapes the step and the GPU tests run.  The expected records and refusal codes were RECORDED from the launchers as they stood
before the planners were split out of them (their launches and uploaded descriptor tables intercepted, the same arguments;
profiles/gemm_tn_plan_sweep.txt), not derived by hand."""
import ctypes
import random

import pytest

from lc2is_amd import ops


@pytest.fixture(scope="module", autouse=True)
def _library():
    from lc2is_amd import _lib
    if not _lib.lib_path().exists():
        import __graft_entry__ as ge
        ge.build()
    yield
    ops.set_cu_budget(0)


def _with_budget(budget, f, *a, **kw):
    ops.set_cu_budget(budget)
    try:
        return f(*a, **kw)
    finally:
        ops.set_cu_budget(0)


# (M, N, K, {CU budget: (big, ntn, ntk, splits, chunk, grid, red_grid, workspace_bytes)}); budget 0 = all 256 CUs
SINGLE = [
    # the weight gradients of a ViT-B/16 layer (q / k / v / out-proj, fused qkv, fc1, fc2) at 32 and 16 images of 1025 tokens
    (32800, 768, 768, {0: (1, 3, 3, 27, 1216, 243, 576, 63783936), 240: (1, 3, 3, 27, 1216, 243, 576, 63783936),
                       200: (1, 3, 3, 22, 1536, 198, 576, 51972096)}),
    (32800, 2304, 768, {0: (1, 9, 3, 9, 3648, 243, 1728, 63783936), 240: (1, 9, 3, 9, 3648, 243, 1728, 63783936),
                        200: (1, 9, 3, 7, 4736, 189, 1728, 49609728)}),
    (32800, 3072, 768, {0: (1, 12, 3, 7, 4736, 252, 2048, 66146304), 240: (1, 12, 3, 7, 4736, 252, 2048, 66146304),
                        200: (1, 12, 3, 6, 5504, 216, 2048, 56696832)}),
    (32800, 768, 3072, {0: (1, 3, 12, 7, 4736, 252, 2048, 66081792), 240: (1, 3, 12, 7, 4736, 252, 2048, 66081792),
                        200: (1, 3, 12, 6, 5504, 216, 2048, 56641536)}),
    (16416, 768, 768, {0: (1, 3, 3, 26, 640, 234, 576, 61421568), 240: (1, 3, 3, 26, 640, 234, 576, 61421568),
                       200: (1, 3, 3, 22, 768, 198, 576, 51972096)}),
    (16416, 2304, 768, {0: (1, 9, 3, 9, 1856, 243, 1728, 63783936), 240: (1, 9, 3, 9, 1856, 243, 1728, 63783936),
                        200: (1, 9, 3, 7, 2368, 189, 1728, 49609728)}),
    (16416, 3072, 768, {0: (1, 12, 3, 7, 2368, 252, 2048, 66146304), 240: (1, 12, 3, 7, 2368, 252, 2048, 66146304),
                        200: (1, 12, 3, 6, 2752, 216, 2048, 56696832)}),
    (16416, 768, 3072, {0: (1, 3, 12, 7, 2368, 252, 2048, 66081792), 240: (1, 3, 12, 7, 2368, 252, 2048, 66081792),
                        200: (1, 3, 12, 6, 2752, 216, 2048, 56641536)}),
    # every row of test_gemm_tn (the 128x128 form does not depend on the budget)
    (300, 128, 128, {b: (0, 1, 1, 1, 320, 1, 0, 0) for b in (0, 240, 200)}),
    (1025, 768, 768, {b: (0, 6, 6, 3, 384, 108, 576, 7087104) for b in (0, 240, 200)}),
    (4100, 2304, 768, {0: (1, 9, 3, 9, 512, 243, 1728, 63783936), 240: (1, 9, 3, 9, 512, 243, 1728, 63783936),
                       200: (1, 9, 3, 7, 640, 189, 1728, 49609728)}),
    (2050, 152, 512, {b: (0, 2, 4, 5, 448, 40, 76, 1559520) for b in (0, 240, 200)}),
    (64, 64, 64, {b: (0, 1, 1, 1, 64, 1, 0, 0) for b in (0, 240, 200)}),
    (5000, 3072, 768, {0: (1, 12, 3, 7, 768, 252, 2048, 66146304), 240: (1, 12, 3, 7, 768, 252, 2048, 66146304),
                       200: (1, 12, 3, 6, 896, 216, 2048, 56696832)}),
    (33, 8, 8, {b: (0, 1, 1, 1, 64, 1, 0, 0) for b in (0, 240, 200)}),
    (300, 3072, 3072, {b: (1, 12, 12, 1, 320, 144, 0, 0) for b in (0, 240, 200)}),    # 256x256 tiles, one split: direct epilogue
    # test_cu_budget_changes_plans_not_results: the 512-row floor binds under every budget
    (32800, 768, 256, {b: (1, 3, 1, 65, 512, 195, 192, 51317760) for b in (0, 240, 200)}),
]

_LAYER = [(768, 768)] * 4 + [(3072, 768), (768, 3072)]            # q, k, v, o, fc1, fc2 as (N, K)
_TOWER_TEST = [(256, 256)] * 5 + [(256, 512)] * 4 + [(512, 256)] * 4 + [(768, 256)] * 4 + [(512, 512)] * 3 + [(512, 768)] * 3 + \
              [(768, 512)] * 36
GROUPS = {
    "layer": (_LAYER, 32800),                                          # test_cpu_host.py
    "tower": (_LAYER * 12, 32800),
    "swin": ([(384, 384)] * 4 + [(1536, 384), (384, 1536)], 32800),
    "grouped": ([(256, 768), (768, 256), (256, 256), (512, 256)], 4100),      # test_gemm_tn_grouped
    "small_tiles": ([(96, 96), (288, 96), (384, 96), (96, 384), (200, 136), (768, 192)], 9000),   # ..._small_tiles
    "tower_test": (_TOWER_TEST, 4160),                                 # ..._whole_tower_table_and_tail_split
    "small_table": ([[(96, 96), (200, 136), (288, 96)][i % 3] for i in range(17)], 1100),    # ..._small_tiles_table
}
# (group, CU budget, (small, table, grid, red_grid, workspace_bytes, table_bytes), splits, chunk, indices of the split problems in grid
# order); the other problems run unsplit, in the caller's order, in front of the split ones
GROUPED = [
    ("layer", 0, (0, 0, 216, 4379, 56678400, 0), 2, 16448, list(range(6))),
    ("layer", 240, (0, 0, 216, 4379, 56678400, 0), 2, 16448, list(range(6))),
    ("layer", 200, (0, 0, 540, 4379, 141696000, 0), 5, 6592, list(range(6))),
    ("tower", 0, (0, 1, 1530, 1158, 66163968, 17664), 14, 2368, [68, 69]),
    ("tower", 240, (0, 1, 1395, 6369, 51989760, 17664), 2, 16448, [55, 56, 57, 60, 61, 62, 63, 66, 67, 68, 69]),
    ("tower", 200, (0, 1, 1395, 6369, 51989760, 17664), 2, 16448, [55, 56, 57, 60, 61, 62, 63, 66, 67, 68, 69]),
    ("swin", 0, (1, 0, 972, 1744, 63825408, 0), 9, 3648, list(range(6))),
    ("swin", 240, (1, 0, 972, 1744, 63825408, 0), 9, 3648, list(range(6))),
    ("swin", 200, (1, 0, 972, 1744, 63825408, 0), 9, 3648, list(range(6))),
    ("grouped", 0, (0, 0, 81, 583, 21298176, 0), 9, 512, list(range(4))),
    ("grouped", 240, (0, 0, 81, 583, 21298176, 0), 9, 512, list(range(4))),
    ("grouped", 200, (0, 0, 81, 583, 21298176, 0), 9, 512, list(range(4))),
    ("small_tiles", 0, (1, 0, 468, 289, 20669760, 0), 18, 512, list(range(6))),
    ("small_tiles", 240, (1, 0, 468, 289, 20669760, 0), 18, 512, list(range(6))),
    ("small_tiles", 200, (1, 0, 468, 289, 20669760, 0), 18, 512, list(range(6))),
    ("tower_test", 0, (0, 1, 471, 1556, 56825088, 17664), 9, 512, list(range(13)) + [16]),
    ("tower_test", 240, (0, 1, 443, 2657, 53926144, 17664), 5, 832, list(range(17)) + [18, 19]),
    ("tower_test", 200, (0, 1, 360, 5237, 42593536, 17664), 2, 2112, list(range(20)) + list(range(53, 59))),
    ("small_table", 0, (1, 1, 135, 373, 4337088, 17664), 3, 384, list(range(17))),
    ("small_table", 240, (1, 1, 135, 373, 4337088, 17664), 3, 384, list(range(17))),
    ("small_table", 200, (1, 1, 135, 373, 4337088, 17664), 3, 384, list(range(17))),
]


def test_single_plans_are_the_recorded_ones():
    wrong = []
    for M, N, K, by_budget in SINGLE:
        for budget, want in by_budget.items():
            got = tuple(_with_budget(budget, ops.gemm_tn_plan, M, N, K).values())
            if got != want:
                wrong.append((M, N, K, budget, want, got))
    assert not wrong, wrong
    forms = {(p[0], p[3] > 1) for _, _, _, by_budget in SINGLE for p in by_budget.values()}
    assert forms == {(0, False), (0, True), (1, False), (1, True)}       # both kernels, with and without slabs


def test_grouped_plans_are_the_recorded_ones():
    wrong = []
    for name, budget, summary, splits, chunk, split_idx in GROUPED:
        shapes, M = GROUPS[name]
        s, recs = _with_budget(budget, ops.gemm_tn_grouped_plan, shapes, M=M)
        whole = [i for i in range(len(shapes)) if i not in split_idx]
        want = [(i, 1, (M + 63) // 64 * 64) for i in whole] + [(i, splits, chunk) for i in split_idx]
        got = [(r["index"], r["splits"], r["chunk"]) for r in recs]
        if tuple(s.values()) != summary or got != want:
            wrong.append((name, budget, tuple(s.values()), got))
    assert not wrong, wrong


def _check_group(shapes, Ms, db, s, recs):
    n = len(shapes)
    assert s["table"] == (n > 16) and s["table_bytes"] == (17664 if n > 16 else 0)
    assert s["small"] == any(N % 256 or K % 256 for N, K in shapes)
    assert sorted(r["index"] for r in recs) == list(range(n))
    tile = 128 if s["small"] else 256
    blk = red = 0
    regions = []
    for r in recs:
        N, K = shapes[r["index"]]
        M = Ms[r["index"]]
        assert r["chunk"] % 64 == 0 and r["splits"] == -(-M // r["chunk"]) and (r["splits"] - 1) * r["chunk"] < M
        assert (r["ntn"], r["ntk"]) == (-(-N // tile), -(-K // tile))
        blk += r["ntn"] * r["ntk"] * r["splits"]
        assert r["blk_end"] == blk                       # strictly increasing: every problem has at least one block
        has_db = db[r["index"]]
        if r["splits"] > 1:
            assert r["red_blocks"] == min(-(-(N * K // 4) // 256), 1024)
            red += r["red_blocks"] + (-(-N // 256) if has_db else 0)
            regions.append((r["slab_offset"], r["splits"] * N * K * 4))
            assert (r["bias_offset"] >= 0) == has_db
            if has_db:
                regions.append((r["bias_offset"], r["splits"] * N * 4))
        else:
            assert (r["red_blocks"], r["slab_offset"], r["bias_offset"]) == (0, -1, -1)
        assert r["red_end"] == red
    assert (s["grid"], s["red_grid"]) == (blk, red)
    at = s["table_bytes"]
    for off, size in sorted(regions):
        assert off % 16 == 0 and off >= at, (off, at)   # disjoint, behind the table
        at = off + size
    assert at <= s["workspace_bytes"]


def test_plan_invariants_over_a_sweep():
    """Random shapes and groups under three budgets: chunks are whole 64-row steps that cover M with no empty split, block and
    reduce ranges are contiguous and end at the grid sizes, the grid order is a permutation, slabs and bias partials are disjoint
    16-byte aligned regions inside the reported workspace (behind the table), the table is used exactly when n > 16, and the
    reported bytes are what the workspace queries return."""
    rng = random.Random(5)
    ws_single, ws_group = ops._fn("lc2is_gemm_tn_workspace_bytes"), ops._fn("lc2is_gemm_tn_grouped_workspace_bytes")
    for budget in (0, 240, 200):
        ops.set_cu_budget(budget)
        for _ in range(1500):
            M = rng.choice((rng.randint(1, 3000), rng.randint(1, 70000), 1025 * rng.randint(1, 64), rng.randint(1, 250000)))
            N, K = (256 * rng.randint(1, 16), 256 * rng.randint(1, 16)) if rng.random() < 0.5 else (8 * rng.randint(1, 512), 8 * rng.randint(1, 512))
            p = ops.gemm_tn_plan(M, N, K)
            tile = 256 if p["big"] else 128
            assert p["chunk"] % 64 == 0 and p["splits"] == -(-M // p["chunk"]) and (p["splits"] - 1) * p["chunk"] < M, (M, N, K, p)
            assert (p["ntn"], p["ntk"]) == (-(-N // tile), -(-K // tile)) and p["grid"] == p["ntn"] * p["ntk"] * p["splits"]
            assert not p["big"] or (N % 256 == 0 and K % 256 == 0)
            assert p["red_grid"] == (min(-(-(N * K // 4) // 256), 2048) if p["splits"] > 1 else 0)
            assert p["workspace_bytes"] == (p["splits"] * N * (K + 1) * 4 if p["splits"] > 1 else 0) == ws_single(M, N, K)
        for _ in range(150):
            n = rng.choice((rng.randint(1, 16), 16, 17, rng.randint(17, 128), 128))
            kind = rng.randrange(3)                      # all on the 256 grid / mixed / none
            on = [kind == 0 or (kind == 1 and rng.random() < 0.8) for _ in range(n)]
            shapes = [(256 * rng.randint(1, 6), 256 * rng.randint(1, 6)) if o else (8 * rng.randint(1, 150), 8 * rng.randint(1, 150))
                      for o in on]
            M = rng.choice((rng.randint(1, 70000), 1025 * rng.randint(1, 64)))
            Ms = [M] * n if rng.random() < 0.7 else [rng.randint(1, 70000) for _ in range(n)]
            lds = [(N + 8 * rng.randrange(3), K + 8 * rng.randrange(3), K + 4 * rng.randrange(3)) for N, K in shapes]
            db = [rng.random() < 0.7 for _ in range(n)]
            arr = (ops.TnProblem * n)()
            for i, (N, K) in enumerate(shapes):
                arr[i] = ops.TnProblem(0x1000, 0x1000, 0x1000, 0x1000 if db[i] else None, *lds[i], Ms[i], N, K, 0)
            summary, recs = ops._TnGroupPlan(), (ops._TnGroupRec * n)()
            assert ops._fn("lc2is_gemm_tn_grouped_plan")(arr, n, ctypes.addressof(summary), recs, n) == 0
            as_dict = lambda x: {f: getattr(x, f) for f, _ in x._fields_}      # noqa: E731
            _check_group(shapes, Ms, db, as_dict(summary), [as_dict(r) for r in recs])
            assert ws_group(arr, n) == summary.workspace_bytes
    ops.set_cu_budget(0)


# ---- refusals: each launcher's checks in its order; a case breaks the named check AND a later one, the earlier code wins ----
_A = 1 << 40    # never dereferenced
TN_OK = dict(dY=_A, ldy=768, X=_A, ldx=768, dW=_A, ldw=768, db=None, M=32800, N=768, K=768, accumulate=0, workspace=_A,
             workspace_bytes=1 << 40)
TN_REFUSALS = [
    (dict(dY=None, M=0), -2), (dict(X=None, N=772), -2), (dict(dW=None, ldw=8), -2),      # NULL operands, before the shape
    (dict(M=0, ldy=8), -1), (dict(N=772, ldy=776), -1), (dict(K=772, ldx=776, ldw=772), -1),   # empty, N % 8, K % 8: LC2IS_ERR_SHAPE here
    (dict(ldy=760, M=4000000), -1), (dict(ldx=760, M=4000000), -1), (dict(ldw=760, M=4000000), -1),   # short rows, before the 2 GiB limit
    (dict(ldy=772, M=4000000), -1), (dict(ldw=770, M=4000000), -1),                      # rows off 16 bytes
    (dict(M=4000000, workspace=None), -3), (dict(M=1400000, ldx=776, workspace=None), -3),    # a panel past 2 GiB, before the workspace
    (dict(workspace=None), -4), (dict(workspace_bytes=63783936 - 1), -4),                 # this plan has slabs (asserted below)
]
_P0 = dict(dY=_A, X=_A, dW=_A, db=_A, ldy=768, ldx=768, ldw=768, M=32800, N=768, K=768, accumulate=0)
# (changes to problem 0, changes to problem 1, n or None, workspace, code)
TG_REFUSALS = [
    (None, None, 0, _A, -3), (None, None, 129, _A, -3), (None, None, -1, _A, -3),        # the count, before any operand
    (dict(dY=None), None, 129, _A, -3),
    (dict(dY=None, N=772), None, None, _A, -2), (dict(dW=None, ldw=8), None, None, _A, -2),    # NULL, before the shape
    (dict(N=772, ldy=8), None, None, _A, -3), (dict(K=772, ldx=8), None, None, _A, -3),        # N % 8, K % 8: LC2IS_ERR_UNSUPPORTED here
    (dict(M=0, ldy=8), None, None, _A, -3),
    (dict(ldy=760, M=4000000), None, None, _A, -1), (dict(ldw=770, M=4000000), None, None, _A, -1),   # rows, before the 2 GiB limit
    (dict(M=4000000), None, None, None, -3),                                             # 2 GiB, before the workspace
    (dict(ldx=760), dict(X=None), None, _A, -1), (dict(), dict(X=None, ldx=8), None, None, -2),   # problem 0 before problem 1
    (dict(), dict(), None, None, -4),                                                    # two problems, both split (asserted below)
]


def _tn_problems(p0, p1, n):
    arr = (ops.TnProblem * 2)()
    for i, change in enumerate((p0, p1)):
        q = {**_P0, **(change or {})}
        arr[i] = ops.TnProblem(*[q[f] for f, _ in ops.TnProblem._fields_])
    return (None if p0 is None else arr), (2 if n is None else n)


def test_launchers_refuse_in_order_before_any_gpu_call():
    f = ops._fn("lc2is_gemm_tn_bf16")
    got = [(change, f(*{**TN_OK, **change}.values(), None)) for change, _ in TN_REFUSALS]
    assert got == [(change, rc) for change, rc in TN_REFUSALS]
    assert {rc for _, rc in TN_REFUSALS} == {-1, -2, -3, -4}
    g = ops._fn("lc2is_gemm_tn_grouped")
    got = [g(*_tn_problems(p0, p1, n), ws, 0 if ws is None else 1 << 40, None) for p0, p1, n, ws, _ in TG_REFUSALS]
    assert got == [rc for *_, rc in TG_REFUSALS]
    assert {rc for *_, rc in TG_REFUSALS} == {-1, -2, -3, -4}


def test_plan_queries_refuse_what_the_launchers_refuse():
    """The queries return the launchers' codes (all but the workspace one, which they report as bytes instead), and the plans the
    workspace refusals above rely on do have slabs."""
    p = ops.gemm_tn_plan(TN_OK["M"], TN_OK["N"], TN_OK["K"])
    assert p["splits"] > 1 and p["workspace_bytes"] == 63783936
    s, recs = ops.gemm_tn_grouped_plan([(768, 768)] * 2, M=32800)
    assert all(r["splits"] > 1 for r in recs) and s["workspace_bytes"] > 0
    q = ops._fn("lc2is_gemm_tn_plan")
    rec = ops._TnPlan()
    assert [q(M, N, K, ctypes.addressof(rec)) for M, N, K in [(0, 8, 8), (8, 12, 8), (8, 8, 4), (4000000, 768, 768), (8, 8, 8)]] == \
        [-1, -1, -1, -3, 0]
    assert q(8, 8, 8, None) == -2
    gq = ops._fn("lc2is_gemm_tn_grouped_plan")
    summary, out = ops._TnGroupPlan(), (ops._TnGroupRec * 2)()
    for p0, p1, n, ws, rc in TG_REFUSALS:
        assert gq(*_tn_problems(p0, p1, n), ctypes.addressof(summary), out, 2) == (0 if rc == -4 else rc)
    assert gq(*_tn_problems({}, {}, None), None, out, 2) == -2
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.gemm_tn_grouped_plan([(772, 768)], M=4100)
    with pytest.raises(RuntimeError, match="rc=-1"):
        ops.gemm_tn_plan(4100, 772, 768)
