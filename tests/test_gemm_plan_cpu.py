"""The launch plans of the fused MPQ GEMM (plan_gemm, csrc/mpq_gemm.hip), seen host-only through bie_test_mpq_gemm_plan: every plan the
dispatcher selects on the measured grid -- from the table csrc/mpq_gemm_plan_table.inc and from the cost model alone -- is a valid launch
shape whose workspace the sizing functions cover, the table is honoured exactly where plan_gemm says, and no selectable (BM, S) is missing
from gemm_plan_ref.PLANS, the list tests/test_gemm_plan_gpu.py forces against the oracle.  No kernel is launched here.
(BIE_TUNING, set by tests/conftest.py, makes the library re-read its knobs per call.)"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gemm_plan_ref as ref  # noqa: E402
from gemm_plan_ref import cdiv  # noqa: E402

# table cells of gemm_plan_ref.table_cells (or their neighbouring row counts) that reach the fused kernel in none of bf16 W4, fp16 W4, bf16 W8:
# tests/test_gemm_plan_gpu.py could not run them.  Checked against the host-only functions below.
CELLS_NOT_FUSED = []


@pytest.fixture(scope="module")
def L():
    from bitorch_engine import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def tab():
    return ref.parse_table()


def check_answer(L, M, K, N):
    """What must hold of every answer.  Returns (flag, (BM, S, tiles_per_split))."""
    flag, BM, S, tps = ref.query(L, M, K, N)
    what = (M, K, N, flag, BM, S, tps)
    T = K // ref.BK
    assert flag in (0, 1), what
    assert BM in ref.BMS, what
    assert M <= 16 or not (BM > 32 and BM >= 2 * M), what
    assert 1 <= S <= 16, what
    assert tps * S >= T and tps * (S - 1) < T, what  # every K tile covered, no split empty
    assert S == 1 or T // S >= 2, what
    if M >= 3:  # W8 is never decoded and takes the MFMA GEMM from 3 rows; below 897 rows (every row count here) its fused form
        form, need = ref.forward_plan(L, M, K, N, 8, 128, 1)
        assert form == ref.GEMM_FUSED, what
        want = ref.WS_HEAD + (S * M * N * 4 if S > 1 else 0)
        assert need == want, what + (need, want)
        for w in (1, 2, 4, 8):
            assert L.bie_mpq_workspace_bytes(M, K, N, w) >= want, what + (w,)
    return flag, (BM, S, tps)


def rows_around(Mg, BM):
    """Mg, the two row counts at the ends of its row-tile count, and the first one on each side that changes the count."""
    c = cdiv(Mg, BM)
    return [m for m in (Mg, (c - 1) * BM + 1, c * BM, (c - 1) * BM, c * BM + 1) if m >= 1]


def walk(L, tab):
    """Every grid point with the row counts around it, and the off-grid shapes: {(M, K, N): (flag, plan)}."""
    Kg, Ng, Mg, _ = tab
    out = {}
    for K in Kg:
        for N in Ng:
            for M in Mg:
                _, plan = check_answer(L, M, K, N)
                cell = ref.table_plan(tab, M, K, N)
                for m in sorted(set(rows_around(M, plan[0]) + (rows_around(M, cell[0]) if cell else []))):
                    out[(m, K, N)] = check_answer(L, m, K, N)
    for (K, N) in ((2048, 2048), (4096, 4096), (4096, 11008), (11008, 4096), (14336, 28672)):
        for (k, n) in ((K, N - 64), (K, N + 64), (K - 64, N), (K + 64, N), (64, N), (128, N), (1088, N)):
            for M in (17, 33, 64, 100, 300, 768, 896):
                out[(M, k, n)] = check_answer(L, M, k, n)
    return out


def test_every_selected_plan_is_a_valid_launch_and_is_in_PLANS(L, tab, monkeypatch):
    """The whole 6 x 7 x 11 grid with the row counts around each point and off-grid shapes, with the table and with the model alone: every
    answer is a launch shape the kernel can run (check_answer), the workspace functions cover it, and the (BM, S) pairs are all in PLANS."""
    Kg, Ng, Mg, _ = tab
    assert (len(Kg), len(Ng), len(Mg)) == (6, 7, 11)
    assert len(set(ref.PLANS)) == len(ref.PLANS) and all(bm in ref.BMS and 1 <= s <= 16 for (bm, s) in ref.PLANS)
    with_table = walk(L, tab)
    monkeypatch.setenv("BIE_GEMM_PLAN_TABLE", "0")
    model = walk(L, tab)
    assert not any(flag for (flag, _) in model.values()), "BIE_GEMM_PLAN_TABLE=0 must leave the model alone"
    for (key, (flag, plan)) in with_table.items():
        if not flag:
            assert model[key][1] == plan, (key, plan, model[key], "off the table's cells the model's own plan stays")
    table_pairs = {plan[:2] for (flag, plan) in with_table.values() if flag}
    model_pairs = {plan[:2] for (_, plan) in model.values()}
    classes = {plan + (K // ref.BK - (plan[1] - 1) * plan[2],) for ((_, K, _), (_, plan)) in list(with_table.items()) + list(model.items())}
    print(f"\n[gemm plan] {len(with_table)} shapes walked; (BM, S) pairs: {len(table_pairs)} from the table, {len(model_pairs)} from the model, "
          f"{len(table_pairs | model_pairs)} in all; {len(classes)} (BM, S, tiles per split, tiles in the last split) classes, "
          f"{sum(1 for c in classes if c[1] > 8)} with S > 8, {sum(1 for c in classes if c[3] < c[2])} with a short last split")
    print(f"[gemm plan] table pairs {sorted(table_pairs)}")
    print(f"[gemm plan] model pairs {sorted(model_pairs)}")
    missing = (table_pairs | model_pairs) - set(ref.PLANS)
    assert not missing, f"selected (BM, S) pairs no GPU test forces -- add them to gemm_plan_ref.PLANS: {sorted(missing)}"


def test_the_query_reads_the_knobs_and_refuses_a_ragged_k(L, monkeypatch):
    assert L.bie_test_mpq_gemm_plan(64, 2048 + 32, 2048, None, None, None) < 0
    assert L.bie_test_mpq_gemm_plan(64, 2048, 2048, None, None, None) == 1  # NULL outputs are allowed
    monkeypatch.setenv("BIE_GEMM_BM", "128")
    monkeypatch.setenv("BIE_GEMM_S", "10")
    assert ref.query(L, 300, 2048, 264) == (0, 128, 8, 4), "a forced S = 10 on 32 K tiles runs as 8 splits of 4"
    assert ref.query(L, 64, 2048, 2048)[0] == 0, "a forced plan is never the table's"
    monkeypatch.setenv("BIE_GEMM_S", "16")
    assert ref.query(L, 300, 2048, 264) == (0, 128, 16, 2)
    form, need = ref.forward_plan(L, 300, 2048, 264, 4, 128, 0)
    assert form == ref.GEMM_FUSED and need == ref.WS_HEAD + 16 * 300 * 264 * 4
    assert L.bie_mpq_workspace_bytes(300, 2048, 264, 4) >= need


def test_table_entries_are_honoured_exactly_where_plan_gemm_says(L, tab):
    """Every non-zero entry that meets plan_gemm's conditions comes back at its own (K, N, M) with flag 1, stays for every row count with the
    same number of row tiles (whose nearest grid row is the cell's: the lookup is by nearest grid row), and is dropped one row beyond that
    range, at N + 64 and at K + 64.  Entries that do not meet the conditions are never returned."""
    Kg, Ng, Mg, table = tab
    cells = ref.honoured_cells(tab)
    nonzero = sum(1 for plane in table for row in plane for e in row if e)
    print(f"\n[gemm plan] {len(cells)} of {nonzero} non-zero table entries are honoured ({len(Kg) * len(Ng) * len(Mg)} cells); "
          f"{len({c[3][:2] for c in cells})} distinct (BM, S)")
    assert cells, "no table entry is honoured: the table parsed wrong"
    for ki, K in enumerate(Kg):
        for ni, N in enumerate(Ng):
            for mi, M in enumerate(Mg):
                e = table[ki][ni][mi]
                if not ref.honoured(e, K, M):
                    assert ref.query(L, M, K, N)[0] == 0, (K, N, M, hex(e))
    for (K, N, M, plan) in cells:
        BM, c = plan[0], cdiv(M, plan[0])
        assert ref.query(L, M, K, N) == (1,) + plan, (K, N, M, plan)
        kept = 0
        for m in range(max(1, (c - 1) * BM + 1 - 2), c * BM + 3):
            want, got = ref.table_plan(tab, m, K, N), ref.query(L, m, K, N)
            same_cell = ref.grid_index(Mg, m) == Mg.index(M)
            if same_cell and cdiv(m, BM) == c:
                assert want == plan, (K, N, M, m)
                kept += 1
            if same_cell and cdiv(m, BM) != c:
                assert want is None and got[0] == 0, (K, N, M, m, got, "one row beyond the tile count the cell's plan is dropped")
            assert got[0] == (want is not None) and (want is None or got[1:] == want), (K, N, M, m, got, want)
        assert kept >= 1
        assert ref.query(L, M, K, N + 64)[0] == 0 and ref.query(L, M, K + 64, N)[0] == 0, (K, N, M)
        assert ref.query(L, M, K, N - 64)[0] == 0 and ref.query(L, M, K - 64, N)[0] == 0, (K, N, M)


def test_the_table_cells_the_gpu_tests_run_reach_the_fused_kernel(L, tab):
    """gemm_plan_ref.table_cells: one honoured cell per (BM, S) the table yields plus the K = 2048 cells, each with a neighbouring row count.
    Which of them cannot reach the fused kernel (the decode kernels take 17 .. 32 rows on their measured shapes) is CELLS_NOT_FUSED."""
    from bitorch_engine import _hip
    cells = ref.table_cells(tab)
    assert {c[3][:2] for c in cells} == {c[3][:2] for c in ref.honoured_cells(tab)}, "a pair the table yields has no cell"
    assert {c[3][:2] for c in cells} <= set(ref.PLANS)
    assert all(k in {c[:3] for c in cells} for k in ref.ALWAYS_CELLS)
    not_fused = []
    print()
    for (K, N, M, plan, M2) in cells:
        for m in (M, M2):
            assert ref.query(L, m, K, N) == (1,) + plan, (K, N, m, plan)
        v = ref.cell_variant(L, (M, M2), K, N, _hip.F16, _hip.BF16)
        if v is None:
            not_fused.append((K, N, M))
        print(f"[gemm plan] cell K={K} N={N} M={M} (and M={M2}): BM={plan[0]} S={plan[1]} tiles/split={plan[2]}, runs as {v}")
    assert not_fused == CELLS_NOT_FUSED


@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_the_oracle_is_exact_on_the_exact_data_of_the_plan_invariance_test(dtype, asym):
    """gemm_plan_ref.exact_case: every product and partial sum is a small multiple of 2^-6, so the float64 product rounded once to the dtype is
    THE answer, whatever the summation order.  The oracle returns exactly it (both its forms); tests/test_gemm_plan_gpu.py relies on that."""
    import numpy as np
    import torch
    from oracle import oracle as orc
    tdt, dt = (torch.float16, orc.F16) if dtype == "f16" else (torch.bfloat16, orc.BF16)
    x, qw, s, z, y64 = ref.exact_case(tdt, asym, 11 + asym)
    M, K, N, gs = ref.EXACT_SHAPE
    assert np.array_equal(y64 * 64, np.round(y64 * 64)) and np.abs(y64).max() < 2.0 ** 12 and np.abs(y64).max() > 8.0
    want = torch.from_numpy(y64).to(tdt)
    W = orc.mpq_dequant(qw.numpy(), orc.torch_to_np(s), orc.torch_to_np(z), None, 4, gs, asym, dt)
    assert torch.equal(orc.np_to_torch(orc.gemm(orc.torch_to_np(x), W, dt), tdt), want)
    y = orc.mpq_forward(orc.torch_to_np(x), qw.numpy(), orc.torch_to_np(s), orc.torch_to_np(z), None, 4, gs, asym, dt)
    assert torch.equal(orc.np_to_torch(y, tdt), want)
