"""The fused MPQ GEMM (csrc/mpq_gemm.hip + the split-K finalize pass of csrc/splitk.hip) under every launch plan the dispatcher selects
(run with -m gpu on an MI355X).  The kernel's K loop, the fp32 slab layout and the finalize pass depend on the shape only through
(BM, S, tiles_per_split); tests/test_gemm_plan_cpu.py proves that gemm_plan_ref.PLANS holds every (BM, S) plan_gemm selects on the measured
grid, and here
  a. every pair of PLANS is forced on a small ragged shape and checked against the oracle, the plan that ran asserted through
     bie_test_mpq_gemm_plan;
  b. all 4 x 16 forced plans give bit-identical results, equal to the float64 product, on data whose sums are exact in fp32;
  c. the measured table's own cells run unforced against the oracle.
Bars: those of tests/test_gpu_parity.py (assert_close, assert_close_elementwise_f16), whose helpers are used as they are."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gemm_plan_ref as ref  # noqa: E402
import test_gpu_parity as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = T.DEV
CODE = {orc.F16: 0, orc.BF16: 1}  # BIE_F16 / BIE_BF16 of include/bie_hip.h
KNOBS = ("BIE_GEMM_BM", "BIE_GEMM_S", "BIE_GEMM_PLAN_TABLE")


def lib():
    from bitorch_engine import _hip
    assert CODE == {orc.F16: _hip.F16, orc.BF16: _hip.BF16}
    return _hip.lib()


def force(monkeypatch, BM, S):
    monkeypatch.setenv("BIE_GEMM_BM", str(BM))
    monkeypatch.setenv("BIE_GEMM_S", str(S))


def forced_case(monkeypatch, BM, S, Tk, w_bit, dt, asym, with_bias, N=ref.FORCED_N):
    """One forced launch against the oracle: the plan asserted before the launch, the full output checked after it.

    The bars of assert_close / assert_close_elementwise_f16 are those of ONE rounding of a sum: 1e-3 for the fp32 summation order plus one
    ulp of the result.  With a bias the result is dt(dt(acc) + bias): two fp32 sums on either side of a rounding boundary of dt(acc)
    differ by one ulp of |acc| = |y - bias|, which a cancelling bias makes arbitrarily many ulps of y.  So a bias case is three checks:
      * the same launch without the bias against the oracle, at both bars;
      * the biased output is BIT for bit dt(y0 + bias) of that launch's y0 (an fp32 add, one rounding: what the finalize pass and the
        S = 1 epilogue compute, and the oracle from its own y0) -- stricter than any bar, and it leaves no way for the biased output to be
        further from the oracle's than y0 explains;
      * the biased output against the oracle with assert_close, with |bias| <= B = 0.064 max|ref0|: the error is at most one ulp of the
        larger of |acc| and |y|, ulp(acc) <= ulp_rel (|y| + B), and ulp_rel B <= 2^-7 B = 0.5e-3 max|ref0| stays inside the bar's norm-wise
        term (max|ref| >= max|ref0| - B)."""
    L = lib()
    force(monkeypatch, BM, S)
    M, K, gs = ref.forced_m(BM), ref.BK * Tk, 128
    tps = ref.check_forced_tiles(S, Tk)
    what = f"BM={BM} S={S} T={Tk} (tiles/split {tps}) M={M} K={K} N={N} w{w_bit} dt={dt} asym={asym}"
    assert ref.query(L, M, K, N) == (0, BM, S, tps), what
    assert ref.forward_plan(L, M, K, N, w_bit, gs, CODE[dt])[0] == ref.GEMM_FUSED, what
    rng = np.random.default_rng(100000 * w_bit + 1000 * BM + 50 * S + 4 * Tk + 2 * dt + asym)
    qw, scales, zeros, gen = T.rand_case(rng, K, N, w_bit, gs, dt, asym)
    x = torch.randn((M, K), generator=gen).to(T.TDT[dt])
    dev = [t.to(DEV) for t in (x, qw, scales, zeros)]
    y0 = T.hip_forward(*dev, None, w_bit, gs, asym)
    ref0 = T.oracle_forward(x, qw, scales, zeros, None, w_bit, gs, asym, dt)
    T.assert_close(y0, ref0, dt, what)
    if dt == orc.F16:
        T.assert_close_elementwise_f16(y0, ref0, what)
    if with_bias:
        B = 0.064 * float(ref0.float().abs().max())
        bias = (torch.randn((N,), generator=gen) * 0.1).clamp(-B, B).to(T.TDT[dt])
        assert float(bias.float().abs().min()) > 0 and float(bias.float().abs().mean()) > 0.04, "the bias must show in every column"
        y = T.hip_forward(*dev, None, w_bit, gs, asym, bias)
        want = (y0.float().cpu() + bias.float()).to(T.TDT[dt])
        bad = (y.cpu() != want).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} outputs are not dt(y0 + bias); first {bad[:4].tolist()}"
        T.assert_close(y, T.oracle_forward(x, qw, scales, zeros, None, w_bit, gs, asym, dt, bias), dt, what + " with bias")


# ------------------------------------------------------------------------------------------------ a. every selectable (BM, S), forced
@pytest.mark.parametrize("BM,S", ref.PLANS)
def test_every_selectable_plan_forced_against_the_oracle(BM, S, monkeypatch):
    """W4, both dtypes, sym with a bias (the finalize pass adds it when S > 1, the GEMM's epilogue when S = 1) and asym without, at
    group_size 128 on N = 264 (two column tiles, the last 8 columns wide) and M = BM + BM / 2 + 1 rows (a clamped last row tile, never a
    decode call).  K per S from gemm_plan_ref.forced_tiles: a short last split, splits that start inside a quantisation group, and from
    S = 9 -- the second chunk of eight slabs of the finalize pass -- also two tiles per split."""
    for Tk in ref.forced_tiles(S):
        for dt in (orc.BF16, orc.F16):
            forced_case(monkeypatch, BM, S, Tk, 4, dt, 0, True)
            forced_case(monkeypatch, BM, S, Tk, 4, dt, 1, False)


@pytest.mark.parametrize("S", [16, 15])
@pytest.mark.parametrize("w_bit", [2, 8])
def test_w2_and_w8_under_the_longest_split_lists(w_bit, S, monkeypatch):
    """The other bit widths through both chunks of the finalize pass: S = 16 and the largest odd S.  W2 packs 16 columns per zero-point
    word, so the fused kernel takes N % 16 == 0 only: its ragged last column tile is 16 wide (N = 272) where W8 and W4 have 8 (N = 264)."""
    N = 272 if w_bit == 2 else ref.FORCED_N
    for Tk in ref.forced_tiles(S):
        forced_case(monkeypatch, 64, S, Tk, w_bit, orc.F16, 0, True, N)
        forced_case(monkeypatch, 128, S, Tk, w_bit, orc.BF16, 1, False, N)


# ------------------------------------------------------------------------------------------------ b. plan invariance on exact data
@pytest.mark.parametrize("asym", [0, 1])
@pytest.mark.parametrize("dt", [orc.F16, orc.BF16])
def test_the_result_does_not_depend_on_the_plan_where_fp32_sums_are_exact(dt, asym, monkeypatch):
    """gemm_plan_ref.exact_case (M = 300, K = 2048, N = 264, group_size 128, W4): every product and every partial sum is a multiple of
    2^-6 below 2^12, exact in fp32 in any order, so all 4 x 16 forced (BM, S) -- a request whose S collapses to an equivalent smaller one
    is still run -- must give the same bits, and those bits are the float64 product rounded once to the dtype (which is what the oracle
    returns for these inputs: tests/test_gemm_plan_cpu.py).  Tolerance zero."""
    L = lib()
    M, K, N, gs = ref.EXACT_SHAPE
    x, qw, scales, zeros, y64 = ref.exact_case(T.TDT[dt], asym, 11 + asym)
    want = torch.from_numpy(y64).to(T.TDT[dt])
    x, qw, scales, zeros = (t.to(DEV) for t in (x, qw, scales, zeros))
    ran, first, differs, wrong = set(), None, [], []
    for BM in ref.BMS:
        for S in range(1, 17):
            force(monkeypatch, BM, S)
            flag, bm, s, tps = ref.query(L, M, K, N)
            assert (flag, bm, (s, tps)) == (0, BM, ref.effective(K // ref.BK, S)), (BM, S, flag, bm, s, tps)
            assert ref.forward_plan(L, M, K, N, 4, gs, CODE[dt])[0] == ref.GEMM_FUSED
            y = T.hip_forward(x, qw, scales, zeros, None, 4, gs, asym).cpu()
            ran.add((bm, s, tps))
            first = y if first is None else first
            if not torch.equal(y, first):
                differs.append((BM, S))
            if not torch.equal(y, want):
                wrong.append((BM, S, int((y != want).sum())))
    print(f"\n[gemm plan] exact data dt={dt} asym={asym}: 64 forced plans, {len(ran)} distinct launches; differ from (32, 1): {differs}; "
          f"differ from the float64 product: {wrong}")
    assert not differs, f"the result depends on the plan: {differs}"
    assert not wrong, f"(BM, S, elements) off the float64 product rounded once: {wrong}"


# ------------------------------------------------------------------------------------------------ c. the table's own cells, unforced
CELLS = ref.table_cells(ref.parse_table())


@pytest.mark.parametrize("K,N,M,plan,M2", CELLS, ids=[f"{c[0]}x{c[1]}-M{c[2]}-bm{c[3][0]}s{c[3][1]}" for c in CELLS])
def test_table_cells_unforced_against_the_oracle(K, N, M, plan, M2, monkeypatch):
    """One honoured cell of csrc/mpq_gemm_plan_table.inc per (BM, S) the table yields (the smallest) and the K = 2048 cells, at default
    knobs and group_size 128: the query says the table's plan is the one that runs; at most 32 sampled rows -- the first and the last of
    each row tile -- by all columns against the oracle; all rows finite; the sampled rows alone in a second launch agree (row independence);
    and a neighbouring row count with the same tile count takes the same plan and gives the same rows.  bf16 W4 where that reaches the
    fused kernel, else fp16 W4, else W8 (the decode kernels take 17 .. 32 rows on their measured shapes): none is skipped."""
    L = lib()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    variant = ref.cell_variant(L, (M, M2), K, N, CODE[orc.F16], CODE[orc.BF16])
    assert variant is not None, "listed in CELLS_NOT_FUSED of tests/test_gemm_plan_cpu.py?"
    dt = orc.F16 if variant[0] == CODE[orc.F16] else orc.BF16
    w_bit, gs = variant[1], 128
    what = f"cell K={K} N={N} M={M} plan={plan} w{w_bit} dt={dt}"
    for m in (M, M2):
        assert ref.query(L, m, K, N) == (1,) + plan, (what, m)
        form, need = ref.forward_plan(L, m, K, N, w_bit, gs, CODE[dt])
        assert form == ref.GEMM_FUSED and L.bie_mpq_workspace_bytes(m, K, N, w_bit) >= need, (what, m)
    rng = np.random.default_rng(K + 3 * N + 7 * M)
    qw, scales, zeros, gen = T.rand_case(rng, K, N, w_bit, gs, dt, 0)
    x = torch.randn((max(M, M2), K), generator=gen).to(T.TDT[dt])
    qw, scales, zeros, xd = qw.to(DEV), scales.to(DEV), zeros.to(DEV), x.to(DEV)
    y = T.hip_forward(xd[:M], qw, scales, zeros, None, w_bit, gs, 0)
    y2 = T.hip_forward(xd[:M2], qw, scales, zeros, None, w_bit, gs, 0)
    rows = ref.sampled_rows(M, plan[0], extra=tuple(range(M, M2)))
    assert len(rows) <= 32 and {0, M - 1} <= set(rows)
    own = [r for r in rows if r < M]
    ref_y = T.t16(orc.mpq_forward(orc.torch_to_np(x[rows]), qw.cpu().numpy(), orc.torch_to_np(scales), orc.torch_to_np(zeros), None, w_bit, gs, 0, dt), dt)
    T.assert_close(y[own], ref_y[:len(own)], dt, what + " sampled rows vs oracle")
    if dt == orc.F16:
        T.assert_close_elementwise_f16(y[own], ref_y[:len(own)], what + " sampled rows vs oracle")
    assert torch.isfinite(y.float()).all() and torch.isfinite(y2.float()).all(), what
    y3 = T.hip_forward(xd[own], qw, scales, zeros, None, w_bit, gs, 0)
    T.assert_close(y3, y[own], dt, what + " the sampled rows alone (row independence)")
    common = min(M, M2)
    T.assert_close(y2[:common], y[:common], dt, what + f" against M={M2}")
    if M2 > M:
        T.assert_close(y2[M:], ref_y[len(own):], dt, what + f" rows {M} .. {M2 - 1} of M={M2} vs oracle")
