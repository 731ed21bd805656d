"""What tests/test_gemm_plan_cpu.py and tests/test_gemm_plan_gpu.py share about the launch plans of the fused MPQ GEMM (csrc/mpq_gemm.hip):

  * PLANS -- every (tile height BM, split-K factor S) the dispatcher may select.  The CPU test asserts that the walk over the measured grid,
    with the table and with the model alone, selects nothing outside it; the GPU test forces each pair against the oracle.  A regenerated
    table or a changed cost model that selects a new pair fails on the CPU until the pair is added here -- and with that run on the GPU.
  * the measured table csrc/mpq_gemm_plan_table.inc read as data, and the table half of plan_gemm restated over it (the cost model is NOT
    restated: the tests check its answers by their properties only).
  * the K tile counts the forced GPU cases use per S, and the table cells the unforced GPU cases run.

No test in here; the library is only touched through `query` / `forward_plan`, both host-only."""
import ctypes
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_INC = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mpq_gemm_plan_table.inc")
BK, BN = 64, 256          # GEMM_BK, GEMM_BN of csrc/mpq_gemm.hip
WS_HEAD = 16384           # BIE_WS_HEAD_BYTES
GEMM_FUSED = 4            # MpqForm::GemmFused (csrc/mpq_plan.h)
BMS = (32, 64, 128, 256)

PLANS = [
    (32, 1), (32, 2), (32, 4), (32, 5), (32, 6), (32, 8), (32, 9), (32, 10), (32, 11), (32, 12), (32, 13), (32, 15), (32, 16),
    (64, 1), (64, 2), (64, 3), (64, 4), (64, 5), (64, 6), (64, 8), (64, 9), (64, 10), (64, 11), (64, 12), (64, 13), (64, 15), (64, 16),
    (128, 1), (128, 2), (128, 3), (128, 4), (128, 5), (128, 6), (128, 7), (128, 8), (128, 9), (128, 10), (128, 11), (128, 12), (128, 13), (128, 15), (128, 16),
    (256, 1), (256, 2), (256, 3), (256, 4), (256, 5), (256, 8), (256, 10), (256, 16),
]


def cdiv(a, b):
    return (a + b - 1) // b


def effective(T, S):
    """(S, tiles_per_split) a request for S splits of T K tiles runs as: cdiv(T, S) tiles per split and no empty split."""
    tps = cdiv(T, S)
    return cdiv(T, tps), tps


# ------------------------------------------------------------------------------------------------ the library, host-only
def query(L, M, K, N):
    """bie_test_mpq_gemm_plan -> (flag, BM, S, tiles_per_split)."""
    bm, s, tps = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    flag = L.bie_test_mpq_gemm_plan(M, K, N, ctypes.byref(bm), ctypes.byref(s), ctypes.byref(tps))
    return flag, bm.value, s.value, tps.value


def forward_plan(L, M, K, N, w_bit, gs, dt):
    """bie_test_mpq_forward_plan -> (form, workspace need)."""
    need = ctypes.c_size_t(0)
    form = L.bie_test_mpq_forward_plan(M, K, N, w_bit, gs, dt, 0, 0, ctypes.byref(need))
    return form, need.value


# ------------------------------------------------------------------------------------------------ the table as data
def parse_table(path=TABLE_INC):
    """(kPlanK, kPlanN, kPlanM, table[ki][ni][mi]) from the generated .inc: three int grids and one flat run of 0x.. bytes."""
    text = open(path).read()
    grid = lambda name: [int(v) for v in re.search(name + r"\[\d+\]\s*=\s*\{([^}]*)\}", text).group(1).split(",")]
    Kg, Ng, Mg = grid("kPlanK"), grid("kPlanN"), grid("kPlanM")
    body = re.sub(r"//[^\n]*", "", text[text.index("kPlanTable"):])
    flat = [int(v, 16) for v in re.findall(r"0x[0-9a-fA-F]{2}\b", body)]
    assert len(flat) == len(Kg) * len(Ng) * len(Mg), (len(flat), len(Kg), len(Ng), len(Mg))
    it = iter(flat)
    table = [[[next(it) for _ in Mg] for _ in Ng] for _ in Kg]
    return Kg, Ng, Mg, table


def decode_entry(e):
    return 32 << (e >> 5), e & 31


def honoured(e, K, M):
    """The conditions plan_gemm states for taking an entry at its own grid point: non-zero, the tile is not taller than twice the rows
    (BM = 32 always may), and a split keeps two K tiles at least."""
    BM, S = decode_entry(e)
    T = K // BK
    return e != 0 and not (BM > 32 and BM >= 2 * M) and S >= 1 and (S == 1 or T // S >= 2)


def grid_index(g, x):
    """grid_index of csrc/bie_common.h: the nearest point in log space, None beyond 20 % outside."""
    if x * 1.2 < g[0] or x > g[-1] * 1.2:
        return None
    i = 0
    while i + 1 < len(g) and x * x > g[i] * g[i + 1]:
        i += 1
    return i


def table_plan(tab, M, K, N):
    """The table half of plan_gemm: (BM, S, tiles_per_split) when a cell's plan is taken for (M, K, N), None when the model answers."""
    Kg, Ng, Mg, table = tab
    if K not in Kg or N not in Ng:
        return None
    mi = grid_index(Mg, M)
    if mi is None:
        return None
    e = table[Kg.index(K)][Ng.index(N)][mi]
    BM, S = decode_entry(e)
    if not honoured(e, K, M) or cdiv(M, BM) != cdiv(Mg[mi], BM):
        return None
    return (BM,) + effective(K // BK, S)


def honoured_cells(tab):
    """[(K, N, M, (BM, S, tiles_per_split))] of the entries taken at their own grid point, in grid order."""
    Kg, Ng, Mg, table = tab
    return [(K, N, M, (decode_entry(table[ki][ni][mi])[0],) + effective(K // BK, decode_entry(table[ki][ni][mi])[1]))
            for ki, K in enumerate(Kg) for ni, N in enumerate(Ng) for mi, M in enumerate(Mg) if honoured(table[ki][ni][mi], K, M)]


# ------------------------------------------------------------------------------------------------ the forced GPU cases
FORCED_N = 264  # two column tiles, the last one 8 columns wide


def forced_m(BM):
    """One full row tile, then a clamped one; never a decode call (33 rows at least)."""
    return max(33, BM + BM // 2 + 1)


def forced_tiles(S):
    """K tile counts (of 64) for a forced S.  The first: S splits exactly, K = 64 T a multiple of the group size 128, 3 tiles per split --
    every other split starts inside a quantisation group -- and the last split shorter than the others (T = 3 S - 1 for odd S, 3 S - 2 for
    even S).  Two S cannot have a short last split on an even T: S = 1 (one split; T = 4) and S = 2 (two equal halves; T = 6, so that
    the second one still starts mid-group).  From S = 9, where the finalize pass takes its second chunk of eight slabs, a second count
    with 2 tiles per split, the shortest pipeline the dispatcher selects (T = 2 S; no even T leaves a short last split there)."""
    if S <= 2:
        return [4] if S == 1 else [6]
    Ts = [3 * S - 1 if S % 2 else 3 * S - 2]
    if S >= 9:
        Ts.append(2 * S)
    return Ts


def check_forced_tiles(S, T):
    """tiles_per_split of (S, T) after checking what forced_tiles promises."""
    S_eff, tps = effective(T, S)
    assert S_eff == S and (BK * T) % 128 == 0 and tps in (2, 3, 4), (S, T)
    last = T - (S - 1) * tps
    assert 0 < last <= tps and (last < tps or S <= 2 or tps == 2), (S, T, "the last split must be the short one")
    return tps


# ------------------------------------------------------------------------------------------------ the unforced GPU cases
ALWAYS_CELLS = [(2048, 2048, 64), (2048, 2048, 128), (2048, 2048, 256), (2048, 2048, 768), (2048, 4096, 48), (2048, 4096, 96), (2048, 4096, 384)]


def neighbour_rows(tab, M, K, N, plan):
    """A row count next to M (more than 16: never the decode kernels' own range) that takes the same cell's plan with the same tile count."""
    for M2 in (M - 3, M - 1, M + 3, M + 1, M - 2, M + 2):
        if M2 > 16 and cdiv(M2, plan[0]) == cdiv(M, plan[0]) and table_plan(tab, M2, K, N) == plan:
            return M2
    raise AssertionError(f"no neighbouring row count keeps the plan of cell {(K, N, M)}")


def table_cells(tab):
    """The cells the unforced GPU cases run: per distinct (BM, S) the table yields, the honoured cell with the least K * N * M (ties: grid
    order), then the K = 2048 cells of ALWAYS_CELLS.  [(K, N, M, plan, neighbouring M)], sorted."""
    best = {}
    for (K, N, M, plan) in honoured_cells(tab):
        pair = plan[:2]
        if pair not in best or K * N * M < math.prod(best[pair][:3]):
            best[pair] = (K, N, M, plan)
    cells = {c[:3]: c for c in best.values()}
    for (K, N, M) in ALWAYS_CELLS:
        plan = table_plan(tab, M, K, N)
        assert plan is not None, f"cell {(K, N, M)} is no longer honoured"
        cells[(K, N, M)] = (K, N, M, plan)
    return [c + (neighbour_rows(tab, c[2], c[0], c[1], c[3]),) for c in sorted(cells.values())]


def cell_variant(L, rows, K, N, F16, BF16):
    """(dtype, w_bit) under which calls of the cell with each of `rows` rows reach the fused kernel at group_size 128: bf16 W4, then fp16 W4
    (the decode kernels take 17 .. 32 rows on their own measured shapes per dtype), then W8, which is never decoded.  None when none does."""
    for (dt, w) in ((BF16, 4), (F16, 4), (BF16, 8)):
        if all(L.bie_mpq_rows_form(M, K, N, w, 128, dt) == 0 and forward_plan(L, M, K, N, w, 128, dt)[0] == GEMM_FUSED for M in rows):
            return dt, w
    return None


def sampled_rows(M, BM, extra=(), limit=32):
    """At most `limit` rows: the first and the last row of each row tile (of evenly spread tiles when there are too many), then `extra`."""
    tiles = list(range(cdiv(M, BM)))
    room = (limit - len(extra)) // 2
    if len(tiles) > room:
        tiles = sorted({round(i * (len(tiles) - 1) / (room - 1)) for i in range(room)})
    rows = set(extra)
    for t in tiles:
        rows |= {t * BM, min(M, (t + 1) * BM) - 1}
    return sorted(rows)


# ------------------------------------------------------------------------------------------------ exact data: y cannot depend on the plan
EXACT_SHAPE = (300, 2048, 264, 128)  # M, K, N, group_size


def exact_case(torch_dtype, asym, seed, zero_is_nought=False):
    """W4 inputs on which every product and every partial sum of the GEMM is exact in fp32: scales are powers of two in 2^-6 .. 2^-4, the sym
    zero is 8 * scale (or 0), the asym zero a packed integer zero-point, x holds integers in [-2, 2].  A dequantised weight is an integer in
    [-16, 15] times its scale, a product a multiple of 2^-6 of at most 2, and a sum over K = 2048 a multiple of 2^-6 below 2^12: 18 bits.
    Returns torch tensors (x, qweight, scales, zeros) and the float64 product x @ W [M, N] (numpy)."""
    import numpy as np
    import torch
    M, K, N, gs = EXACT_SHAPE
    G = K // gs
    rng = np.random.default_rng(seed)
    qw = rng.integers(-2 ** 31, 2 ** 31 - 1, (K // 8, N), dtype=np.int64).astype(np.int32)
    s = 2.0 ** rng.integers(-6, -3, (G, N))
    x = rng.integers(-2, 3, (M, K)).astype(np.float64)
    q = np.empty((K, N), np.float64)
    qu = qw.view(np.uint32)
    for j in range(8):
        q[j::8] = (qu >> np.uint32(4 * j)) & np.uint32(15)
    if asym:
        zw = rng.integers(-2 ** 31, 2 ** 31 - 1, (G, N // 8), dtype=np.int64).astype(np.int32)
        zq = np.empty((G, N), np.float64)
        for j in range(8):
            zq[:, j::8] = (zw.view(np.uint32) >> np.uint32(4 * j)) & np.uint32(15)
        W = (q - (np.repeat(zq, gs, axis=0) + 1.0)) * np.repeat(s, gs, axis=0)
        zeros = torch.from_numpy(zw)
    else:
        z = np.zeros_like(s) if zero_is_nought else 8.0 * s
        W = q * np.repeat(s, gs, axis=0) - np.repeat(z, gs, axis=0)
        zeros = torch.from_numpy(z).to(torch_dtype)
    return torch.from_numpy(x).to(torch_dtype), torch.from_numpy(qw), torch.from_numpy(s).to(torch_dtype), zeros, x @ W
