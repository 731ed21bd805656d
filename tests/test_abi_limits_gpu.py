"""The MX entries of include/bie_hip.h at the maxima the header states, called through _hip.lib() with raw addresses: K = 2^20, E = 1024,
S = 32, P = 2^22, and calls whose element offsets cross 2^31.  Every case is compared with the float64 restatement.

K = 2^20, P = 2^22 and the 2^31 cases run on exact data (tests/abi_arena.py, "Exact data"): values in {0, +-0.5, +-1} that are fixed points of
every activation quantiser against weight magnitudes {0, 0.5, 1} under scale 2^0, so every partial sum of up to 2^20 products is a
multiple of 2^-2 below 2^24 quanta, exact in fp32 in any order; the result must be the float64 sum rounded once to the dtype.  E = 1024
and S = 32 run inside the arena of tests/abi_arena.py (guards, poison, both workspace fills) under the operators' own tolerance.  A call
that crosses 2^31 must also have the bits of the same entry run on row chunks that each stay below 2^31 (rows are independent); the index
expressions of the kernels involved were read for 32-bit products first (profiles/abi_contract.txt).  tests/test_abi_contract_cpu.py
checks the conditions these cases rest on (the experts hit, the skipped share, the exactness bound) without a GPU."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import abi_arena as A  # noqa: E402

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
KMAX = A.KMAX
ACT_FAMS = ["mxfp4_a4", "mxfp4_a8", "mxfp6_a8", "mxfp6_a6"]
ALL_FAMS = ["mxfp4", "mxfp6"] + ACT_FAMS

_X = {}


def shared_x(M):
    """One exact x [M, 2^20] for every family and dtype (its values are fp16 and bf16 numbers): drawn once, never written."""
    if M not in _X:
        _X[M] = A.exact_x(M, KMAX, A.gen(M, 20), F16)
    return _X[M]


# ---- K = 2^20 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["mxfp4_a4", "mxfp4_a8", "mxfp6", "mxfp6_a8", "mxfp6_a6"])
@pytest.mark.parametrize("M,form", [(1, 0), (65, 1)])
def test_linear_forward_at_k_2_20(fam, M, form):
    be = A.TorchBackend()
    for N, dt in ((1, F16), (5, BF16)) if M > 1 else ((1, F16), (1, BF16), (5, F16), (5, BF16)):
        A.run_tight(A.linear_case(fam, M, N, KMAX, dt, True, form, exact=True, x=shared_x(M)), be)


@pytest.mark.parametrize("fmt", ["fp4", "fp6"])
@pytest.mark.parametrize("M,dt", [(1, F16), (1, BF16), (129, BF16)])
def test_linear_grad_input_at_k_2_20(fmt, M, dt):
    A.run_tight(A.grad_case(fmt, M, 3, KMAX, dt, exact=True), A.TorchBackend())


@pytest.mark.parametrize("fam", ALL_FAMS)
@pytest.mark.parametrize("form", [0, 1])
def test_experts_forward_at_k_2_20(fam, form):
    """E = 2, T = 2 (S = 2, one slot skipped).  Beyond the one-launch bound the decode form of the activation-quantised families is the
    quantise launch and the routed kernel reading the workspace."""
    dt = F16 if form else BF16
    A.run_tight(A.experts_case(fam, 2, 2, 2, 5, KMAX, dt, True, 0, form, exact=True), A.TorchBackend())


# ---- E = 1024 and S = 32, in the arena -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ALL_FAMS)
@pytest.mark.parametrize("form", [0, 1])
def test_experts_forward_at_e_1024(fam, form):
    T, S, idx = A.routing_e1024(form)
    A.check(A.experts_case(fam, T, S, 1024, 17, 32, BF16 if form else F16, True, 0, form, idx=idx), A.TorchBackend())


@pytest.mark.parametrize("fmt", ["fp4", "fp6"])
@pytest.mark.parametrize("out_fp32", [0, 1])
def test_experts_grad_input_at_e_1024(fmt, out_fp32):
    T, S, idx = A.routing_e1024(1)
    A.check(A.moe_grad_case(fmt, T, S, 1024, 17, 32, F16 if out_fp32 else BF16, out_fp32, idx=idx), A.TorchBackend())


@pytest.mark.parametrize("fam", ALL_FAMS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_experts_forward_at_s_32(fam, xpp):
    be = A.TorchBackend()
    for form, dt in ((0, F16), (1, BF16)):
        A.check(A.experts_case(fam, 3, 32, 3, 17, 32, dt, True, xpp, form), be)


@pytest.mark.parametrize("fmt", ["fp4", "fp6"])
def test_experts_grad_input_at_s_32(fmt):
    be = A.TorchBackend()
    for out_fp32, dt in ((0, F16), (1, BF16)):
        A.check(A.moe_grad_case(fmt, 3, 32, 3, 17, 32, dt, out_fp32), be)


# ---- device-side calls for the shapes whose buffers are gigabytes -----------------------------------------------------------------------------------
def L():
    return A.lib()


def p(t):
    return None if t is None else t.data_ptr()


def moe_forward(x, idx, q, s, e_col, bias, T, S, E, N, K, dt, form=1, ws=None):
    """bie_mxfp4_moe_forward on device tensors; y pre-filled with NaN, the workspace with 0xFF.  -> (y [P, N], ws)."""
    P = T * S
    y = torch.full((P, N), float("nan"), dtype=dt, device=DEV)
    if ws is None:
        ws = torch.full((L().bie_mxfp4_moe_workspace_bytes(P, E),), 0xFF, dtype=torch.uint8, device=DEV)
    rc = L().bie_mxfp4_moe_forward(p(x), p(idx), p(q), p(s), p(e_col), p(bias), p(y), p(ws), T, S, E, N, K, 0, A.DT_CODE[dt], form, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return y, ws


def moe_operands(E, N, K, T, S, dt, seed):
    """Exact data of the experts' own exact test: x integers in -2 .. 2, every weight code, scale codes 126 .. 128: the products are
    multiples of 2^-2 below 2 * 12, so a sum of K = 32 of them is exact in fp32."""
    g = A.gen(E, N, K, T, S, seed)
    q, s = A.rand_w("fp4", E * N, K, g, 126, 128)
    x = torch.randint(-2, 3, (T, K), generator=g).to(dt)
    idx = A.routing_big(T, S, E, g)
    W = A.FAMS["mxfp4"].dequant_w(q, s).reshape(E, N, K)
    return x.to(DEV), idx.to(DEV), q.reshape(E, N, -1).to(DEV), s.reshape(E, N, -1).to(DEV), W.to(DEV)


def moe_reference_rows(x, idx, W, S, rows):
    """float64 y of the pairs `rows` (a LongTensor on the device): x[p / S] . W[idx[p]]^T, 0 for a skipped slot."""
    e = idx.reshape(-1)[rows].long()
    live = e >= 0
    xr = x[rows // S].double()
    y = torch.einsum("pk,pnk->pn", xr, W[e.clamp(min=0)])
    return torch.where(live[:, None], y, torch.zeros((), dtype=torch.float64, device=y.device))


@pytest.mark.parametrize("E", [3, 1024])
def test_experts_forward_and_grad_input_at_p_2_22(E):
    """P = 2^22 pairs (T = 2^17 tokens of S = 32 slots), K = 32, N = 1, x per token: the routing kernel's scan, binary search and tile
    table at their largest, and the tile count it writes against the bound the workspace was sized for."""
    T, S, K, N, dt = 1 << 17, 32, 32, 1, BF16 if E == 3 else F16
    P = T * S
    x, idx, q, s, W = moe_operands(E, N, K, T, S, dt, 22)
    e_col = s.amax(dim=2)
    y, ws = moe_forward(x, idx, q, s, e_col, None, T, S, E, N, K, dt)
    max_tiles = A.max_tiles(P, E)
    n_tiles = int(ws[:4].view(torch.int32)[0])
    assert 0 < n_tiles <= max_tiles, (n_tiles, max_tiles)
    assert n_tiles == A.tile_count(idx.cpu(), E)
    for lo in range(0, P, 1 << 20):  # the reference in slices of 2^20 pairs
        rows = torch.arange(lo, lo + (1 << 20), device=DEV)
        want = moe_reference_rows(x, idx, W, S, rows).to(dt)
        assert torch.equal(y[lo:lo + (1 << 20)], want), lo
    # the gradient of the same routing: gx[p, :] = gy[p, 0] * W[idx[p], 0, :]
    g = A.gen(E, 23)
    gy = torch.randint(-2, 3, (P, N), generator=g).to(dt).to(DEV)
    gx = torch.full((P, K), float("nan"), dtype=dt, device=DEV)
    ws.fill_(0)  # the other fill
    rc = L().bie_mxfp4_moe_grad_input(p(gy), p(idx), p(q), p(s), p(s.amax(dim=1)), p(gx), p(ws), T, S, E, N, K, A.DT_CODE[dt], 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and int(ws[:4].view(torch.int32)[0]) == n_tiles
    e = idx.reshape(-1).long()
    want = torch.where((e >= 0)[:, None], gy.double() * W[e.clamp(min=0), 0, :], torch.zeros((), dtype=torch.float64, device=DEV)).to(dt)
    assert torch.equal(gx, want)


# ---- element offsets past 2^31 ------------------------------------------------------------------------------------------------------------------------
BIG_M, BIG_N, CHUNKS, TAIL = 65600, 32800, 4, 70  # M * N = 2^31 + 4.2e6; a quarter of the rows stays below 2^31 bytes as well


def dense_forward(fam, x, q, s, e_col, M, N, K, dt):
    """The family's forward entry, prefill form, on device tensors.  -> y [M, N] (pre-filled with NaN)."""
    y = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
    tail = (M, N, K, A.DT_CODE[dt], 1, None)
    if A.FAMS[fam].act is None:
        rc = getattr(L(), f"bie_{fam}_linear_forward")(p(x), p(q), p(s), p(e_col), None, p(y), *tail)
    else:
        ws = torch.full((getattr(L(), f"bie_{fam}_workspace_bytes")(M, N, K, 1),), 0xFF, dtype=torch.uint8, device=DEV)
        rc = getattr(L(), f"bie_{fam}_linear_forward")(p(x), p(q), p(s), p(e_col), None, p(y), p(ws), *tail)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return y


def device_exact_x(M, K, dt, seed):
    """A.exact_x drawn on the device (gigabytes): values in {0, +-0.5, +-1}, +1 at the head of every block of 32."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randint(-2, 3, (M, K), generator=g, device=DEV, dtype=torch.int8).to(dt)
    x *= 0.5
    x[:, ::32] = 1.0
    return x


def check_chunks_and_tail(full, run_chunk, M, ref_tail):
    """full [M, C] against the same entry on CHUNKS row chunks, and its last TAIL rows against float64 computed on the CPU."""
    step = M // CHUNKS
    assert step * CHUNKS == M
    for c in range(CHUNKS):
        part = run_chunk(c * step, (c + 1) * step)
        assert torch.equal(full[c * step:(c + 1) * step], part), f"rows {c * step} .. differ from the chunked call"
        del part
    want = ref_tail().to(full.dtype)
    assert torch.equal(full[M - TAIL:].cpu(), want), "the last rows differ from the float64 product"


@pytest.mark.parametrize("fam", ALL_FAMS)
def test_dense_prefill_tile_with_y_past_2_31(fam):
    f = A.FAMS[fam]
    M, N, K, dt = BIG_M, BIG_N, 32, BF16 if f.w == "fp6" else F16
    g = A.gen(len(fam), 31)
    q, s = A.exact_w(f.w, N, K, g)
    x = A.exact_x(M, K, g, dt)
    xd, qd, sd = x.to(DEV), q.to(DEV), s.to(DEV)
    e_col = sd.amax(dim=1)
    y = dense_forward(fam, xd, qd, sd, e_col, M, N, K, dt)
    check_chunks_and_tail(y, lambda a, b: dense_forward(fam, xd[a:b], qd, sd, e_col, b - a, N, K, dt), M,
                          lambda: x[M - TAIL:].double() @ f.dequant_w(q, s).t())


@pytest.mark.parametrize("fam", ACT_FAMS)
def test_activation_quantiser_with_x_and_xq_past_2_31(fam):
    """M = 65600 rows of K = 32768: x crosses 2^31 elements (and the MXFP8 xq 2^31 bytes); N = 1, prefill form."""
    f = A.FAMS[fam]
    M, N, K, dt = BIG_M, 1, 32768, F16 if f.w == "fp6" else BF16
    q, s = A.exact_w(f.w, N, K, A.gen(len(fam), 32))
    xd, qd, sd = device_exact_x(M, K, dt, 33), q.to(DEV), s.to(DEV)
    e_col = sd.amax(dim=1)
    y = dense_forward(fam, xd, qd, sd, e_col, M, N, K, dt)
    check_chunks_and_tail(y, lambda a, b: dense_forward(fam, xd[a:b], qd, sd, e_col, b - a, N, K, dt), M,
                          lambda: xd[M - TAIL:].cpu().double() @ f.dequant_w(q, s).t())


@pytest.mark.parametrize("fmt", ["fp4", "fp6"])
def test_gradient_tile_with_gy_past_2_31(fmt):
    """gx [M, 32] = gy [M, 32800] . W: the gy rows of the last tiles start past 2^31 elements."""
    f = A.FAMS["mxfp4" if fmt == "fp4" else "mxfp6"]
    M, N, K, dt = BIG_M, BIG_N, 32, F16 if fmt == "fp4" else BF16
    q, s = A.exact_w(fmt, N, K, A.gen(len(fmt), 34))
    gy, qd, sd = device_exact_x(M, N, dt, 35), q.to(DEV), s.to(DEV)
    e_blk = sd.amax(dim=0)

    def run(a, b):
        gx = torch.full((b - a, K), float("nan"), dtype=dt, device=DEV)
        rc = getattr(L(), f"bie_{f.name}_linear_grad_input")(p(gy[a:b]), p(qd), p(sd), p(e_blk), p(gx), b - a, N, K, A.DT_CODE[dt], None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        return gx

    # exact: |gx| <= N = 32800 products of magnitude <= 1 on a 2^-2 grid, 2^17.1 quanta
    check_chunks_and_tail(run(0, M), run, M, lambda: gy[M - TAIL:].cpu().double() @ f.dequant_w(q, s))


def test_routed_tile_with_y_past_2_31():
    """P = 2^22 pairs of N = 520 columns: y [P, 520] crosses 2^31 elements; the chunks are quarters of the tokens."""
    T, S, E, N, K, dt = 1 << 17, 32, 3, 520, 32, F16
    x, idx, q, s, W = moe_operands(E, N, K, T, S, dt, 36)
    e_col = s.amax(dim=2)
    y, _ = moe_forward(x, idx, q, s, e_col, None, T, S, E, N, K, dt)
    assert y.numel() > 1 << 31
    step = T // CHUNKS
    for c in range(CHUNKS):
        part, _ = moe_forward(x[c * step:(c + 1) * step], idx[c * step:(c + 1) * step], q, s, e_col, None, step, S, E, N, K, dt)
        assert torch.equal(y[c * step * S:(c + 1) * step * S], part), c
        del part
    rows = torch.arange(T * S - TAIL, T * S)
    want = moe_reference_rows(x.cpu(), idx.cpu(), W.cpu(), S, rows).to(dt)
    assert torch.equal(y[T * S - TAIL:].cpu(), want)
