"""MXFP4 W4A6 mixture-of-experts layer on the MI355X: both forms of the expert GEMM (forced) and the plan against the float64 restatement
per pair within the W4A6 linear contract's tolerance, gemm on chosen codes, forward bit-identical to quantize_act + gemm (the one-launch
decode form, whose workgroups quantise their row into LDS, against the from-memory one, up to and beyond the one-launch K), the element
maps of both forms (one-hot rows and one-hot weight selectors per expert), exact data bit-identical across forms and to the W4A6 linear
layer, inexact data bit-identical to the W4A6 linear layer's two forms per expert under both tile widths of the grouped form, row
independence, out-of-range indices, NaN / inf rows, NaN blocks, MXFP4A6ExpertsLinearCuda (checkpoints, latent weight, backward) and
MXFP4A6MoECuda (its public pieces, the distance to the float64 variant restatement, the ordering against the MXFP4 W4A4 block, graph
replay).  The shapes and the routing (make_idx / assert_coverage) are those of test_mxfp6_moe_a6_gpu.py."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
BM = 128  # the row tile of the grouped form
DECODE_PAIRS = 1024  # the largest P the decode form exists for
ONE_K = 16384  # the largest K of the one-launch decode form
WN_KNOB = "BIE_MXFP4_MOE_A6_WN"  # the grouped form's column tile: 2 = 128 x 128, 1 = 128 x 64 (re-read per call under BIE_TUNING)
_spec = importlib.util.spec_from_file_location("mxfp4_moe_a6_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_moe_a6_ref.py"))
aref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(aref)
mref, m6, a6 = aref.mref, aref.m6, aref.a6


def ext():
    from bitorch_engine.extensions import mxfp4_experts_a6_cuda
    return mxfp4_experts_a6_cuda


def dense():
    from bitorch_engine.extensions import mxfp4_a6_linear_cuda
    return mxfp4_a6_linear_cuda


class tile_width:
    """The grouped form's column tile forced for the calls inside (the tests run under BIE_TUNING, so the knob is read per call)."""

    def __init__(self, wn):
        self.wn = wn

    def __enter__(self):
        assert os.environ.get("BIE_TUNING"), "the knob is re-read per call only under BIE_TUNING"
        self.old = os.environ.get(WN_KNOB)
        os.environ[WN_KNOB] = str(self.wn)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(WN_KNOB, None)
        else:
            os.environ[WN_KNOB] = self.old


_WEIGHTS = {}


def rand_mx(E, N, K, seed, lo=118, hi=130):
    """Random code bytes (every 4-bit code occurs) and scale codes on the GPU, with their float64 W (cached: shared by many cases)."""
    key = (E, N, K, seed, lo, hi)
    if key not in _WEIGHTS:
        if E * N * K > 1 << 24:
            _WEIGHTS.clear()  # one large stack at a time
        g = torch.Generator(device=DEV).manual_seed(seed)
        q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        s = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        _WEIGHTS[key] = (q, s, aref.dequant(q, s).to(DEV))
    return _WEIGHTS[key]


def admits_coverage(T, S, E):
    """The grouped form's routing condition needs three experts (one above a row tile, one with exactly one pair, one with none) and
    BM + 1 pairs, one pair and one skipped slot beside them."""
    return E >= 3 and T * S >= BM + 4


def make_idx(T, S, E, seed):
    """A fixed-seed routing.  Where the shape admits it (admits_coverage): expert 0 gets more than one row tile, expert E - 2 exactly one
    pair, expert E - 1 none, about a sixteenth of the slots are skipped (-1), the rest are Zipf-skewed over the experts 0 .. E - 3.
    Smaller shapes: Zipf over all the experts, every fifth slot skipped when there are five."""
    g = torch.Generator().manual_seed(seed)
    P = T * S
    if not admits_coverage(T, S, E):
        prob = 1.0 / torch.arange(1, E + 1, dtype=torch.float64) ** 1.2
        idx = torch.multinomial(prob / prob.sum(), P, replacement=True, generator=g)
        idx[4::5] = -1
        return idx.reshape(T, S).to(torch.int32)
    prob = 1.0 / torch.arange(1, E - 1, dtype=torch.float64) ** 1.2
    idx = torch.multinomial(prob / prob.sum(), P, replacement=True, generator=g)
    perm = torch.randperm(P, generator=g)
    n_skip = max(1, min(P // 16, P - BM - 2))
    idx[perm[:BM + 1]] = 0
    idx[perm[BM + 1]] = E - 2
    idx[perm[BM + 2:BM + 2 + n_skip]] = -1
    return idx.reshape(T, S).to(torch.int32)


def assert_coverage(idx, E):
    """From idx itself, on the CPU: an expert with more pairs than one row tile, one with exactly one pair, one with none, skipped slots."""
    flat = idx.reshape(-1).long()
    live = (flat >= 0) & (flat < E)
    c = torch.bincount(flat[live], minlength=E)
    assert bool((c > BM).any()) and bool((c == 1).any()) and bool((c == 0).any()) and bool((~live).any()), c.tolist()


def check(y, yref, absprod, K, dt, idx=None, E=None):
    """mxfp4_a6_ref.tolerance where the restatement is finite, NaN exactly where it is NaN, +0 in the skipped slots."""
    yref, absprod = yref.to(y.device), absprod.to(y.device)
    nan = torch.isnan(yref)
    assert torch.equal(torch.isnan(y), nan), (int(torch.isnan(y).sum()), int(nan.sum()))
    assert torch.isfinite(y[~nan]).all()
    tol = aref.tolerance(yref, absprod, K, dt)
    err = (y.double() - yref).abs()[~nan]
    assert (err <= tol[~nan]).all(), f"max err {err.max().item()} (tol there {tol[~nan].flatten()[err.argmax()].item()})"
    if idx is not None:
        skipped = ((idx < 0) | (idx >= E)).to(y.device)
        assert (y[skipped] == 0).all() and not torch.signbit(y[skipped]).any()


def forms_for(P):
    return (0, 1, -1) if P <= DECODE_PAIRS else (1, -1)


def case(E, S, K, N, T, dt, xpp, bias_on, seed, coverage_case):
    q, s, W = rand_mx(E, N, K, seed)
    g = torch.Generator().manual_seed(seed + 17 * T + xpp)
    x = (torch.randn((T, S, K) if xpp else (T, K), generator=g) * 0.5).to(dt)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV) if bias_on else None
    idx = make_idx(T, S, E, seed + T)
    if coverage_case:
        assert_coverage(idx, E)
    yref, a = aref.experts(x, idx, W, bias)
    e = ext().col_exp(s)
    for form in forms_for(T * S):
        y = ext().forward(x.to(DEV), idx.to(DEV), q, s, bias, e, form=form)
        assert y.dtype == dt and y.shape == (T, S, N)
        check(y, yref, a, K, dt, idx, E)
    with tile_width(1):  # the grouped form on 128 x 64 tiles
        check(ext().forward(x.to(DEV), idx.to(DEV), q, s, bias, e, form=1), yref, a, K, dt, idx, E)


# E, S, K, N, T: K = 2880 and K = 160 end in a partial 128-k step; N = 7 / 33 / 130 are not multiples of 4 / 16 / 64; the last shape has
# P = 1200 > 1024 pairs (no decode form)
ALL = [(1, 1, 32, 1, 1), (3, 4, 96, 7, 5), (8, 8, 96, 33, 17), (3, 4, 96, 7, 64), (8, 1, 160, 130, 300), (8, 4, 2880, 130, 64), (3, 4, 96, 7, 300)]
COVERAGE = [c for c in ALL if admits_coverage(c[4], c[1], c[0])]
OTHER = [c for c in ALL if not admits_coverage(c[4], c[1], c[0])]  # tiny P, or fewer than three experts: both forms, without the routing claim
assert COVERAGE == [c for c in ALL if c[0] >= 3 and c[4] * c[1] >= BM + 4] and len(COVERAGE) == 5 and len(OTHER) == 2
assert any(c[4] * c[1] > DECODE_PAIRS for c in COVERAGE) and any(c[4] * c[1] <= DECODE_PAIRS for c in COVERAGE)


def run_case(E, S, K, N, T, xpp, dt, coverage_case):
    bias_on = (T + N + xpp + (dt == torch.float16)) % 2 == 0  # on and off alternate over the cases
    case(E, S, K, N, T, dt, xpp, bias_on, seed=E * 1000 + S * 100 + K + N, coverage_case=coverage_case)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("E,S,K,N,T", COVERAGE)
def test_forms_and_plan_against_float64_grouped_coverage_cases(E, S, K, N, T, xpp, dt):
    run_case(E, S, K, N, T, xpp, dt, True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("E,S,K,N,T", OTHER)
def test_forms_and_plan_against_float64_shapes_too_small_for_the_coverage_condition(E, S, K, N, T, xpp, dt):
    run_case(E, S, K, N, T, xpp, dt, False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("K", [160, 2880])
def test_gemm_on_chosen_codes_and_forward_is_quantize_then_gemm(K, form, xpp, dt):
    E, S, N, T = 8, 4, 130, 60
    q, s, W = rand_mx(E, N, K, 7)
    g = torch.Generator().manual_seed(8 + xpp)
    R = T * S if xpp else T
    xq = torch.randint(0, 256, (R, K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)  # every byte is three quarters of valid codes
    xs = torch.randint(114, 125, (R, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)  # random codes reach 7.5: y stays within fp16
    xq[1, 72:96] = 0
    xs[1, 3] = 0  # an all-zero block with its scale code
    flag = torch.zeros(R, dtype=torch.uint8)
    flag[2] = 1
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 9)
    assert_coverage(idx, E)
    yref, a = aref.experts_from_codes(xq, xs, flag, idx, W, bias)
    y = ext().gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), idx.to(DEV), q, s, bias, dtype=dt, form=form)
    check(y, yref, a, K, dt, idx, E)
    # forward = quantize_act then gemm, bit for bit (form 0: the one-launch decode kernel, which quantises into LDS, against the one
    # reading bie_mxfp6_quantize_act's bytes from memory: the two quantisers give the same image)
    x = (torch.randn((T, S, K) if xpp else (T, K), generator=g) * 0.5).to(dt).to(DEV)
    x[3, ..., 5] = float("inf")
    x[5, ..., 32:64] = 0  # an all-zero block
    cq, cs, cf = ext().quantize_act(x.reshape(-1, K))
    want = ext().gemm(cq, cs, cf, idx.to(DEV), q, s, bias, dtype=dt, form=form)
    got = ext().forward(x, idx.to(DEV), q, s, bias, form=form)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
def test_gemm_routed_form_on_a_small_ragged_case_against_float64(dt):
    """E = 3, S = 4, T = 17, 96 -> 33, x per pair, form 0 of gemm: the routed kernel that reads the quantised rows from memory (forward
    never runs it at this K), with K = 96 (one 128-k step whose last block lies past K, three waves without work), N = 33 (the last
    strip holds one column) and skipped slots."""
    E, S, K, N, T = 3, 4, 96, 33, 17
    q, s, W = rand_mx(E, N, K, 3433)
    g = torch.Generator().manual_seed(3433 + T)
    x = (torch.randn((T, S, K), generator=g) * 0.5).to(dt)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 3433)
    assert bool(((idx < 0) | (idx >= E)).any())
    yref, a = aref.experts(x, idx, W, bias)
    cq, cs, cf = ext().quantize_act(x.to(DEV).reshape(-1, K))
    y = ext().gemm(cq, cs, cf, idx.to(DEV), q, s, bias, dtype=dt, form=0)
    assert y.dtype == dt and y.shape == (T, S, N)
    check(y, yref, a, K, dt, idx, E)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", [ONE_K, ONE_K + 32])
def test_decode_form_at_and_beyond_the_one_launch_k(K, dt):
    """K = 16384 is one launch (the row image fills its 12800 bytes of LDS); K = 16416 is the quantise launch and the routed kernel
    reading the workspace.  Either way the result is gemm(quantize_act(x)) bit for bit and within the tolerance of float64."""
    E, S, N, T = 2, 2, 16, 2
    q, s, W = rand_mx(E, N, K, 11, 120, 126)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((T, K), generator=g) * 0.25).to(dt)
    idx = torch.tensor([[0, 1], [1, -1]], dtype=torch.int32)
    yref, a = aref.experts(x, idx, W)
    y = ext().forward(x.to(DEV), idx.to(DEV), q, s, form=0)
    check(y, yref, a, K, dt, idx, E)
    cq, cs, cf = ext().quantize_act(x.to(DEV))
    assert torch.equal(y.view(torch.int16), ext().gemm(cq, cs, cf, idx.to(DEV), q, s, dtype=dt, form=0).view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", [0, 1])
def test_one_hot_rows_select_their_own_weight_at_every_k(form, dt):
    """The element map of the weight operand in both forms: row t of x is 1.0 at k = t and zero elsewhere (amax 1 -> scale 2^-2, code
    4.0: kept exactly; the other blocks are all-zero blocks), so y[t, s, :] must be column t of its expert's weights exactly.  The
    columns of W differ pairwise over k within an expert (asserted), so a 4-bit code read from another nibble or another place of the step
    shows."""
    E, S, K, N = 3, 2, 256, 24
    T = K
    q, s, W = rand_mx(E, N, K, 15, 125, 129)
    W = W.cpu()
    for e in range(E):
        assert torch.unique(W[e].t().contiguous(), dim=0).shape[0] == K  # every k has its own column of weights
    x = torch.eye(K).to(dt)
    assert torch.equal(aref.fake_quant(x), x.double())
    g = torch.Generator().manual_seed(16)
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32)
    want = W[idx.long(), :, torch.arange(T)[:, None]]  # [T, S, N]: W[idx[t, s], :, t]
    assert want.shape == (T, S, N) and torch.equal(want.to(dt).double(), want)
    y = ext().forward(x.to(DEV), idx.to(DEV), q, s, form=form)
    assert torch.equal(y.cpu().double(), want)
    cq, cs, cf = ext().quantize_act(x.to(DEV))
    assert torch.equal(ext().gemm(cq, cs, cf, idx.to(DEV), q, s, dtype=dt, form=form), y)  # form 0: the kernel reading xq6 from memory


def selector_x(R, K):
    """selector_x of test_mxfp6_a6_gpu.py: x codes distinct per k within a block of a row (the 62 codes with a nonzero value), blocks told
    apart by their scales 2^-12, 2^-6, ..: every value is exact in fp16 and bf16 and no two k of a row give one value."""
    xc = (torch.arange(K)[None, :] * 5 + torch.arange(R)[:, None] * 11) % 62 + 1
    xc = torch.where(xc >= 32, xc + 1, xc).to(torch.uint8)
    xs = (127 + 6 * (torch.arange(K // 32) - 2))[None, :].repeat(R, 1).to(torch.uint8)
    return m6.pack(xc), xs


def selector_codes(E, N, K):
    """Unpacked E2M1 codes [E, N, K]: code 2 (1.0) at k = pi[e, n], zero elsewhere; pi [E, N], all distinct, every block in every expert."""
    pi = ((torch.arange(E)[:, None] * N + torch.arange(N)[None, :]) * 37 + 3) % K
    codes = torch.zeros((E, N, K), dtype=torch.uint8)
    codes[torch.arange(E)[:, None], torch.arange(N)[None, :], pi] = 2
    return codes, pi


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", [0, 1])
def test_selector_weights_per_expert_pin_the_k_of_the_x_codes(form, dt):
    """The selector construction of test_mxfp4_a6_gpu.py per expert: row n of expert e holds FP4 code 1.0 (E2M1 code 2) at k = pi_e(n)
    under scale 2^0 and zero codes elsewhere; the rows of x hold a distinct value per k.  Then
    y[p, n] == x^[row(p), pi_e(n)] exactly.  pi differs between the experts and visits every block (K = 160: the last 128-k step holds
    one block), so a pair read against another expert's rows, or an x code taken from another k or another bit position, shows.  With
    the one-hot rows above this pins the element maps of both operands in both forms."""
    E, S, K, N = 3, 2, 160, 24
    T = 40
    codes, pi = selector_codes(E, N, K)
    assert len(set(pi.flatten().tolist())) == E * N and set((pi // 32).flatten().tolist()) == set(range(K // 32))
    assert all(set((pi[e] // 32).tolist()) == set(range(K // 32)) for e in range(E))
    q = torch.stack([aref.pack(codes[e]) for e in range(E)]).to(DEV)
    s = torch.full((E, N, K // 32), 127, dtype=torch.uint8, device=DEV)
    R = T * S
    xq, xs = selector_x(R, K)
    flag = torch.zeros(R, dtype=torch.uint8)
    xh = a6.dequant_act(xq, xs)
    assert all(len(set(row.tolist())) == K for row in xh) and torch.equal(xh.to(dt).double(), xh)
    g = torch.Generator().manual_seed(17)
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32)
    for xpp in (0, 1):
        rows = torch.arange(R) if xpp else torch.arange(R) // S
        nrows = R if xpp else T
        want = xh[rows[:, None], pi[idx.reshape(-1).long()]].reshape(T, S, N)
        y = ext().gemm(xq[:nrows].to(DEV), xs[:nrows].to(DEV), flag[:nrows].to(DEV), idx.to(DEV), q, s, dtype=dt, form=form)
        assert torch.equal(y.cpu().double(), want), (xpp, (y.cpu().double() != want).nonzero()[:5].tolist())


def exact_x(R, K, dt):
    """Per block x[0] = 4 and the others m * 0.5, |m| <= 7: every block's amax is 4, so x is a fixed point of the quantiser (steps 0.125 /
    0.25 below 4) under one scale code."""
    m = ((torch.arange(K)[None, :] * 3 + torch.arange(R)[:, None]) % 15 - 7).float() * 0.5
    m[:, ::32] = 4.0  # the block maximum
    return m.to(dt)


def exact_case(R, E, N, K, g, dt):
    """One scale code everywhere (weights 127, x 2^0 per block: exact_x), so every instruction is exact (profiles/mxfp4_a6_probe.txt
    part (c)).  Weight codes random.  Products are multiples of 2^-4 and every partial sum of K = 256 stays below 256 * 4 * 6 < 2^13:
    17 bits, exact in fp32."""
    q, s, W = rand_mx(E, N, K, 21, 127, 127)
    return exact_x(R, K, dt), q, s, W


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("T", [1, 5, 64, 300])
def test_exact_data_is_bit_identical_across_forms_and_to_the_dense_layer(T, xpp, dt):
    """Exact data (exact_case) and an integer bias: the result is the float64 product rounded once, in every form and under both tile
    widths, and it is what the W4A6 linear layer gives per expert on that expert's rows."""
    E, S, N, K = 4, 4, 72, 256
    g = torch.Generator().manual_seed(T)
    x, q, s, W = exact_case(T * S if xpp else T, E, N, K, g, dt)
    assert len(set(s.flatten().tolist())) == 1
    if xpp:
        x = x.reshape(T, S, K)
    assert torch.equal(aref.fake_quant(x), x.double())  # the construction, checked against float64 on the CPU
    assert len(set(aref.quantize_rows(x)[1].flatten().tolist())) == 1  # one x scale code
    bias = torch.randint(-8, 9, (E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, T)
    yref, _ = mref.experts(x.double().to(DEV), idx, W, bias)
    yq, _ = aref.experts(x, idx, W, bias)
    assert torch.equal(yref, yq) and torch.equal(yref.float().double(), yref)
    want = yref.to(dt)
    xd = x.to(DEV)
    xr = (xd if xpp else xd[:, None, :].expand(T, S, K)).reshape(T * S, K)
    rows = torch.zeros((T * S, N), dtype=dt, device=DEV)
    for e in range(E):
        sel = (idx.reshape(-1) == e).nonzero().reshape(-1).to(DEV)
        if sel.numel():
            rows[sel] = dense().forward(xr[sel].contiguous(), q[e], s[e], bias[e])
    assert torch.equal(rows.reshape(T, S, N), want)
    ys = {}
    for form in forms_for(T * S):
        ys[form] = ext().forward(xd, idx.to(DEV), q, s, bias, form=form)
        assert torch.equal(ys[form], want), (form, (ys[form].double() - want.double()).abs().max().item())
    if 0 in ys:
        assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))
    with tile_width(1):
        assert torch.equal(ext().forward(xd, idx.to(DEV), q, s, bias, form=1).view(torch.int16), ys[1].view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("wn", [2, 1])
def test_grouped_prefill_form_equals_the_dense_prefill_form_bit_for_bit_on_inexact_data(wn, xpp, dt):
    """Random normal x (quantised once, by quantize_act), random weights and a bias: the sums round, and the grouped prefill form still
    gives the bits of the W4A6 linear layer's prefill form called once per expert on that expert's rows, because both run the one tile
    body (mx4a6_gemm_tile) and a row's sum order is fixed by K alone; the linear layer takes 64 x 64 tiles at this size and the grouped
    kernel 128 x 128 (wn = 2) or 128 x 64 (wn = 1), which moves an element to another lane, not its sum to another order.  K = 160 is
    not a whole 128-k stage, N = 130 gives column tiles with the last partial, and the routing holds an expert with more than one row
    tile and a partial one beside an expert without pairs."""
    E, S, K, N, T = 3, 2, 160, 130, 70
    q, s, _ = rand_mx(E, N, K, 91)
    g = torch.Generator().manual_seed(92 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 93)
    assert_coverage(idx, E)
    cq, cs, cf = ext().quantize_act(x.reshape(-1, K))
    with tile_width(wn):
        y = ext().gemm(cq, cs, cf, idx.to(DEV), q, s, bias, dtype=dt, form=1)
        assert torch.equal(y.view(torch.int16), ext().forward(x, idx.to(DEV), q, s, bias, form=1).view(torch.int16))
    rows = torch.zeros((T * S, N), dtype=dt, device=DEV)  # a skipped slot is +0
    for e in range(E):
        sel = (idx.reshape(-1) == e).nonzero().reshape(-1).to(DEV)
        if sel.numel():
            r = sel if xpp else sel // S  # the stored row of every pair
            rows[sel] = dense().gemm(cq[r], cs[r], cf[r], q[e], s[e], bias[e], dtype=dt, form=1)
    assert torch.equal(y.view(torch.int16), rows.reshape(T, S, N).view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_routed_decode_form_equals_the_dense_decode_form_bit_for_bit_on_inexact_data(xpp, dt):
    """The routed decode kernel sums a row's 128-k steps per wave and the four waves' partials as ((w0 + w1) + w2) + w3, the order of the
    W4A6 linear layer's decode form, so a pair's row has that form's bits on that expert's rows.  The dense decode form takes at most 64
    rows: every expert holds at most 64 pairs here (asserted), and one of them more than 32 (the 64-row instance)."""
    E, S, K, N, T = 3, 2, 160, 130, 50
    q, s, _ = rand_mx(E, N, K, 91)
    g = torch.Generator().manual_seed(94 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = torch.multinomial(torch.tensor([0.5, 0.3, 0.1, 0.1]), T * S, replacement=True, generator=g).reshape(T, S).to(torch.int32)
    idx[idx == E] = -1
    counts = torch.bincount(idx[idx >= 0].long(), minlength=E)
    assert counts.max() <= 64 and counts.max() > 32 and counts.min() >= 1 and bool((idx < 0).any()), counts.tolist()
    cq, cs, cf = ext().quantize_act(x.reshape(-1, K))
    y = ext().gemm(cq, cs, cf, idx.to(DEV), q, s, bias, dtype=dt, form=0)
    assert torch.equal(y, ext().forward(x, idx.to(DEV), q, s, bias, form=0))  # the one-launch kernel: the same bits
    rows = torch.zeros((T * S, N), dtype=dt, device=DEV)  # a skipped slot is +0
    for e in range(E):
        sel = (idx.reshape(-1) == e).nonzero().reshape(-1).to(DEV)
        r = sel if xpp else sel // S  # the stored row of every pair
        rows[sel] = dense().gemm(cq[r], cs[r], cf[r], q[e], s[e], bias[e], dtype=dt, form=0)
    assert torch.equal(y.view(torch.int16), rows.reshape(T, S, N).view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("form", [0, 1])
def test_a_row_depends_on_its_own_pair_only(form, xpp, dt):
    E, S, K, N, T = 8, 4, 288, 130, 60
    q, s, _ = rand_mx(E, N, K, 31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 33)
    e = ext().col_exp(s)
    y = ext().forward(x, idx.to(DEV), q, s, bias, e, form=form)
    assert torch.equal(y, ext().forward(x, idx.to(DEV), q, s, bias, e, form=form))  # two runs of one call
    live = [(t, sl) for t in range(T) for sl in range(S) if idx[t, sl] >= 0]
    for t, sl in (live[0], live[len(live) // 2], live[-1]):
        # every other pair's idx and x changed: the pair alone in a call of its own ...
        alone = ext().forward(x[t:t + 1, sl:sl + 1] if xpp else x[t:t + 1], idx[t:t + 1, sl:sl + 1].to(DEV), q, s, bias, e, form=form)
        assert torch.equal(alone[0, 0], y[t, sl])
        # ... and in place, among other pairs with other rows and other experts
        x2, idx2 = torch.randn(x.shape, generator=g).to(dt).to(DEV), make_idx(T, S, E, 34 + t)
        if xpp:
            x2[t, sl] = x[t, sl]
        else:
            x2[t] = x[t]
        idx2[t, sl] = idx[t, sl]
        y2 = ext().forward(x2, idx2.to(DEV), q, s, bias, e, form=form)
        assert torch.equal(y2[t, sl], y[t, sl]) and not torch.equal(y2, y)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", [0, 1])
def test_out_of_range_indices_give_zero_rows_and_touch_nothing_else(form, dt):
    E, S, K, N, T = 6, 4, 128, 40, 50
    q, s, _ = rand_mx(E, N, K, 41)
    g = torch.Generator().manual_seed(42)
    x = torch.randn((T, S, K), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 43)
    y = ext().forward(x, idx.to(DEV), q, s, form=form)
    bad = idx.clone()
    vals = torch.tensor([-1, E, 2 ** 31 - 1, -2 ** 31, E + 1000, -7], dtype=torch.int32)
    where = torch.randperm(T * S, generator=g)[:60]
    bad.reshape(-1)[where] = vals[torch.arange(60) % len(vals)]
    m = torch.zeros(T * S, dtype=torch.bool)
    m[where] = True
    m = m.reshape(T, S).to(DEV)
    yb = ext().forward(x, bad.to(DEV), q, s, form=form)
    assert (yb[m] == 0).all() and not torch.signbit(yb[m]).any()
    assert torch.equal(yb[~m], y[~m])
    # a flagged row of x whose slots are all skipped still gives +0 (x per token: token 7; x per pair: the pair itself)
    xt = torch.randn((T, K), generator=g).to(dt).to(DEV)
    xt[7, 3] = float("nan")
    idx7 = idx.clone()
    idx7[7] = torch.tensor([-1, E, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    y7 = ext().forward(xt, idx7.to(DEV), q, s, torch.ones((E, N), dtype=dt, device=DEV), form=form)
    assert (y7[7] == 0).all() and not torch.signbit(y7[7]).any()
    live = ((idx7 >= 0) & (idx7 < E)).to(DEV)
    assert torch.isfinite(y7[live]).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("special", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_row_of_x_gives_nan_in_its_live_slots_only(special, form, dt):
    E, S, K, N, T = 5, 4, 160, 24, 40
    q, s, _ = rand_mx(E, N, K, 45)
    g = torch.Generator().manual_seed(46)
    idx = make_idx(T, S, E, 47)
    idx[9] = torch.tensor([0, -1, 2, 1], dtype=torch.int32)
    live = ((idx >= 0) & (idx < E)).to(DEV)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)  # x per token: all live slots of token 9
    x[9, 77] = special
    y = ext().forward(x, idx.to(DEV), q, s, form=form)
    nan = torch.isnan(y).all(dim=-1)
    want = torch.zeros((T, S), dtype=torch.bool, device=DEV)
    want[9] = live[9]
    assert torch.equal(nan, want) and torch.isfinite(y[~want]).all() and (y[9, 1] == 0).all()
    x = torch.randn((T, S, K), generator=g).to(dt).to(DEV)  # x per pair: that pair only
    x[9, 2, 5] = special
    y = ext().forward(x, idx.to(DEV), q, s, form=form)
    want = torch.zeros((T, S), dtype=torch.bool, device=DEV)
    want[9, 2] = True
    assert torch.equal(torch.isnan(y).all(dim=-1), want) and torch.isfinite(y[~want]).all()


@pytest.mark.parametrize("dt", DTS)
def test_a_nan_block_reaches_only_the_pairs_of_its_expert(dt):
    E, S, K, N, T = 4, 2, 256, 40, 80
    q, s, _ = rand_mx(E, N, K, 51)
    s = s.clone()
    s[2, 3, 1] = 255
    g = torch.Generator().manual_seed(52)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 53)
    idx[0, 0], idx[1, 1] = 2, 2
    on2 = (idx == 2).to(DEV)
    for form in (0, 1):
        y = ext().forward(x, idx.to(DEV), q, s, form=form)
        assert torch.isnan(y[..., 3][on2]).all()
        assert not torch.isnan(y[..., 3][~on2]).any()
        keep = torch.ones(N, dtype=torch.bool, device=DEV)
        keep[3] = False
        assert torch.isfinite(y[..., keep]).all()


# ---- MXFP4A6ExpertsLinearCuda --------------------------------------------------------------------------------------------------------------
def experts_layer(E, N, K, dt, bias=False, seed=0, **kw):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A6ExpertsLinearCuda
    torch.manual_seed(seed)
    return MXFP4A6ExpertsLinearCuda(E, K, N, bias=bias, dtype=dt, **kw).to(DEV)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("blocked", [True, False])
def test_set_mx_weight_in_both_layouts_and_state_dict(blocked, dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A4ExpertsLinearCuda, MXFP4A8ExpertsLinearCuda, MXFP4ExpertsLinearCuda
    E, N, K, T, S = 4, 48, 192, 9, 2
    q, s, W = rand_mx(E, N, K, 61)
    layer = experts_layer(E, N, K, dt, bias=True).eval()
    g = torch.Generator().manual_seed(62)
    with torch.no_grad():
        layer.bias.copy_(torch.randn((E, N), generator=g).to(dt))
    layer.set_mx_weight((q.reshape(E, N, K // 32, 16) if blocked else q).cpu(), s.cpu())  # [E, N, K/32, 16] blocks, or [E, N, K/2]
    assert layer.weight is None and torch.equal(layer.qweight, q) and tuple(layer.qweight.shape) == (E, N, K // 2)
    x = torch.randn((T, K), generator=g).to(dt)
    idx = make_idx(T, S, E, 63)
    y = layer(x.to(DEV), idx.to(DEV))
    yref, a = aref.experts(x, idx, W, layer.bias.detach())
    check(y, yref, a, K, dt, idx, E)
    assert torch.equal(y, ext().forward(x.to(DEV), idx.to(DEV), q, s, layer.bias.detach()))
    assert torch.equal(layer(x.to(DEV), idx.long().to(DEV)), y)  # int64 indices (torch.topk's) are converted
    sd = layer.state_dict()
    assert set(sd) == {"qweight", "scales", "bias"}
    other = experts_layer(E, N, K, dt, bias=True, seed=9).eval()
    other.load_state_dict(sd)
    assert other.weight is None and torch.equal(other(x.to(DEV), idx.to(DEV)), y)
    # the W4A16, W4A4 and W4A8 expert layers load this state dict and give it back
    for cls in (MXFP4ExpertsLinearCuda, MXFP4A4ExpertsLinearCuda, MXFP4A8ExpertsLinearCuda):
        sib = cls(E, K, N, bias=True, dtype=dt).to(DEV).eval()
        sib.load_state_dict(sd)
        assert sib.weight is None and torch.equal(sib.qweight, q)
        back = experts_layer(E, N, K, dt, bias=True, seed=10).eval()
        back.load_state_dict(sib.state_dict())
        assert torch.equal(back(x.to(DEV), idx.to(DEV)), y)


@pytest.mark.parametrize("dt", DTS)
def test_latent_weight_quantises_like_the_restatement_and_round_trips(dt):
    E, N, K, T, S = 3, 33, 96, 6, 2
    layer = experts_layer(E, N, K, dt, bias=True).eval()
    x = torch.randn((T, S, K), device=DEV).to(dt)
    idx = make_idx(T, S, E, 71).to(DEV)
    y0 = layer(x, idx)
    for e in range(E):  # prepare_params from the latent weight: mxfp4_ref.quantize + pack per expert, bit for bit
        codes, scales = aref.quantize(layer.weight[e].detach().cpu())
        assert torch.equal(layer.scales[e].cpu(), scales) and torch.equal(layer.qweight[e].cpu(), aref.pack(codes))
    assert torch.equal(y0, ext().forward(x, idx, layer.qweight, layer.scales, layer.bias.detach()))
    assert torch.equal(ext().dequant(layer.qweight, layer.scales).cpu().double(), aref.dequant(layer.qweight.cpu(), layer.scales.cpu()))
    full = layer.state_dict()
    assert set(full) == {"weight", "qweight", "scales", "bias"}
    layer.generate_quantized_weight(qweight_only=True)
    sd = layer.state_dict()
    assert "weight" not in sd
    fresh = experts_layer(E, N, K, dt, bias=True, seed=4).eval()
    fresh.load_state_dict(sd)
    assert fresh.weight is None and torch.equal(fresh(x, idx), y0)
    back = experts_layer(E, N, K, dt, bias=True, seed=5).eval()
    back.load_state_dict(full)  # a latent weight re-derives qweight / scales
    assert back.weight is not None and torch.equal(back(x, idx), y0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("grad_input", ["torch", "kernel"])
def test_backward_against_float64_autograd_of_the_restatement(grad_input, xpp, dt):
    """Bound: the forward's contract applied to the backward products (mxfp4_a6_ref.tolerance: one rounding to the dtype plus the
    accumulation term on sum|products|; the backward's sums are torch's in fp32, or the input-gradient kernel's).  grad_weight is taken
    at the E2M3-QUANTISED activations, grad_x is the identity through the quantiser: the float64 autograd runs on y = x^ . W^T with
    x^ = x + (fake_quant(x) - x).detach()."""
    E, N, K, T, S = 4, 64, 128, 24, 3
    layer = experts_layer(E, N, K, dt, bias=True, grad_input=grad_input).train()
    g = torch.Generator().manual_seed(81)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV).requires_grad_(True)
    idx = make_idx(T, S, E, 82)
    y = layer(x, idx.to(DEV))
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), idx.to(DEV), q, s, layer.bias.detach()))
    gy = torch.randn(y.shape, generator=g).to(dt).to(DEV)
    y.backward(gy)
    xh = aref.fake_quant(x.detach()).to(DEV)
    Wq = aref.dequant(q, s).to(DEV)

    def grads(absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        x64 = f(x.detach().double()).requires_grad_(True)
        W64 = f(Wq.detach().clone()).requires_grad_(True)
        b64 = f(layer.bias.detach().double()).requires_grad_(True)
        mref.experts(x64 + (f(xh) - x64).detach(), idx, W64, b64)[0].backward(f(gy.double()))
        return x64.grad, W64.grad, b64.grad

    (gx, gw, gb), (ax, aw, ab) = grads(False), grads(True)
    n_pairs = int(torch.bincount(idx[idx >= 0].long(), minlength=E).max())

    def close(got, want, absprod, n):
        tol = aref.tolerance(want, absprod, n, dt)
        assert ((got.double() - want).abs() <= tol).all()

    close(x.grad, gx, ax, N * (1 if xpp else S))
    close(layer.weight.grad, gw, aw, n_pairs)
    close(layer.bias.grad, gb, ab, n_pairs)
    # the weight gradient is NOT the one at the unquantised x
    W64 = Wq.detach().clone().requires_grad_(True)
    gw_plain = torch.autograd.grad(mref.experts(x.detach().double(), idx, W64, None)[0], W64, gy.double())[0]
    assert not ((layer.weight.grad.double() - gw_plain).abs() <= aref.tolerance(gw_plain, aw, n_pairs, dt)).all()
    # eval with the packed weight: differentiable in x and bias
    layer.eval()
    x2 = x.detach().clone().requires_grad_(True)
    layer.bias.grad = None
    layer(x2, idx.to(DEV)).backward(gy)
    assert torch.equal(x2.grad, x.grad) and layer.bias.grad is not None


# ---- MXFP4A6MoECuda ---------------------------------------------------------------------------------------------------------------------
def block_inputs(dt, T, seed=0, H=256, inter=128, E=8, k=2):
    """tests/test_mxfp4_moe_a8_gpu.py's construction: on the CPU, MXFP4 weights of scale codes 122 .. 124 in the checkpoint's
    [E, N, K/32, 16] layout, biases, and x whose first E features hold a permutation of 0, 0.5, ..., (E - 1) / 2 per token, read by an
    identity router: exact logits 0.5 apart, no ties."""
    g = torch.Generator().manual_seed(seed + 1)
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.uint8)  # noqa: E731
    gu_q, gu_s = u8(0, 256, E, 2 * inter, H // 32, 16), u8(122, 125, E, 2 * inter, H // 32)
    d_q, d_s = u8(0, 256, E, H, inter // 32, 16), u8(122, 125, E, H, inter // 32)
    gu_b, d_b = torch.randn((E, 2 * inter), generator=g).to(dt), torch.randn((E, H), generator=g).to(dt)
    rw, x = router_and_x(dt, T, g, H, E)
    ref_args = (x, rw, torch.zeros(E), k, aref.dequant(gu_q.reshape(E, 2 * inter, H // 2), gu_s), gu_b.double(),
                aref.dequant(d_q.reshape(E, H, inter // 2), d_s), d_b.double())
    return (gu_q, gu_s, gu_b, d_q, d_s, d_b), rw, x, ref_args


def router_and_x(dt, T, g, H, E):
    rw = torch.zeros((E, H))
    rw[:, :E] = torch.eye(E)
    x = torch.randn((T, H), generator=g) * 0.5
    x[:, :E] = torch.stack([torch.randperm(E, generator=g) for _ in range(T)]).float() * 0.5
    x = x.to(dt)
    assert x[:, :E].double().sort(dim=-1).values.diff(dim=-1).min().item() >= 0.5
    return rw, x


def set_router(moe, rw, dt):
    with torch.no_grad():
        moe.router.weight.copy_(rw.to(dt))
        moe.router.bias.zero_()


def moe_block(dt, T, seed=0, k=2, cls=None, **kw):
    """The block with the gpt-oss layout loaded through load_gpt_oss_experts (cls: MXFP4MoECuda with its activations for the siblings)."""
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A6MoECuda
    tensors, rw, x, ref_args = block_inputs(dt, T, seed, k=k)
    torch.manual_seed(seed)
    moe = (cls or MXFP4A6MoECuda)(256, 128, 8, k, bias=True, dtype=dt, **kw).to(DEV).eval()
    moe.load_gpt_oss_experts(*tensors)
    set_router(moe, rw, dt)
    return moe, x, ref_args


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 64, 300])
def test_block_is_bit_identical_to_its_public_pieces(T, dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import mxfp4_moe_layer as M, MXFP4A6ExpertsLinearCuda, MXFP4MoECuda
    moe, x, _ = moe_block(dt, T)
    assert type(moe.gate_up) is MXFP4A6ExpertsLinearCuda and type(moe.down) is MXFP4A6ExpertsLinearCuda and moe.activations == "mxfp6"
    assert moe.gate_up.weight is None and moe.down.weight is None
    xd = x.to(DEV)
    with torch.no_grad():
        y = moe(xd)
        w, idx = moe.route(xd)
        v, tidx = torch.topk(moe.router(xd), moe.top_k, dim=-1)
        assert torch.equal(idx, tidx.to(torch.int32)) and torch.equal(w, torch.softmax(v, dim=-1))
        h = moe.gate_up(xd, idx)
        assert torch.equal(h, ext().forward(xd, idx, moe.gate_up.qweight, moe.gate_up.scales, moe.gate_up.bias))
        a = M.swiglu(h, 7.0, 1.702)
        o = moe.down(a, idx)
        assert torch.equal(o, ext().forward(a, idx, moe.down.qweight, moe.down.scales, moe.down.bias))
        want = M.combine(w, o)
    assert y.shape == (T, moe.hidden) and torch.equal(y, want)
    # MXFP4MoECuda's state_dict loads, and back: the same weights, this block's arithmetic
    other = MXFP4MoECuda(256, 128, 8, 2, bias=True, dtype=dt).to(DEV).eval()
    other.load_state_dict(moe.state_dict())
    assert torch.equal(other.gate_up.qweight, moe.gate_up.qweight)
    again = moe_block(dt, T, seed=3)[0]
    again.load_state_dict(other.state_dict())
    with torch.no_grad():
        assert torch.equal(again(xd), y)
    # expert_mask: the slots of the other experts are skipped
    mask = torch.arange(8) % 2 == 0
    moe.set_expert_mask(mask)
    with torch.no_grad():
        _, midx = moe.route(xd)
        ym = moe(xd)
    assert torch.equal(midx, torch.where(mask.to(DEV)[idx.long()], idx, torch.full_like(idx, -1)))
    with torch.no_grad():
        om = ext().forward(a, midx, moe.down.qweight, moe.down.scales, moe.down.bias)
    assert (om[midx < 0] == 0).all() and torch.equal(ym, M.combine(w, om))


@pytest.mark.parametrize("dt", DTS)
def test_block_distance_to_the_float64_variant_restatement(dt):
    """The rule of profiles/mxfp4_moe_block_tolerance.txt on the variant restatement (mxfp4_moe_a6_ref.block, which quantises x and a to
    MXFP6 where the layer does): d = |R_dt - R_64|_F / |R_64|_F recomputed here on the CPU, the bound 2 d.  Measured values:
    profiles/mxfp4_moe_a6_block_tolerance.txt.  The distance of MXFP4MoECuda(activations="mxfp8") (W4A8) on the same weights and x to its
    own restatement is printed beside it and not asserted."""
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4MoECuda
    T = 64
    moe, x, ref_args = moe_block(dt, T)
    y64, idx64 = aref.block(*ref_args)
    ydt, idxdt = aref.block(*ref_args, dt=dt)
    assert torch.equal(idx64, idxdt)
    d = ((ydt - y64).norm() / y64.norm()).item()
    assert 0 < d < 0.1
    with torch.no_grad():
        y = moe(x.to(DEV))
        _, idx = moe.route(x.to(DEV))
    assert torch.equal(idx.cpu().long(), idx64)
    got = ((y.double().cpu() - y64).norm() / y64.norm()).item()
    print(f"mxfp4 a6 moe block {dt}: restatement-with-roundings distance {d:.3e}, bound {2 * d:.3e}, gpu distance {got:.3e}")
    moe8 = moe_block(dt, T, cls=MXFP4MoECuda, activations="mxfp8")[0]
    y8_64, _ = aref.m8.block(*ref_args)
    with torch.no_grad():
        y8 = moe8(x.to(DEV)).double().cpu()
    print(f"mxfp4 a6 moe block {dt}: beside it MXFP4MoECuda mxfp8 (W4A8) to its own restatement {((y8 - y8_64).norm() / y8_64.norm()).item():.3e}; "
          f"W4A6 block to the W4A8 restatement {((y.double().cpu() - y8_64).norm() / y8_64.norm()).item():.3e}, "
          f"W4A6 block to the W4A8 block {((y.double().cpu() - y8).norm() / y8.norm()).item():.3e}")
    assert got <= 2 * d, (got, d)


def ordering_inputs(dt, T=64, H=256, inter=128, E=8, k=2):
    """Gaussian float expert stacks quantised ONCE to MXFP4 (the same weights for every block), biases, the identity router and x: the
    packed tensors on the CPU and the arguments of the restatements on their dequantised values."""
    g = torch.Generator().manual_seed(5)
    Wgu = (torch.randn((E, 2 * inter, H), generator=g) * H ** -0.5).to(dt)
    Wd = (torch.randn((E, H, inter), generator=g) * inter ** -0.5).to(dt)
    bgu, bd = (torch.randn((E, 2 * inter), generator=g) * 0.1).to(dt), (torch.randn((E, H), generator=g) * 0.1).to(dt)
    rw, x = router_and_x(dt, T, g, H, E)
    (gq, gs), (dq, ds) = aref.quantize_packed(Wgu.float()), aref.quantize_packed(Wd.float())
    ref_args = (x, rw, torch.zeros(E), k, aref.dequant(gq, gs), bgu.double(), aref.dequant(dq, ds), bd.double())
    return (gq, gs, bgu, dq, ds, bd), rw, x, ref_args


@pytest.mark.parametrize("dt", DTS)
def test_block_is_closer_to_unquantised_activations_than_the_w4a4_block(dt):
    """On the same MXFP4 weights, MXFP4A6MoECuda's output lies closer than MXFP4MoECuda(activations="mxfp4") to the float64 block with
    UNQUANTISED activations (mxfp4_moe_ref.block on the dequantised weights: no activation quantiser anywhere): E2M3 against E2M1
    activations.  The ordering was first evaluated on the CPU restatements with the roundings of the dtype (mxfp4_moe_a6_ref.block
    against mxfp4_moe_a4_ref.block on ordering_inputs): 4.30e-2 against 2.00e-1 in fp16, 4.38e-2 against 2.03e-1 in bf16 (the W4A8
    restatement: 4.30e-2 / 4.39e-2).  Only the ordering is asserted; the W4A8 block is printed beside it and not asserted."""
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A6MoECuda, MXFP4MoECuda
    T, H, inter, E, k = 64, 256, 128, 8, 2
    tensors, rw, x, ref_args = ordering_inputs(dt, T, H, inter, E, k)
    y64, idx64 = mref.block(*ref_args)
    dist = {}
    for name, cls, kw in (("w4a6", MXFP4A6MoECuda, {}), ("w4a4", MXFP4MoECuda, {"activations": "mxfp4"}), ("w4a8", MXFP4MoECuda, {"activations": "mxfp8"})):
        torch.manual_seed(0)
        moe = cls(H, inter, E, k, bias=True, dtype=dt, **kw).to(DEV).eval()
        moe.load_gpt_oss_experts(*tensors)
        set_router(moe, rw, dt)
        with torch.no_grad():
            y = moe(x.to(DEV))
            _, idx = moe.route(x.to(DEV))
        assert torch.equal(idx.cpu().long(), idx64)
        dist[name] = ((y.double().cpu() - y64).norm() / y64.norm()).item()
    print(f"distance to the float64 block with unquantised activations {dt}: w4a6 {dist['w4a6']:.3e}, w4a4 {dist['w4a4']:.3e}, "
          f"w4a8 (not asserted) {dist['w4a8']:.3e}")
    assert dist["w4a6"] < dist["w4a4"], dist


def _replay_equals_eager(fn, make_x, xd):
    with torch.no_grad():
        eager = fn(xd).clone()  # the warm-up call
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            fn(xd)
        torch.cuda.current_stream().wait_stream(st)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = fn(xd)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        xd.copy_(make_x())
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, fn(xd)) and not torch.equal(out, eager)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 64])
def test_block_graph_replay_equals_eager(T, dt):
    moe, x, _ = moe_block(dt, T, k=4)
    _replay_equals_eager(moe, lambda: moe_block(dt, T, seed=5, k=4)[1].to(DEV), x.to(DEV))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("T", [1, 64])
def test_expert_call_graph_replay_equals_eager(T, form, dt):
    E, S, K, N = 8, 4, 288, 130
    q, s, _ = rand_mx(E, N, K, 91)
    g = torch.Generator().manual_seed(92)
    idx = make_idx(T, S, E, 93).to(DEV)
    e = ext().col_exp(s)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    _replay_equals_eager(lambda t: ext().forward(t, idx, q, s, None, e, form=form), lambda: torch.randn((T, K), generator=g).to(dt).to(DEV), x)
