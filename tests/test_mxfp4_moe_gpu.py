"""MXFP4 mixture-of-experts layer on the MI355X: both forms of the expert GEMM against a float64 product per pair within the MXFP4 linear
contract's tolerance, bit-identical on exact data (to the rounded float64 product and to mxfp4_linear_cuda.forward row by row), row
independence, skipped and out-of-range indices, NaN blocks, the fp16 range of the decode form, MXFP4ExpertsLinearCuda (checkpoints,
quantiser, backward) and MXFP4MoECuda (bit-identical to its public pieces, a measured distance to the float64 block, graph replay)."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
BM = 128  # the row tile of the grouped form
DECODE_PAIRS = 1024  # the largest P the decode form exists for
_spec = importlib.util.spec_from_file_location("mxfp4_moe_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_moe_ref.py"))
mref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mref)
ref = mref.ref


def ext():
    from bitorch_engine.extensions import mxfp4_experts_cuda
    return mxfp4_experts_cuda


def lin():
    from bitorch_engine.extensions import mxfp4_linear_cuda
    return mxfp4_linear_cuda


_WEIGHTS = {}


def rand_mx(E, N, K, seed, lo=118, hi=130):
    """Random codes and scale codes on the GPU, with their float64 W (cached: the large stacks are shared by many cases)."""
    key = (E, N, K, seed, lo, hi)
    if key not in _WEIGHTS:
        if E * N * K > 1 << 24:
            _WEIGHTS.clear()  # one large stack at a time
        g = torch.Generator(device=DEV).manual_seed(seed)
        q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        s = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        _WEIGHTS[key] = (q, s, mref.dequant(q, s))
    return _WEIGHTS[key]


def make_idx(T, S, E, seed):
    """Zipf-skewed routing with a fixed seed and planted rows: the last expert gets no pair (E >= 2), expert 0 more than one row tile
    and not a whole number of tiles (P >= BM + 2)."""
    g = torch.Generator().manual_seed(seed)
    P = T * S
    live = max(E - 1, 1)
    prob = 1.0 / torch.arange(1, live + 1, dtype=torch.float64) ** 1.2
    idx = torch.multinomial(prob / prob.sum(), P, replacement=True, generator=g)
    if P >= BM + 2:
        idx[torch.randperm(P, generator=g)[:BM + 2]] = 0
    if int((idx == 0).sum()) % BM == 0 and (idx == 0).any():
        idx[(idx == 0).nonzero()[0]] = 1 if live > 1 else -1  # a single expert: one skipped slot breaks the whole number of tiles
    return idx.reshape(T, S).to(torch.int32)


def coverage(idx, E):
    """(an expert without pairs, a count that is not a multiple of the row tile, a segment of more than one tile)."""
    flat = idx.reshape(-1).long()
    c = torch.bincount(flat[(flat >= 0) & (flat < E)], minlength=E)
    return bool((c == 0).any()), bool((c % BM != 0).any()), bool((c > BM).any())


def admits_coverage(T, S, E):
    """Whether a shape can hold the grouped form's routing condition at all: an empty expert needs E >= 2, a segment of more than one
    row tile beside a partial one needs P >= BM + 2.  The issue's shape list also holds E = 1 and P down to 1, which cannot."""
    return E >= 2 and T * S >= BM + 2


def assert_coverage(idx, E):
    """The routing condition of the grouped form, asserted on the CPU before the GPU call: an expert without pairs, a count that is not a
    multiple of the row tile and a segment of more than one tile."""
    zero, partial, multi = coverage(idx, E)
    assert zero and partial and multi, (zero, partial, multi)


def check(y, yref, absprod, K, dt):
    """The contract of tests/test_mxfp4_gpu.py: exact or once-rounded products, an fp32 sum, one rounding to dt."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    tol = eps * yref.abs() + (K + 2) * 2.0 ** -23 * absprod + tiny
    err = (y.double() - yref).abs()
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), f"max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def forms_for(P):
    return (0, 1) if P <= DECODE_PAIRS else (1,)


def case(E, S, K, N, T, dt, xpp, bias_on, seed, coverage_case):
    q, s, W = rand_mx(E, N, K, seed)
    g = torch.Generator().manual_seed(seed + 17 * T + xpp)
    x = (torch.randn((T, S, K) if xpp else (T, K), generator=g) * 0.5).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV) if bias_on else None
    idx = make_idx(T, S, E, seed + T)
    if coverage_case:
        assert_coverage(idx, E)
    yref, a = mref.experts(x, idx, W, bias)
    e = ext().col_exp(s)
    for form in forms_for(T * S):
        y = ext().forward(x, idx.to(DEV), q, s, bias, e, form=form)
        assert y.dtype == dt and y.shape == (T, S, N)
        check(y, yref, a, K, dt)


TS = [1, 2, 5, 16, 17, 64, 300, 4096]
SMALL = [(1, 1, 32, 1), (3, 4, 96, 7), (3, 8, 96, 33), (1, 8, 32, 33), (3, 1, 96, 1), (3, 4, 32, 7)]
GPT_OSS = [(32, 4, 2880, 5760), (32, 4, 2880, 2880)]
ALL = [(E, S, K, N, T) for E, S, K, N in SMALL + GPT_OSS for T in TS]
# The grouped form's coverage cases are the shapes that can hold the routing condition; the condition is asserted for every one of them.
# The other shapes of the list (a single expert, or fewer than BM + 2 pairs) run both forms too, without that claim.
COVERAGE = [c for c in ALL if admits_coverage(c[4], c[1], c[0])]
OTHER = [c for c in ALL if not admits_coverage(c[4], c[1], c[0])]
assert {c[:4] for c in COVERAGE} >= set(GPT_OSS) | {(3, 4, 96, 7), (3, 8, 96, 33), (3, 1, 96, 1)} and {c[4] for c in COVERAGE} >= {17, 64, 300, 4096}


def run_case(E, S, K, N, T, xpp, dt, coverage_case):
    big = K == 2880
    bias_on = (T + xpp + (dt == torch.float16)) % 2 == 0 if big else (T + N + xpp) % 2 == 0  # on and off alternate over the cases
    case(E, S, K, N, T, dt, xpp, bias_on, seed=N if big else E * 1000 + S * 100 + K + N, coverage_case=coverage_case)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("E,S,K,N,T", COVERAGE)
def test_both_forms_against_float64_grouped_coverage_cases(E, S, K, N, T, xpp, dt):
    run_case(E, S, K, N, T, xpp, dt, True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("E,S,K,N,T", OTHER)
def test_both_forms_against_float64_shapes_too_small_for_the_coverage_condition(E, S, K, N, T, xpp, dt):
    run_case(E, S, K, N, T, xpp, dt, False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("which", ["one_expert", "all_skipped", "mixed"])
def test_degenerate_routings(which, dt):
    E, S, K, N, T = 5, 4, 96, 130, 70
    q, s, W = rand_mx(E, N, K, 3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    if which == "one_expert":
        idx = torch.full((T, S), 3, dtype=torch.int32)
    elif which == "all_skipped":
        idx = torch.full((T, S), -1, dtype=torch.int32)
    else:
        idx = make_idx(T, S, E, 5)
        idx[torch.rand((T, S), generator=g) < 0.4] = -1
        assert (idx == -1).any() and (idx >= 0).any()
    yref, a = mref.experts(x, idx, W, bias)
    for form in (0, 1):
        y = ext().forward(x, idx.to(DEV), q, s, bias, form=form)
        check(y, yref, a, K, dt)
        assert (y[(idx < 0).to(DEV)] == 0).all() and not torch.signbit(y[(idx < 0).to(DEV)]).any()
        if which == "all_skipped":
            assert (y == 0).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("T", [1, 5, 16, 64, 300])
def test_exact_data_is_bit_identical_across_forms_and_to_the_linear_layer(T, xpp, dt):
    E, S, N, K = 4, 4, 72, 4096
    q, s, W = rand_mx(E, N, K, 21, 125, 129)  # scales 2^-2 .. 2^2: every partial sum is a multiple of 2^-3 below 2^21, exact in fp32
    g = torch.Generator().manual_seed(T)
    x = torch.randint(-2, 3, (T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randint(-8, 9, (E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, T)
    yref, _ = mref.experts(x, idx, W, bias)
    want = yref.to(dt)
    # the linear layer on every pair's row with its expert's weights, called once per expert on that expert's rows: a batch beyond 16 rows
    # takes the linear layer's prefill form, which on this data is exact as well, so the comparison is bit for bit whichever form it takes
    xr = (x if xpp else x[:, None, :].expand(T, S, K)).reshape(T * S, K)
    rows = torch.empty((T * S, N), dtype=dt, device=DEV)
    for e in range(E):
        sel = (idx.reshape(-1) == e).nonzero().reshape(-1).to(DEV)
        if sel.numel():
            rows[sel] = lin().forward(xr[sel].contiguous(), q[e], s[e], bias[e])
    assert torch.equal(rows.reshape(T, S, N), want)
    for form in forms_for(T * S) + (-1,):
        y = ext().forward(x, idx.to(DEV), q, s, bias, form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
# (32, 1): two units, 254 idle threads; (96, 7): N is no multiple of C = 4, the clamped reads; (4128, 33): 258 units, two threads take a
# second trip; (2880, 33): gpt-oss's K
@pytest.mark.parametrize("K,N", [(32, 1), (96, 7), (4128, 33), (2880, 33)])
def test_routed_decode_form_equals_the_dense_decode_form_bit_for_bit_on_inexact_data(K, N, xpp, dt):
    """Gaussian x, random weights and a bias: the sums round, and a live pair's row still has the bits of MXFP4LinearCuda's decode form
    at M = 1 on its expert, because the unit-to-thread map and the order of the sums are the same.  A skipped pair's row is +0."""
    E, S, T = 3, 2, 5
    q, s, _ = rand_mx(E, N, K, 71)
    g = torch.Generator().manual_seed(72 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32)
    idx[1, 1], idx[3, 0] = -1, E
    y = ext().forward(x, idx.to(DEV), q, s, bias, form=0).reshape(T * S, N)
    xr = (x if xpp else x[:, None, :].expand(T, S, K)).reshape(T * S, K)
    for p, e in enumerate(idx.reshape(-1).tolist()):
        if not 0 <= e < E:
            assert (y[p].view(torch.int16) == 0).all(), (p, e)  # +0: no sign bit
            continue
        want = lin().forward(xr[p:p + 1].contiguous(), q[e], s[e], bias[e], form=0)[0]
        assert torch.equal(y[p].view(torch.int16), want.view(torch.int16)), (p, e)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_grouped_prefill_form_equals_the_dense_prefill_form_bit_for_bit_on_inexact_data(xpp, dt):
    """Random normal x, random weights and a bias: the sums round, and the grouped prefill form still gives the bits of the linear
    layer's prefill form called once per expert on that expert's rows, because both run the one tile body (mx_gemm_tile) and a row's
    sum order is fixed by K alone.  K = 160 is not a whole 64-k stage, N = 130 gives two column tiles with the second partial, and the
    routing holds an expert with more than one row tile and a partial one beside an expert without pairs."""
    E, S, K, N, T = 3, 2, 160, 130, 70
    q, s, _ = rand_mx(E, N, K, 91)
    g = torch.Generator().manual_seed(92 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 93)
    assert_coverage(idx, E)
    y = ext().forward(x, idx.to(DEV), q, s, bias, form=1)
    xr = (x if xpp else x[:, None, :].expand(T, S, K)).reshape(T * S, K)
    rows = torch.zeros((T * S, N), dtype=dt, device=DEV)  # a skipped slot is +0
    for e in range(E):
        sel = (idx.reshape(-1) == e).nonzero().reshape(-1).to(DEV)
        if sel.numel():
            rows[sel] = lin().forward(xr[sel].contiguous(), q[e], s[e], bias[e], form=1)
    assert torch.equal(y.view(torch.int16), rows.reshape(T, S, N).view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", [0, 1])
def test_a_row_depends_on_its_own_pair_only(form, dt):
    E, S, K, N, T = 8, 4, 256, 130, 60
    q, s, _ = rand_mx(E, N, K, 31)
    g = torch.Generator().manual_seed(32)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 33)
    e = ext().col_exp(s)
    y = ext().forward(x, idx.to(DEV), q, s, bias, e, form=form)
    assert torch.equal(y, ext().forward(x, idx.to(DEV), q, s, bias, e, form=form))  # two identical calls
    for t, sl in ((0, 0), (7, 3), (59, 1)):  # the pair in a call of its own
        alone = ext().forward(x[t:t + 1], idx[t:t + 1, sl:sl + 1].to(DEV), q, s, bias, e, form=form)
        assert torch.equal(alone[0, 0], y[t, sl])
    perm = torch.randperm(T - 1, generator=g) + 1  # the routing of every other token permuted, token 0's kept
    idx2 = idx.clone()
    idx2[1:] = idx[perm]
    y2 = ext().forward(x, idx2.to(DEV), q, s, bias, e, form=form)
    assert torch.equal(y2[0], y[0]) and not torch.equal(y2, y)
    skip = torch.rand((T, S), generator=g) < 0.5  # live rows beside skipped slots
    idx3 = torch.where(skip, torch.full_like(idx, -1), idx)
    y3 = ext().forward(x, idx3.to(DEV), q, s, bias, e, form=form)
    assert torch.equal(y3[~skip.to(DEV)], y[~skip.to(DEV)]) and (y3[skip.to(DEV)] == 0).all()


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
    assert (yb[m] == 0).all()
    assert torch.equal(yb[~m], y[~m])


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


@pytest.mark.parametrize("T", [1, 8, 64])
def test_decode_form_keeps_the_fp32_range_of_the_weights(T):
    g = torch.Generator(device=DEV).manual_seed(11)
    E, S, N, K = 3, 2, 64, 2048
    q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
    s = torch.randint(103, 144, (E, N, K // 32), generator=g, dtype=torch.int32, device=DEV)  # 2^-24 .. 2^16
    s[0, 0], s[1, 1] = 143, 103
    s = s.to(torch.uint8)
    W = mref.dequant(q, s)
    assert W.abs().max() > 65504
    x = (torch.randn((T, K), generator=g, device=DEV) * 2.0 ** -12).half()
    idx = make_idx(T, S, E, 12)
    yref, a = mref.experts(x, idx, W)
    y = ext().forward(x, idx.to(DEV), q, s, form=0)
    assert torch.isfinite(y).all()
    tol = 2.0 ** -10 * yref.abs() + (K + 2) * 2.0 ** -23 * a + 2.0 ** -24
    assert ((y.double() - yref).abs() <= tol).all()


# ---- MXFP4ExpertsLinearCuda ----------------------------------------------------------------------------------------------------------------
def experts_layer(E, N, K, dt, bias=False, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4ExpertsLinearCuda
    torch.manual_seed(seed)
    return MXFP4ExpertsLinearCuda(E, K, N, bias=bias, dtype=dt).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_set_mx_weight_checkpoint_layout_and_state_dict(dt):
    E, N, K, T, S = 4, 48, 192, 9, 2
    q, s, W = rand_mx(E, N, K, 61)
    layer = experts_layer(E, N, K, dt, bias=True).eval()
    g = torch.Generator().manual_seed(62)
    with torch.no_grad():
        layer.bias.copy_(torch.randn((E, N), generator=g).to(dt))
    layer.set_mx_weight(q.reshape(E, N, K // 32, 16).cpu(), s.cpu())  # the checkpoint's [E, N, K/32, 16] blocks
    assert layer.weight is None and torch.equal(layer.qweight, q)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 63)
    y = layer(x, idx.to(DEV))
    yref, a = mref.experts(x, idx, W, layer.bias.detach())
    check(y, yref, a, K, dt)
    assert torch.equal(layer(x, idx.long().to(DEV)), y)  # int64 indices (torch.topk's) are converted
    sd = layer.state_dict()
    assert set(sd) == {"qweight", "scales", "bias"}
    other = experts_layer(E, N, K, dt, bias=True, seed=9).eval()
    other.load_state_dict(sd)
    assert other.weight is None and torch.equal(other(x, idx.to(DEV)), y)


@pytest.mark.parametrize("dt", DTS)
def test_latent_weight_quantises_like_the_restatement_and_round_trips(dt):
    E, N, K, T, S = 3, 33, 96, 6, 2
    layer = experts_layer(E, N, K, dt, bias=True).eval()
    x = torch.randn((T, S, K), device=DEV).to(dt)
    idx = make_idx(T, S, E, 71).to(DEV)
    y0 = layer(x, idx)
    for e in range(E):  # prepare_params from the latent weight: ref.quantize per expert, bit for bit
        codes, scales = ref.quantize(layer.weight[e].detach().cpu())
        assert torch.equal(layer.scales[e].cpu(), scales) and torch.equal(layer.qweight[e].cpu(), ref.pack(codes))
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
    assert torch.equal(back(x, idx), y0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_backward_against_float64_autograd_of_the_restatement(xpp, dt):
    """Bound: the forward's contract applied to the backward products (exact products of two dtype values or of a dtype value and an
    MXFP4 weight, an fp32 sum over n terms, one rounding): eps_dt |g| + (n + 2) 2^-23 sum|products| + tiny."""
    E, N, K, T, S = 4, 64, 128, 24, 3
    layer = experts_layer(E, N, K, dt, bias=True).train()
    g = torch.Generator().manual_seed(81)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV).requires_grad_(True)
    idx = make_idx(T, S, E, 82)
    idx[torch.rand((T, S), generator=g) < 0.2] = -1
    y = layer(x, idx.to(DEV))
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), idx.to(DEV), q, s, layer.bias.detach()))
    gy = torch.randn(y.shape, generator=g).to(dt).to(DEV)
    y.backward(gy)

    def grads(absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        x64 = f(x.detach().double()).requires_grad_(True)
        W64 = f(mref.dequant(q, s)).requires_grad_(True)
        b64 = f(layer.bias.detach().double()).requires_grad_(True)
        mref.experts(x64, idx, W64, b64)[0].backward(f(gy.double()))
        return x64.grad, W64.grad, b64.grad

    (gx, gw, gb), (ax, aw, ab) = grads(False), grads(True)
    n_pairs = int(torch.bincount(idx[idx >= 0].long(), minlength=E).max())
    check(x.grad, gx, ax, N * (1 if xpp else S), dt)
    check(layer.weight.grad, gw, aw, n_pairs, dt)
    check(layer.bias.grad, gb, ab, n_pairs, dt)
    assert (layer.weight.grad[E - 1] == 0).all()  # make_idx leaves the last expert without pairs
    before = layer(x, idx.to(DEV)).detach()
    torch.optim.SGD(layer.parameters(), lr=0.5).step()
    assert not torch.equal(layer(x, idx.to(DEV)).detach(), before)


# ---- MXFP4MoECuda --------------------------------------------------------------------------------------------------------------------------
def block_inputs(dt, T, seed=0, H=256, inter=128, E=8, k=2):
    """On the CPU: MXFP4 expert weights of scale codes 122 .. 124 (h and o of order 1), biases, and x whose first E features hold a
    permutation of 0, 0.5, ..., (E - 1) / 2 per token.  The router reads those features through an identity, so the logits are exact
    in every precision and 0.5 apart: top-k has no ties (asserted here)."""
    g = torch.Generator().manual_seed(seed + 1)
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.uint8)  # noqa: E731
    gu_q, gu_s = u8(0, 256, E, 2 * inter, H // 32, 16), u8(122, 125, E, 2 * inter, H // 32)
    d_q, d_s = u8(0, 256, E, H, inter // 32, 16), u8(122, 125, E, H, inter // 32)
    gu_b, d_b = torch.randn((E, 2 * inter), generator=g).to(dt), torch.randn((E, H), generator=g).to(dt)
    rw = torch.zeros((E, H))
    rw[:, :E] = torch.eye(E)
    x = torch.randn((T, H), generator=g) * 0.5
    x[:, :E] = torch.stack([torch.randperm(E, generator=g) for _ in range(T)]).float() * 0.5
    x = x.to(dt)
    if E > 1:
        assert x[:, :E].double().sort(dim=-1).values.diff(dim=-1).min().item() >= 0.5
    ref_args = (x, rw, torch.zeros(E), k, mref.dequant(gu_q.reshape(E, 2 * inter, H // 2), gu_s), gu_b.double(),
                mref.dequant(d_q.reshape(E, H, inter // 2), d_s), d_b.double())
    return (gu_q, gu_s, gu_b, d_q, d_s, d_b), rw, x, ref_args


def moe_block(dt, T, seed=0, H=256, inter=128, E=8, k=2):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4MoECuda
    tensors, rw, x, ref_args = block_inputs(dt, T, seed, H, inter, E, k)
    torch.manual_seed(seed)
    moe = MXFP4MoECuda(H, inter, E, k, bias=True, dtype=dt).to(DEV).eval()
    moe.load_gpt_oss_experts(*tensors)
    with torch.no_grad():
        moe.router.weight.copy_(rw.to(dt))
        moe.router.bias.zero_()
    return moe, x, ref_args


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 64, 300])
def test_block_is_bit_identical_to_its_public_pieces(T, dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import mxfp4_moe_layer as M
    moe, x, _ = moe_block(dt, T)
    xd = x.to(DEV)
    with torch.no_grad():
        y = moe(xd)
        v, idx = torch.topk(moe.router(xd), moe.top_k, dim=-1)
        w = torch.softmax(v, dim=-1)
        idx = idx.to(torch.int32)
        h = ext().forward(xd, idx, moe.gate_up.qweight, moe.gate_up.scales, moe.gate_up.bias)
        gf, uf = h[..., 0::2].float(), h[..., 1::2].float()
        gf = gf.clamp(max=7.0)
        a = ((uf.clamp(min=-7.0, max=7.0) + 1.0) * (gf * torch.sigmoid(1.702 * gf))).to(dt)
        assert torch.equal(a, M.swiglu(h, 7.0, 1.702))
        o = ext().forward(a, idx, moe.down.qweight, moe.down.scales, moe.down.bias)
        want = (w.float()[..., None] * o.float()).sum(dim=1).to(dt)
    assert y.shape == (T, moe.hidden) and torch.equal(y, want)
    # an expert mask turns foreign experts into skipped slots: the two halves of the experts sum to the whole (up to the one rounding each)
    mask = torch.arange(moe.num_experts) < moe.num_experts // 2
    with torch.no_grad():
        moe.set_expert_mask(mask)
        w_, idx_ = moe.route(xd)
        assert torch.equal(idx_ < 0, ~mask.to(DEV)[idx.long()])
        ya = moe(xd)
        moe.set_expert_mask(~mask)
        yb = moe(xd)
        moe.set_expert_mask(None)
    assert ((ya.double() + yb.double() - y.double()).abs() <= 3 * (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7) * (ya.double().abs() + yb.double().abs() + y.double().abs())).all()


@pytest.mark.parametrize("dt", DTS)
def test_block_distance_to_the_float64_restatement(dt):
    """Norm-wise bound, measured and not chosen: d = |R_dt - R_64|_F / |R_64|_F, where R_dt is the restatement that rounds to the dtype at
    the layer's rounding points, on this test's own inputs on the CPU; the bound is 2 d (the GPU sums in another order inside the same
    rounding points).  Measured (profiles/mxfp4_moe_block_tolerance.txt): d = 4.96e-04 (fp16), 4.19e-03 (bf16); bounds 9.91e-04, 8.39e-03."""
    T = 64
    moe, x, ref_args = moe_block(dt, T)
    y64, idx64 = mref.block(*ref_args)
    ydt, idxdt = mref.block(*ref_args, dt=dt)
    assert torch.equal(idx64, idxdt)
    d = ((ydt - y64).norm() / y64.norm()).item()
    assert 0 < d < 0.05
    with torch.no_grad():
        y = moe(x.to(DEV))
        _, idx = moe.route(x.to(DEV))
    assert torch.equal(idx.cpu().long(), idx64)
    got = ((y.double().cpu() - y64).norm() / y64.norm()).item()
    print(f"mxfp4 moe block {dt}: restatement-with-roundings distance {d:.3e}, bound {2 * d:.3e}, gpu distance {got:.3e}")
    assert got <= 2 * d, (got, d)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 64])
def test_block_graph_replay_equals_eager(T, dt):
    moe, x, _ = moe_block(dt, T, k=4)
    xd = x.to(DEV)
    with torch.no_grad():
        eager = moe(xd)  # the warm-up call
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            moe(xd)
        torch.cuda.current_stream().wait_stream(st)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = moe(xd)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        _, x2, _ = moe_block(dt, T, seed=5, k=4)
        xd.copy_(x2.to(DEV))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, moe(xd)) and not torch.equal(out, eager)
