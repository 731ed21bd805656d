"""MXFP6 W6A16 mixture-of-experts layer on the MI355X: both forms of the expert GEMM against a float64 product per pair within the
weight-only contract's tolerance, bit-identical on exact data (to the rounded float64 product and to mxfp6_linear_cuda.forward per
expert), each form bit-identical to the dense form of the same name on Gaussian data, row independence, skipped and out-of-range
indices, NaN blocks, non-finite rows, the fp16 range of both forms, MXFP6ExpertsLinearCuda (checkpoints, cross-loading with the W6A8
layer, quantiser, both backward modes, graph capture of the frozen backward) and MXFP6A16MoECuda (bit-identical to its public pieces, a
measured distance to the float64 block, graph replay).  The reference is mxfp4_moe_ref.experts / .block on mxfp6_ref.dequant of the
stacked weights; the routing generator (make_idx / assert_coverage) is test_mxfp4_moe_gpu.py's.  Importing this module touches no GPU
(test_mxfp6_moe_cpu.py reads its case lists)."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
BM = 128  # the row tile of the grouped form
DECODE_PAIRS = 1024  # the largest P the decode form exists for
_spec = importlib.util.spec_from_file_location("mxfp6_moe_a8_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp6_moe_a8_ref.py"))
aref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(aref)
mref, m6 = aref.mref, aref.m6  # mxfp4_moe_ref (experts, block: they take W as float64), mxfp6_ref (the format)


def ext():
    from bitorch_engine.extensions import mxfp6_experts_cuda
    return mxfp6_experts_cuda


def lin():
    from bitorch_engine.extensions import mxfp6_linear_cuda
    return mxfp6_linear_cuda


def dequant(q, s):
    """mxfp6_ref.dequant per expert: W float64 [E, N, K] (exact), on the CPU."""
    return aref.dequant(q, s)


_WEIGHTS = {}


def rand_mx(E, N, K, seed, lo=118, hi=130):
    """Random code bytes (every 6-bit code occurs) and scale codes on the GPU, with their float64 W there (cached, never written)."""
    key = (E, N, K, seed, lo, hi)
    if key not in _WEIGHTS:
        g = torch.Generator(device=DEV).manual_seed(seed)
        q = torch.randint(0, 256, (E, N, K // 32 * 24), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        s = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        _WEIGHTS[key] = (q, s, dequant(q, s).to(DEV))
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
        idx[(idx == 0).nonzero()[0]] = 1 if live > 1 else -1  # a single live expert: one skipped slot breaks the whole number of tiles
    return idx.reshape(T, S).to(torch.int32)


def coverage(idx, E):
    """(an expert without pairs, a count that is not a multiple of the row tile, a segment of more than one tile)."""
    flat = idx.reshape(-1).long()
    c = torch.bincount(flat[(flat >= 0) & (flat < E)], minlength=E)
    return bool((c == 0).any()), bool((c % BM != 0).any()), bool((c > BM).any())


def admits_coverage(T, S, E):
    """An empty expert needs E >= 2; a segment of more than one row tile beside a partial one needs P >= BM + 2."""
    return E >= 2 and T * S >= BM + 2


def assert_coverage(idx, E):
    zero, partial, multi = coverage(idx, E)
    assert zero and partial and multi, (zero, partial, multi)


def check(y, yref, absprod, K, dt):
    """The weight-only contract: exact products, an fp32 sum, one rounding to dt."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    tol = eps * yref.abs() + (K + 2) * 2.0 ** -23 * absprod + tiny
    err = (y.double() - yref).abs()
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), f"max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def forms_for(P):
    return (0, 1) if P <= DECODE_PAIRS else (1,)


def case_seed(E, S, K, N):
    return E * 1000 + S * 100 + K + N


def case(E, S, K, N, T, dt, xpp, coverage_case):
    seed = case_seed(E, S, K, N)
    bias_on = (T + N + xpp + (dt == torch.float16)) % 2 == 0  # on and off alternate over the cases
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
        y = ext().forward(x, idx.to(DEV), q, s, bias, e if form else None, form=form)
        assert y.dtype == dt and y.shape == (T, S, N)
        check(y, yref, a, K, dt)
        dead = ((idx < 0) | (idx >= E)).to(DEV)
        assert (y[dead] == 0).all() and not torch.signbit(y[dead]).any()


# (E, S, K, N): one block and one column; three blocks (the last 64-k stage half empty), N below a column group; N not a multiple of C;
# G = 64 with two column tiles, one of a single live column; G = 128; 129 blocks (G = 32 with a padded pass); gpt-oss's K (90 blocks)
SHAPES = [(1, 1, 32, 1), (3, 4, 96, 7), (3, 8, 96, 33), (3, 1, 2048, 129), (3, 2, 4096, 40), (4, 4, 4128, 24), (8, 4, 2880, 160)]
TS = [1, 2, 5, 17, 64, 300]
ALL = [(E, S, K, N, T) for E, S, K, N in SHAPES for T in TS] + [(3, 4, 96, 7, 4096)]  # 16384 pairs: many row tiles per expert
COVERAGE = [c for c in ALL if admits_coverage(c[4], c[1], c[0])]
OTHER = [c for c in ALL if not admits_coverage(c[4], c[1], c[0])]
assert {c[:4] for c in COVERAGE} == set(SHAPES[1:]) and (3, 4, 96, 7, 4096) in COVERAGE


def coverage_idx(E, S, K, N, T):
    """The routing of a coverage case, as case() draws it."""
    return make_idx(T, S, E, case_seed(E, S, K, N) + T)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("E,S,K,N,T", COVERAGE)
def test_both_forms_against_float64_grouped_coverage_cases(E, S, K, N, T, xpp, dt):
    case(E, S, K, N, T, dt, xpp, True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("E,S,K,N,T", OTHER)
def test_both_forms_against_float64_shapes_too_small_for_the_coverage_condition(E, S, K, N, T, xpp, dt):
    case(E, S, K, N, T, dt, xpp, False)


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
    for form in (0, 1, -1):
        y = ext().forward(x, idx.to(DEV), q, s, bias, form=form)
        check(y, yref, a, K, dt)
        assert (y[(idx < 0).to(DEV)] == 0).all() and not torch.signbit(y[(idx < 0).to(DEV)]).any()
        if which == "all_skipped":
            assert (y == 0).all()


def rows_of(x, T, S, K, xpp):
    return (x if xpp else x[:, None, :].expand(T, S, K)).reshape(T * S, K)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("T", [1, 5, 64, 300])
def test_exact_data_is_bit_identical_across_forms_and_to_the_linear_layer(T, xpp, dt):
    E, S, N, K = 4, 4, 72, 4128
    q, s, W = rand_mx(E, N, K, 21, 125, 129)  # scales 2^-2 .. 2^2: every partial sum is a multiple of 2^-5 below 2^19, exact in fp32
    g = torch.Generator().manual_seed(T)
    x = torch.randint(-2, 3, (T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randint(-8, 9, (E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, T)
    yref, _ = mref.experts(x, idx, W, bias)
    want = yref.to(dt)
    xr = rows_of(x, T, S, K, xpp)
    rows = torch.zeros((T * S, N), dtype=dt, device=DEV)
    for e in range(E):  # MXFP6LinearCuda's kernels per expert on that expert's rows, whichever form its plan takes: exact as well
        sel = (idx.reshape(-1) == e).nonzero().reshape(-1).to(DEV)
        if sel.numel():
            rows[sel] = lin().forward(xr[sel].contiguous(), q[e], s[e], bias[e])
    assert torch.equal(rows.reshape(T, S, N), want)
    for form in forms_for(T * S) + (-1,):
        y = ext().forward(x, idx.to(DEV), q, s, bias, form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("K,N", [(4096, 40), (2048, 129), (2880, 33), (4128, 7)])  # G = 128, 64, 32, 32 with a padded pass
def test_routed_decode_form_equals_the_dense_decode_form_bit_for_bit_on_inexact_data(K, N, xpp, dt):
    """Gaussian x, random weights and a bias: the sums round, and a live pair's row still has the bits of MXFP6LinearCuda's decode form
    at M = 1 on its expert, because the block-to-thread map and the order of the sums are the same."""
    E, S, T = 3, 4, 5
    q, s, _ = rand_mx(E, N, K, 71)
    g = torch.Generator().manual_seed(72 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32)
    idx[1, 2] = -1
    y = ext().forward(x, idx.to(DEV), q, s, bias, form=0).reshape(T * S, N)
    xr = rows_of(x, T, S, K, xpp)
    for p, e in enumerate(idx.reshape(-1).tolist()):
        if e < 0:
            assert (y[p] == 0).all()
            continue
        want = lin().forward(xr[p:p + 1].contiguous(), q[e], s[e], bias[e], form=0)[0]
        assert torch.equal(y[p].view(torch.int16), want.view(torch.int16)), (p, e)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_grouped_prefill_form_equals_the_dense_prefill_form_bit_for_bit_on_inexact_data(xpp, dt):
    """Both run the one tile body (mx6_gemm_tile) and a row's sum order is fixed by K alone.  K = 160 is not a whole 64-k stage, N = 130
    gives two column tiles with the second partial, and the routing holds an expert with more than one row tile and a partial one
    beside an expert without pairs."""
    E, S, K, N, T = 3, 2, 160, 130, 70
    q, s, _ = rand_mx(E, N, K, 91)
    g = torch.Generator().manual_seed(92 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 93)
    assert_coverage(idx, E)
    y = ext().forward(x, idx.to(DEV), q, s, bias, form=1)
    xr = rows_of(x, T, S, K, xpp)
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
    perm = torch.randperm(T - 1, generator=g) + 1  # the routing and the rows of every other token permuted, token 0's kept
    idx2, x2 = idx.clone(), x.clone()
    idx2[1:] = idx[perm]
    x2[1:] = x[perm.to(DEV)] * 3
    y2 = ext().forward(x2, idx2.to(DEV), q, s, bias, e, form=form)
    assert torch.equal(y2[0], y[0]) and not torch.equal(y2, y)
    pp = torch.randperm(T, generator=g)  # the pairs in another order: every row moves with its pair
    y4 = ext().forward(x[pp.to(DEV)].contiguous(), idx[pp].to(DEV), q, s, bias, e, form=form)
    assert torch.equal(y4, y[pp.to(DEV)])
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
    bias = torch.randn((E, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 43)
    y = ext().forward(x, idx.to(DEV), q, s, bias, form=form)
    bad = idx.clone()
    vals = torch.tensor([-1, E, 2 ** 31 - 1, -2 ** 31, E + 1000, -7], dtype=torch.int32)
    where = torch.randperm(T * S, generator=g)[:60]
    bad.reshape(-1)[where] = vals[torch.arange(60) % len(vals)]
    m = torch.zeros(T * S, dtype=torch.bool)
    m[where] = True
    m = m.reshape(T, S).to(DEV)
    yb = ext().forward(x, bad.to(DEV), q, s, bias, form=form)
    assert (yb[m] == 0).all() and not torch.signbit(yb[m]).any()
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


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
@pytest.mark.parametrize("form", [0, 1])
def test_a_non_finite_row_of_x_reaches_only_its_own_pairs(form, xpp, dt):
    E, S, K, N, T = 4, 3, 160, 70, 50
    q, s, _ = rand_mx(E, N, K, 55)
    g = torch.Generator().manual_seed(56 + xpp)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt)
    idx = make_idx(T, S, E, 57)
    assert_coverage(idx, E)
    xb = x.clone()
    hit = torch.zeros((T, S), dtype=torch.bool)
    if xpp:
        xb[3, 1, 37], xb[49, 2, 150] = float("nan"), float("inf")
        hit[3, 1] = hit[49, 2] = True
    else:
        xb[3, 37], xb[49, 150] = float("nan"), float("inf")
        hit[3] = hit[49] = True
    y0 = ext().forward(x.to(DEV), idx.to(DEV), q, s, form=form)
    y1 = ext().forward(xb.to(DEV), idx.to(DEV), q, s, form=form)
    live = (idx >= 0)
    assert torch.isfinite(y0).all()
    assert not torch.isfinite(y1[(hit & live).to(DEV)]).any()
    assert torch.equal(y1[(~hit).to(DEV)], y0[(~hit).to(DEV)])
    assert (y1[(hit & ~live).to(DEV)] == 0).all()


@pytest.mark.parametrize("T", [1, 8, 64])
def test_fp16_range_wider_than_an_fp16_image(T):
    """Scale codes up to 143 (|W| > 65504) and small x: the decode form is within the contract (it keeps the fp32 range of W), the prefill
    form within the contract plus the rebias term of test_mxfp6_gpu.py's test of the same name: a weight keeps 2^-24 of its column's
    largest scale."""
    g = torch.Generator().manual_seed(11)
    E, S, N, K = 3, 2, 64, 2048
    q = torch.randint(0, 256, (E, N, K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)
    lo = torch.randint(103, 144, (E, N, 1), generator=g)  # per column a range of scale codes inside 103 .. 143 (2^-24 .. 2^16)
    hi = torch.minimum(lo + torch.randint(0, 41, (E, N, 1), generator=g), torch.tensor(143))
    s = (lo + (torch.rand((E, N, K // 32), generator=g) * (hi - lo + 1)).floor().long()).clamp(103, 143)
    s[0, 0], s[1, 1], s[2, 2] = 143, 103, torch.arange(K // 32) % 41 + 103  # all 2^16, all 2^-24, the whole range within one column
    s = s.to(torch.uint8)
    W = dequant(q, s).to(DEV)
    assert W.abs().max() > 65504
    x = (torch.randn((T, K), generator=g) * 2.0 ** -12).half().to(DEV)
    idx = make_idx(T, S, E + 1, 12)  # experts 0 .. E - 1 all live
    assert int(idx.max()) < E
    yref, a = mref.experts(x, idx, W)
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext().col_exp(sd)
    colmax = m6.mx.e8m0(e.cpu()).to(DEV)[idx.long().to(DEV)]  # [T, S, N]: 2^(e_col - 127) of every pair's expert
    for form in (0, 1):
        y = ext().forward(x, idx.to(DEV), qd, sd, None, e, form=form)
        assert torch.isfinite(y).all()
        rebias = x.double().abs().sum(1)[:, None, None] * colmax * 2.0 ** -24 if form == 1 else 0.0
        tol = 2.0 ** -10 * yref.abs() + (K + 2) * 2.0 ** -23 * a + rebias + 2.0 ** -24
        err = (y.double() - yref).abs()
        assert (err <= tol).all(), (form, err.max().item())


# ---- MXFP6ExpertsLinearCuda ----------------------------------------------------------------------------------------------------------------
def experts_layer(E, N, K, dt, bias=False, seed=0, **kw):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6ExpertsLinearCuda
    torch.manual_seed(seed)
    return MXFP6ExpertsLinearCuda(E, K, N, bias=bias, dtype=dt, **kw).to(DEV)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("blocked", [True, False])
def test_set_mx_weight_in_both_layouts_and_state_dict(blocked, dt):
    E, N, K, T, S = 4, 48, 192, 9, 2
    q, s, W = rand_mx(E, N, K, 61)
    layer = experts_layer(E, N, K, dt, bias=True).eval()
    g = torch.Generator().manual_seed(62)
    with torch.no_grad():
        layer.bias.copy_(torch.randn((E, N), generator=g).to(dt))
    layer.set_mx_weight((q.reshape(E, N, K // 32, 24) if blocked else q).cpu(), s.cpu())  # [E, N, K/32, 24] blocks, or [E, N, 3K/4]
    assert layer.weight is None and torch.equal(layer.qweight, q) and tuple(layer.qweight.shape) == (E, N, 3 * K // 4)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 63)
    y = layer(x, idx.to(DEV))
    yref, a = mref.experts(x, idx, W, layer.bias.detach())
    check(y, yref, a, K, dt)
    assert torch.equal(y, ext().forward(x, idx.to(DEV), q, s, layer.bias.detach()))
    assert torch.equal(layer(x, idx.long().to(DEV)), y)  # int64 indices (torch.topk's) are converted
    sd = layer.state_dict()
    assert set(sd) == {"qweight", "scales", "bias"}
    other = experts_layer(E, N, K, dt, bias=True, seed=9).eval()
    other.load_state_dict(sd)
    assert other.weight is None and torch.equal(other(x, idx.to(DEV)), y)


@pytest.mark.parametrize("dt", DTS)
def test_cross_loads_with_the_w6a8_experts_layer(dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A8ExpertsLinearCuda
    E, N, K, T, S = 3, 40, 96, 7, 2
    torch.manual_seed(3)
    a8 = MXFP6A8ExpertsLinearCuda(E, K, N, bias=True, dtype=dt).to(DEV).eval()
    x = torch.randn((T, K), device=DEV).to(dt)
    idx = make_idx(T, S, E, 64).to(DEV)
    a8(x, idx)  # packs
    for drop in (False, True):  # with the latent weight, and a packed-only checkpoint
        sd = {k: v for k, v in a8.state_dict().items() if not (drop and k == "weight")}
        mine = experts_layer(E, N, K, dt, bias=True, seed=8).eval()
        mine.load_state_dict(sd)
        y = mine(x, idx)
        assert torch.equal(mine.qweight, a8.qweight) and torch.equal(mine.scales, a8.scales) and (mine.weight is None) == drop
        assert torch.equal(y, ext().forward(x, idx, a8.qweight, a8.scales, a8.bias.detach()))
        back = MXFP6A8ExpertsLinearCuda(E, K, N, bias=True, dtype=dt).to(DEV).eval()
        back.load_state_dict(mine.state_dict())
        assert torch.equal(back(x, idx), a8(x, idx))


@pytest.mark.parametrize("dt", DTS)
def test_latent_weight_quantises_like_the_restatement_and_round_trips(dt):
    E, N, K, T, S = 3, 33, 96, 6, 2
    layer = experts_layer(E, N, K, dt, bias=True).eval()
    x = torch.randn((T, S, K), device=DEV).to(dt)
    idx = make_idx(T, S, E, 71).to(DEV)
    y0 = layer(x, idx)
    for e in range(E):  # prepare_params from the latent weight: mxfp6_ref.quantize + pack per expert, bit for bit
        codes, scales = m6.quantize(layer.weight[e].detach().cpu())
        assert torch.equal(layer.scales[e].cpu(), scales) and torch.equal(layer.qweight[e].cpu(), m6.pack(codes))
    assert torch.equal(y0, ext().forward(x, idx, layer.qweight, layer.scales, layer.bias.detach()))
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
@pytest.mark.parametrize("mode", ["torch", "kernel"])
def test_backward_against_float64_autograd_of_the_restatement(mode, xpp, dt):
    """Bound (test_mxfp4_moe_gpu.py's): the forward's contract applied to the backward products (exact products of two dtype values or of
    a dtype value and an MXFP6 weight, an fp32 sum over n terms, one rounding): eps_dt |g| + (n + 2) 2^-23 sum|products| + tiny.
    grad_weight is gy^T . x at the UNQUANTISED x: the float64 autograd runs on y = x . W^T with x as it is."""
    E, N, K, T, S = 4, 64, 128, 24, 3
    layer = experts_layer(E, N, K, dt, bias=True, grad_input=mode).train()
    g = torch.Generator().manual_seed(81)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV).requires_grad_(True)
    idx = make_idx(T, S, E, 82)
    idx[torch.rand((T, S), generator=g) < 0.2] = -1
    y = layer(x, idx.to(DEV))
    q, s = ext().quantize(layer.weight.detach())
    assert int(s.max()) - int(s.min()) <= 11  # the kernel's rebias by e_blk keeps every block exact in fp16 (include/bie_hip.h)
    assert torch.equal(y.detach(), ext().forward(x.detach(), idx.to(DEV), q, s, layer.bias.detach()))
    gy = torch.randn(y.shape, generator=g).to(dt).to(DEV)
    y.backward(gy)
    Wq = dequant(q, s).to(DEV)

    def grads(absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        x64 = f(x.detach().double()).requires_grad_(True)
        W64 = f(Wq.clone()).requires_grad_(True)
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
    # eval with the packed weight: differentiable in x and bias
    layer.eval()
    x2 = x.detach().clone().requires_grad_(True)
    layer.bias.grad = None
    layer(x2, idx.to(DEV)).backward(gy)
    assert x2.grad is not None and layer.bias.grad is not None


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_frozen_kernel_backward_is_captured_in_a_graph(xpp, dt):
    """Frozen packed experts with grad_input="kernel": on exact data grad_x is bit-identical to the "torch" layer's and to float64, and
    forward + backward are captured in a graph (a host synchronisation would fail the capture)."""
    T, S, E, K, N = 40, 2, 4, 96, 40
    q, s, W = rand_mx(E, N, K, 85, 125, 129)
    g = torch.Generator().manual_seed(86)
    x = torch.randint(-2, 3, (T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    gi = torch.randint(-2, 3, (T, S, N), generator=g).to(dt).to(DEV)
    idx = make_idx(T, S, E, 87)
    idx[5, 1] = -1
    idxd = idx.to(DEV)
    layers = {}
    for mode in ("kernel", "torch"):
        layers[mode] = experts_layer(E, N, K, dt, bias=True, grad_input=mode).eval()
        layers[mode].set_mx_weight(q, s)
        layers[mode].bias.requires_grad_(False)

    def grad_x(mode, gout):
        xi = x.clone().requires_grad_(True)
        return torch.autograd.grad(layers[mode](xi, idxd), xi, gout)[0]

    eager = grad_x("kernel", gi)
    assert torch.equal(eager, grad_x("torch", gi))
    x64 = x.double().requires_grad_(True)
    want = torch.autograd.grad(mref.experts(x64, idx, W)[0], x64, gi.double())[0]
    assert torch.equal(eager, want.to(dt))
    xs, gs = x.clone().requires_grad_(True), gi.clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        torch.autograd.grad(layers["kernel"](xs, idxd), xs, gs)
    torch.cuda.current_stream().wait_stream(st)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = torch.autograd.grad(layers["kernel"](xs, idxd), xs, gs)[0]
    g2 = torch.randint(-2, 3, (T, S, N), generator=g).to(dt).to(DEV)
    gs.copy_(g2)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, grad_x("kernel", g2)) and not torch.equal(out, eager)


# ---- MXFP6A16MoECuda -----------------------------------------------------------------------------------------------------------------------
def block_inputs(dt, T, seed=0, H=256, inter=128, E=8, k=2):
    """test_mxfp4_moe_gpu.py's construction with MXFP6 expert tensors: on the CPU, weights of scale codes 122 .. 124 in the
    [E, N, K/32, 24] layout, biases, and x whose first E features hold a permutation of 0, 0.5, ..., (E - 1) / 2 per token, read by an
    identity router: exact logits 0.5 apart, no ties."""
    g = torch.Generator().manual_seed(seed + 1)
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.uint8)  # noqa: E731
    gu_q, gu_s = u8(0, 256, E, 2 * inter, H // 32, 24), u8(122, 125, E, 2 * inter, H // 32)
    d_q, d_s = u8(0, 256, E, H, inter // 32, 24), u8(122, 125, E, H, inter // 32)
    gu_b, d_b = torch.randn((E, 2 * inter), generator=g).to(dt), torch.randn((E, H), generator=g).to(dt)
    rw = torch.zeros((E, H))
    rw[:, :E] = torch.eye(E)
    x = torch.randn((T, H), generator=g) * 0.5
    x[:, :E] = torch.stack([torch.randperm(E, generator=g) for _ in range(T)]).float() * 0.5
    x = x.to(dt)
    assert x[:, :E].double().sort(dim=-1).values.diff(dim=-1).min().item() >= 0.5
    ref_args = (x, rw, torch.zeros(E), k, dequant(gu_q.reshape(E, 2 * inter, H // 32 * 24), gu_s), gu_b.double(),
                dequant(d_q.reshape(E, H, inter // 32 * 24), d_s), d_b.double())
    return (gu_q, gu_s, gu_b, d_q, d_s, d_b), rw, x, ref_args


def moe_block(dt, T, seed=0, k=2):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A16MoECuda
    tensors, rw, x, ref_args = block_inputs(dt, T, seed, k=k)
    torch.manual_seed(seed)
    moe = MXFP6A16MoECuda(256, 128, 8, k, bias=True, dtype=dt).to(DEV).eval()
    moe.load_mx_experts(*tensors)
    with torch.no_grad():
        moe.router.weight.copy_(rw.to(dt))
        moe.router.bias.zero_()
    return moe, x, ref_args


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 64, 300])
def test_block_is_bit_identical_to_its_public_pieces(T, dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import mxfp6_moe_layer as M, MXFP6ExpertsLinearCuda
    moe, x, _ = moe_block(dt, T)
    assert type(moe.gate_up) is MXFP6ExpertsLinearCuda and type(moe.down) is MXFP6ExpertsLinearCuda
    assert moe.gate_up.weight is None and moe.down.weight is None
    xd = x.to(DEV)
    with torch.no_grad():
        y = moe(xd)
        v, idx = torch.topk(moe.router(xd), moe.top_k, dim=-1)
        w = torch.softmax(v, dim=-1)
        idx = idx.to(torch.int32)
        h = ext().forward(xd, idx, moe.gate_up.qweight, moe.gate_up.scales, moe.gate_up.bias)
        a = M.swiglu(h, 7.0, 1.702)
        o = ext().forward(a, idx, moe.down.qweight, moe.down.scales, moe.down.bias)
        want = M.combine(w, o)
    assert y.shape == (T, moe.hidden) and torch.equal(y, want)
    # an expert mask turns foreign experts into skipped slots: the two halves of the experts sum to the whole within three roundings
    mask = torch.arange(moe.num_experts) < moe.num_experts // 2
    with torch.no_grad():
        moe.set_expert_mask(mask)
        _, idx_ = moe.route(xd)
        assert torch.equal(idx_ < 0, ~mask.to(DEV)[idx.long()])
        ya = moe(xd)
        moe.set_expert_mask(~mask)
        yb = moe(xd)
        moe.set_expert_mask(None)
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    assert ((ya.double() + yb.double() - y.double()).abs() <= 3 * eps * (ya.double().abs() + yb.double().abs() + y.double().abs())).all()


@pytest.mark.parametrize("dt", DTS)
def test_block_distance_to_the_float64_restatement(dt):
    """The rule of profiles/mxfp4_moe_block_tolerance.txt: d = |R_dt - R_64|_F / |R_64|_F, where R_dt is the restatement that rounds to
    the dtype at the layer's rounding points, recomputed here on the CPU on this test's own inputs; the bound is 2 d (the GPU sums in
    another order inside the same rounding points).  Measured values: profiles/mxfp6_moe_block_tolerance.txt."""
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
    print(f"mxfp6 a16 moe block {dt}: restatement-with-roundings distance {d:.3e}, bound {2 * d:.3e}, gpu distance {got:.3e}")
    assert got <= 2 * d, (got, d)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 64])
def test_block_graph_replay_equals_eager(T, dt):
    moe, x, _ = moe_block(dt, T, k=4)
    xd = x.to(DEV)
    with torch.no_grad():
        eager = moe(xd).clone()  # the warm-up call
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
        xd.copy_(moe_block(dt, T, seed=5, k=4)[1].to(DEV))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, moe(xd)) and not torch.equal(out, eager)
