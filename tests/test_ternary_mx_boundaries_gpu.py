"""The ternary linear, ternary conv2d, ternary W1.58A8 and MXFP4 kernels on both sides of every form boundary the host code draws: decode
grids wider than one 16-column sweep (N > 16384), the last K inside each decode form's LDS bound and the first K past it, the A8 GEMM's
256 x 256 tile switch, every MXFP4 decode row bucket and its column tails, the conv forms' OW / pixel / channel bounds, and the sign and
scale edges (exact cancellation, -0, NaN, +-inf).  Each case runs every form that accepts it against the references of the fixed-shape
tests, through the checks of tests/sweeps/fuzz_ternary_mx.py.  tests/test_ternary_mx_boundaries_cpu.py checks that the shapes below
really straddle the host predicates."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda"
ROW_KINDS = ["normal", "zero", "dominant", "subnormal", "extreme", "spread", "normal", "spread"]

# (M, N, K, forms the case must run).  The CPU guard asserts the same forms from the host predicates.
TERN_CASES = [(M, N, 256, {"mfma", "decode_wide" if N > 16384 else "decode"}) for M in (1, 4) for N in (16384, 16385, 28672, 32000)] + \
             [(1, 40, 131040, {"mfma", "decode"}), (4, 40, 131040, {"mfma", "decode"}), (1, 40, 131072, {"mfma"}), (4, 40, 131072, {"mfma"})]
TA8_CASES = [(M, 33, K, {"gemm128", f"decode{M}"}) for M, K in ((1, 64512), (2, 32256), (4, 16128), (8, 8064))] + \
            [(M, 33, K + 32, {"gemm128"}) for M, K in ((1, 64512), (2, 32256), (4, 16128), (8, 8064))] + \
            [(M, 40, 8064, {"gemm128", "decode8"}) for M in (5, 6, 7, 8)] + \
            [(M, N, 128, {"gemm128", f"decode{M}", "decode_wide"}) for M in (1, 8) for N in (16385, 32000)] + \
            [(2048, 5888, 64, {"gemm128"}), (2048, 6144, 64, {"gemm256"}), (3000, 4100, 96, {"gemm256"})]
MX_NS = (1, 3, 4, 5, 7, 8, 9, 4097)
# (B, C, H, W, OC, k, stride, pad, form INTEGRATION.md gives it)
TCONV_CASES = [(1, 128, 2, 64, 64, 3, 1, 1, 1), (1, 128, 2, 65, 64, 3, 1, 1, 2),      # OW 64 / 65: the VALU form's bound
               (1, 512, 2, 64, 64, 3, 1, 1, 1), (1, 512, 2, 65, 64, 3, 1, 1, 2),
               (1, 64, 2, 128, 64, 3, 1, 1, 2), (1, 64, 2, 129, 64, 3, 1, 1, 0),      # OW 128 / 129: the matrix-pipe form's bound
               (1, 128, 112, 7, 64, 3, 1, 1, 1), (1, 128, 157, 5, 64, 3, 1, 1, 2),    # 784 / 785 output pixels: the choice between them
               (16, 128, 7, 7, 64, 1, 1, 0, 1), (157, 128, 1, 5, 64, 1, 1, 0, 2),
               (1, 512, 7, 7, 64, 3, 1, 1, 1), (1, 544, 7, 7, 64, 3, 1, 1, 0)]        # C 512 / 544


def fz():
    import fuzz_ternary_mx
    return fuzz_ternary_mx


DT_NAMES = ["f16", "bf16", "f32"]


@pytest.mark.parametrize("M,N,K,forms", TERN_CASES)
def test_ternary_linear_decode_grid_and_lds_bounds(M, N, K, forms):
    for i, x in enumerate(("normal", "ties", "zeros", "nonfinite")):
        c = dict(op="tern", M=M, N=N, K=K, dt=DT_NAMES[i % 3], x=x, bias=i != 2, seed=M * 7 + N + K + i)
        assert set(fz().run_tern(c)) == forms, c


@pytest.mark.parametrize("M,N,K,forms", TA8_CASES)
def test_ternary_a8_decode_lds_bounds_wide_grids_and_gemm_tiles(M, N, K, forms):
    dts = DT_NAMES if M * N <= 4096 * 1024 else ["bf16"]
    for i, dt in enumerate(dts):
        c = dict(op="ta8", M=M, N=N, K=K, dt=dt, seed=M + N + K + i, rows=ROW_KINDS[i:i + min(M, 6)])
        assert set(fz().run_ta8(c)) == forms, c


@pytest.mark.parametrize("M", list(range(1, 18)))
def test_mxfp4_every_decode_bucket_and_column_tail(M):
    for N in MX_NS:
        for i, mode in enumerate(("narrow", "exact", "wide")):
            c = dict(op="mx", M=M, N=N, K=96 if N == 4097 else 160, dt=("f16", "bf16")[(N + i) % 2], scales=mode, bias=bool((M + N + i) % 2),
                     seed=M * 100 + N + i)
            assert set(fz().run_mx(c)) == set(fz().forms_of("mx", c)) and len(fz().forms_of("mx", c)) == (2 if M <= 16 else 1)


@pytest.mark.parametrize("M,N", [(200, N) for N in (127, 128, 129, 257)] + [(M, N) for M in (1, 9, 16, 200) for N in (5, 132)])
@pytest.mark.parametrize("K", [32, 64, 96, 160, 4128])
def test_mxfp4_prefill_tiles_and_k_tails(M, N, K):
    for i, mode in enumerate(("narrow", "exact", "wide")):
        c = dict(op="mx", M=M, N=N, K=K, dt=("f16", "bf16")[(K + i) % 2], scales=mode, bias=bool(i % 2), seed=M + N + K + i)
        fz().run_mx(c)


def test_mxfp4_largest_k():
    """K = 2^20, the contract's upper bound, at M = 1 on both forms."""
    for dt in ("f16", "bf16"):
        c = dict(op="mx", M=1, N=5, K=1 << 20, dt=dt, scales="narrow", bias=True, seed=20)
        assert set(fz().run_mx(c)) == {"decode1", "prefill"}


@pytest.mark.parametrize("B,C,H,W,OC,k,st,pad,form", TCONV_CASES)
def test_ternary_conv_form_bounds(B, C, H, W, OC, k, st, pad, form):
    from bitorch_engine.extensions import ternary_conv2d_cuda
    assert ternary_conv2d_cuda.form(B, C, H, W, OC, k, st, pad, 1) == form
    for i, dt in enumerate(DT_NAMES):
        c = dict(op="tconv", B=B, C=C, H=H, W=W, OC=OC, k=k, st=st, pad=pad, dil=1, dt=dt, seed=B + C + H + W + i)
        ran = fz().run_tconv(c)
        assert fz().TCONV_FORMS[form] in ran, (ran, c)


# ---- special values ------------------------------------------------------------------------------------------------------------------
def _tern_special(M, K, dt, g):
    """x, bias_a and the signs the contract gives: x = -bias_a (exact cancellation), -0 under a -0 bias, NaN, +inf and -inf, each at
    about a sixth of the positions; the rest random."""
    x = torch.randn((M, K), generator=g).to(dt)
    bias = (torch.randn(K, generator=g) * 0.3).to(dt)
    bias[1::6] = -0.0
    cls = torch.randint(0, 6, (M, K), generator=g)
    cls[:, 1::6] = torch.where(cls[:, 1::6] == 0, 1, cls[:, 1::6])
    x = torch.where(cls == 0, -bias.expand(M, K), x)
    x[(cls == 1) & (torch.arange(K) % 6 == 1)] = -0.0
    x[cls == 2] = float("nan")
    x[cls == 3] = float("inf")
    x[cls == 4] = float("-inf")
    return x, bias, cls


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M", [1, 4, 40])
def test_ternary_linear_sign_rule_at_zero_nan_and_inf(dt, M):
    """Both forms: x + bias_a == 0 (exact cancellation) and -0 give +1, NaN gives -1, +-inf its sign; with and without bias_a."""
    import test_ternary_gpu as TG
    ext = TG.ext()
    g = torch.Generator().manual_seed(M)
    K, N = 256, 72
    t = TG.rand_trits(N, K, g)
    q = ext.w_pack(t.to(DEV))
    x, bias, cls = _tern_special(M, K, dt, g)
    sa = torch.tensor(0.25, dtype=dt)
    alpha = (torch.rand(N, generator=g) * 0.1).to(dt)
    for b in (bias, None):
        s = TG.signs(x, b)
        zero = (cls == 1) & (torch.arange(K) % 6 == 1)
        assert (s[zero] == 1).all() and zero.any() and (cls == 0).any()  # -0 (+ -0): +1
        if b is not None:
            assert (s[cls == 0] == 1).all()  # x + bias_a = 0 exactly: +1
        assert (s[cls == 2] == -1).all() and (s[cls == 3] == 1).all() and (s[cls == 4] == -1).all()
        if b is None:
            assert (s[x == 0] == 1).all()
        want_D = TG.ref_D(s, t)
        want_y = ((want_D.to(dt) * sa) * alpha)
        bd = None if b is None else b.to(DEV)
        assert torch.equal(ext.linear_fp4(x.to(DEV).float(), q, None if b is None else b.to(DEV).float()).cpu().double(), want_D)
        assert torch.equal(ext.linear_fp4(x.to(DEV), q, bd, sa.to(DEV), alpha.to(DEV)).cpu(), want_y)
        if ext.fused_ok(M, N, K):
            assert torch.equal(ext.linear_fused(x.to(DEV), q, bd, raw=True).cpu().double(), want_D)
            assert torch.equal(ext.linear_fused(x.to(DEV), q, bd, sa.to(DEV), alpha.to(DEV)).cpu(), want_y)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M", [4, 16, 40])
def test_mxfp4_non_finite_x_gives_nan_and_inf_where_float64_does(dt, M):
    """Both forms: a NaN in x makes its row NaN, +-inf gives +-inf where every infinite product has one sign and the weight is non-zero, and
    NaN where it meets a zero weight or both signs -- exactly the positions of the float64 product; the other outputs within the contract."""
    import test_mxfp4_gpu as MX
    ext = MX.ext()
    g = torch.Generator().manual_seed(M + 3)
    N, K = 40, 256
    qw, sc = MX.rand_mx(N, K, g)
    W = MX.ref.dequant(qw, sc)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    x[0, 17] = float("nan")
    x[1, 3] = float("inf")
    x[2, 200] = float("-inf")
    x[3, 5], x[3, 6] = float("inf"), float("-inf")
    if M > 8:
        x[9, 31] = float("inf")
        x[9, 32] = float("inf")
    prod = x.double()[:, None, :] * W[None, :, :]     # [M, N, K] float64: inf * 0 = NaN, inf - inf = NaN, as IEEE gives them
    bias = torch.randn(N, generator=g).to(dt)
    yref = prod.sum(-1) + bias.double()
    assert yref.isnan().any() and yref.isposinf().any() and yref.isneginf().any()
    fin = torch.isfinite(yref)
    _, a = MX.ref_y(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), W, bias)
    for form in ((0, 1) if M <= 16 else (1,)):
        y = ext.forward(x.to(DEV), qw.to(DEV), sc.to(DEV), bias.to(DEV), form=form).cpu()
        assert torch.equal(y.isnan(), yref.isnan()), (form, y.isnan().nonzero()[:5], yref.isnan().nonzero()[:5])
        assert torch.equal(y.isposinf(), yref.isposinf()) and torch.equal(y.isneginf(), yref.isneginf()), form
        MX.check(y[fin].to(DEV), yref[fin].to(DEV), a.cpu()[fin].to(DEV), K, dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M", [5, 8, 40])
def test_ternary_a8_non_finite_x_row_is_nan_on_both_forms(dt, M):
    """INTEGRATION.md "Ternary W1.58A8": a row of x holding a NaN or an infinity has a_m = NaN, so r_m is NaN and every y of that row is
    NaN, on the decode and the GEMM form alike; the other rows are untouched (bit-exact against the restatement)."""
    import test_ternary_a8_gpu as TA
    ext = TA.ext()
    N, K = 72, 1024
    t, qw = TA.weights(N, K)
    g = torch.Generator().manual_seed(M)
    alpha = (torch.rand(N, generator=g) * 0.05 + 0.001).to(dt)
    x = TA.rand_x(M, K, dt, M + 1).cpu()
    x[1, 7] = float("nan")
    x[2, 1000] = float("inf")
    x[3, 0] = float("-inf")
    x[4, :] = 0.0
    x[4, 9] = float("nan")          # a NaN in an otherwise all-zero row
    x = x.to(DEV)
    bad = torch.zeros(M, dtype=torch.bool)
    bad[1:5] = True
    q, r = ext.quantize(x)
    assert r.cpu()[bad].isnan().all() and not r.cpu()[~bad].isnan().any()
    rq, rr = TA.ref_quant(x[~bad.to(DEV)])
    assert torch.equal(q.cpu()[~bad], rq) and torch.equal(r.cpu()[~bad], rr)
    want = TA.ref_y(TA.ref_D(rq, t), rr, alpha, dt)
    yg = ext.linear_gemm(x, qw, alpha.to(DEV)).cpu()
    assert yg[bad].isnan().all() and torch.equal(yg[~bad], want)
    if ext.fused_ok(M, N, K):
        yf = ext.linear_fused(x, qw, alpha.to(DEV)).cpu()
        assert torch.equal(yf.isnan(), yg.isnan()) and torch.equal(yf[~bad], yg[~bad])
    assert torch.equal(ext.layer_forward(x, qw, alpha.to(DEV)).cpu().isnan(), yg.isnan())
