"""MXFP8 W8A8 linear layer on the MI355X, in the structure of test_mxfp4_a6_gpu.py: the selector test that pins the k of every byte of
both E4M3 operands, the weight quantiser bit for bit against the restatement, both forward forms against the float64 product of the
restated x^ and W^ within the tolerance of mxfp8_a8_ref.py (its accumulation term from the probe's figure), exact data bit-identical
across forms, forward == gemm(quantize_act), the test that tells the layer from the W6A8 and the W4A8 one on the same latent weight,
scale sums, the non-finite row rule, the scale-255 column rule, the checkpoint rules, the straight-through backward, graph replay,
3-D / non-contiguous x and the refusals."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("mxfp8_a8_ref")
ref48 = ref.a8                   # mxfp4_a8_ref: the W4A8 restatement (and the activation side of all three)
mx4 = ref.mx                     # mxfp4_ref: the MXFP4 weight side
mx6 = _load("mxfp6_ref")         # the MXFP6 weight side and the W6A8 tolerance

DECODE_ROWS = 64  # the decode form's largest M (bie_mx8a8_linear_forward refuses it beyond)


def ext():
    from bitorch_engine.extensions import mxfp8_a8_linear_cuda
    return mxfp8_a8_linear_cuda


def forms(M):
    return (0, 1) if M <= DECODE_ROWS else (1,)


def check(y, yref, absprod, K, dt, what="", tolerance=None):
    tol = (tolerance or ref.tolerance)(yref, absprod, K, dt)
    err = (y.double() - yref).abs()
    print(f"{what} max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), f"{what} max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def selector_codes(R, K):
    """E4M3 codes distinct per k within a row: the 32 codes 0x38 .. 0x57 (1.0 .. 15: four exponents, eight mantissas) in an order that
    differs per row, blocks told apart by their scales 2^-8, 2^-4, 2^0, ..: the values of block b lie in [2^(4 b - 8), 2^(4 b - 4)), so no
    two k of a row give one value, and every value has four significant bits (exact in fp16 and bf16)."""
    c = (0x38 + (torch.arange(K)[None, :] * 5 + torch.arange(R)[:, None] * 11) % 32).to(torch.uint8)
    s = (127 + 4 * (torch.arange(K // 32) - 2))[None, :].repeat(R, 1).to(torch.uint8)
    return c, s


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", [128, 160])
def test_selector_pins_the_k_of_every_byte_of_both_operands(K, dt):
    """Weights one-hot: E4M3 code 1.0 (0x38) at k = pi(n) under scale 2^0, all other bytes 0; pi covers every k.  x holds a distinct value
    per k of a row.  Then y[m, n] == x^[m, pi(n)] exactly, in every form: a byte of either operand taken from another place of the row,
    or a block under another block's scale, selects another value.  Then the mirror image: x one-hot, y[m, n] == W^[n, k(m)], the
    weights distinct per k of a row.  This holds probe parts (a) and (b) in the suite."""
    g = torch.Generator().manual_seed(K)
    N = 2 * K + 3
    pi = torch.cat([torch.randperm(K, generator=g), torch.randperm(K, generator=g), torch.tensor([0, K - 1, K // 2])])
    q = torch.zeros((N, K), dtype=torch.uint8)
    q[torch.arange(N), pi] = 0x38
    s = torch.full((N, K // 32), 127, dtype=torch.uint8)
    for M in (1, 17, 65):
        xq, xs = selector_codes(M, K)
        flag = torch.zeros(M, dtype=torch.uint8)
        xh = ref.dequant_act(xq, xs)
        assert all(len(set(row.tolist())) == K for row in xh)
        want = xh[:, pi].to(dt)
        assert torch.equal(want.double(), xh[:, pi])
        for form in forms(M):
            y = ext().gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), q.to(DEV), s.to(DEV), dtype=dt, form=form)
            assert torch.equal(y.cpu(), want), (M, form, (y.cpu() != want).nonzero()[:5].tolist())
    # and the other way round: x one-hot (1.0 at one k per row m; every k is taken at M = K), weights distinct per k of a row
    wq, sw = selector_codes(N, K)
    Wd = ref.dequant(wq, sw)
    assert all(len(set(row.tolist())) == K for row in Wd)
    for M in (1, 17, 65, K):
        xq = torch.zeros((M, K), dtype=torch.uint8)
        ks = (torch.arange(M) * 37 + 5) % K  # 37 is coprime to 128 and 160: M = K visits every k
        xq[torch.arange(M), ks] = 0x38  # 1.0
        xs = torch.full((M, K // 32), 127, dtype=torch.uint8)
        flag = torch.zeros(M, dtype=torch.uint8)
        want = Wd[:, ks].t().contiguous()
        assert torch.equal(want.to(dt).double(), want)
        for form in forms(M):
            y = ext().gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), wq.to(DEV), sw.to(DEV), dtype=dt, form=form)
            assert torch.equal(y.cpu().double(), want), (M, form, (y.cpu().double() != want).nonzero()[:5].tolist())


def quantizer_rows(dt):
    """Rows of 32-value blocks that meet every rule: ties between E4M3 codes, saturation beyond 448 * 2^e, subnormal codes, both zeros,
    an all-zero block, block maxima of every kind, Gaussian blocks of many magnitudes; then a NaN block and two inf blocks."""
    g = torch.Generator().manual_seed(8)
    rows = []
    base = torch.zeros(32)
    base[0] = 256.0                                             # amax 2^8: e = 0, the values below are the scaled values themselves
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, 1.0625, 1.1875, 2.125, 2.375, 0.001953125 * 0.5, 0.001953125 * 1.5, 0.001953125 * 2.5])
    t = base.clone()
    t[1:1 + len(ties)] = ties                                   # halfway between two codes (steps 2, 0.125, 0.25) and between subnormals
    t[12:23] = -ties
    t[23], t[24], t[25] = 0.0, -0.0, 0.001953125                # both zeros, the smallest subnormal 2^-9
    rows.append(t)
    sat = torch.full((32,), 1.0)
    sat[0], sat[1], sat[2], sat[3] = 500.0, -508.0, 452.0, 464.0  # amax in (448, 512): e = 0 and the values beyond 448 saturate
    rows.append(sat)
    rows.append(torch.zeros(32))                                # an all-zero block: scale 0, zero bytes
    neg0 = torch.zeros(32)
    neg0[::2] = -0.0
    rows.append(neg0)                                           # zeros of both signs only
    for e in (-14, -7, 0, 5, 12):
        rows.append(torch.randn(32, generator=g) * 2.0 ** e)
        one = torch.zeros(32)
        one[5] = -(2.0 ** e) * 1.75
        rows.append(one)
    if dt != torch.float16:
        rows.append(torch.randn(32, generator=g) * 2.0 ** 100)
        rows.append(torch.randn(32, generator=g) * 2.0 ** -100)  # fp32 and bf16 keep the exponent range; W^ stays a normal fp32 value
    if len(rows) % 2:
        rows.append(torch.ones(32))
    w = torch.stack(rows).reshape(-1, 64).to(dt)  # two blocks per row
    return w


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_quantize_is_bit_exact_against_the_restatement(dt):
    w = quantizer_rows(dt)
    g = torch.Generator().manual_seed(9)
    big = (torch.randn((37, 416), generator=g) * torch.exp2(torch.randint(-12, 6, (37, 1), generator=g).float())).to(dt)
    for t in (w, big):
        q, s = ext().quantize(t.to(DEV))
        rq, rs = ref.quantize(t)
        assert torch.equal(s.cpu(), rs), (s.cpu() != rs).nonzero()[:5].tolist()
        assert torch.equal(q.cpu(), rq), (q.cpu() != rq).nonzero()[:5].tolist()
        assert not ((q & 0x7F) == 0x7F).any()                   # never a NaN code
        wh = ext().dequant(q, s, torch.float32)
        assert torch.equal(wh.cpu().double(), ref.dequant(rq, rs))
        q2, s2 = ext().quantize(wh)                             # idempotent on W^
        assert torch.equal(q2, q) and torch.equal(s2, s)
        if dt != torch.float32:                                 # on finite 16-bit rows: the activation quantiser's bytes
            xq, xs, flag = ext().quantize_act(t.to(DEV))
            assert not flag.any() and torch.equal(xq, q) and torch.equal(xs, s)
            assert torch.equal(ext().dequant(xq, xs, torch.float32), ext().dequant_act(xq, xs, torch.float32))  # dequant decodes xq / xs too
    # a NaN block and an inf block: scale 255 and zero bytes there, the other blocks of the row as before
    bad = big.clone()
    bad[3, 40], bad[5, 0], bad[36, 415] = float("nan"), float("inf"), float("-inf")
    q, s = ext().quantize(bad.to(DEV))
    rq, rs = ref.quantize(bad)
    assert torch.equal(q.cpu(), rq) and torch.equal(s.cpu(), rs)
    assert s[3, 1] == 255 and s[5, 0] == 255 and s[36, 12] == 255 and (s == 255).sum() == 3
    assert not q[3, 32:64].any() and not q[5, :32].any() and not q[36, 384:].any()
    q0, s0 = ext().quantize(big.to(DEV))
    same = torch.ones_like(s0, dtype=torch.bool)
    same[3, 1] = same[5, 0] = same[36, 12] = False
    assert torch.equal(s[same], s0[same]) and torch.equal(q.reshape(37, 13, 32)[same], q0.reshape(37, 13, 32)[same])
    assert torch.isnan(ext().dequant(q, s, torch.float32)[3, 32:64]).all()


# every K of {32, 96, 160, 1024, 4096} (one block, an odd block count, a partial stage, waves with and without work) and every N of
# {1, 3, 16, 17, 130, 257} (scalar and vector stores, a partial tile) at every M; the decode-range M also forced to the prefill form
KN = ((32, 1), (96, 3), (160, 16), (1024, 17), (4096, 130), (160, 257), (32, 130), (96, 17), (1024, 3), (4096, 16))
DECODE_M = (1, 5, 16, 17, 33, 64)
PREFILL_M = (65, 130, 300)

SHAPES = [(M, K, N) for M in DECODE_M + PREFILL_M for K, N in KN] + [(257, 160, 21846)] + [(33, 96, 130)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_forward_every_form_against_float64(M, K, N, dt):
    """(257, 160, 21846): 3 x 171 = 513 tiles of 128 x 128, the large tile instance with ragged edges in M, N and K."""
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    q, s = ref.rand_w(N, K, g)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    bias = (torch.randn(N, generator=g)).to(dt) if (M + N) % 2 else None
    xq, xs, flag = ref.quantize_act(x)
    yref, a = ref.reference(xq, xs, flag, q, s, bias, DEV)
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext().col_exp(sd)
    for form in forms(M) + (-1,):
        y = ext().forward(x.to(DEV), qd, sd, None if bias is None else bias.to(DEV), e, form=form)
        assert y.dtype == dt and y.shape == (M, N)
        check(y, yref, a, K, dt, f"form {form}")


def int_codes(shape, g):
    """The E4M3 codes of random integers -7 .. 7."""
    return torch.randint(-7, 8, shape, generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)


def exact_case(M, N, K, g, dt):
    """Per block x[0] = 8 * 2^j and the others m * 2^j, integers |m| <= 7, j in -1 .. 1: every block's amax is 8 * 2^j, so e = j - 5 and
    the scaled values 32 m and 256 are E4M3 values: x is a fixed point of the quantiser.  Weight codes the E4M3 codes of -7 .. 7, scales
    125 .. 129.  Products are multiples of 2^-1 * 2^-2 and every partial sum of K = 256 stays below 256 * 16 * 28 < 2^17: 20 bits, exact
    in fp32."""
    q = int_codes((N, K), g)
    s = torch.randint(125, 130, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    j = torch.randint(-1, 2, (M, K // 32), generator=g).repeat_interleave(32, dim=1)
    m = ((torch.arange(K)[None, :] * 3 + torch.arange(M)[:, None]) % 15 - 7).float()
    m[:, ::32] = 8.0  # the block maximum
    x = (m * torch.exp2(j.float())).to(dt)
    return x, q, s


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 5, 16, 33, 64, 300])
def test_exact_data_is_bit_identical_across_forms_and_against_float64(M, dt):
    g = torch.Generator().manual_seed(M)
    N, K = 72, 256
    x, q, s = exact_case(M, N, K, g, dt)
    xq, xs, flag = ref.quantize_act(x)
    assert torch.equal(ref.dequant_act(xq, xs), x.double())  # x is a fixed point: x^ == x
    bias = torch.randint(-8, 9, (N,), generator=g).to(dt)
    yref, _ = ref.reference(xq, xs, flag, q, s, bias, DEV)
    assert torch.equal(yref.float().double(), yref)
    want = yref.to(dt)
    for form in forms(M) + (-1,):
        y = ext().gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), q.to(DEV), s.to(DEV), bias.to(DEV), dtype=dt, form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())
        y = ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), bias.to(DEV), form=form)
        assert torch.equal(y, want), ("forward", form)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [3, 40, 64, 130])
def test_forward_is_gemm_of_quantize_act(M, dt):
    g = torch.Generator().manual_seed(M + 11)
    N, K = 77, 416
    q, s = ref.rand_w(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt)
    bias = torch.randn(N, generator=g).to(dt).to(DEV)
    xq, xs, flag = ext().quantize_act(x.to(DEV))
    rq, rs, rf = ref.quantize_act(x)  # the quantiser is the W4A8 layer's: the restatement's bytes
    assert torch.equal(xq.cpu(), rq) and torch.equal(xs.cpu(), rs) and torch.equal(flag.cpu(), rf)
    for form in forms(M):
        assert torch.equal(ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), bias, form=form),
                           ext().gemm(xq, xs, flag, q.to(DEV), s.to(DEV), bias, dtype=dt, form=form)), form


def layer_with(cls, N, K, dt, bias=False, seed=0, **kw):
    torch.manual_seed(seed)
    return cls(K, N, bias=bias, dtype=dt, **kw).to(DEV)


def layers():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A8LinearCuda, MXFP4LinearCuda, MXFP6A8LinearCuda, MXFP6LinearCuda, MXFP8A8LinearCuda
    return MXFP8A8LinearCuda, MXFP6A8LinearCuda, MXFP4A8LinearCuda, MXFP6LinearCuda, MXFP4LinearCuda


def discriminating_w(N, K, g, dt):
    """discriminating_x of test_mxfp4_a6_gpu.py on the weight side.  Per block w[0] = 4 * 2^j, the rest +- odd multiples of 2^-5 * 2^j
    below 2^-1 * 2^j: E4M3-exact under the block's MXFP8 scale (e = j - 6: scaled values 256 and odd multiples of 2 below 32, at most 4
    significant bits), while E2M3 (e = j, step 0.125 = 4 * 2^-5 below 2) rounds every one of them to a multiple of 0.125 * 2^j, and
    E2M1 (e = j, step 0.5) to 0 or 0.5 * 2^j: the three weight quantisers disagree on every small value."""
    j = torch.randint(-1, 2, (N, K // 32), generator=g).repeat_interleave(32, dim=1).float()
    odd = (2 * torch.randint(0, 8, (N, K), generator=g) + 1).float() * torch.where(torch.rand((N, K), generator=g) < 0.5, -1.0, 1.0)
    v = odd * 2.0 ** -5
    v[:, ::32] = 4.0
    return (v * torch.exp2(j)).to(dt)


def restated(w, x, dt, device="cpu"):
    """((y, absprod) of the W8A8, the W6A8 and the W4A8 restatement) of one latent weight and one x, and the three weight images."""
    xq, xs, flag = ref.quantize_act(x)
    q8, s8 = ref.quantize(w)
    c6, s6 = mx6.quantize(w)
    q6 = mx6.pack(c6)
    c4, s4 = mx4.quantize(w)
    q4 = mx4.pack(c4)
    xh = ref.dequant_act(xq, xs).to(device)
    out = []
    for W in (ref.dequant(q8, s8), mx6.dequant(q6, s6), mx4.dequant(q4, s4)):
        W = W.to(device)
        out.append((xh @ W.t(), xh.abs() @ W.abs().t()))
    return out, (q8, s8), (q6, s6), (q4, s4)


DISCRIMINATING = [(8, 4096, 256), (64, 1024, 128), (3, 32, 16), (200, 1024, 128), (5, 160, 40)]
# The share of outputs where the W8A8 restatement of the same latent weight (discriminating_w) and the same Gaussian x lies outside the
# W6A8 tolerance (constant 1853) of the W6A8 restatement, and outside the W4A8 tolerance (constant 1552) of the W4A8 restatement, from
# the restatements alone on the CPU (tests/test_mxfp8_a8_cpu.py::test_discriminating_shares_are_the_ones_written_in_the_gpu_test
# recomputes them), fp16 / bf16 per shape of DISCRIMINATING in its order:
#   against W6A8: 0.806 0.704 | 0.889 0.778 | 0.896 0.625 | 0.889 0.788 | 0.940 0.790
#   against W4A8: 0.962 0.939 | 0.978 0.953 | 0.979 0.938 | 0.980 0.958 | 0.985 0.965
# Neither tolerance depends on this layer's PROBE_ULPS.  Less than half of the smallest share of each list (0.625, 0.938) is asked of the
# layer and of the restatement.
SHARES_W6A8 = (0.806, 0.704, 0.889, 0.778, 0.896, 0.625, 0.889, 0.788, 0.940, 0.790)
SHARES_W4A8 = (0.962, 0.939, 0.978, 0.953, 0.979, 0.938, 0.980, 0.958, 0.985, 0.965)
OUTSIDE_W6A8 = 0.31
OUTSIDE_W4A8 = 0.46


def discriminating_case(M, K, N, dt):
    g = torch.Generator().manual_seed(K + M)
    w = discriminating_w(N, K, g, dt)
    x = torch.randn((M, K), generator=g).to(dt)
    return w, x


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", DISCRIMINATING)
def test_the_layer_is_w8a8_and_not_w6a8_or_w4a8(M, K, N, dt):
    W88, W68, W48 = layers()[:3]
    w, x = discriminating_case(M, K, N, dt)
    l88, l68, l48 = (layer_with(c, N, K, dt).eval() for c in (W88, W68, W48))
    with torch.no_grad():
        for l in (l88, l68, l48):
            l.weight.copy_(w)
        y88, y68, y48 = (l(x.to(DEV)) for l in (l88, l68, l48))
    assert not torch.equal(y88, y68) and not torch.equal(y88, y48)
    (r88, r68, r48), (q8, s8), (q6, s6), (q4, s4) = restated(w, x, dt, DEV)
    assert torch.equal(l88.qweight.cpu(), q8) and torch.equal(l88.scales.cpu(), s8)
    assert torch.equal(ref.dequant(q8, s8), w.double())                      # E4M3-exact
    rest = torch.ones(K, dtype=torch.bool)
    rest[::32] = False
    W6, W4 = mx6.dequant(q6, s6), mx4.dequant(q4, s4)
    assert (W6[:, rest] != w.double()[:, rest]).all()                        # E2M3 rounds every one of the small values
    assert (W4[:, rest] != W6[:, rest]).any(dim=1).all()                     # and E2M1 rounds them differently in every row
    check(y88, r88[0], r88[1], K, dt, "w8a8 layer against the w8a8 restatement")
    for name, (r, a), tolf, bound in (("W6A8", r68, mx6.tolerance, OUTSIDE_W6A8), ("W4A8", r48, ref48.tolerance, OUTSIDE_W4A8)):
        tol = tolf(r, a, K, dt)
        out_ref = ((r88[0] - r).abs() > tol).double().mean().item()
        out = ((y88.double() - r).abs() > tol).double().mean().item()
        print(f"outside the {name} tolerance of the {name} restatement: the W8A8 restatement {100 * out_ref:.1f} %, the layer {100 * out:.1f} %")
        assert out_ref > bound and out > bound, name
    check(y68, r68[0], r68[1], K, dt, "w6a8 layer against the w6a8 restatement", mx6.tolerance)  # each layer passes its own
    check(y48, r48[0], r48[1], K, dt, "w4a8 layer against the w4a8 restatement", ref48.tolerance)


@pytest.mark.parametrize("dt", DTS)
def test_scale_sums_between_minus_100_and_100(dt):
    """Chosen scales at the ends of the tested range: sx + sw - 254 in [-100, 100], one block of integer codes so the fp32 value is exact."""
    g = torch.Generator().manual_seed(4)
    N, K, M = 48, 32, 40
    q = int_codes((N, K), g)
    xq = int_codes((M, K), g)
    for sx, sw in ((27, 127), (127, 27), (77, 77), (227, 127), (127, 227), (177, 177), (2, 252), (252, 2)):
        xs = torch.full((M, 1), sx, dtype=torch.uint8)
        s = torch.full((N, 1), sw, dtype=torch.uint8)
        flag = torch.zeros(M, dtype=torch.uint8)
        yref, a = ref.reference(xq, xs, flag, q, s, None, DEV)
        want = yref.float()  # exact: one block sum (32 integer products, |p| <= 49) times a power of two
        assert torch.equal(want.double(), yref)
        for form in forms(M):
            # through the fp32 value: the dtype's rounding of the exact result (fp16 saturates to inf / flushes, as torch's cast does)
            y = ext().gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), q.to(DEV), s.to(DEV), dtype=dt, form=form)
            assert torch.equal(y, want.to(dt)), (sx, sw, form)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [3, 64, 70])
def test_non_finite_row_gives_a_nan_row_and_leaves_the_others_alone(M, dt):
    g = torch.Generator().manual_seed(6)
    N, K = 45, 256
    q, s = ref.rand_w(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt)
    clean = {form: ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), form=form) for form in forms(M)}
    for bad, pos in ((float("inf"), 0), (float("-inf"), K - 1), (float("nan"), 5), (float("nan"), K - 32)):
        for row in (0, M - 1, M // 2):
            xb = x.clone()
            xb[row, pos] = bad
            for form in forms(M):
                y = ext().forward(xb.to(DEV), q.to(DEV), s.to(DEV), form=form)
                assert torch.isnan(y[row]).all(), (bad, pos, row, form)
                keep = torch.ones(M, dtype=torch.bool)
                keep[row] = False
                assert torch.equal(y[keep], clean[form][keep]), (bad, pos, row, form)


@pytest.mark.parametrize("dt", DTS)
def test_scale_255_gives_nan_in_that_column_only(dt):
    g = torch.Generator().manual_seed(5)
    N, K = 40, 256
    q, s = ref.rand_w(N, K, g)
    x = torch.randn((70, K), generator=g).to(dt)
    bias = torch.randn(N, generator=g).to(dt)
    s_bad = s.clone()
    s_bad[3, 2] = 255
    s_bad[39, 7] = 255
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[3] = keep[39] = False
    for M in (1, 16, 64, 70):
        xq, xs, flag = ref.quantize_act(x[:M])
        yref, a = ref.reference(xq, xs, flag, q, s_bad, bias, DEV)
        for form in forms(M):
            clean = ext().forward(x[:M].to(DEV), q.to(DEV), s.to(DEV), bias.to(DEV), form=form)
            y = ext().forward(x[:M].to(DEV), q.to(DEV), s_bad.to(DEV), bias.to(DEV), form=form)
            assert torch.isnan(y[:, 3]).all() and torch.isnan(y[:, 39]).all()
            assert torch.equal(y[:, keep], clean[:, keep])  # the other columns are bit-identical to the run without the NaN blocks
            check(y[:, keep], yref[:, keep], a[:, keep], K, dt, f"M {M} form {form}")


@pytest.mark.parametrize("dt", DTS)
def test_state_dict_round_trips_and_refusals(dt):
    W88, W68, W48, W616, W4 = layers()
    g = torch.Generator().manual_seed(3)
    N, K = 48, 192
    q, s = ref.rand_w(N, K, g)
    x = torch.randn((5, K), generator=g).to(dt).to(DEV)
    a = layer_with(W88, N, K, dt, bias=True).eval()
    a.set_mx_weight(q.reshape(N, K // 32, 32), s)
    assert set(a.state_dict()) == {"qweight", "scales", "bias"} and a.weight is None
    assert torch.equal(a(x), ext().forward(x, q.to(DEV), s.to(DEV), a.bias.detach()))
    b = layer_with(W88, N, K, dt, bias=True, seed=5).eval()
    b.load_state_dict(a.state_dict())  # a packed checkpoint drops the latent weight
    assert b.weight is None and torch.equal(b.qweight, a.qweight) and torch.equal(b(x), a(x))
    b.set_mx_weight(q, s)              # the flat [N, K] spelling
    assert torch.equal(b(x), a(x))
    lat = layer_with(W88, N, K, dt, bias=True, seed=7).eval()
    y_lat = lat(x)
    assert set(lat.state_dict()) == {"weight", "qweight", "scales", "bias"}
    fresh = layer_with(W88, N, K, dt, bias=True, seed=8).eval()
    fresh.load_state_dict(lat.state_dict())  # a latent-weight checkpoint: qweight is re-derived from the weight
    assert torch.equal(fresh(x), y_lat) and torch.equal(fresh.qweight, lat.qweight) and torch.equal(fresh.scales, lat.scales)
    b.load_state_dict(lat.state_dict())  # ... also into a layer that had dropped its own
    assert b.weight is not None and torch.equal(b(x), y_lat)
    fresh.generate_quantized_weight(qweight_only=True)
    assert "weight" not in fresh.state_dict() and torch.equal(fresh(x), y_lat)
    for cls, what in ((W68, "MXFP6 weight"), (W616, "MXFP6 weight"), (W48, "MXFP4 weight"), (W4, "MXFP4 weight")):
        other = layer_with(cls, N, K, dt, bias=True).eval()
        other(x)
        before = fresh.qweight.clone()
        with pytest.raises(RuntimeError, match=what + ".*MXFP8A8LinearCuda"):
            fresh.load_state_dict(other.state_dict())
        assert torch.equal(fresh.qweight, before) and torch.equal(fresh(x), y_lat)
    qn = q.clone()
    qn[7, 100] = 0xFF
    with pytest.raises(ValueError, match=r"blocks\[7, 100\] = 0xFF is an E4M3 NaN code"):
        a.set_mx_weight(qn, s)
    assert torch.equal(a.qweight.cpu(), q)


@pytest.mark.parametrize("dt", DTS)
def test_backward_and_one_optimiser_step(dt):
    W88 = layers()[0]
    N, K, M = 64, 128, 24
    layer = layer_with(W88, N, K, dt, bias=True).train()
    x = torch.randn((M, K), device=DEV).to(dt).requires_grad_(True)
    y = layer(x)
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), q, s, layer.bias.detach()))
    gy = torch.randn_like(y)
    y.backward(gy)
    W = ref.dequant(q.cpu(), s.cpu()).to(DEV)
    xq, xs, _ = ref.quantize_act(x.detach().cpu())
    xh = ref.dequant_act(xq, xs).to(DEV)
    # the float64 formulas; the layer computes them in fp32 and rounds once to the dtype
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    for got, want, absw in ((x.grad, gy.double() @ W, gy.double().abs() @ W.abs()),
                            (layer.weight.grad, gy.double().t() @ xh, gy.double().abs().t() @ xh.abs()),
                            (layer.bias.grad, gy.double().sum(0), gy.double().abs().sum(0))):
        tol = eps * want.abs() + (M + N + 2) * 2.0 ** -23 * absw + 2.0 ** -24
        assert ((got.double() - want).abs() <= tol).all()
    # the weight gradient uses the E4M3-QUANTISED activations: it differs from gy^T . x
    assert not torch.equal(layer.weight.grad, gy.float().t().mm(x.detach().float()).to(dt))
    before = layer(x).detach()
    torch.optim.SGD(layer.parameters(), lr=0.5).step()
    assert not torch.equal(layer(x).detach(), before)
    # eval with grad enabled is differentiable in x
    layer.eval()
    x2 = torch.randn((M, K), device=DEV).to(dt).requires_grad_(True)
    layer(x2).sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 8, 64, 200])
def test_graph_replay_equals_eager(M, dt):
    W88 = layers()[0]
    N, K = 256, 512
    layer = layer_with(W88, N, K, dt, bias=True).eval()
    x = torch.randn((M, K), device=DEV).to(dt)
    with torch.no_grad():
        eager = layer(x)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            layer(x)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = layer(x)
        x.copy_(torch.randn((M, K), device=DEV).to(dt))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, layer(x))
        assert not torch.equal(out, eager)


@pytest.mark.parametrize("dt", DTS)
def test_3d_and_non_contiguous_x(dt):
    W88 = layers()[0]
    N, K = 40, 256
    layer = layer_with(W88, N, K, dt).eval()
    base = torch.randn((K, 6), device=DEV).to(dt)
    x = base.t()
    assert not x.is_contiguous()
    with torch.no_grad():
        assert torch.equal(layer(x), layer(x.contiguous()))
        x3 = torch.randn((2, 3, K), device=DEV).to(dt)
        y3 = layer(x3)
        assert y3.shape == (2, 3, N) and torch.equal(y3.reshape(6, N), layer(x3.reshape(6, K)))


def test_host_tensor_and_forced_decode_past_64_rows_are_refused():
    W88 = layers()[0]
    layer = layer_with(W88, 8, 64, torch.float16).eval()
    with pytest.raises(RuntimeError):
        layer(torch.randn((2, 64)).half())
    with pytest.raises(RuntimeError):
        ext().quantize(torch.randn((2, 64)))
    with pytest.raises(RuntimeError, match="M=65"):
        ext().forward(torch.zeros((65, 64), dtype=torch.half, device=DEV), layer.qweight, layer.scales, form=0)  # no fallback past M = 64
