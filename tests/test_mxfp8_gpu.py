"""MXFP8 weight-only linear layer (W8A16, csrc/mxfp8.hip) on the MI355X: both forward forms against a float64 product of x and
mxfp8_a8_ref.dequant within the weight-only contract's tolerance (fuzz_mxfp6.check: exact products, an fp32 sum, one rounding), the
convert's element map on one-hot rows, bit-identity on exact data, the special codes, the fp16 range, and the layer."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import mxfp8_a8_ref as ref  # noqa: E402
import fuzz_mxfp6 as F  # noqa: E402
from test_mxfp8_cpu import decode_bound  # noqa: E402

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ref_y, check = F.ref_y, F.check
B = decode_bound()  # the decode form's largest M: a host call, nothing is launched
# tools/probe/probe_fp8_cvt.hip part (c), profiles/mxfp8_cvt_probe.txt: below 2^-14 the fp16 convert rounds to an fp16 subnormal, so a
# weight of the prefill form's fragments is off by at most one subnormal step of its column's largest scale
FP16_STEP = 2.0 ** -24


def ext():
    from bitorch_engine.extensions import mxfp8_linear_cuda
    return mxfp8_linear_cuda


def forms_for(M):
    return (0, 1, -1) if M <= B else (1, -1)


_WEIGHTS = {}


def weights(K, N):
    """One random weight per (K, N), with its restatement on the GPU: shared by every M and dtype, never written."""
    if (K, N) not in _WEIGHTS:
        q, s = ref.rand_w(N, K, torch.Generator().manual_seed(K * 3 + N), 118, 130)
        _WEIGHTS[(K, N)] = (q.to(DEV), s.to(DEV), ref.dequant(q, s).to(DEV))
    return _WEIGHTS[(K, N)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N", [(32, 1), (96, 7), (2880, 33), (4096, 129), (96, 4096)])
@pytest.mark.parametrize("M", sorted({1, 2, 3, 8, 17, B, B + 1, 64, 129, 300}))
def test_forward_both_forms_against_float64(M, K, N, dt):
    qd, sd, W = weights(K, N)
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x = (torch.randn((M, K), generator=g) * 0.25).to(dt)
    bias = torch.randn(N, generator=g).to(dt)
    e = ext().col_exp(sd)
    for b in (None, bias):
        yref, a = ref_y(x, W, b)
        for form in forms_for(M):
            y = ext().forward(x.to(DEV), qd, sd, None if b is None else b.to(DEV), e if form else None, form=form)
            assert y.dtype == dt and y.shape == (M, N)
            check(y, yref, a, K, dt, f"form {form} bias {b is not None}")


@pytest.mark.parametrize("dt", DTS)
def test_one_hot_rows_select_every_weight_exactly(dt):
    """x row i has a single 1 at k = i: y[i] = W[:, i] exactly, for every k and both forms.  Row n of W holds 128 distinct codes (all 254
    codes but the NaNs over the 9 rows), so any slip in the byte order or the op_sel halves moves a value."""
    N, K = 9, 128
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F])
    q = codes[(torch.arange(K)[None, :] + 31 * torch.arange(N)[:, None]) % 254].to(torch.uint8)
    s = (125 + (torch.arange(N)[:, None] + torch.arange(K // 32)[None, :]) % 5).to(torch.uint8)  # 2^-2 .. 2^2: W is exact in fp16 and bf16
    want = ref.dequant(q, s).t().to(dt).to(DEV)  # [K, N]
    eye = torch.eye(K, dtype=dt, device=DEV)
    for form in (0, 1):
        step = B if form == 0 else K
        y = torch.cat([ext().forward(eye[i:i + step], q.to(DEV), s.to(DEV), form=form) for i in range(0, K, step)])
        assert torch.equal(y, want), (form, (y != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", sorted({1, 5, B, 64, 300}))
def test_exact_data_is_bit_identical_across_forms_and_to_the_reference(M, dt):
    g = torch.Generator().manual_seed(M)
    N, K = 72, 4096
    ints = torch.tensor([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=torch.uint8)  # 0, +-1, +-2, +-3, +-4
    q = ints[torch.randint(0, 9, (N, K), generator=g)]
    s = torch.randint(125, 130, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    x = torch.randint(-2, 3, (M, K), generator=g).to(dt)  # every partial sum a multiple of 2^-2 below 4096 * 2 * 16 = 2^17: exact in fp32
    bias = torch.randint(-8, 9, (N,), generator=g).to(dt)
    yref, _ = ref_y(x, ref.dequant(q, s), bias)
    want = yref.to(dt)
    for form in forms_for(M):
        y = ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), bias.to(DEV), form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("dt", DTS)
def test_special_codes_stay_in_their_column_and_non_finite_x_in_its_row(dt):
    g = torch.Generator().manual_seed(5)
    N, K = 40, 256
    q, s = ref.rand_w(N, K, g, 118, 130)
    s[3, 2] = 255     # a NaN block
    s[7, :] = 0       # a whole row of 2^-127 blocks
    q[11, 77] = 0x7F  # E4M3 NaN codes
    q[12, 200] = 0xFF
    nan_cols = [3, 11, 12]
    x = (torch.randn((64, K), generator=g) * 0.25).to(dt)
    xb = x.clone()
    xb[1, 37], xb[0, 150] = float("nan"), float("inf")
    W = ref.dequant(q, s)
    assert torch.isnan(W[11, 77]) and torch.isnan(W[12, 200])
    yref, a = ref_y(x, torch.nan_to_num(W, nan=0.0))
    keep = torch.ones(N, dtype=torch.bool)
    keep[nan_cols] = False
    keep[7] = False  # may flush to zero: checked on its own
    for M in sorted({2, B, 64}):
        for form in forms_for(M):
            y = ext().forward(x[:M].to(DEV), q.to(DEV), s.to(DEV), form=form)
            assert torch.isnan(y[:, nan_cols]).all() and not torch.isnan(y[:, keep]).any()
            assert (y[:, 7].double().abs() <= 2.0 ** -100).all()
            check(y[:, keep], yref[:M][:, keep.to(DEV)], a[:M][:, keep.to(DEV)], K, dt, f"form {form}")
            yb = ext().forward(xb[:M].to(DEV), q.to(DEV), s.to(DEV), form=form)
            assert torch.isnan(yb[1, keep]).all() and not torch.isfinite(yb[0, keep]).any()
            assert torch.equal(yb[2:, keep], y[2:, keep]), form


@pytest.mark.parametrize("M", sorted({1, B, 64}))
def test_fp16_range_wider_than_an_fp16_image(M):
    g = torch.Generator().manual_seed(11)
    N, K = 64, 2048
    q = ref.rand_w(N, K, g)[0] & 0xBF  # |code| <= 1.875, so that 2048 products under scale 2^16 stay inside fp16
    s = torch.randint(103, 144, (N, K // 32), generator=g)
    s[0], s[1], s[2] = 143, 103, torch.arange(K // 32) % 41 + 103  # all 2^16, all 2^-24, the whole range within one column
    s = s.to(torch.uint8)
    W = ref.dequant(q, s)
    assert W.abs().max() > 65504
    x = (torch.randn((M, K), generator=g) * 2.0 ** -12).half()
    yref, a = ref_y(x, W)
    e = ext().col_exp(s.to(DEV))
    colmax = ref.mx.e8m0(e.cpu()).to(DEV)
    for form in forms_for(M):
        y = ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), None, e, form=form)
        assert torch.isfinite(y).all()
        prefill = (ext().form(M, N, K, torch.float16) if form < 0 else form) == 1
        # the prefill form's rebias: a weight keeps FP16_STEP of its column's largest scale, the decode form all of it
        rebias = x.to(DEV).double().abs().sum(1, keepdim=True) * colmax[None, :] * FP16_STEP if prefill else 0.0
        tol = F.tolerance(yref, a, K, torch.float16) + rebias
        err = (y.double() - yref).abs()
        assert (err <= tol).all(), (form, err.max().item())


def layer_with(N, K, dt, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP8LinearCuda
    torch.manual_seed(seed)
    return MXFP8LinearCuda(K, N, bias=True, dtype=dt).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_layer_checkpoints_and_set_mx_weight(dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda, MXFP6LinearCuda, MXFP8A8LinearCuda
    N, K = 24, 128
    w16 = layer_with(N, K, dt, seed=1).eval()
    w16.prepare_params()
    a8 = MXFP8A8LinearCuda(K, N, bias=True, dtype=dt).to(DEV).eval()
    a8.load_state_dict(w16.state_dict())
    a8.prepare_params()
    assert torch.equal(a8.qweight, w16.qweight) and torch.equal(a8.scales, w16.scales) and torch.equal(a8.e_col, w16.e_col)
    a8.generate_quantized_weight(qweight_only=True)
    back = layer_with(N, K, dt, seed=4).eval()
    back.load_state_dict(a8.state_dict())
    assert back.weight is None and torch.equal(back.qweight, a8.qweight) and torch.equal(back.scales, a8.scales)
    for other, what in ((MXFP4LinearCuda, "MXFP4 weight"), (MXFP6LinearCuda, "MXFP6 weight")):
        with pytest.raises(RuntimeError, match=what):
            back.load_state_dict(other(K, N, bias=True, dtype=dt).state_dict())
    q, s = ref.rand_w(N, K, torch.Generator().manual_seed(3), 118, 130)
    x = torch.randn((5, K), device=DEV).to(dt)
    ys = []
    for blocks in (q.reshape(N, K // 32, 32), q):
        back.set_mx_weight(blocks, s)
        assert back.weight is None and torch.equal(back.qweight.cpu(), q)
        ys.append(back(x))
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ext().forward(x, q.to(DEV), s.to(DEV), back.bias.detach()))
    with pytest.raises(RuntimeError):  # a host tensor is refused
        back(x.cpu())


@pytest.mark.parametrize("dt", DTS)
def test_layer_backward_is_the_torch_composition(dt):
    N, K, M = 64, 128, 24
    layer = layer_with(N, K, dt).train()
    x = torch.randn((M, K), device=DEV).to(dt).requires_grad_(True)
    y = layer(x)
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), q, s, layer.bias.detach()))
    gy = torch.randn_like(y)
    y.backward(gy)
    torch.testing.assert_close(x.grad, gy.float().mm(ext().dequant(q, s, torch.float32)).to(dt), rtol=0, atol=0)
    torch.testing.assert_close(layer.weight.grad, gy.float().t().mm(x.detach().float()).to(dt), rtol=0, atol=0)
    torch.testing.assert_close(layer.bias.grad, gy.float().sum(0).to(dt), rtol=0, atol=0)


@pytest.mark.parametrize("M", sorted({1, B + 1}))
def test_graph_replay_equals_eager(M):
    dt, N, K = torch.float16, 256, 512
    layer = layer_with(N, K, dt).eval()
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
        for _ in range(3):  # several replays, each against the eager result on new data
            x.copy_(torch.randn((M, K), device=DEV).to(dt))
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, layer(x)) and not torch.equal(out, eager)
