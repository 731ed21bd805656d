"""MXFP4 W4A4 linear layer on the MI355X: the activation quantiser bit-exact against the torch restatement (mxfp4_a4_ref.py), both forward
forms against the float64 product of the restated x^ and W^ within the weight-only layer's tolerance, the test that tells the layer from
the weight-only one, exact data bit-identical across forms, the non-finite row rule, the scale-255 column rule, weight interchange with
MXFP4LinearCuda, the straight-through backward, graph replay and host-tensor refusal."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
_spec = importlib.util.spec_from_file_location("mxfp4_a4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_a4_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

DECODE_ROWS = 64  # the decode form's largest M (bie_mxfp4_a4_linear_forward refuses it beyond)


def ext():
    from bitorch_engine.extensions import mxfp4_a4_linear_cuda
    return mxfp4_a4_linear_cuda


def forms(M):
    return (0, 1) if M <= DECODE_ROWS else (1,)


def rand_mx(N, K, g, lo=118, hi=130):
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


def check(y, yref, absprod, K, dt, what=""):
    tol = ref.tolerance(yref, absprod, K, dt)
    err = (y.double() - yref).abs()
    print(f"{what} max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), f"{what} max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


@pytest.mark.parametrize("dt", DTS)
def test_activation_quantiser_is_bit_exact(dt):
    g = torch.Generator().manual_seed(1)
    M, K = 37, 1024
    lo, hi = (-24, 12) if dt == torch.float16 else (-130, 120)
    e = torch.randint(lo, hi, (M, K // 32), generator=g).float().repeat_interleave(32, dim=1)
    x = torch.randn((M, K), generator=g) * torch.exp2(e)
    # ties and saturation at the block's own scale: amax 4 * 2^t, values on the E2M1 midpoints, both zeros
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.99, 6.0, 0.1, -0.0, 0.0])
    for r in range(0, M, 3):
        t = float(torch.randint(-10, 10, (1,), generator=g))
        x[r, :32] = 0.0
        x[r, 0] = 4.0 * 2.0 ** t
        x[r, 1:1 + len(mids)] = mids * 2.0 ** t * torch.where(torch.rand(len(mids), generator=g) < 0.5, -1.0, 1.0)
    x[M - 1, 32:64] = 0.0   # an all-zero block
    x[M - 2, 64:96] = -0.0  # a block of negative zeros
    x = x.to(dt)
    # subnormal blocks of the dtype
    sub = torch.arange(32, dtype=torch.int16).repeat(K // 32)
    x[5] = (sub + 1).view(dt) if dt == torch.float16 else (sub * 3 + 1).view(dt)
    assert torch.isfinite(x.float()).all()
    xq, xs, flag = ref.quantize_act(x)
    q, s, f = ext().quantize_act(x.to(DEV))
    assert torch.equal(f.cpu(), flag) and not flag.any()
    assert torch.equal(s.cpu(), xs)
    assert torch.equal(q.cpu(), xq)
    for Kx in (32, 96, 11008):  # one block, K % 128 != 0, more than one pass of the workgroup over the row
        x2 = torch.randn((3, Kx), generator=g).to(dt)
        xq, xs, flag = ref.quantize_act(x2)
        q, s, f = ext().quantize_act(x2.to(DEV))
        assert torch.equal(q.cpu(), xq) and torch.equal(s.cpu(), xs) and torch.equal(f.cpu(), flag)


SHAPES = [(M, K, N) for M in (1, 2, 3, 8, 16, 17, 64) for K, N in ((32, 1), (96, 7), (4096, 33))] + \
         [(M, K, N) for M in (1, 8, 16, 17, 64) for K, N in ((4096, 4096), (11008, 33), (96, 4096))] + \
         [(4096, 4096, 33), (4096, 96, 4096), (4096, 11008, 7), (4096, 4096, 4096)] + \
         [(M, K, N) for M in (32, 33, 65, 128, 129) for K, N in ((160, 70), (32, 130), (1056, 258))] + \
         [(7, 4096, 11008), (64, 4096, 11008), (300, 4096, 11008)] + [(257, 160, 21846)] + [(33, 96, 130)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_forward_every_form_against_float64(M, K, N, dt):
    """(257, 160, 21846): 3 x 171 = 513 tiles of 128 x 128, the (2, 2) tile instance with ragged edges in M, N and K."""
    g =torch.Generator().manual_seed(M * 7 + K * 3 + N)
    q, s = rand_mx(N, K, g)
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


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", [(8, 4096, 256), (64, 1024, 128), (3, 32, 16), (200, 1024, 128)])
def test_the_layer_is_w4a4_and_not_the_weight_only_layer(M, K, N, dt):
    """On Gaussian x the result matches the x^ reference within tol, and the weight-only result x . W^^T lies OUTSIDE tol for more than
    half of the outputs: activation rounding moves y by about 12 % rms."""
    g = torch.Generator().manual_seed(K + M)
    q, s = rand_mx(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt)
    xq, xs, flag = ref.quantize_act(x)
    yref, a = ref.reference(xq, xs, flag, q, s, None, DEV)
    tol = ref.tolerance(yref, a, K, dt)
    y_wonly = x.to(DEV).double() @ ref.mx.dequant(q, s).to(DEV).t()
    outside = ((y_wonly - yref).abs() > tol).double().mean().item()
    print(f"weight-only result outside tol: {100 * outside:.1f} %")
    assert outside > 0.5
    for form in forms(M):
        y = ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), form=form)
        check(y, yref, a, K, dt, f"form {form}")
        assert ((y.double() - y_wonly).abs() > tol).double().mean().item() > 0.5


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 5, 16, 33, 64, 300])
def test_exact_data_is_bit_identical_across_forms_and_against_float64(M, dt):
    g = torch.Generator().manual_seed(M)
    N, K = 72, 4096 + 32
    q, s = rand_mx(N, K, g, 126, 128)
    xq, xs = rand_mx(M, K, g, 126, 128)  # chosen codes and scales 2^-1 .. 2^1: every partial sum is a multiple of 2^-4 below 2^20, exact in fp32
    flag = torch.zeros(M, dtype=torch.uint8)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dt)
    yref, _ = ref.reference(xq, xs, flag, q, s, bias, DEV)
    want = yref.to(dt)
    for form in forms(M) + (-1,):
        y = ext().gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), q.to(DEV), s.to(DEV), bias.to(DEV), dtype=dt, form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("dt", DTS)
def test_scale_sums_between_minus_100_and_100(dt):
    """Chosen scales at the ends of the tested range: sx + sw - 254 in [-100, 100], one block so the fp32 value is exact."""
    g = torch.Generator().manual_seed(4)
    N, K, M = 48, 32, 40
    q, _ = rand_mx(N, K, g)
    xq, _ = rand_mx(M, K, g)
    for sx, sw in ((27, 127), (127, 27), (77, 77), (227, 127), (127, 227), (177, 177), (2, 252), (252, 2)):
        xs = torch.full((M, 1), sx, dtype=torch.uint8)
        s = torch.full((N, 1), sw, dtype=torch.uint8)
        flag = torch.zeros(M, dtype=torch.uint8)
        yref, a = ref.reference(xq, xs, flag, q, s, None, DEV)
        want = yref.float()  # exact: one block sum times a power of two
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
    q, s = rand_mx(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt)
    clean = {form: ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), form=form) for form in forms(M)}
    for bad, pos in ((float("inf"), 0), (float("-inf"), K - 1), (float("nan"), 5), (float("nan"), K - 32)):
        for row in (0, M - 1, M // 2):
            xb = x.clone()
            xb[row, pos] = bad
            _, _, f = ext().quantize_act(xb.to(DEV))
            want_flag = torch.zeros(M, dtype=torch.uint8)
            want_flag[row] = 1
            assert torch.equal(f.cpu(), want_flag)
            for form in forms(M):
                y = ext().forward(xb.to(DEV), q.to(DEV), s.to(DEV), form=form)
                assert torch.isnan(y[row]).all(), (bad, pos, row, form)
                keep = torch.ones(M, dtype=torch.bool)
                keep[row] = False
                assert torch.equal(y[keep], clean[form][keep]), (bad, pos, row, form)


@pytest.mark.parametrize("dt", DTS)
def test_scale_255_gives_nan_in_that_column(dt):
    g = torch.Generator().manual_seed(5)
    N, K = 40, 256
    q, s = rand_mx(N, K, g)
    s[3, 2] = 255
    s[39, 7] = 255
    x = torch.randn((70, K), generator=g).to(dt)
    bias = torch.randn(N, generator=g).to(dt)
    for M in (1, 16, 64, 70):
        xq, xs, flag = ref.quantize_act(x[:M])
        yref, a = ref.reference(xq, xs, flag, q, s, bias, DEV)
        keep = torch.ones(N, dtype=torch.bool, device=DEV)
        keep[3] = keep[39] = False
        for form in forms(M):
            y = ext().forward(x[:M].to(DEV), q.to(DEV), s.to(DEV), bias.to(DEV), form=form)
            assert torch.isnan(y[:, 3]).all() and torch.isnan(y[:, 39]).all()
            check(y[:, keep], yref[:, keep], a[:, keep], K, dt, f"M {M} form {form}")


def layer_with(cls, N, K, dt, bias=False, seed=0):
    torch.manual_seed(seed)
    return cls(K, N, bias=bias, dtype=dt).to(DEV)


def layers():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A4LinearCuda, MXFP4LinearCuda
    return MXFP4A4LinearCuda, MXFP4LinearCuda


@pytest.mark.parametrize("dt", DTS)
def test_weights_interchange_with_the_weight_only_layer(dt):
    A4, W4 = layers()
    g = torch.Generator().manual_seed(3)
    N, K = 48, 192
    q, s = rand_mx(N, K, g)
    x = torch.randn((5, K), generator=g).to(dt).to(DEV)
    a4 = layer_with(A4, N, K, dt, bias=True).eval()
    a4.set_mx_weight(q.reshape(N, K // 32, 16), s)
    w4 = layer_with(W4, N, K, dt, bias=True, seed=3).eval()
    w4.load_state_dict(a4.state_dict())  # A4 -> weight-only
    assert set(a4.state_dict()) == {"qweight", "scales", "bias"}
    assert torch.equal(w4.qweight, a4.qweight) and torch.equal(w4.scales, a4.scales)
    from bitorch_engine.extensions import mxfp4_linear_cuda
    assert torch.equal(w4(x), mxfp4_linear_cuda.forward(x, q.to(DEV), s.to(DEV), a4.bias.detach()))
    back = layer_with(A4, N, K, dt, bias=True, seed=5).eval()
    back.load_state_dict(w4.state_dict())  # weight-only -> A4
    assert torch.equal(back(x), a4(x))
    assert torch.equal(a4(x), ext().forward(x, q.to(DEV), s.to(DEV), a4.bias.detach()))
    # a latent-weight state dict of the weight-only layer
    lat = layer_with(W4, N, K, dt, seed=7).eval()
    lat(x)
    fresh = layer_with(A4, N, K, dt, seed=8).eval()
    fresh.load_state_dict(lat.state_dict())
    fresh(x)
    assert torch.equal(fresh.qweight, lat.qweight) and torch.equal(fresh.scales, lat.scales)
    fresh.generate_quantized_weight(qweight_only=True)
    assert "weight" not in fresh.state_dict()


@pytest.mark.parametrize("dt", DTS)
def test_backward_and_one_optimiser_step(dt):
    A4, _ = layers()
    N, K, M = 64, 128, 24
    layer = layer_with(A4, N, K, dt, bias=True).train()
    x = torch.randn((M, K), device=DEV).to(dt).requires_grad_(True)
    y = layer(x)
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), q, s, layer.bias.detach()))
    gy = torch.randn_like(y)
    y.backward(gy)
    W = ref.mx.dequant(q, s).to(DEV)
    xq, xs, _ = ref.quantize_act(x.detach().cpu())
    xh = ref.dequant_act(xq, xs).to(DEV)
    # the float64 formulas; the layer computes them in fp32 and rounds once to the dtype
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    for got, want, absw in ((x.grad, gy.double() @ W, gy.double().abs() @ W.abs()),
                            (layer.weight.grad, gy.double().t() @ xh, gy.double().abs().t() @ xh.abs()),
                            (layer.bias.grad, gy.double().sum(0), gy.double().abs().sum(0))):
        tol = eps * want.abs() + (M + N + 2) * 2.0 ** -23 * absw + 2.0 ** -24
        assert ((got.double() - want).abs() <= tol).all()
    # the weight gradient uses the QUANTISED activations: it differs from gy^T . x
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
    A4, _ = layers()
    N, K = 256, 512
    layer = layer_with(A4, N, K, dt, bias=True).eval()
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
    A4, _ = layers()
    N, K = 40, 256
    layer = layer_with(A4, N, K, dt).eval()
    base = torch.randn((K, 6), device=DEV).to(dt)
    x = base.t()
    assert not x.is_contiguous()
    with torch.no_grad():
        assert torch.equal(layer(x), layer(x.contiguous()))
        x3 = torch.randn((2, 3, K), device=DEV).to(dt)
        y3 = layer(x3)
        assert y3.shape == (2, 3, N) and torch.equal(y3.reshape(6, N), layer(x3.reshape(6, K)))


def test_host_tensor_is_refused():
    A4, _ = layers()
    layer = layer_with(A4, 8, 64, torch.float16).eval()
    with pytest.raises(RuntimeError):
        layer(torch.randn((2, 64)).half())
    with pytest.raises(RuntimeError):
        ext().quantize_act(torch.randn((2, 64)).half())
    with pytest.raises(RuntimeError):
        ext().forward(torch.zeros((65, 64), dtype=torch.half, device=DEV), layer.qweight, layer.scales, form=0)  # no fallback past M = 64
