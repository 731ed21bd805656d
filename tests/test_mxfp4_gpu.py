"""MXFP4 linear layer on the MI355X: the quantise kernel bit-exact against the torch restatement (mxfp4_ref.py), dequant exact, both forward
forms against a float64 product of x and the restated W within the contract's tolerance, bit-identical on exact data, the fp16 range, NaN
and scale-0 blocks, checkpoints, the straight-through backward, graph replay and host-tensor refusal."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
_spec = importlib.util.spec_from_file_location("mxfp4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def ext():
    from bitorch_engine.extensions import mxfp4_linear_cuda
    return mxfp4_linear_cuda


def rand_mx(N, K, g, lo=118, hi=130):
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


def ref_y(x, W, bias=None):
    """float64 x . W^T (+ bias) on the GPU, with the absolute-value product the tolerance scales with."""
    xd, Wd = x.to(DEV).double(), W.to(DEV)
    y = xd @ Wd.t()
    a = xd.abs() @ Wd.abs().t()
    if bias is not None:
        y = y + bias.to(DEV).double()
        a = a + bias.to(DEV).double().abs()
    return y, a


def check(y, yref, absprod, K, dt):
    """The contract: exact or once-rounded products, an fp32 sum, one rounding to dt."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    tol = eps * yref.abs() + (K + 2) * 2.0 ** -23 * absprod + tiny
    err = (y.double() - yref).abs()
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), f"max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


@pytest.mark.parametrize("wdt", [torch.float32, torch.float16, torch.bfloat16])
def test_quantise_kernel_is_bit_exact(wdt):
    g = torch.Generator().manual_seed(1)
    N, K = 37, 1024
    lo, hi = {torch.float32: (-140, 120), torch.float16: (-24, 12), torch.bfloat16: (-130, 120)}[wdt]
    e = torch.randint(lo, hi, (N, K // 32), generator=g).float().repeat_interleave(32, dim=1)
    w = torch.randn((N, K), generator=g) * torch.exp2(e)
    # ties and saturation at the block's own scale: amax 4 * 2^t, values on the E2M1 midpoints
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.99, 6.0, 0.1, -0.0, 0.0])
    for r in range(0, N, 3):
        t = float(torch.randint(-10, 10, (1,), generator=g))
        w[r, :32] = 0.0
        w[r, 0] = 4.0 * 2.0 ** t
        w[r, 1:1 + len(mids)] = mids * 2.0 ** t * torch.where(torch.rand(len(mids), generator=g) < 0.5, -1.0, 1.0)
    w[N - 1, 32:64] = 0.0  # an all-zero block
    w = w.to(wdt)
    codes, scales = ref.quantize(w)
    q, s = ext().quantize(w.to(DEV))
    assert torch.equal(s.cpu(), scales)
    assert torch.equal(q.cpu(), ref.pack(codes))


def test_dequant_is_exact():
    g = torch.Generator().manual_seed(2)
    N, K = 16, 256 * 32
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.arange(256, dtype=torch.int32).repeat(N, 1).reshape(N, K // 32).to(torch.uint8)
    W = ref.dequant(q, s)
    got = ext().dequant(q.to(DEV), s.to(DEV), torch.float32).cpu()
    torch.testing.assert_close(got, W.float(), rtol=0, atol=0, equal_nan=True)
    for dt in DTS:
        got = ext().dequant(q.to(DEV), s.to(DEV), dt).cpu()
        torch.testing.assert_close(got, W.to(dt), rtol=0, atol=0, equal_nan=True)
    assert torch.equal(ext().col_exp(s.to(DEV)).cpu(), torch.full((N,), 255, dtype=torch.uint8))
    s2 = torch.randint(0, 255, (N, 7), generator=g, dtype=torch.int32).to(torch.uint8)
    assert torch.equal(ext().col_exp(s2.to(DEV)).cpu(), s2.amax(dim=1))


SHAPES = [(M, K, N) for M in (1, 2, 3, 8, 16, 17, 64) for K, N in ((32, 1), (96, 7), (4096, 33))] + \
         [(M, K, N) for M in (1, 8, 16, 17, 64) for K, N in ((4096, 4096), (11008, 33), (96, 4096))] + \
         [(4096, 4096, 33), (4096, 96, 4096), (4096, 11008, 7), (4096, 4096, 4096)] + \
         [(M, 96, 7) for M in (4, 5, 9)]  # a full 4-row decode instance, the first rows of the 8-row and the 16-row instance


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_forward_both_forms_against_float64(M, K, N, dt):
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    q, s = rand_mx(N, K, g)
    W = ref.dequant(q, s)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    bias = (torch.randn(N, generator=g)).to(dt) if (M + N) % 2 else None
    yref, a = ref_y(x, W, bias)
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext().col_exp(sd)
    for form in ((0, 1) if M <= 16 else (1,)):
        y = ext().forward(x.to(DEV), qd, sd, None if bias is None else bias.to(DEV), e, form=form)
        assert y.dtype == dt and y.shape == (M, N)
        check(y, yref, a, K, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 5, 16, 64, 300])
def test_exact_data_is_bit_identical_across_forms(M, dt):
    g = torch.Generator().manual_seed(M)
    N, K = 72, 4096
    q, s = rand_mx(N, K, g, 125, 129)  # scales 2^-2 .. 2^2: every partial sum is a multiple of 2^-3 below 2^21, exact in fp32
    x = torch.randint(-2, 3, (M, K), generator=g).to(dt)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dt)
    yref, _ = ref_y(x, ref.dequant(q, s), bias)
    want = yref.to(dt)
    qd, sd = q.to(DEV), s.to(DEV)
    for form in ((0, 1) if M <= 16 else (1, -1)):
        y = ext().forward(x.to(DEV), qd, sd, bias.to(DEV), form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("M", [1, 8, 64])
def test_fp16_range_wider_than_an_fp16_image(M):
    g = torch.Generator().manual_seed(11)
    N, K = 64, 2048
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    lo = torch.randint(103, 144, (N, 1), generator=g)  # per column a range of scale codes inside 103 .. 143 (2^-24 .. 2^16)
    hi = torch.minimum(lo + torch.randint(0, 41, (N, 1), generator=g), torch.tensor(143))
    s = (lo + (torch.rand((N, K // 32), generator=g) * (hi - lo + 1)).floor().long()).clamp(103, 143)
    s[0], s[1], s[2] = 143, 103, torch.arange(K // 32) % 41 + 103  # all 2^16, all 2^-24, the whole range within one column
    s = s.to(torch.uint8)
    W = ref.dequant(q, s)
    assert W.abs().max() > 65504
    x = (torch.randn((M, K), generator=g) * 2.0 ** -12).half()
    yref, a = ref_y(x, W)
    e = ext().col_exp(s.to(DEV))
    colmax = ref.e8m0(e.cpu()).to(DEV)
    for form in ((0, 1) if M <= 16 else (1,)):
        y = ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), None, e, form=form)
        assert torch.isfinite(y).all()
        # the prefill form's rebias: a weight keeps 2^-24 of its column's largest scale (fp16 subnormal step), the decode form all of it
        rebias = x.to(DEV).double().abs().sum(1, keepdim=True) * colmax[None, :] * 2.0 ** -24 if form == 1 else 0.0
        tol = 2.0 ** -10 * yref.abs() + (K + 2) * 2.0 ** -23 * a + rebias + 2.0 ** -24
        err = (y.double() - yref).abs()
        assert (err <= tol).all(), (form, err.max().item())


@pytest.mark.parametrize("dt", DTS)
def test_scale_255_gives_nan_in_that_column_and_scale_0_is_tiny(dt):
    g = torch.Generator().manual_seed(5)
    N, K = 40, 256
    q, s = rand_mx(N, K, g)
    s[3, 2] = 255
    s[7, :] = 0      # a whole row of 2^-127 blocks
    s[9, 1] = 0      # one scale-0 block among normal ones
    x = torch.randn((64, K), generator=g).to(dt)
    W = ref.dequant(q, s)
    Wf = torch.nan_to_num(W, nan=0.0)
    yref, a = ref_y(x, Wf)
    for M in (1, 16, 64):
        for form in ((0, 1) if M <= 16 else (1,)):
            y = ext().forward(x[:M].to(DEV), q.to(DEV), s.to(DEV), form=form)
            assert torch.isnan(y[:, 3]).all()
            keep = torch.ones(N, dtype=torch.bool)
            keep[3] = False
            assert not torch.isnan(y[:, keep]).any()
            keep[7] = False  # may flush to zero: checked just below
            assert (y[:, 7].double().abs() <= 2.0 ** -100).all()  # 2^-127 weights: at most subnormal fp32 partials, zero in the dtype
            check(y[:, keep], yref[:M][:, keep.to(DEV)], a[:M][:, keep.to(DEV)], K, dt)


def layer_with(N, K, dt, bias=False, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda
    torch.manual_seed(seed)
    return MXFP4LinearCuda(K, N, bias=bias, dtype=dt).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_set_mx_weight_checkpoint_layout_and_state_dict(dt):
    g = torch.Generator().manual_seed(3)
    N, K = 48, 192
    q, s = rand_mx(N, K, g)
    layer = layer_with(N, K, dt, bias=True).eval()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(N, generator=g).to(dt))
    layer.set_mx_weight(q.reshape(N, K // 32, 16), s)  # the checkpoint's [N, K/32, 16] blocks
    assert layer.weight is None and torch.equal(layer.qweight.cpu(), q)
    x = torch.randn((5, K), generator=g).to(dt).to(DEV)
    y = layer(x)
    yref, a = ref_y(x.cpu(), ref.dequant(q, s), layer.bias.detach().cpu())
    check(y, yref, a, K, dt)
    sd = layer.state_dict()
    assert set(sd) == {"qweight", "scales", "bias"}
    other = layer_with(N, K, dt, bias=True, seed=9).eval()
    other.load_state_dict(sd)
    assert other.weight is None and torch.equal(other(x), y)


@pytest.mark.parametrize("dt", DTS)
def test_qweight_only_checkpoint_and_latent_round_trip(dt):
    N, K = 33, 96
    layer = layer_with(N, K, dt, bias=True).eval()
    x = torch.randn((3, 4, K), device=DEV).to(dt)
    y0 = layer(x)
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y0.reshape(12, N), ext().forward(x.reshape(12, K), q, s, layer.bias.detach()))
    full = layer.state_dict()
    assert set(full) == {"weight", "qweight", "scales", "bias"}
    layer.generate_quantized_weight(qweight_only=True)
    sd = layer.state_dict()
    assert "weight" not in sd
    fresh = layer_with(N, K, dt, bias=True, seed=4).eval()
    fresh.load_state_dict(sd)
    assert fresh.weight is None and torch.equal(fresh(x), y0)
    back = layer_with(N, K, dt, bias=True, seed=5).eval()
    back.load_state_dict(full)  # a latent weight re-derives qweight / scales
    assert torch.equal(back(x), y0)


@pytest.mark.parametrize("dt", DTS)
def test_backward_and_one_optimiser_step(dt):
    N, K, M = 64, 128, 24
    layer = layer_with(N, K, dt, bias=True).train()
    x = torch.randn((M, K), device=DEV).to(dt).requires_grad_(True)
    y = layer(x)
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), q, s, layer.bias.detach()))
    gy = torch.randn_like(y)
    y.backward(gy)
    W = ext().dequant(q, s, torch.float32)
    torch.testing.assert_close(x.grad, gy.float().mm(W).to(dt), rtol=0, atol=0)
    torch.testing.assert_close(layer.weight.grad, gy.float().t().mm(x.detach().float()).to(dt), rtol=0, atol=0)
    torch.testing.assert_close(layer.bias.grad, gy.float().sum(0).to(dt), rtol=0, atol=0)
    before = layer(x).detach()
    torch.optim.SGD(layer.parameters(), lr=0.5).step()
    assert not torch.equal(layer(x).detach(), before)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 8, 64])
def test_graph_replay_equals_eager(M, dt):
    N, K = 256, 512
    layer = layer_with(N, K, dt, bias=True).eval()
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
    N, K = 40, 256
    layer = layer_with(N, K, dt).eval()
    base = torch.randn((K, 6), device=DEV).to(dt)
    x = base.t()  # [6, K], not contiguous
    assert not x.is_contiguous()
    with torch.no_grad():
        assert torch.equal(layer(x), layer(x.contiguous()))
        x3 = torch.randn((2, 3, K), device=DEV).to(dt)
        y3 = layer(x3)
        assert y3.shape == (2, 3, N) and torch.equal(y3.reshape(6, N), layer(x3.reshape(6, K)))


def test_host_tensor_is_refused():
    layer = layer_with(8, 64, torch.float16).eval()
    with pytest.raises(RuntimeError):
        layer(torch.randn((2, 64)).half())
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda
    cpu_layer = MXFP4LinearCuda(64, 8).eval()
    with pytest.raises(RuntimeError):
        cpu_layer(torch.randn((2, 64)).half())


@pytest.mark.parametrize("dt", DTS)
def test_e_col_is_only_needed_by_the_prefill_form(dt):
    g = torch.Generator().manual_seed(8)
    N, K = 1000, 11008
    q, s = rand_mx(N, K, g, 110, 135)
    s[17, 300] = 255
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext().col_exp(sd)
    assert torch.equal(e.cpu(), s.amax(dim=1))  # one wave per row: 344 scale bytes, a NaN block in row 17
    for M in (1, 16, 40):
        x = torch.randn((M, K), generator=g).to(dt).to(DEV)
        y = ext().forward(x, qd, sd)
        assert torch.isnan(y[:, 17]).all() and torch.isfinite(y[:, :17]).all()
        torch.testing.assert_close(y, ext().forward(x, qd, sd, None, e, form=ext().form(M, N, K, dt)), rtol=0, atol=0, equal_nan=True)
