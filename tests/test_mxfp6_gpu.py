"""MXFP6 weight-only linear layer (W6A16, csrc/mxfp6.hip) on the MI355X: both forward forms against a float64 product of x and the restated
W (mxfp6_ref.dequant) within the contract's tolerance, bit-identical on exact data, the fp16 range, NaN and scale-0 blocks, row
independence under non-finite x, checkpoints (its own and MXFP6A8LinearCuda's), the straight-through backward with either grad_input,
graph replay and host-tensor refusal.  The tolerance is tests/test_mxfp4_gpu.py::check's: the arithmetic is the same (exact products,
an fp32 sum, one rounding)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import mxfp6_ref as ref  # noqa: E402
import fuzz_mxfp6 as F  # noqa: E402

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
rand_mx, ref_y, check = F.rand_mx, F.ref_y, F.check
B = F.decode_bound()  # the decode form's largest M: a host call, nothing is launched


def ext():
    from bitorch_engine.extensions import mxfp6_linear_cuda
    return mxfp6_linear_cuda


def forms_for(M):
    return (0, 1, -1) if M <= B else (1, -1)


def test_the_decode_bound_is_the_plan_bound():
    assert B >= 1 and F.plan_bound() == B
    for dt in DTS:
        assert ext().form(B, 4096, 4096, dt) == 0 and ext().form(B + 1, 4096, 4096, dt) == 1


_WEIGHTS = {}


def weights(K, N):
    """One random weight per (K, N), with its restatement on the GPU: shared by every M and dtype, never written."""
    if (K, N) not in _WEIGHTS:
        g = torch.Generator().manual_seed(K * 3 + N)
        q, s = rand_mx(N, K, g)
        _WEIGHTS[(K, N)] = (q.to(DEV), s.to(DEV), ref.dequant(q, s).to(DEV))
    return _WEIGHTS[(K, N)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N", [(32, 1), (96, 7), (2880, 33), (4096, 129), (96, 4096)])
# M = 17 and M = B = 32: the first and the last row of the 32-row decode instance
@pytest.mark.parametrize("M", sorted({1, 2, 3, 8, 17, B, B + 1, 64, 129, 300}))
def test_forward_both_forms_against_float64(M, K, N, dt):
    qd, sd, W = weights(K, N)
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    bias = torch.randn(N, generator=g).to(dt)
    e = ext().col_exp(sd)
    for b in (None, bias):
        yref, a = ref_y(x, W, b)
        for form in forms_for(M):
            y = ext().forward(x.to(DEV), qd, sd, None if b is None else b.to(DEV), e if form else None, form=form)
            assert y.dtype == dt and y.shape == (M, N)
            check(y, yref, a, K, dt, f"form {form} bias {b is not None}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", sorted({1, 5, B, 64, 300}))
def test_exact_data_is_bit_identical_across_forms_and_to_the_reference(M, dt):
    g = torch.Generator().manual_seed(M)
    N, K = 72, 4096
    q, s = rand_mx(N, K, g, 125, 129)  # scales 2^-2 .. 2^2: every partial sum is a multiple of 2^-5 below 2^18, exact in fp32
    x = torch.randint(-2, 3, (M, K), generator=g).to(dt)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dt)
    yref, _ = ref_y(x, ref.dequant(q, s), bias)
    want = yref.to(dt)
    qd, sd = q.to(DEV), s.to(DEV)
    for form in forms_for(M):
        y = ext().forward(x.to(DEV), qd, sd, bias.to(DEV), form=form)
        assert torch.equal(y, want), (form, (y.double() - want.double()).abs().max().item())


@pytest.mark.parametrize("M", sorted({1, 8, B, 64}))
def test_fp16_range_wider_than_an_fp16_image(M):
    g = torch.Generator().manual_seed(11)
    N, K = 64, 2048
    q = torch.randint(0, 256, (N, K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)
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
    colmax = ref.mx.e8m0(e.cpu()).to(DEV)
    for form in forms_for(M):
        y = ext().forward(x.to(DEV), q.to(DEV), s.to(DEV), None, e, form=form)
        assert torch.isfinite(y).all()
        prefill = (ext().form(M, N, K, torch.float16) if form < 0 else form) == 1
        # the prefill form's rebias: a weight keeps 2^-24 of its column's largest scale (fp16 subnormal step), the decode form all of it
        rebias = x.to(DEV).double().abs().sum(1, keepdim=True) * colmax[None, :] * 2.0 ** -24 if prefill else 0.0
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
    for M in sorted({1, B, 64}):
        for form in forms_for(M):
            y = ext().forward(x[:M].to(DEV), q.to(DEV), s.to(DEV), form=form)
            assert torch.isnan(y[:, 3]).all()
            keep = torch.ones(N, dtype=torch.bool)
            keep[3] = False
            assert not torch.isnan(y[:, keep]).any()
            keep[7] = False  # may flush to zero: checked just below
            assert (y[:, 7].double().abs() <= 2.0 ** -100).all()  # 2^-127 weights: at most subnormal fp32 partials, zero in the dtype
            check(y[:, keep], yref[:M][:, keep.to(DEV)], a[:M][:, keep.to(DEV)], K, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", sorted({min(B, 7), 130}))
def test_non_finite_rows_leave_the_other_rows_bit_identical(M, dt):
    g = torch.Generator().manual_seed(17 + M)
    N, K = 70, 160
    q, s = rand_mx(N, K, g)
    qd, sd = q.to(DEV), s.to(DEV)
    x = torch.randn((M, K), generator=g).to(dt)
    xb = x.clone()
    r_nan, r_inf = 1 % M, (M - 1)
    xb[r_nan, 37], xb[r_inf, 150] = float("nan"), float("inf")
    keep = torch.ones(M, dtype=torch.bool)
    keep[r_nan] = keep[r_inf] = False
    for form in forms_for(M):
        y0 = ext().forward(x.to(DEV), qd, sd, form=form)
        y1 = ext().forward(xb.to(DEV), qd, sd, form=form)
        assert torch.isfinite(y0).all()
        assert torch.isnan(y1[r_nan]).all() and not torch.isfinite(y1[r_inf]).any()
        assert torch.equal(y1[keep], y0[keep]), form


def layer_with(N, K, dt, bias=False, seed=0, **kw):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6LinearCuda
    torch.manual_seed(seed)
    return MXFP6LinearCuda(K, N, bias=bias, dtype=dt, **kw).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_set_mx_weight_both_layouts_and_state_dict(dt):
    g = torch.Generator().manual_seed(3)
    N, K = 48, 192
    q, s = rand_mx(N, K, g)
    layer = layer_with(N, K, dt, bias=True).eval()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(N, generator=g).to(dt))
    x = torch.randn((5, K), generator=g).to(dt).to(DEV)
    yref, a = ref_y(x.cpu(), ref.dequant(q, s), layer.bias.detach().cpu())
    ys = []
    for blocks in (q.reshape(N, K // 32, 24), q):
        layer.set_mx_weight(blocks, s)
        assert layer.weight is None and torch.equal(layer.qweight.cpu(), q)
        ys.append(layer(x))
        check(ys[-1], yref, a, K, dt)
    assert torch.equal(ys[0], ys[1])
    sd = layer.state_dict()
    assert set(sd) == {"qweight", "scales", "bias"}
    other = layer_with(N, K, dt, bias=True, seed=9).eval()
    other.load_state_dict(sd)
    assert other.weight is None and torch.equal(other(x), ys[0])


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
def test_cross_loads_with_the_w6a8_layer(dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A8LinearCuda
    N, K = 24, 128
    w16 = layer_with(N, K, dt, bias=True, seed=1).eval()
    w16.prepare_params()
    torch.manual_seed(2)
    a8 = MXFP6A8LinearCuda(K, N, bias=True, dtype=dt).to(DEV).eval()
    a8.load_state_dict(w16.state_dict())
    a8.prepare_params()
    assert torch.equal(a8.qweight, w16.qweight) and torch.equal(a8.scales, w16.scales) and torch.equal(a8.e_col, w16.e_col)
    torch.manual_seed(3)
    a8b = MXFP6A8LinearCuda(K, N, bias=True, dtype=dt).to(DEV).eval()
    a8b.generate_quantized_weight(qweight_only=True)
    back = layer_with(N, K, dt, bias=True, seed=4).eval()
    back.load_state_dict(a8b.state_dict())
    assert back.weight is None and torch.equal(back.qweight, a8b.qweight) and torch.equal(back.scales, a8b.scales)
    x = torch.randn((4, K), device=DEV).to(dt)
    W = ref.dequant(a8b.qweight, a8b.scales)
    yref, a = ref_y(x.cpu(), W, a8b.bias.detach().cpu())
    check(back(x), yref, a, K, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["torch", "kernel"])
def test_backward_and_one_optimiser_step(mode, dt):
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as w6a8
    N, K, M = 64, 128, 24
    layer = layer_with(N, K, dt, bias=True, grad_input=mode).train()
    x = torch.randn((M, K), device=DEV).to(dt).requires_grad_(True)
    y = layer(x)
    q, s = ext().quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext().forward(x.detach(), q, s, layer.bias.detach()))
    gy = torch.randn_like(y)
    y.backward(gy)
    if mode == "torch":
        W = ext().dequant(q, s, torch.float32)
        torch.testing.assert_close(x.grad, gy.float().mm(W).to(dt), rtol=0, atol=0)
    else:
        torch.testing.assert_close(x.grad, w6a8.grad_input(gy, q, s), rtol=0, atol=0)
    torch.testing.assert_close(layer.weight.grad, gy.float().t().mm(x.detach().float()).to(dt), rtol=0, atol=0)
    torch.testing.assert_close(layer.bias.grad, gy.float().sum(0).to(dt), rtol=0, atol=0)
    before = layer(x).detach()
    torch.optim.SGD(layer.parameters(), lr=0.5).step()
    assert not torch.equal(layer(x).detach(), before)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", sorted({1, B, 64}))
def test_graph_replay_equals_eager(M, dt):
    N, K = 256, 512
    layer = layer_with(N, K, dt, bias=True).eval()
    x = torch.randn((M, K), device=DEV).to(dt)
    assert ext().form(M, N, K, dt) == (0 if M <= B else 1)  # both forms are replayed
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
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6LinearCuda
    cpu_layer = MXFP6LinearCuda(64, 8).eval()
    with pytest.raises(RuntimeError):
        cpu_layer(torch.randn((2, 64)).half())


@pytest.mark.parametrize("dt", DTS)
def test_e_col_is_only_needed_by_the_prefill_form(dt):
    g = torch.Generator().manual_seed(8)
    N, K = 200, 2880
    q, s = rand_mx(N, K, g, 110, 135)
    s[17, 60] = 255
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext().col_exp(sd)
    assert torch.equal(e.cpu(), s.amax(dim=1))
    for M in sorted({1, B, B + 8}):
        x = torch.randn((M, K), generator=g).to(dt).to(DEV)
        y = ext().forward(x, qd, sd)  # no e_col given: computed where the prefill form needs it
        assert torch.isnan(y[:, 17]).all() and torch.isfinite(y[:, :17]).all()
        torch.testing.assert_close(y, ext().forward(x, qd, sd, None, e, form=ext().form(M, N, K, dt)), rtol=0, atol=0, equal_nan=True)
