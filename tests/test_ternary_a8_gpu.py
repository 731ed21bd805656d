"""Ternary weights x int8 per-token activations on the MI355X: the quantiser exactly against its torch restatement, the raw D of both
forms exactly against a float64 product of the trits and q (exact: |D| < 2^53), the two forms bit-identical, the layer output bit-exact
against the torch composition dt((float(D) * r) * alpha), checkpoints, the straight-through backward, graph replay and host-tensor refusal."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16, torch.float32]


def ext():
    from bitorch_engine.extensions import ternary_a8_linear_cuda
    return ternary_a8_linear_cuda


def rand_trits(N, K, g, p0=0.4):
    t = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1
    return torch.where(torch.rand((N, K), generator=g) < p0, torch.zeros_like(t), t)


def ref_quant(x):
    """The INTEGRATION.md restatement on the CPU in fp32: (q int8 [M, K], r fp32 [M])."""
    xf = x.detach().cpu().float()
    a = xf.abs().amax(dim=1).clamp(min=1e-5) if xf.shape[1] else torch.full((xf.shape[0],), 1e-5)
    s = torch.full_like(a, 127.0) / a  # a correctly rounded division (127.0 / a would be 127 * reciprocal(a) in torch)
    q = torch.round(xf * s[:, None]).clamp(-128, 127).to(torch.int8)
    return q, a / 127.0


def ref_D(q, t):
    """Exact int64 D = q . t^T (a float64 product on the GPU: every partial sum is an integer below 2^53)."""
    return (q.to(DEV).double() @ t.to(DEV).double().t()).cpu().long()


def ref_y(D, r, alpha, dt):
    return ((D.float() * r[:, None]) * alpha.cpu().float()[None, :]).to(dt)


_W = {}


def weights(N, K):
    if (N, K) not in _W:
        t = rand_trits(N, K, torch.Generator().manual_seed(N * 31 + K))
        _W[(N, K)] = (t, ext().w_pack(t.to(DEV)))
    return _W[(N, K)]


def rand_x(M, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, K), generator=g) * torch.rand((M, 1), generator=g) * 4
    return x.to(dt).to(DEV)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 3, 4, 5, 64, 4096])
@pytest.mark.parametrize("K", [32, 96, 4096, 11008])
def test_quantize_matches_the_torch_restatement(dt, M, K):
    x = rand_x(M, K, dt, M * 7 + K)
    if M > 2:
        x[1] = 0                      # all-zero row: a = 1e-5, q = 0
        x[2, : K // 2] = 0.5          # exact ties after the scale: x * s hits .5 steps
        x[2, K // 2:] = -127.0
    q, r = ext().quantize(x)
    rq, rr = ref_quant(x)
    assert q.dtype == torch.int8 and q.shape == (M, K) and r.dtype == torch.float32
    assert torch.equal(q.cpu(), rq)
    assert torch.equal(r.cpu(), rr)


# (N, K) pairs per M: every N of {1, 33, 4096, 11008} and every K of {32, 96, 4096, 4128, 11008} appears for each M
PAIRS_SMALL = [(1, 4128), (33, 96), (4096, 4096), (11008, 32), (4096, 11008), (33, 4128), (11008, 4096), (1, 32)]
PAIRS_LARGE = [(1, 4128), (33, 96), (4096, 4096), (11008, 32), (4096, 11008)]


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8, 16, 17, 33, 64, 65, 128, 512, 4096])
def test_raw_D_is_exact_and_the_forms_agree(M):
    pairs = PAIRS_SMALL if M <= 128 else PAIRS_LARGE
    for N, K in pairs:
        t, qw = weights(N, K)
        x = rand_x(M, K, torch.float16, M + N + K)
        q, _ = ref_quant(x)
        want = ref_D(q, t)
        d = ext().forward(x, qw)
        assert d.dtype == torch.int32 and torch.equal(d.cpu().long(), want), (M, N, K)
        g = ext().linear_gemm(x, qw, raw=True)
        assert torch.equal(g.cpu().long(), want), (M, N, K)
        if ext().fused_ok(M, N, K):
            f = ext().linear_fused(x, qw, raw=True)
            assert torch.equal(f.cpu().long(), want), (M, N, K)


def test_fused_bound_reaches_the_decode_shapes():
    for K in (4096, 11008):
        for M in (1, 2, 3, 4):
            assert ext().fused_ok(M, 11008, K)
    assert not ext().fused_ok(4096, 4096, 4096)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(1, 4096, 4096), (3, 11008, 4096), (8, 33, 96), (16, 3072, 4128), (64, 1, 32), (512, 3072, 4096),
                                   (4096, 11008, 4096), (4096, 4096, 11008)])
def test_layer_output_is_bit_exact(dt, M, N, K):
    t, qw = weights(N, K)
    g = torch.Generator().manual_seed(M + N)
    alpha = (torch.rand(N, generator=g) * 0.05 + 0.001).to(dt)
    alpha[0] = 0  # an alpha_n = 0 row
    x = rand_x(M, K, dt, N + K)
    x[0] = 0      # an all-zero x row: y = 0
    q, r = ref_quant(x)
    want = ref_y(ref_D(q, t), r, alpha, dt)
    y = ext().layer_forward(x, qw, alpha.to(DEV))
    assert y.dtype == dt and torch.equal(y.cpu(), want), (dt, M, N, K)
    assert (y[0] == 0).all() and (y[:, 0] == 0).all()
    yg = ext().linear_gemm(x, qw, alpha.to(DEV))
    assert torch.equal(yg, y)
    if ext().fused_ok(M, N, K):
        assert torch.equal(ext().linear_fused(x, qw, alpha.to(DEV)), y)


def test_edge_cases_M0_and_extremes():
    t, qw = weights(33, 96)
    alpha = torch.full((33,), 0.5, dtype=torch.float16, device=DEV)
    y = ext().layer_forward(torch.empty((0, 96), dtype=torch.float16, device=DEV), qw, alpha)
    assert y.shape == (0, 33)
    q, r = ext().quantize(torch.empty((0, 96), dtype=torch.float16, device=DEV))
    assert q.shape == (0, 96) and r.shape == (0,)
    x = torch.zeros((3, 96), dtype=torch.float16)
    x[0, 5], x[0, 6] = 65504.0, -65504.0
    x[1, :] = torch.finfo(torch.float16).tiny
    x = x.to(DEV)
    rq, rr = ref_quant(x)
    q, r = ext().quantize(x)
    assert torch.equal(q.cpu(), rq) and torch.equal(r.cpu(), rr)
    xb = torch.tensor([[3.3895e38, -3.3895e38] + [1e-38] * 30, [0.0] * 32], dtype=torch.bfloat16).to(DEV)
    q, r = ext().quantize(xb)
    rq, rr = ref_quant(xb)
    assert torch.equal(q.cpu(), rq) and torch.equal(r.cpu(), rr)


def _layer(K, N, dt, **kw):
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryA8LinearCuda
    torch.manual_seed(K + N)
    return TernaryA8LinearCuda(K, N, dtype=dt, **kw).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_layer_module_eval_and_flatten(dt):
    from bitorch_engine.layers.qlinear.ternary import ternarize_absmean
    layer = _layer(256, 96, dt).eval()
    x = rand_x(6, 256, dt, 1).reshape(2, 3, 256)
    with torch.no_grad():
        y = layer(x)
    t, alpha = ternarize_absmean(layer.weight)
    q, r = ref_quant(x.reshape(6, 256))
    want = ref_y(ref_D(q, t.cpu()), r, alpha.to(dt), dt).reshape(2, 3, 96)
    assert y.shape == (2, 3, 96) and torch.equal(y.cpu(), want)


def test_state_dict_round_trips():
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryA8LinearCuda
    a = _layer(128, 40, torch.float16).eval()
    x = rand_x(5, 128, torch.float16, 2)
    with torch.no_grad():
        y = a(x)
    # with the latent weight
    sd = a.state_dict()
    assert set(sd) == {"weight", "qweight", "scale_w"}
    b = TernaryA8LinearCuda(128, 40, dtype=torch.float16).to(DEV).eval()
    b.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(b(x), y)
    # qweight only
    a.generate_quantized_weight(qweight_only=True)
    sd = a.state_dict()
    assert set(sd) == {"qweight", "scale_w"}
    c = TernaryA8LinearCuda(128, 40, dtype=torch.float16).to(DEV).eval()
    c.load_state_dict(sd)
    assert c.weight is None
    with torch.no_grad():
        assert torch.equal(c(x), y)
    # a CPU checkpoint onto the GPU layer
    d = TernaryA8LinearCuda(128, 40, dtype=torch.float16).to(DEV).eval()
    d.load_state_dict({k: v.cpu() for k, v in sd.items()})
    assert d.qweight.is_cuda
    with torch.no_grad():
        assert torch.equal(d(x), y)
    e = TernaryA8LinearCuda(128, 40, dtype=torch.float16).to(DEV)
    e.generate_quantized_weight(qweight_only=True)
    e.load_state_dict({k: v.cpu() for k, v in b.state_dict().items()})  # a latent weight back into a qweight-only layer
    assert e.weight is not None and e.weight.is_cuda


def test_ternary_linear_qweight_loads_into_the_a8_layer():
    from bitorch_engine.extensions import ternary_linear_cuda
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda, TernaryA8LinearCuda
    src = TernaryLinearCuda(256, 48, dtype=torch.float16).to(DEV).eval()
    src.prepare_params()
    src.generate_quantized_weight(qweight_only=True)
    sd = {k: v for k, v in src.state_dict().items() if k in ("qweight", "scale_w")}
    dst = TernaryA8LinearCuda(256, 48, dtype=torch.float16).to(DEV).eval()
    dst.load_state_dict(sd)
    assert torch.equal(ext().w_unpack(dst.qweight), ternary_linear_cuda.w_unpack(src.qweight))
    assert torch.equal(dst.scale_w, src.scale_w)


def test_set_ternary_weight():
    layer = _layer(64, 10, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    t = rand_trits(10, 64, g)
    alpha = torch.rand(10, generator=g)
    layer.set_ternary_weight(t, alpha)
    assert layer.weight is None and torch.equal(ext().w_unpack(layer.qweight).cpu(), t)
    x = rand_x(3, 64, torch.bfloat16, 9)
    q, r = ref_quant(x)
    with torch.no_grad():
        assert torch.equal(layer.train()(x).cpu(), ref_y(ref_D(q, t), r, alpha.to(torch.bfloat16), torch.bfloat16))


def test_backward_matches_the_float64_formula():
    layer = _layer(128, 24, torch.float32).train()
    x = rand_x(7, 128, torch.float32, 4).requires_grad_(True)
    gy = torch.randn((7, 24), generator=torch.Generator().manual_seed(1)).to(DEV)
    y = layer(x)
    y.backward(gy)
    from bitorch_engine.layers.qlinear.ternary import ternarize_absmean
    t, alpha = ternarize_absmean(layer.weight)
    q, r = ref_quant(x)
    w_hat = t.double().cpu() * alpha.double().cpu()[:, None]
    gx = gy.double().cpu() @ w_hat
    gw = gy.double().cpu().t() @ (q.double() * r.double()[:, None])
    np.testing.assert_allclose(x.grad.cpu().double().numpy(), gx.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(layer.weight.grad.cpu().double().numpy(), gw.numpy(), rtol=1e-5, atol=1e-5)
    # an eval forward with grad enabled is differentiable in x
    layer.eval()
    x2 = x.detach().clone().requires_grad_(True)
    layer(x2).sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all()


def test_a_toy_training_loss_decreases():
    torch.manual_seed(0)
    layer = _layer(64, 16, torch.float32).train()
    target = torch.randn((64, 16), device=DEV) * 0.1
    opt = torch.optim.Adam(layer.parameters(), lr=1e-2)
    g = torch.Generator().manual_seed(2)
    losses = []
    for _ in range(60):
        x = torch.randn((32, 64), generator=g).to(DEV)
        loss = ((layer(x) - x @ target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.mean(losses[-10:]) < 0.7 * np.mean(losses[:10]), losses


@pytest.mark.parametrize("M", [2, 300])
def test_graph_replay_equals_eager(M):
    layer = _layer(4096, 1024, torch.float16).eval()
    layer.prepare_params()
    x = rand_x(M, 4096, torch.float16, 3)
    with torch.no_grad():
        eager = layer(x)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            layer(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = layer(x)
        x.copy_(rand_x(M, 4096, torch.float16, 8))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, layer(x))
        assert not torch.equal(out, eager)


def test_host_tensors_are_refused():
    t, qw = weights(33, 96)
    x = torch.randn((2, 96), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        ext().forward(x, qw)
    with pytest.raises(RuntimeError, match="GPU"):
        ext().quantize(x)
    with pytest.raises(RuntimeError, match="GPU"):
        ext().layer_forward(x.to(DEV), qw.cpu(), torch.ones(33, dtype=torch.float16))
