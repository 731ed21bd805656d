"""Ternary linear layer on the MI355X: pack / unpack against the numpy packer, the raw product D bit-exact against a float64 matmul, the
decode and matrix-pipe forms bit-identical to each other, the layer output bit-exact against the torch CPU composition
`(D.to(dt) * scale_a) * alpha`, the qweight-only state_dict, and the straight-through backward against its float64 formula."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16, torch.float32]


def np_pack(t):
    return np.stack([np.packbits(t != 0, axis=1, bitorder="little"), np.packbits(t > 0, axis=1, bitorder="little")])


def rand_trits(N, K, g, p0=0.4):
    t = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1
    return torch.where(torch.rand((N, K), generator=g) < p0, torch.zeros_like(t), t)


def signs(x, bias=None):
    """+-1 of (x + bias) >= 0, the sum rounded in x's dtype (as torch adds), as float64 on the CPU."""
    xb = x if bias is None else x + bias
    return torch.where(xb.cpu() >= 0, 1.0, -1.0).double()


def ref_D(s, t):
    return s @ t.double().t()


def ext():
    from bitorch_engine.extensions import ternary_linear_cuda
    return ternary_linear_cuda


@pytest.mark.parametrize("N", [1, 33, 4096, 11008])
@pytest.mark.parametrize("K", [32, 4096, 11008])
def test_pack_unpack_match_the_numpy_packer(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    t = rand_trits(N, K, g)
    q = ext().w_pack(t.to(DEV))
    assert q.shape == (2, N, K // 8) and q.dtype == torch.uint8
    assert np.array_equal(q.cpu().numpy(), np_pack(t.numpy()))
    assert torch.equal(ext().w_unpack(q).cpu(), t)


def _both_forms(x, q, bias, sa, alpha, dt):
    """y of the two C entries, called directly: the decode form and the matrix-pipe form."""
    from bitorch_engine import _hip
    L = _hip.lib()
    M, K = x.shape
    N = q.shape[1]
    y1 = torch.empty((M, N), dtype=dt, device=DEV)
    y2 = torch.empty((M, N), dtype=dt, device=DEV)
    assert L.bie_ternary_linear_fused(_hip.ptr(x), _hip.ptr(bias), _hip.ptr(q), _hip.ptr(sa), _hip.ptr(alpha), _hip.ptr(y1), M, N, K, _hip.dt(x), 0, None) == 0
    img = ext().fp4_image(q)
    ximg = torch.empty(L.bie_binary_fp4_image_bytes(M, K), dtype=torch.uint8, device=DEV)
    assert L.bie_binary_fp4_image_from_values(_hip.ptr(x), _hip.ptr(bias), _hip.ptr(ximg), M, K, _hip.dt(x), None) == 0
    assert L.bie_ternary_linear_layer_fp4(_hip.ptr(ximg), _hip.ptr(img), _hip.ptr(sa), _hip.ptr(alpha), _hip.ptr(y2), M, N, K, _hip.dt(x), None) == 0
    torch.cuda.synchronize()
    return y1, y2


_WEIGHTS = {}


def _weights(K, N):
    """(trits on the CPU, qweight on the GPU), made once per shape for the module."""
    if (K, N) not in _WEIGHTS:
        t = rand_trits(N, K, torch.Generator().manual_seed(K + N))
        _WEIGHTS[(K, N)] = (t, ext().w_pack(t.to(DEV)))
    return _WEIGHTS[(K, N)]


@pytest.mark.parametrize("M", [1, 2, 3, 4, 8, 16, 17, 33, 64, 65, 128, 512, 4096])
def test_raw_product_is_exact_and_the_two_forms_agree(M):
    g = torch.Generator().manual_seed(M)
    for (K, N) in ((4096, 4096), (4096, 11008), (11008, 4096), (96, 40)):
        t, q = _weights(K, N)
        x = torch.randn((M, K), generator=g).half()
        D = ext().forward(x.to(DEV), q).cpu()
        rows = torch.arange(M) if M <= 64 else torch.randperm(M, generator=g)[:48]
        cols = torch.arange(N) if N <= 64 else torch.randperm(N, generator=g)[:96]
        ref = ref_D(signs(x[rows]), t[cols])
        assert torch.equal(D[rows][:, cols].double(), ref), (M, K, N)
        if ext().fused_ok(M, N, K):
            for dt in DTS:
                bias = (torch.randn(K, generator=g) * 0.3).to(dt).to(DEV)
                sa = torch.tensor(0.037, dtype=dt, device=DEV)
                alpha = (torch.rand(N, generator=g) * 0.1).to(dt).to(DEV)
                y1, y2 = _both_forms(x.to(dt).to(DEV), q, bias, sa, alpha, dt)
                assert torch.equal(y1, y2), (M, K, N, dt)


def _layer(K, N, dt, trits=None, alpha=None, g=None):
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    layer = TernaryLinearCuda(K, N, dtype=dt).to(DEV)
    if trits is None:
        trits = rand_trits(N, K, g)
        alpha = torch.rand(N, generator=g) * 0.05 + 0.001
    layer.set_ternary_weight(trits, alpha)
    with torch.no_grad():
        layer.bias_a.copy_((torch.randn(K, generator=g) * 0.2).to(dt))
    return layer.eval(), trits


def _ref_layer(x, layer, trits, dt):
    """(D.to(dt) * scale_a) * alpha on the CPU in dt, D from float64."""
    x2 = x.reshape(-1, x.shape[-1]).cpu()
    D = ref_D(signs(x2, layer.bias_a.detach().cpu()), trits)
    y = (D.to(dt) * layer.scale_a.detach().cpu()) * layer.scale_w.cpu()
    return y.reshape(list(x.shape[:-1]) + [trits.shape[0]])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 3, 4, 16, 40, 300])
def test_layer_forward_bit_exact(dt, M):
    g = torch.Generator().manual_seed(M + 11)
    K, N = 512, 200
    layer, trits = _layer(K, N, dt, g=g)
    x = torch.randn((M, K), generator=g).to(dt).to(DEV)
    with torch.no_grad():
        y = layer(x)
    assert layer.scale_a.item() != 0  # lazily initialised from the first x
    assert torch.equal(layer.scale_a.detach().cpu(), (2 * x.abs().mean()).to(dt).cpu())
    assert y.dtype == dt
    assert torch.equal(y.cpu(), _ref_layer(x, layer, trits, dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [3072, 1024])
def test_layer_forward_on_the_large_gemm_tiles(dt, N):
    """M = 4096: N = 3072 takes the matrix-pipe form's 256 x 256 tile instance, N = 1024 the 128 x 128 one, each with the per-column
    alpha epilogue; bit-exact."""
    g = torch.Generator().manual_seed(17)
    K, M = 256, 4096
    layer, trits = _layer(K, N, dt, g=g)
    x = torch.randn((M, K), generator=g).to(dt).to(DEV)
    with torch.no_grad():
        y = layer(x)
    assert torch.equal(y.cpu(), _ref_layer(x, layer, trits, dt))


@pytest.mark.parametrize("dt", DTS)
def test_layer_forward_edges(dt):
    g = torch.Generator().manual_seed(5)
    # all-zero rows (alpha 0), all-+1 rows, K = 32
    K, N = 32, 70
    trits = rand_trits(N, K, g)
    trits[3] = 0
    trits[4] = 1
    alpha = torch.rand(N) * 0.1
    alpha[3] = 0
    layer, _ = _layer(K, N, dt, trits, alpha, g=g)
    with torch.no_grad():
        layer.scale_a.fill_(0.5)
        for shape in ((1, K), (2, 5, K), (40, K), (4, 70, K)):  # 3-D inputs, both forms
            x = torch.randn(shape, generator=g).to(dt).to(DEV)
            y = layer(x)
            assert y.shape == shape[:-1] + (N,)
            ref = _ref_layer(x, layer, trits, dt)
            assert torch.equal(y.cpu(), ref)
            assert (y[..., 3] == 0).all()
        # non-contiguous input
        xt = torch.randn((K, 24), generator=g).to(dt).to(DEV).t()
        assert not xt.is_contiguous()
        assert torch.equal(layer(xt).cpu(), _ref_layer(xt.contiguous(), layer, trits, dt))
    # N = 1
    layer1, t1 = _layer(256, 1, dt, g=g)
    with torch.no_grad():
        for M in (1, 9, 300):
            x = torch.randn((M, 256), generator=g).to(dt).to(DEV)
            assert torch.equal(layer1(x).cpu(), _ref_layer(x, layer1, t1, dt))


def test_prepare_params_ternarizes_the_latent_weight():
    from bitorch_engine.layers.qlinear.ternary import ternarize
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    torch.manual_seed(0)
    layer = TernaryLinearCuda(256, 96, dtype=torch.half, threshold_factor=0.6).to(DEV)
    layer.prepare_params()
    t, alpha, _ = ternarize(layer.weight, 0.6)
    assert torch.equal(ext().w_unpack(layer.qweight).cpu(), t.cpu())
    assert torch.equal(layer.scale_w.cpu(), alpha.half().cpu())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_state_dict_qweight_only_round_trip(dt):
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    torch.manual_seed(1)
    a = TernaryLinearCuda(512, 130, dtype=dt).to(DEV).eval()
    x = torch.randn((7, 512), device=DEV).to(dt)
    with torch.no_grad():
        a.bias_a.normal_(0, 0.1)
        a.generate_quantized_weight(qweight_only=True)
        ya = a(x)
    sd = a.state_dict()
    assert set(sd) == {"qweight", "scale_w", "bias_a", "scale_a"}
    assert sd["qweight"].shape == (2, 130, 64) and sd["scale_w"].shape == (130,)
    b = TernaryLinearCuda(512, 130, dtype=dt).to(DEV).eval()
    b.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert b.weight is None
    with torch.no_grad():
        assert torch.equal(b(x), ya)
        x2 = torch.randn((300, 512), device=DEV).to(dt)
        assert torch.equal(b(x2), a(x2))


def test_backward_matches_the_float64_formula():
    from bitorch_engine.layers.qlinear.ternary import ternarize
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    torch.manual_seed(2)
    K, N, M = 256, 48, 20
    layer = TernaryLinearCuda(K, N, dtype=torch.float32).to(DEV).train()
    with torch.no_grad():
        layer.bias_a.normal_(0, 0.1)
        layer.scale_a.fill_(0.8)
    x = torch.randn((M, K), device=DEV, requires_grad=True)
    y = layer(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    t, alpha, _ = ternarize(layer.weight, 0.7)
    xb = (x.detach() + layer.bias_a.detach()).double().cpu()
    s = torch.where(xb >= 0, 1.0, -1.0).double()
    sa = layer.scale_a.detach().double().cpu()
    G = gy.double().cpu()
    assert torch.equal(y.detach().cpu().double(), ((s @ t.double().cpu().t()).float() * layer.scale_a.detach().cpu() * alpha.cpu()).double())
    inside = ((xb / sa >= -1) & (xb / sa <= 1)).double()
    gx = (G @ (t.double().cpu() * alpha.double().cpu()[:, None])) * inside
    torch.testing.assert_close(x.grad.double().cpu(), gx, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(layer.bias_a.grad.double().cpu(), gx.sum(0), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(layer.weight.grad.double().cpu(), G.t() @ (s * sa), rtol=1e-4, atol=1e-4)
    gsa = (gx * s).sum() / np.sqrt(s.numel())
    torch.testing.assert_close(layer.scale_a.grad.double().cpu(), gsa, rtol=1e-4, atol=1e-4)


def test_toy_training_loss_decreases_and_eval_forward_with_grad_runs():
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    torch.manual_seed(4)
    K, N, M = 128, 16, 64
    layer = TernaryLinearCuda(K, N, dtype=torch.float32).to(DEV).train()
    x = torch.randn((M, K), device=DEV)
    target = torch.randn((M, N), device=DEV) * 3
    opt = torch.optim.Adam(layer.parameters(), lr=2e-2)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(layer(x), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    layer.eval()
    xg = torch.randn((3, K), device=DEV, requires_grad=True)
    y = layer(xg)  # eval mode, grad enabled: runs, and is differentiable in x
    y.sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
    with torch.no_grad():
        assert torch.equal(layer(xg.detach()), y.detach())


def test_cpu_checkpoint_with_a_latent_weight_loads_onto_the_layers_device():
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    torch.manual_seed(6)
    src = TernaryLinearCuda(128, 32, dtype=torch.float32)  # a CPU checkpoint with its latent weight
    dst = TernaryLinearCuda(128, 32, dtype=torch.float32).to(DEV)
    dst.generate_quantized_weight(qweight_only=True)
    assert dst.weight is None
    dst.load_state_dict(src.state_dict())
    assert dst.weight.device.type == "cuda" and torch.equal(dst.weight.detach().cpu(), src.weight.detach())
    dst.train()
    y = dst(torch.randn((5, 128), device=DEV))
    y.sum().backward()
    assert dst.weight.grad is not None
