"""Ternary conv2d on the MI355X: the raw D of every form (VALU one-launch, matrix-pipe one-launch, general path) bit-exact against a float64
CPU conv2d of the -1-padded signs, the forms bit-identical to each other, the layer output bit-exact against the torch CPU composition
`((D.to(dt) * scale_a).to(dt) * alpha).to(dt)`, the checkpoint contract, the straight-through backward against its float64 formula, and a
graph-captured eval forward (no host sync)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16, torch.float32]

# the binary one-launch test's geometries (tests/test_gpu_parity.py): ResNet stages, stride 2 and 3, 1x1, pad 0 and 2, OC not a multiple of
# 64 / 128, one and several row chunks, and the batch sizes of the issue; plus the 64-channel stage (matrix pipe only)
GEOMS = [(1, 512, 7, 7, 512, 3, 1, 1), (32, 512, 7, 7, 512, 3, 1, 1), (128, 512, 7, 7, 512, 3, 1, 1), (5, 512, 7, 7, 200, 3, 1, 1),
         (2, 256, 14, 14, 256, 3, 1, 1), (3, 256, 14, 14, 512, 3, 2, 1), (1, 128, 28, 28, 128, 3, 1, 1), (9, 128, 28, 28, 256, 3, 2, 1),
         (2, 256, 14, 14, 512, 1, 2, 0), (3, 128, 9, 11, 64, 3, 2, 1), (2, 512, 5, 60, 72, 3, 1, 1), (1, 128, 13, 64, 130, 1, 1, 0),
         (2, 256, 6, 6, 96, 3, 1, 0), (70, 128, 4, 4, 64, 3, 1, 2), (1, 128, 19, 12, 32, 3, 3, 1), (8, 512, 29, 6, 200, 3, 3, 1),
         (10, 256, 9, 7, 129, 1, 3, 1), (2, 64, 56, 56, 64, 3, 1, 1), (1, 64, 56, 56, 128, 1, 2, 0)]


def ext():
    from bitorch_engine.extensions import ternary_conv2d_cuda
    return ternary_conv2d_cuda


def rand_trits(shape, g, p0=0.4):
    t = torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1
    return torch.where(torch.rand(shape, generator=g) < p0, torch.zeros_like(t), t)


def special_input(shape, g):
    x = torch.randn(shape, generator=g)
    x.view(-1)[::97] = 0.0
    x.view(-1)[5::131] = -0.0
    x.view(-1)[11::257] = float("nan")
    return x


def ref_D(x, t, stride, pad, dil):
    """float64 CPU conv2d of pad(s, value=-1) with the trits; s = +1 where x >= 0 (NaN: -1)."""
    s = torch.where(x.cpu() >= 0, 1.0, -1.0).double()
    return F.conv2d(F.pad(s, (pad,) * 4, value=-1.0), t.double(), stride=stride, dilation=dil)


def all_forms(x, q, k, st, pad, dil, **kw):
    """{form: y} for every form that can run the geometry: 1 / 2 through their C entries, 0 (general path) always."""
    e = ext()
    out = {0: e.conv_general(x, q, k, st, pad, dil, **kw)}
    for f, fn in ((1, e.conv_fused), (2, e.conv_mfma)):
        try:
            out[f] = fn(x, q, k, st, pad, dil, **kw)
        except RuntimeError as err:  # a geometry outside that form (the C entry's BIE_ERR_UNSUPPORTED, or no lane image below 128 channels)
            assert "outside the one-launch" in str(err) or "multiple of 128" in str(err), str(err)
    return out


@pytest.mark.parametrize("B,C,H,W,OC,k,st,pad", GEOMS)
def test_raw_D_is_exact_on_every_form_and_the_forms_agree(B, C, H, W, OC, k, st, pad):
    e = ext()
    g = torch.Generator().manual_seed(B * 7 + C + H + W + OC + k)
    f = e.form(B, C, H, W, OC, k, st, pad, 1)
    assert f in (1, 2), (B, C, H, W, OC, k, st, pad)  # every geometry of the list takes a one-launch form
    x = special_input((B, C, H, W), g)
    for p0 in (0.0, 0.4, 1.0):
        t = rand_trits((OC, C, k, k), g, p0)
        q = e.w_pack(t.to(DEV))
        assert torch.equal(e.w_unpack(q, C, k).cpu(), t)
        want = ref_D(x, t, st, pad, 1)
        for dt in DTS:
            ys = all_forms(x.to(dt).to(DEV), q, k, st, pad, 1, raw=True)
            assert f in ys and (len(ys) >= 2)
            for form, y in ys.items():
                assert y.dtype == torch.float32
                assert torch.equal(y.cpu().double(), want), (form, dt, p0)
        # the dispatch agrees
        assert torch.equal(e.forward(x.to(DEV), q, k, st, pad, 1).cpu().double(), want)


@pytest.mark.parametrize("B,C,H,W,OC,k,st,pad,dil", [(2, 512, 7, 7, 64, 5, 1, 2, 1), (3, 128, 9, 9, 40, 3, 1, 2, 2), (2, 32, 12, 12, 48, 3, 1, 1, 1),
                                                    (1, 96, 10, 10, 33, 3, 2, 1, 1), (1, 1024, 5, 5, 64, 3, 1, 1, 1), (1, 64, 4, 140, 16, 3, 1, 1, 1),
                                                    (2, 64, 9, 9, 16, 7, 1, 3, 1)])
def test_general_path_is_exact(B, C, H, W, OC, k, st, pad, dil):
    e = ext()
    assert e.form(B, C, H, W, OC, k, st, pad, dil) == 0
    g = torch.Generator().manual_seed(C + OC + k + dil)
    x = special_input((B, C, H, W), g)
    t = rand_trits((OC, C, k, k), g)
    q = e.w_pack(t.to(DEV))
    want = ref_D(x, t, st, pad, dil)
    for dt in DTS:
        assert torch.equal(e.forward(x.to(dt).to(DEV), q, k, st, pad, dil).cpu().double(), want), dt


def ref_layer(D, sa, alpha, dt):
    return ((D.to(dt) * sa.cpu()).to(dt) * alpha.cpu()[None, :, None, None]).to(dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,C,H,W,OC,k,st,pad", [(2, 512, 7, 7, 200, 3, 1, 1), (32, 256, 14, 14, 256, 3, 1, 1), (3, 128, 9, 11, 64, 3, 2, 1),
                                                 (2, 64, 56, 56, 64, 3, 1, 1), (2, 32, 8, 8, 40, 3, 1, 1)])
def test_layer_output_bit_exact_on_every_form(dt, B, C, H, W, OC, k, st, pad):
    e = ext()
    g = torch.Generator().manual_seed(B + C + OC)
    x = special_input((B, C, H, W), g).to(dt)
    t = rand_trits((OC, C, k, k), g)
    t[3] = 0                                   # an all-zero output channel
    alpha = (torch.rand(OC, generator=g) * 0.1).to(dt)
    alpha[5] = 0                               # an alpha = 0 channel
    sa = torch.tensor(0.37, dtype=dt)
    q = e.w_pack(t.to(DEV))
    want = ref_layer(ref_D(x.float(), t, st, pad, 1), sa, alpha, dt)
    ys = all_forms(x.to(DEV), q, k, st, pad, 1, scale_a=sa.to(DEV), alpha=alpha.to(DEV))
    for form, y in ys.items():
        assert y.dtype == dt
        assert torch.equal(y.cpu(), want), (form, dt)
    # an all-zero weight: y = 0 everywhere, on every form
    q0 = e.w_pack(torch.zeros((OC, C, k, k), dtype=torch.int8, device=DEV))
    for form, y in all_forms(x.to(DEV), q0, k, st, pad, 1, scale_a=sa.to(DEV), alpha=alpha.to(DEV)).items():
        assert (y == 0).all(), form


def _layer(C, OC, k, st, pad, dt, g, dil=1):
    from bitorch_engine.layers.qconv.ternary.cuda import TernaryConv2dCuda
    layer = TernaryConv2dCuda(C, OC, k, st, pad, dil, dtype=dt).to(DEV)
    t = rand_trits((OC, C, k, k), g)
    alpha = torch.rand(OC, generator=g) * 0.05 + 0.001
    layer.set_ternary_weight(t, alpha)
    with torch.no_grad():
        layer.bias_a.copy_((torch.randn(C, generator=g) * 0.2).to(dt))
    return layer.eval(), t


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,C,H,OC,k,st,pad,dil", [(1, 512, 7, 512, 3, 1, 1, 1), (8, 256, 14, 128, 3, 2, 1, 1), (4, 64, 28, 64, 1, 2, 0, 1),
                                                   (2, 96, 9, 48, 5, 1, 2, 1), (2, 128, 9, 32, 3, 1, 2, 2)])
def test_layer_forward_bit_exact(dt, B, C, H, OC, k, st, pad, dil):
    g = torch.Generator().manual_seed(B + C + H + OC)
    layer, t = _layer(C, OC, k, st, pad, dt, g, dil)
    x = torch.randn((B, C, H, H), generator=g).to(dt).to(DEV)
    with torch.no_grad():
        y = layer(x)
    assert torch.equal(layer.scale_a.detach().cpu(), (2 * x.abs().mean()).to(dt).cpu())
    xb = (x + layer.bias_a.detach().view(1, -1, 1, 1)).cpu()
    want = ref_layer(ref_D(xb.float(), t, st, pad, dil), layer.scale_a.detach(), layer.scale_w, dt)
    assert y.dtype == dt and torch.equal(y.cpu(), want)


def np_pack_conv(t):
    """The numpy restatement of the plane layout (tests/test_ternary_conv_cpu.py): the linear's planes over the OIHW flatten order."""
    r = t.reshape(t.shape[0], -1)
    return np.stack([np.packbits(r != 0, axis=1, bitorder="little"), np.packbits(r > 0, axis=1, bitorder="little")])


@pytest.mark.parametrize("OC,C,k", [(2, 32, 3), (33, 64, 1), (200, 512, 3), (16, 96, 5)])
def test_w_pack_matches_the_numpy_packer(OC, C, k):
    g = torch.Generator().manual_seed(OC + C + k)
    t = rand_trits((OC, C, k, k), g)
    q = ext().w_pack(t.to(DEV))
    assert q.shape == (2, OC, C * k * k // 8) and q.dtype == torch.uint8
    assert np.array_equal(q.cpu().numpy(), np_pack_conv(t.numpy()))
    assert torch.equal(ext().w_unpack(q, C, k).cpu(), t)


def test_a_host_qweight_is_refused_before_any_launch():
    """x on the GPU, qweight (or an image) still on the host, e.g. from a CPU checkpoint: RuntimeError from the device check, nothing
    launched on a host pointer (the stream stays clean and the next call computes the right D)."""
    e = ext()
    g = torch.Generator().manual_seed(9)
    t = rand_trits((64, 128, 3, 3), g)
    q_host = e.w_pack(t.to(DEV)).cpu()
    x = torch.randn((2, 128, 7, 7), generator=g).half().to(DEV)
    sa, alpha = torch.tensor(0.5, dtype=torch.half, device=DEV), torch.ones(64, dtype=torch.half, device=DEV)
    calls = [lambda: e.forward(x, q_host, 3, 1, 1, 1), lambda: e.layer_forward(x, q_host, sa, alpha, 3, 1, 1, 1),
             lambda: e.conv_fused(x, q_host, 3, 1, 1, 1), lambda: e.conv_mfma(x, q_host, 3, 1, 1, 1),
             lambda: e.conv_general(x, q_host, 3, 1, 1, 1), lambda: e.weight_lanes(q_host, 128, 3), lambda: e.weight_fp4_image(q_host, 128, 3)]
    for call in calls:
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    q = q_host.to(DEV)
    lanes = tuple(w.cpu() for w in e.weight_lanes(q, 128, 3))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        e.conv_fused(x, q, 3, 1, 1, 1, lanes=lanes)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        e.conv_mfma(x, q, 3, 1, 1, 1, wimage=e.weight_fp4_image(q, 128, 3).cpu())
    torch.cuda.synchronize()
    assert torch.equal(e.forward(x, q, 3, 1, 1, 1).cpu().double(), ref_D(x.float(), t, 1, 1, 1))


def test_constructor_refuses_channels_not_a_multiple_of_32():
    from bitorch_engine.layers.qconv.ternary.cuda import TernaryConv2dCuda
    with pytest.raises(ValueError):
        TernaryConv2dCuda(48, 16, 3)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_state_dict_qweight_only_round_trip(dt):
    from bitorch_engine.layers.qconv.ternary.cuda import TernaryConv2dCuda
    torch.manual_seed(1)
    a = TernaryConv2dCuda(128, 72, 3, 1, 1, dtype=dt).to(DEV).eval()
    x = torch.randn((3, 128, 9, 9), device=DEV).to(dt)
    with torch.no_grad():
        a.bias_a.normal_(0, 0.1)
        a.generate_quantized_weight(qweight_only=True)
        ya = a(x)
    sd = a.state_dict()
    assert set(sd) == {"qweight", "scale_w", "bias_a", "scale_a"}
    assert sd["qweight"].shape == (2, 72, 128 * 9 // 8) and sd["scale_w"].shape == (72,)
    b = TernaryConv2dCuda(128, 72, 3, 1, 1, dtype=dt).to(DEV).eval()
    b.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert b.weight is None
    with torch.no_grad():
        assert torch.equal(b(x), ya)
        x2 = torch.randn((64, 128, 9, 9), device=DEV).to(dt)   # the matrix-pipe form
        assert torch.equal(b(x2), a(x2))


def test_cpu_checkpoint_with_a_latent_weight_loads_onto_the_layers_device():
    from bitorch_engine.layers.qconv.ternary import TernaryConv2dBase  # noqa: F401
    from bitorch_engine.layers.qconv.ternary.cuda import TernaryConv2dCuda
    torch.manual_seed(6)
    src = TernaryConv2dCuda(64, 32, 3, 1, 1, dtype=torch.float32)      # a CPU checkpoint with its latent weight
    dst = TernaryConv2dCuda(64, 32, 3, 1, 1, dtype=torch.float32).to(DEV)
    dst.generate_quantized_weight(qweight_only=True)
    assert dst.weight is None
    dst.load_state_dict(src.state_dict())
    assert dst.weight.device.type == "cuda" and torch.equal(dst.weight.detach().cpu(), src.weight.detach())
    dst.train()
    y = dst(torch.randn((2, 64, 8, 8), device=DEV))
    y.sum().backward()
    assert dst.weight.grad is not None
    dst.eval()
    with torch.no_grad():  # the packed form of the loaded latent weight
        from bitorch_engine.layers.qlinear.ternary import ternarize
        t, alpha, _ = ternarize(dst.weight.reshape(32, -1), 0.7)
        dst.prepare_params()
        assert torch.equal(ext().w_unpack(dst.qweight, 64, 3).cpu(), t.reshape(32, 64, 3, 3).cpu())


@pytest.mark.parametrize("st,pad,dil", [(1, 1, 1), (2, 1, 1), (1, 2, 2)])
def test_backward_matches_the_float64_formula(st, pad, dil):
    from bitorch_engine.layers.qlinear.ternary import ternarize
    from bitorch_engine.layers.qconv.ternary.cuda import TernaryConv2dCuda
    torch.manual_seed(2)
    B, C, H, OC, k = 3, 64, 9, 40, 3
    layer = TernaryConv2dCuda(C, OC, k, st, pad, dil, dtype=torch.float32).to(DEV).train()
    with torch.no_grad():
        layer.bias_a.normal_(0, 0.1)
        layer.scale_a.fill_(0.8)
    x = torch.randn((B, C, H, H), device=DEV, requires_grad=True)
    y = layer(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    t, alpha, _ = ternarize(layer.weight.reshape(OC, -1), 0.7)
    t = t.reshape(OC, C, k, k).double().cpu()
    xb = (x.detach() + layer.bias_a.detach().view(1, -1, 1, 1)).double().cpu()
    s = torch.where(xb >= 0, 1.0, -1.0).double()
    sa = layer.scale_a.detach().double().cpu()
    G = gy.double().cpu()
    D = F.conv2d(F.pad(s, (pad,) * 4, value=-1.0), t, stride=st, dilation=dil)
    assert torch.equal(y.detach().cpu(), (D.float() * layer.scale_a.detach().cpu() * alpha.cpu()[None, :, None, None]))
    w_hat = t * alpha.double().cpu()[:, None, None, None]
    inside = ((xb / sa >= -1) & (xb / sa <= 1)).double()
    gx = torch.nn.grad.conv2d_input(xb.shape, w_hat, G, stride=st, padding=pad, dilation=dil) * inside
    torch.testing.assert_close(x.grad.double().cpu(), gx, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(layer.bias_a.grad.double().cpu(), gx.sum((0, 2, 3)), rtol=1e-4, atol=1e-4)
    gw = torch.nn.grad.conv2d_weight(F.pad(s, (pad,) * 4, value=-1.0) * sa, w_hat.shape, G, stride=st, dilation=dil)
    torch.testing.assert_close(layer.weight.grad.double().cpu(), gw, rtol=1e-4, atol=1e-3)
    gsa = (gx * s).sum() / s.numel() ** 0.5
    torch.testing.assert_close(layer.scale_a.grad.double().cpu(), gsa, rtol=1e-4, atol=1e-4)


def test_toy_training_loss_decreases_and_eval_forward_with_grad_runs():
    from bitorch_engine.layers.qconv.ternary.cuda import TernaryConv2dCuda
    torch.manual_seed(4)
    layer = TernaryConv2dCuda(64, 16, 3, 1, 1, dtype=torch.float32).to(DEV).train()
    x = torch.randn((8, 64, 8, 8), device=DEV)
    target = torch.randn((8, 16, 8, 8), device=DEV) * 3
    opt = torch.optim.Adam(layer.parameters(), lr=2e-2)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = F.mse_loss(layer(x), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    layer.eval()
    xg = torch.randn((2, 64, 8, 8), device=DEV, requires_grad=True)
    y = layer(xg)  # eval mode, grad enabled: runs, and is differentiable in x, bias_a and scale_a
    y.sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
    assert layer.bias_a.grad is not None and layer.scale_a.grad is not None
    with torch.no_grad():
        assert torch.equal(layer(xg.detach()), y.detach())


@pytest.mark.parametrize("B,C,H,OC", [(1, 512, 7, 512), (32, 512, 7, 512), (2, 64, 16, 48)])
def test_eval_forward_replays_under_graph_capture(B, C, H, OC):
    """No host sync in the eval forward: after warm-up (scale_a initialised, images cached) it captures and replays bit-identically."""
    g = torch.Generator().manual_seed(B + C)
    layer, _ = _layer(C, OC, 3, 1, 1, torch.float16, g)
    x = torch.randn((B, C, H, H), generator=g).half().to(DEV)
    with torch.no_grad():
        want = layer(x)
        layer(x)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            layer(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = layer(x)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, want)
