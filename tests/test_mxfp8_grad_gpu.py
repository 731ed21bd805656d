"""MXFP8 input gradient on the MI355X (csrc/mxfp8_grad.hip) against a float64 product within the project's gradient contract
(mxfp6_grad_ref.tolerance, N as the length).  Scale codes are 124 .. 129, so e_blk - s <= 5 and every fp16 fragment is a normal number."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
_spec = importlib.util.spec_from_file_location("mxfp6_grad_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp6_grad_ref.py"))
gref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gref)
tolerance = gref.tolerance
dequant = gref._load("mxfp8_a8_ref").dequant  # float64, exact; NaN at a NaN code and over a scale-255 block
from bitorch_engine.extensions import mxfp8_grad_cuda as G  # noqa: E402


def rand_mx(N, K, g, lo=124, hi=129, exact=False):
    """Random bytes without the NaN codes (exact: exponent field 7 .. 10 or zero, |value| in 1 .. 15), scale codes lo .. hi."""
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    if exact:
        q = torch.where(q % 5 == 0, q & 0x80, (q & 0x87) | ((7 + (q >> 3) % 4) << 3))
    q = torch.where((q & 0x7F) == 0x7F, q - 1, q).to(torch.uint8)
    return q, torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)


def check(y, yref, absprod, n, dt):
    tol = tolerance(yref, absprod, n, dt)
    err = (y.double() - yref).abs()
    print(f"max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert torch.isfinite(y).all() and (err <= tol).all(), f"max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


@pytest.mark.parametrize("dt", DTS)
def test_dense_against_float64(dt):
    for K, N in ((32, 1), (96, 7), (160, 33), (256, 63), (256, 64), (256, 65), (128, 136)):
        g = torch.Generator().manual_seed(K + N)
        q, s = rand_mx(N, K, g)
        W = dequant(q, s).to(DEV)
        for M in (1, 129, 300):
            print(f"K {K} N {N} M {M}:", end=" ")
            gy = (torch.randn((M, N), generator=g) * 0.5).to(dt).to(DEV)
            check(G.grad_input(gy, q.to(DEV), s.to(DEV)), gy.double() @ W, gy.double().abs() @ W.abs(), N, dt)


@pytest.mark.parametrize("dt", DTS)
def test_element_map_on_one_hot_rows(dt):
    N, K = 140, 160
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    c = (n + 5 * k) % 254  # the 254 non-NaN bytes: 0 .. 126 and 128 .. 254
    codes = torch.where(c < 127, c, c + 1).to(torch.uint8)
    nonnan = set(range(256)) - {0x7F, 0xFF}
    assert set(codes[:, 0::2].flatten().tolist()) == nonnan and set(codes[:, 1::2].flatten().tolist()) == nonnan
    s = torch.randint(124, 130, (N, K // 32), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(torch.uint8)
    gx = G.grad_input(torch.eye(N).to(dt).to(DEV), codes.to(DEV), s.to(DEV))
    bad = (gx.double() != dequant(codes, s).to(DEV)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, the first at (n, k) = {bad[0].tolist()}"


@pytest.mark.parametrize("dt", DTS)
def test_exact_data_is_bit_identical(dt):
    from bitorch_engine.extensions import mxfp8_linear_cuda
    for M, K, N in ((1, 32, 1), (129, 160, 33), (300, 256, 2048)):
        g = torch.Generator().manual_seed(M + K + N)
        q, s = rand_mx(N, K, g, 125, 129, exact=True)
        gy = torch.randint(-2, 3, (M, N), generator=g).to(dt).to(DEV)
        qd, sd = q.to(DEV), s.to(DEV)
        gx = G.grad_input(gy, qd, sd)
        assert torch.equal(gx, (gy.double() @ dequant(q, s).to(DEV)).to(dt)), (M, K, N)
        assert torch.equal(gx, gy.float().mm(mxfp8_linear_cuda.dequant(qd, sd, torch.float32)).to(dt)), (M, K, N)  # the parent's torch path
        assert torch.equal(gx, G.grad_input(gy, qd, sd, G.blk_exp(sd))), (M, K, N)


@pytest.mark.parametrize("dt", DTS)
def test_nan_rule(dt):
    g = torch.Generator().manual_seed(6)
    N, K, M = 77, 352, 130
    q, s = rand_mx(N, K, g)
    gy = torch.randn((M, N), generator=g).to(dt).to(DEV)
    clean = G.grad_input(gy, q.to(DEV), s.to(DEV))
    assert torch.isfinite(clean).all()
    s2, q2 = s.clone(), q.clone()
    s2[40, 5] = 255
    q2[70, 131] = 0x7F
    for got, lo, hi in ((G.grad_input(gy, q.to(DEV), s2.to(DEV)), 160, 192), (G.grad_input(gy, q2.to(DEV), s.to(DEV)), 131, 132)):
        keep = torch.ones(K, dtype=torch.bool, device=DEV)
        keep[lo:hi] = False
        assert torch.isnan(got[:, lo:hi]).all() and torch.equal(got[:, keep], clean[:, keep])


def routing(T, S, E, seed):  # experts 0 .. E - 2 (the last one stays empty), some slots skipped by -1 and by E
    idx = torch.randint(0, E - 1, (T * S,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    idx[::7], idx[3::11] = -1, E
    return idx.reshape(T, S)


@pytest.mark.parametrize("dt", DTS)
def test_grouped_rows_are_the_dense_rows_of_their_expert(dt):
    for T, S in ((127, 1), (100, 3)):
        grouped_case(T, S, dt)


def grouped_case(T, S, dt):
    E, K, N, P = 4, 96, 33, T * S
    g = torch.Generator().manual_seed(T + S)
    q, s = rand_mx(E * N, K, g)
    qd, sd = q.reshape(E, N, K).to(DEV), s.reshape(E, N, K // 32).to(DEV)
    idx = routing(T, S, E, T)
    flat = idx.reshape(-1).to(DEV)
    live = (flat >= 0) & (flat < E)
    gy = torch.randn((P, N), generator=g).to(dt).to(DEV)
    gx = G.experts_grad_input(gy, idx.to(DEV), qd, sd)
    g32 = G.experts_grad_input(gy, idx.to(DEV), qd, sd, G.experts_blk_exp(sd), out_dtype=torch.float32)
    assert gx.shape == (P, K) and gx.dtype == dt and g32.dtype == torch.float32
    assert (gx[~live].view(torch.int16) == 0).all() and (g32[~live].view(torch.int32) == 0).all()  # +0, not -0
    W = dequant(q, s).reshape(E, N, K).to(DEV)
    for e in range(E - 1):
        rows = (flat == e).nonzero().reshape(-1)
        assert torch.equal(gx[rows], G.grad_input(gy[rows], qd[e], sd[e]))
        check(g32[rows], gy[rows].double() @ W[e], gy[rows].double().abs() @ W[e].abs(), N, torch.float32)
    assert torch.equal(g32.to(dt), gx)


def packed_layers(name, dims, dt, q, s):  # an eval layer on a loaded weight per grad_input mode
    from bitorch_engine.layers.qlinear.nbit import cuda
    layers = {mode: getattr(cuda, name)(*dims, dtype=dt).to(DEV).eval() for mode in ("kernel", "torch")}
    for mode, layer in layers.items():
        layer.set_mx_weight(q, s)
        layer.grad_input = mode
    return layers


@pytest.mark.parametrize("dt", DTS)
def test_layers_with_the_kernel_backward(dt):
    g = torch.Generator().manual_seed(21)
    M, K, N, T, S, E = 130, 160, 72, 40, 2, 4
    q, s = rand_mx(N, K, g, 125, 129, exact=True)
    xi = torch.randn((2, M // 2, K), generator=g).to(dt).to(DEV).requires_grad_(True)
    gi = torch.randint(-2, 3, (2, M // 2, N), generator=g).to(dt).to(DEV)
    got = {mode: torch.autograd.grad(layer(xi), xi, gi)[0] for mode, layer in packed_layers("MXFP8LinearCuda", (K, N), dt, q, s).items()}
    assert torch.equal(got["kernel"], got["torch"]) and got["kernel"].abs().sum() > 0
    qe, se = rand_mx(E * N, K, g, 125, 129, exact=True)
    idx = routing(T, S, E, 32).to(DEV)
    layers = packed_layers("MXFP8ExpertsLinearCuda", (E, K, N), dt, qe.reshape(E, N, K), se.reshape(E, N, K // 32))
    ge = torch.randint(-2, 3, (T, S, N), generator=g).to(dt).to(DEV)
    for shape in ((T, K), (T, S, K)):
        xs = torch.randn(shape, generator=g).to(dt).to(DEV).requires_grad_(True)
        eager = torch.autograd.grad(layers["kernel"](xs, idx), xs, ge)[0]
        assert torch.equal(eager, torch.autograd.grad(layers["torch"](xs, idx), xs, ge)[0]) and eager.abs().sum() > 0
        gs = ge.clone()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):  # a host synchronisation in the backward would fail the capture
            out = torch.autograd.grad(layers["kernel"](xs, idx), xs, gs)[0]
        for _ in range(3):
            gs.copy_(-ge)
            gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, -eager)
    # a condition, not a measurement: the "kernel" backward allocates less than the fp32 image of W alone, the "torch" backward does not
    N = K = 2048
    q, s = rand_mx(N, K, g)
    x, gy = torch.randn((128, K), generator=g).to(dt).to(DEV), torch.randn((128, N), generator=g).to(dt).to(DEV)
    peak = {}
    for mode, layer in packed_layers("MXFP8LinearCuda", (K, N), dt, q, s).items():
        y = layer(x.clone().requires_grad_(True))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y.backward(gy)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
    print(f"dense backward peak bytes: {peak}")
    assert peak["kernel"] < N * K * 4 and peak["torch"] >= N * K * 4
