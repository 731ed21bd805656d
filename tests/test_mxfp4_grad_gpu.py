"""MXFP4 input gradient on the MI355X (csrc/mxfp4_grad.hip): the dense and the grouped gx = gy . W on the packed weights against a float64
product within the forward's contract with N as the length, bit-identical on exact data (to the rounded float64 product and to the
torch composition), blk_exp and the NaN rule, the range of the block-column rebias, the layers with grad_input="kernel" against the
float64 restatement and bit for bit against the "torch" layers' weight and bias gradients, row independence of the grouped form, the
backward's peak memory with and without an image of W, and graph replay."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
_spec = importlib.util.spec_from_file_location("mxfp4_moe_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_moe_ref.py"))
mref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mref)
ref = mref.ref


def lin():
    from bitorch_engine.extensions import mxfp4_linear_cuda
    return mxfp4_linear_cuda


def ext():
    from bitorch_engine.extensions import mxfp4_experts_cuda
    return mxfp4_experts_cuda


def rand_mx(N, K, g, lo=118, hi=130):
    """tests/test_mxfp4_gpu.py's draw: every code byte, scale codes lo .. hi (118 .. 130: every fp16 fragment is exact)."""
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


def check(y, yref, absprod, n, dt):
    """The forward's contract (tests/test_mxfp4_gpu.py check) with the contraction length n: exact products, an fp32 sum, one rounding."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    tol = eps * yref.abs() + (n + 2) * 2.0 ** -23 * absprod + tiny
    err = (y.double() - yref).abs()
    assert torch.isfinite(y).all()
    print(f"max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), f"max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


_DENSE = {}


def dense_weights(K, N):
    """Codes, scale codes and the float64 W of a dense shape on the GPU: computed once, shared by the cases, never written."""
    if (K, N) not in _DENSE:
        g = torch.Generator().manual_seed(K * 3 + N)
        q, s = rand_mx(N, K, g)
        _DENSE[(K, N)] = (q.to(DEV), s.to(DEV), ref.dequant(q, s).to(DEV))
    return _DENSE[(K, N)]


MS = (1, 127, 128, 129, 300)
KN = [(32, 1), (96, 7), (160, 33), (256, 63), (256, 64), (256, 65), (4096, 200), (128, 1000)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N", KN)
def test_dense_against_float64(K, N, dt):
    """Odd N: gy rows that are no 16-byte multiples; N = 63 / 64 / 65: the edge of a contraction stage; K = 32 / 96 / 160: partial column
    tiles; M around 128: the edge of a row tile."""
    q, s, W = dense_weights(K, N)
    g = torch.Generator().manual_seed(K + N)
    for M in MS:
        gy = (torch.randn((M, N), generator=g) * 0.5).to(dt).to(DEV)
        gx = lin().grad_input(gy, q, s)
        assert gx.dtype == dt and gx.shape == (M, K)
        check(gx, gy.double() @ W, gy.double().abs() @ W.abs(), N, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", [(1, 32, 1), (129, 160, 33), (64, 4096, 72), (300, 256, 4096)])
def test_exact_data_is_bit_identical(M, K, N, dt):
    """Scales 2^-2 .. 2^2 and integer gy in [-2, 2]: every partial sum is a multiple of 2^-3 below 2^21, exact in fp32."""
    g = torch.Generator().manual_seed(M + K + N)
    q, s = rand_mx(N, K, g, 125, 129)
    gy = torch.randint(-2, 3, (M, N), generator=g).to(dt).to(DEV)
    qd, sd = q.to(DEV), s.to(DEV)
    gx = lin().grad_input(gy, qd, sd)
    want = (gy.double() @ ref.dequant(q, s).to(DEV)).to(dt)
    assert torch.equal(gx, want), (gx.double() - want.double()).abs().max().item()
    assert torch.equal(gx, gy.float().mm(lin().dequant(qd, sd, torch.float32)).to(dt))  # the torch path of the layer
    assert torch.equal(gx, lin().grad_input(gy, qd, sd, lin().blk_exp(sd)))
    base = torch.randint(-2, 3, (N, M), generator=g).to(dt).to(DEV)  # a non-contiguous gy is made contiguous
    assert torch.equal(lin().grad_input(base.t(), qd, sd), lin().grad_input(base.t().contiguous(), qd, sd))


@pytest.mark.parametrize("dt", DTS)
def test_blk_exp_and_the_nan_rule(dt):
    g = torch.Generator().manual_seed(6)
    N, K, M = 77, 352, 130  # 11 block-columns: three workgroups of four, the last one partial
    q, s = rand_mx(N, K, g, 100, 140)
    e = lin().blk_exp(s.to(DEV))
    assert e.dtype == torch.uint8 and e.shape == (K // 32,) and torch.equal(e.cpu(), s.amax(0))
    s3 = torch.randint(0, 255, (5, 300, 9), generator=g, dtype=torch.int32).to(torch.uint8)
    assert torch.equal(ext().blk_exp(s3.to(DEV)).cpu(), s3.amax(1))
    q, s = rand_mx(N, K, g)
    gy = torch.randn((M, N), generator=g).to(dt).to(DEV)
    clean = lin().grad_input(gy, q.to(DEV), s.to(DEV))
    s2 = s.clone()
    s2[40, 5] = 255
    e2 = lin().blk_exp(s2.to(DEV)).cpu()
    assert e2[5] == 255 and torch.equal(e2, s2.amax(0))
    nan = lin().grad_input(gy, q.to(DEV), s2.to(DEV))
    assert torch.isnan(nan[:, 160:192]).all()
    keep = torch.ones(K, dtype=torch.bool, device=DEV)
    keep[160:192] = False
    assert torch.equal(nan[:, keep], clean[:, keep]) and torch.isfinite(clean).all()
    assert lin().grad_input(gy[:0], q.to(DEV), s.to(DEV)).shape == (0, K)


def test_range_bf16_stays_within_the_bound():
    """One block-column rebiased by e_blk = 254, one by e_blk = 3: the fragments stay below 6 and the fp32 epilogue carries the scale."""
    g = torch.Generator().manual_seed(12)
    N, K, M = 8, 96, 130
    q, s = rand_mx(N, K, g)
    s[:, 0] = torch.randint(250, 255, (N,), generator=g).to(torch.uint8)
    s[:, 1] = torch.randint(0, 4, (N,), generator=g).to(torch.uint8)
    s[3, 0], s[5, 1] = 254, 3
    assert lin().blk_exp(s.to(DEV)).cpu().tolist() == [254, 3, int(s[:, 2].max())]
    W = ref.dequant(q, s).to(DEV)
    gy = (torch.randn((M, N), generator=g).clamp(-4, 4) * 2.0 ** -8).to(torch.bfloat16).to(DEV)  # |gx| <= 8 * 2^-6 * 6 * 2^127 < 2^127
    gx = lin().grad_input(gy, q.to(DEV), s.to(DEV))
    assert gx[:, :32].abs().max() > 2.0 ** 110 and gx[:, 32:64].abs().max() < 2.0 ** -110
    check(gx, gy.double() @ W, gy.double().abs() @ W.abs(), N, torch.bfloat16)


def test_range_fp16_saturates_and_underflows_as_one_rounding_of_the_fp32_value():
    g = torch.Generator().manual_seed(13)
    N, K, M = 40, 96, 130
    q, s = rand_mx(N, K, g, 125, 129)
    s[:, 0] = torch.randint(252, 255, (N,), generator=g).to(torch.uint8)
    s[:, 1] = torch.randint(1, 4, (N,), generator=g).to(torch.uint8)
    s[3, 0], s[5, 1] = 254, 3
    gy = torch.randint(-2, 3, (M, N), generator=g).half().to(DEV)
    gx = lin().grad_input(gy, q.to(DEV), s.to(DEV))
    f32 = (gy.double() @ ref.dequant(q, s).to(DEV)).float()  # exact sums; beyond the fp32 range they are inf, as the kernel's product is
    want = f32.half()
    assert torch.isinf(want[:, :32]).any() and (want[:, 32:64] == 0).all() and torch.isfinite(want[:, 64:]).all()
    assert torch.equal(gx, want)


# ---- layers --------------------------------------------------------------------------------------------------------------------------------
def dense_layer(N, K, dt, mode, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda
    torch.manual_seed(seed)
    return MXFP4LinearCuda(K, N, bias=True, dtype=dt, grad_input=mode).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_dense_layer_train_and_eval(dt):
    N, K, M = 72, 160, 130
    g = torch.Generator().manual_seed(21)
    x = torch.randn((M, K), generator=g).to(dt).to(DEV)
    gy = torch.randn((M, N), generator=g).to(dt).to(DEV)
    grads = {}
    for mode in ("kernel", "torch"):
        layer = dense_layer(N, K, dt, mode).train()
        xi = x.clone().requires_grad_(True)
        layer(xi).backward(gy)
        grads[mode] = (xi.grad, layer.weight.grad, layer.bias.grad)
        q, s = lin().quantize(layer.weight.detach())
    W = ref.dequant(q.cpu(), s.cpu()).to(DEV)
    check(grads["kernel"][0], gy.double() @ W, gy.double().abs() @ W.abs(), N, dt)
    assert torch.equal(grads["kernel"][1], grads["torch"][1]) and torch.equal(grads["kernel"][2], grads["torch"][2])
    # eval on a loaded MXFP4 weight: only the packed pair exists
    q, s = rand_mx(N, K, g)
    layer = dense_layer(N, K, dt, "kernel").eval()
    layer.set_mx_weight(q, s)
    assert set(layer.state_dict()) == {"qweight", "scales", "bias"}
    xi = x.reshape(2, M // 2, K).clone().requires_grad_(True)  # a 3-d input
    layer(xi).backward(gy.reshape(2, M // 2, N))
    W = ref.dequant(q, s).to(DEV)
    check(xi.grad.reshape(M, K), gy.double() @ W, gy.double().abs() @ W.abs(), N, dt)
    assert torch.equal(layer.bias.grad, gy.float().sum(0).to(dt))


def experts_layer(E, N, K, dt, mode, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4ExpertsLinearCuda
    torch.manual_seed(seed)
    return MXFP4ExpertsLinearCuda(E, K, N, bias=True, dtype=dt, grad_input=mode).to(DEV)


def routing(T, S, E, seed):
    """Indices over experts 0 .. E - 2 (the last expert stays empty), with some slots skipped by -1 and by E."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, max(E - 1, 1), (T, S), generator=g, dtype=torch.int32)
    r = torch.rand((T, S), generator=g)
    idx[r < 0.1] = -1
    idx[r > 0.9] = E
    assert (idx == -1).any() and (idx == E).any() and not (idx == E - 1).any()
    return idx


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_experts_layer_against_float64_autograd_of_the_restatement(xpp, dt):
    """Bound: that of tests/test_mxfp4_moe_gpu.py's backward test: the contract over N terms per pair, S pairs per token for x [T, K]."""
    E, N, K, T, S = 5, 72, 160, 40, 3
    g = torch.Generator().manual_seed(31)
    x = torch.randn((T, S, K) if xpp else (T, K), generator=g).to(dt).to(DEV)
    idx = routing(T, S, E, 32)
    gy = torch.randn((T, S, N), generator=g).to(dt).to(DEV)
    grads = {}
    for mode in ("kernel", "torch"):
        layer = experts_layer(E, N, K, dt, mode).train()
        xi = x.clone().requires_grad_(True)
        layer(xi, idx.to(DEV)).backward(gy)
        grads[mode] = (xi.grad, layer.weight.grad, layer.bias.grad)
        q, s = ext().quantize(layer.weight.detach())

    def grad_x(absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        x64 = f(x.double()).requires_grad_(True)
        mref.experts(x64, idx, f(mref.dequant(q, s)))[0].backward(f(gy.double()))
        return x64.grad

    gk = grads["kernel"][0]
    check(gk, grad_x(False), grad_x(True), N * (1 if xpp else S), dt)
    assert torch.equal(grads["kernel"][1], grads["torch"][1]) and torch.equal(grads["kernel"][2], grads["torch"][2])
    assert (grads["kernel"][1][E - 1] == 0).all()
    if xpp:  # skipped pairs give zero rows
        dead = ((idx < 0) | (idx >= E)).to(DEV)
        assert dead.any() and (gk[dead] == 0).all() and (gk[~dead] != 0).any()
    # frozen packed weights and no bias gradient: the backward is the grouped call alone
    layer = experts_layer(E, N, K, dt, "kernel").eval()
    layer.set_mx_weight(q, s)
    layer.bias.requires_grad_(False)
    xi = x.clone().requires_grad_(True)
    layer(xi, idx.to(DEV)).backward(gy)
    assert torch.equal(xi.grad, gk)


@pytest.mark.parametrize("dt", DTS)
def test_a_pairs_row_is_its_own(dt):
    E, N, K, T, S = 4, 70, 160, 50, 3
    g = torch.Generator().manual_seed(41)
    q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    s = torch.randint(118, 131, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    idx = routing(T, S, E, 42)
    idx[:44] = 0  # 132 pairs of expert 0: more than one row tile, the second one partial
    idx[45, 0], idx[46, 1] = -1, E
    gy = torch.randn((T * S, N), generator=g).to(dt).to(DEV)
    e_blk = ext().blk_exp(s)
    for out_dtype in (None, torch.float32):
        gx = ext().grad_input(gy, idx.to(DEV), q, s, e_blk, out_dtype=out_dtype)
        assert gx.shape == (T * S, K) and gx.dtype == (out_dtype or dt)
        flat = idx.reshape(-1)
        for p in range(T * S):
            e = int(flat[p])
            if 0 <= e < E:
                if out_dtype is None:
                    assert torch.equal(gx[p:p + 1], lin().grad_input(gy[p:p + 1], q[e], s[e], e_blk[e])), p
            else:
                assert (gx[p] == 0).all(), p
        perm = torch.randperm(T * S, generator=g)
        gxp = ext().grad_input(gy[perm.to(DEV)].reshape(T, S, N), flat[perm].reshape(T, S).to(DEV), q, s, out_dtype=out_dtype)
        assert torch.equal(gxp, gx[perm.to(DEV)])
    assert torch.equal(gx.to(dt), ext().grad_input(gy, idx.to(DEV), q, s))  # the fp32 rows round to the dtype rows
    assert ext().grad_input(gy[:0], idx[:0].to(DEV), q, s).shape == (0, K)


def backward_peak(layer, args, gy):
    y = layer(*args)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y.backward(gy)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_no_weight_image_in_the_backward():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4ExpertsLinearCuda, MXFP4LinearCuda
    dt = torch.float16
    g = torch.Generator().manual_seed(51)
    N = K = 2048
    M = 64
    q, s = rand_mx(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt).to(DEV)
    gy = torch.randn((M, N), generator=g).to(dt).to(DEV)
    peak = {}
    for mode in ("kernel", "torch"):
        layer = MXFP4LinearCuda(K, N, dtype=dt, grad_input=mode).to(DEV).eval()
        layer.set_mx_weight(q, s)
        peak[mode] = backward_peak(layer, (x.clone().requires_grad_(True),), gy)
    print(f"dense backward peak bytes: {peak}")
    assert peak["kernel"] < N * K * 2 and peak["torch"] >= N * K * 4
    E, N, K, T, S = 8, 512, 512, 16, 2
    q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(118, 131, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    idx = torch.randint(0, E, (T, S), generator=g, dtype=torch.int32).to(DEV)
    x = torch.randn((T, K), generator=g).to(dt).to(DEV)
    gy = torch.randn((T, S, N), generator=g).to(dt).to(DEV)
    for mode in ("kernel", "torch"):
        layer = MXFP4ExpertsLinearCuda(E, K, N, dtype=dt, grad_input=mode).to(DEV).eval()
        layer.set_mx_weight(q, s)
        peak[mode] = backward_peak(layer, (x.clone().requires_grad_(True), idx), gy)
    print(f"experts backward peak bytes: {peak}")
    assert peak["kernel"] < N * K * 2 and peak["torch"] >= N * K * 4


@pytest.mark.parametrize("dt", DTS)
def test_graph_replay_equals_eager(dt):
    E, N, K, T, S = 4, 70, 160, 50, 3
    g = torch.Generator().manual_seed(61)
    q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    s = torch.randint(118, 131, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    idx = routing(T, S, E, 62).to(DEV)
    gy = torch.randn((T, S, N), generator=g).to(dt).to(DEV)
    eager = ext().grad_input(gy, idx, q, s)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ext().grad_input(gy, idx, q, s)
    torch.cuda.current_stream().wait_stream(st)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = ext().grad_input(gy, idx, q, s)
    gy.copy_(torch.randn((T, S, N), generator=g).to(dt))
    idx.copy_(routing(T, S, E, 63))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ext().grad_input(gy, idx, q, s))
    assert not torch.equal(out, eager)
