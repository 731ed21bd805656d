"""MXFP6 input gradient on the MI355X (csrc/mxfp6_grad.hip): the dense and the grouped gx = gy . W on the packed MXFP6 weights against a
float64 product within the contract with N as the length, the element map of the convert and the transposed read on one-hot rows,
bit-identical on exact data (to the rounded float64 product and to the torch composition), blk_exp and the NaN rule, row independence
of the grouped form, the layers with grad_input="kernel" against the float64 restatement and bit for bit against the "torch" layers'
weight and bias gradients, graph replay of a frozen expert layer's backward, and the backward's peak memory with and without an image
of W.  Scale codes are drawn from 119 .. 130, so e_blk - s <= 11 and every fp16 fragment is a normal number."""
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
ref = gref.ref
rand_mx = gref.rand_mx


def lin():
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda
    return mxfp6_a8_linear_cuda


def ext():
    from bitorch_engine.extensions import mxfp6_experts_a8_cuda
    return mxfp6_experts_a8_cuda


def check(y, yref, absprod, n, dt):
    """The contract with the contraction length n: exact products, an fp32 sum, one rounding."""
    tol = gref.tolerance(yref, absprod, n, dt)
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
KN = [(32, 1), (96, 7), (160, 33), (256, 31), (256, 32), (256, 33), (256, 63), (256, 64), (256, 65), (4096, 200), (128, 1000)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N", KN)
def test_dense_against_float64(K, N, dt):
    """Odd N: gy rows that are no 16-byte multiples; N = 31 / 32 / 33 and 63 / 64 / 65: the edge of a contraction stage (32 n) and of two;
    K = 32 / 96 / 160: partial column tiles; M around 128: the edge of a row tile."""
    q, s, W = dense_weights(K, N)
    g = torch.Generator().manual_seed(K + N)
    for M in MS:
        gy = (torch.randn((M, N), generator=g) * 0.5).to(dt).to(DEV)
        gx = lin().grad_input(gy, q, s)
        assert gx.dtype == dt and gx.shape == (M, K)
        check(gx, gy.double() @ W, gy.double().abs() @ W.abs(), N, dt)


@pytest.mark.parametrize("dt", DTS)
def test_element_map_on_one_hot_rows(dt):
    """gy = the identity: gx[m, :] must be W[m, :] exactly.  Row n holds code (n + 3 k) mod 64 at column k, so over the 70 rows every one
    of the 64 codes stands at every position j of a block, in rows on both sides of the stage edges at n = 32 and 64; K = 160 is five
    block-columns, the fifth in a partial column tile.  This pins the convert's output order and the transposed read."""
    g = torch.Generator().manual_seed(5)
    N, K = 70, 160
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = ((n + 3 * k) % 64).to(torch.uint8)
    for j in range(32):
        assert set(codes[:, j::32].flatten().tolist()) == set(range(64))
        assert set(codes[:32, j].tolist()) | set(codes[32:64, j].tolist()) == set(range(64))
    q = ref.pack(codes)
    s = torch.randint(119, 131, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    W = ref.dequant(q, s).to(DEV)
    gx = lin().grad_input(torch.eye(N).to(dt).to(DEV), q.to(DEV), s.to(DEV))
    bad = (gx.double() != W).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, the first at (n, k) = {bad[0].tolist()}"
    # a single one-hot row anywhere in a row tile: M = 130, row m reads weight row (7 m) mod N
    M = 130
    pick = (7 * torch.arange(M)) % N
    gy = torch.zeros((M, N))
    gy[torch.arange(M), pick] = 1.0
    gx = lin().grad_input(gy.to(dt).to(DEV), q.to(DEV), s.to(DEV))
    assert torch.equal(gx.double(), W[pick.to(DEV)])


EXACT = [(1, 32, 1), (129, 160, 33), (64, 4096, 72), (300, 256, 4096)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N", EXACT)
def test_exact_data_is_bit_identical(M, K, N, dt):
    """Scales 2^-2 .. 2^2 and integer gy in [-2, 2]: every partial sum is a multiple of 2^-5 below 2^21, exact in fp32."""
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
    N, K, M = 77, 352, 130  # 11 block-columns: three column tiles, the last one partial
    _, s = rand_mx(N, K, g, 100, 140)
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


# ---- grouped form -------------------------------------------------------------------------------------------------------------------------
def routing(T, S, E, seed):
    """Indices over experts 0 .. E - 2 (the last expert stays empty), with some slots skipped by -1 and by E."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, max(E - 1, 1), (T, S), generator=g, dtype=torch.int32)
    r = torch.rand((T, S), generator=g)
    idx[r < 0.1] = -1
    idx[r > 0.9] = E
    assert (idx == -1).any() and (idx == E).any() and not (idx == E - 1).any()
    return idx


def rand_experts(E, N, K, g, lo=119, hi=130):
    q, s = rand_mx(E * N, K, g, lo, hi)
    return q.reshape(E, N, -1), s.reshape(E, N, -1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,N", [(96, 33), (256, 200)])
@pytest.mark.parametrize("T,S", [(127, 1), (43, 3), (100, 3)])
def test_grouped_rows_are_the_dense_rows_of_their_expert(T, S, K, N, dt):
    """P = 127, 129, 300 around a row tile; E = 4 with the last expert empty, indices out of range on both sides.  Every live row equals
    the dense call of its expert on its own gy row bit for bit, skipped rows are +0, the fp32 rows meet the contract against float64,
    and a permutation of the pairs permutes the rows."""
    E, P = 4, T * S
    g = torch.Generator().manual_seed(T + K + N)
    q, s = rand_experts(E, N, K, g)
    qd, sd = q.to(DEV), s.to(DEV)
    idx = routing(T, S, E, T + S)
    if P >= 256:
        idx[:44] = 0  # 132 pairs of expert 0: more than one row tile, the second one partial
        idx[45, 0], idx[46, 1] = -1, E
    flat = idx.reshape(-1)
    live = (flat >= 0) & (flat < E)
    gy = torch.randn((P, N), generator=g).to(dt).to(DEV)
    e_blk = ext().blk_exp(sd)
    gx = ext().grad_input(gy, idx.to(DEV), qd, sd, e_blk)
    assert gx.shape == (P, K) and gx.dtype == dt
    for p in range(P):
        e = int(flat[p])
        if live[p]:
            assert torch.equal(gx[p:p + 1], lin().grad_input(gy[p:p + 1], qd[e], sd[e], e_blk[e])), p
        else:
            assert (gx[p].view(torch.int16) == 0).all(), p  # +0, not -0
    g32 = ext().grad_input(gy, idx.to(DEV), qd, sd, out_dtype=torch.float32)
    assert g32.dtype == torch.float32 and (g32[~live.to(DEV)].view(torch.int32) == 0).all()
    W = torch.stack([ref.dequant(q[e], s[e]) for e in range(E)]).to(DEV)
    rows = live.nonzero().reshape(-1).to(DEV)
    We = W[flat[live].long().to(DEV)]  # [live pairs, N, K]
    gl = gy[rows].double()
    check(g32[rows], torch.einsum("pn,pnk->pk", gl, We), torch.einsum("pn,pnk->pk", gl.abs(), We.abs()), N, torch.float32)
    assert torch.equal(g32.to(dt), gx)  # the fp32 rows round to the dtype rows
    perm = torch.randperm(P, generator=g)
    for out_dtype, base in ((None, gx), (torch.float32, g32)):
        gxp = ext().grad_input(gy[perm.to(DEV)].reshape(T, S, N), flat[perm].reshape(T, S).to(DEV), qd, sd, out_dtype=out_dtype)
        assert torch.equal(gxp, base[perm.to(DEV)])
    assert ext().grad_input(gy[:0], idx[:0].to(DEV), qd, sd).shape == (0, K)


# ---- layers --------------------------------------------------------------------------------------------------------------------------------
def dense_layer(N, K, dt, mode, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A8LinearCuda
    torch.manual_seed(seed)
    return MXFP6A8LinearCuda(K, N, bias=True, dtype=dt, grad_input=mode).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_dense_layer_train_and_eval(dt):
    M, K, N = 130, 160, 72
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
    assert int(s.max()) - int(s.min()) <= 11
    gxref, a = gref.grad_reference(gy, q, s, DEV)
    check(grads["kernel"][0], gxref, a, N, dt)
    assert torch.equal(grads["kernel"][1], grads["torch"][1]) and torch.equal(grads["kernel"][2], grads["torch"][2])
    # eval on a loaded MXFP6 weight, exact data, a 3-d input: bit-identical to the "torch" layer
    q, s = rand_mx(N, K, g, 125, 129)
    gi = torch.randint(-2, 3, (M, N), generator=g).to(dt).to(DEV)
    got = {}
    for mode in ("kernel", "torch"):
        layer = dense_layer(N, K, dt, mode).eval()
        layer.set_mx_weight(q, s)
        assert set(layer.state_dict()) == {"qweight", "scales", "bias"}
        xi = x.reshape(2, M // 2, K).clone().requires_grad_(True)
        layer(xi).backward(gi.reshape(2, M // 2, N))
        got[mode] = (xi.grad, layer.bias.grad)
    assert torch.equal(got["kernel"][0], got["torch"][0]) and torch.equal(got["kernel"][1], got["torch"][1])
    assert torch.equal(got["kernel"][0].reshape(M, K), (gi.double() @ ref.dequant(q, s).to(DEV)).to(dt))


def experts_layer(E, N, K, dt, mode, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A8ExpertsLinearCuda
    torch.manual_seed(seed)
    return MXFP6A8ExpertsLinearCuda(E, K, N, bias=True, dtype=dt, grad_input=mode).to(DEV)


def experts_grad_reference(gy, idx, q, s, per_pair):
    """float64 grad_x and its absolute-value product: gy[t, s] . W[idx[t, s]] per pair, summed over a token's slots for x [T, K]."""
    E = q.shape[0]
    T, S, N = gy.shape
    W = torch.stack([ref.dequant(q[e].cpu(), s[e].cpu()) for e in range(E)]).to(DEV)
    flat = idx.reshape(-1).long().to(DEV)
    live = ((flat >= 0) & (flat < E)).double()[:, None]
    We = W[flat.clamp(0, E - 1)]
    g = gy.reshape(T * S, N).double() * live
    gx, a = torch.einsum("pn,pnk->pk", g, We), torch.einsum("pn,pnk->pk", g.abs(), We.abs())
    if per_pair:
        return gx.reshape(T, S, -1), a.reshape(T, S, -1)
    return gx.reshape(T, S, -1).sum(1), a.reshape(T, S, -1).sum(1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("xpp", [0, 1])
def test_experts_layer_train_eval_and_graph(xpp, dt):
    T, S, E, K, N = 40, 2, 4, 96, 40
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
    assert int(s.max()) - int(s.min()) <= 11
    gk = grads["kernel"][0]
    gxref, a = experts_grad_reference(gy, idx, q, s, xpp)
    check(gk, gxref, a, N * (1 if xpp else S), dt)
    assert torch.equal(grads["kernel"][1], grads["torch"][1]) and torch.equal(grads["kernel"][2], grads["torch"][2])
    assert (grads["kernel"][1][E - 1] == 0).all()
    if xpp:  # skipped pairs give zero rows
        dead = ((idx < 0) | (idx >= E)).to(DEV)
        assert dead.any() and (gk[dead] == 0).all() and (gk[~dead] != 0).any()
    # frozen packed experts, exact data: bit-identical to the "torch" layer, and the "kernel" backward replays from a graph
    q, s = rand_experts(E, N, K, g, 125, 129)
    gi = torch.randint(-2, 3, (T, S, N), generator=g).to(dt).to(DEV)
    idxd = idx.to(DEV)
    layers = {}
    for mode in ("kernel", "torch"):
        layers[mode] = experts_layer(E, N, K, dt, mode).eval()
        layers[mode].set_mx_weight(q, s)
        layers[mode].bias.requires_grad_(False)

    def grad_x(mode, gout):
        xi = x.clone().requires_grad_(True)
        return torch.autograd.grad(layers[mode](xi, idxd), xi, gout)[0]

    eager = grad_x("kernel", gi)
    assert torch.equal(eager, grad_x("torch", gi))
    want, _ = experts_grad_reference(gi, idx, q, s, xpp)
    assert torch.equal(eager, want.to(dt))
    xs, gs = x.clone().requires_grad_(True), gi.clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        torch.autograd.grad(layers["kernel"](xs, idxd), xs, gs)
    torch.cuda.current_stream().wait_stream(st)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):  # a host synchronisation in the backward would fail the capture
        out = torch.autograd.grad(layers["kernel"](xs, idxd), xs, gs)[0]
    g2 = torch.randint(-2, 3, (T, S, N), generator=g).to(dt).to(DEV)
    gs.copy_(g2)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, grad_x("kernel", g2)) and not torch.equal(out, eager)


def backward_peak(layer, args, gy):
    y = layer(*args)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y.backward(gy)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_no_weight_image_in_the_backward():
    """A condition, not a measurement: the "kernel" backward allocates less than the fp32 image of W alone, the "torch" backward does not."""
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A8LinearCuda
    dt = torch.float16
    g = torch.Generator().manual_seed(51)
    N = K = 2048
    M = 128
    q, s = rand_mx(N, K, g)
    x = torch.randn((M, K), generator=g).to(dt).to(DEV)
    gy = torch.randn((M, N), generator=g).to(dt).to(DEV)
    peak = {}
    for mode in ("kernel", "torch"):
        layer = MXFP6A8LinearCuda(K, N, dtype=dt, grad_input=mode).to(DEV).eval()
        layer.set_mx_weight(q, s)
        peak[mode] = backward_peak(layer, (x.clone().requires_grad_(True),), gy)
    print(f"dense backward peak bytes: {peak}")
    assert peak["kernel"] < N * K * 4 and peak["torch"] >= N * K * 4
