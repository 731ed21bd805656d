"""MXFP8 weight-only expert layers (W8A16, csrc/mxfp8_moe.hip) on the MI355X, against float64 within the weight-only contract's tolerance
(fuzz_mxfp6.check: exact products, an fp32 sum of length K, one rounding) and against the dense layer's bits."""
import itertools
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
from bitorch_engine.extensions import mxfp8_experts_cuda as ext, mxfp8_linear_cuda as dense  # noqa: E402

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
SHAPES = [(32, 1, 1), (96, 7, 3), (1056, 33, 3), (2880, 33, 2), (4096, 129, 2)]  # (K, N, E): G = 32 (2, 6, 66 units), 64, 128
PAIRS = [(1, 1), (3, 2), (5, 4), (40, 4)]  # (T, S)
_WEIGHTS = {}


def weights(K, N, E):
    if (K, N, E) not in _WEIGHTS:  # one random stacked weight per shape with its float64 restatement: shared, never written
        g = torch.Generator().manual_seed(K * 3 + N + E)
        q, s = ref.rand_w(E * N, K, g, 118, 130)
        W, bias = ref.dequant(q, s).reshape(E, N, K), torch.randn((E, N), generator=g)
        _WEIGHTS[(K, N, E)] = (q.reshape(E, N, K).to(DEV), s.reshape(E, N, K // 32).to(DEV), W.to(DEV), bias.to(DEV))
    return _WEIGHTS[(K, N, E)]


def make_idx(T, S, E, seed):
    # random experts, expert E - 1 left without pairs (E >= 2), every fifth slot skipped
    idx = torch.randint(0, max(E - 1, 1), (T * S,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    idx[1::5] = -1
    return idx.reshape(T, S).to(DEV)


def make_x(T, S, K, dt, seed):
    return (torch.randn((T, S, K), generator=torch.Generator().manual_seed(seed)) * 0.25).to(dt).to(DEV)


@pytest.mark.parametrize("K,N,E,pairs", [s + (PAIRS,) for s in SHAPES] + [(96, 7, 1, [(70, 2)])])  # the last: 140 pairs on one expert
def test_both_forms_against_float64(K, N, E, pairs):
    q, s, W, bias = weights(K, N, E)
    for (T, S), dt in itertools.product(pairs, DTS):
        idx = torch.zeros((T, S), dtype=torch.int32, device=DEV) if T == 70 else make_idx(T, S, E, T * 7 + S)
        x3, e_col, flat = make_x(T, S, K, dt, K + T), ext.col_exp(s), idx.reshape(-1)
        for x in (x3[:, 0].contiguous(), x3):
            xr = (x if x.dim() == 3 else x[:, None, :].expand(T, S, K)).reshape(T * S, K)
            for b in (None, bias.to(dt)):
                yref = torch.zeros((T * S, N), dtype=torch.float64, device=DEV)  # a skipped row: 0, with the tolerance `tiny`
                a = torch.zeros_like(yref)
                for e in range(E):
                    rows = (flat == e).nonzero().reshape(-1)
                    yref[rows], a[rows] = F.ref_y(xr[rows], W[e], None if b is None else b[e])
                for form in (0, 1, -1):
                    y = ext.forward(x, idx, q, s, b, e_col if form else None, form=form)
                    assert y.dtype == dt and y.shape == (T, S, N)
                    F.check(y.reshape(T * S, N), yref, a, K, dt, f"T {T} S {S} form {form} x {x.dim()}d bias {b is not None}")


@pytest.mark.parametrize("dt", DTS)
def test_a_pairs_row_has_the_dense_forms_bits(dt):
    for K, N, E in SHAPES:
        q, s, _, bias = weights(K, N, E)
        bias, idx, x = bias.to(dt), make_idx(5, 4, E, 93), make_x(5, 4, K, dt, 17)
        idx[0, 0] = E - 1  # the last expert too: a non-zero offset at every G and in the partial column tile
        for form in (0, 1):
            y = ext.forward(x, idx, q, s, bias, form=form)
            for t, sl in (idx >= 0).nonzero().tolist():
                e = idx[t, sl]
                assert torch.equal(y[t, sl][None], dense.forward(x[t, sl][None], q[e], s[e], bias[e], form=form)), (K, form, t, sl)


@pytest.mark.parametrize("dt", DTS)
def test_skipped_slots_are_plus_zero_and_rows_are_independent(dt):
    for K, N, E in ((96, 7, 3), (2880, 33, 2)):
        q, s, _, bias = weights(K, N, E)
        idx, x = make_idx(40, 4, E, 5), make_x(40, 4, K, dt, 3)
        idx[2, 1], idx[7, 3] = E, E + 5  # beyond the range as well as -1
        skipped = (idx < 0) | (idx >= E)
        for form in (0, 1):  # ym: the skipped slots on a live expert
            y, ym = (ext.forward(x, i, q, s, bias.to(dt), form=form) for i in (idx, torch.where(skipped, torch.zeros_like(idx), idx)))
            assert (y[skipped].view(torch.int16) == 0).all(), (K, form)  # +0: the sign bit too
            assert torch.equal(y[~skipped], ym[~skipped]) and (ym[skipped] != 0).any(), (K, form)


@pytest.mark.parametrize("dt", DTS)
def test_a_nan_block_stays_in_its_expert_and_column(dt):
    K, N, E = 96, 7, 3
    q, s, _, bias = weights(K, N, E)
    idx, x, bad = make_idx(40, 4, E, 9), make_x(40, 4, K, dt, 4), s.clone()
    bad[1, 4, 2] = 255
    hit = (idx == 1)[..., None] & (torch.arange(N, device=DEV) == 4)
    for form in (0, 1):
        y, yc = (ext.forward(x, idx, q, sc, bias.to(dt), form=form) for sc in (bad, s))
        assert hit.any() and torch.isnan(y[hit]).all() and torch.equal(y[~hit], yc[~hit]), form


def layer_with(E, K, N, dt, seed=0):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP8ExpertsLinearCuda
    torch.manual_seed(seed)
    return MXFP8ExpertsLinearCuda(E, K, N, bias=True, dtype=dt).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_layer_forward_checkpoint_and_set_mx_weight(dt):
    K, N, E = 96, 7, 3
    q, s, _, _ = weights(K, N, E)
    idx, x = make_idx(5, 4, E, 1), make_x(5, 4, K, dt, 2)
    layer = layer_with(E, K, N, dt, seed=1).eval()
    assert torch.equal(layer(x, idx), ext.forward(x, idx, layer.qweight, layer.scales, layer.bias.detach()))
    layer.generate_quantized_weight(qweight_only=True)
    back = layer_with(E, K, N, dt, seed=2).eval()
    back.load_state_dict(layer.state_dict())
    assert back.weight is None and torch.equal(back.qweight, layer.qweight) and torch.equal(back(x, idx.long()), layer(x, idx))
    for blocks in (q.reshape(E, N, K // 32, 32), q):
        back.set_mx_weight(blocks, s)
        assert back.weight is None and torch.equal(back.qweight, q) and torch.equal(back.e_col, ext.col_exp(s))
        assert torch.equal(back(x[:, 0].contiguous(), idx), ext.forward(x[:, 0].contiguous(), idx, q, s, back.bias.detach()))


@pytest.mark.parametrize("dt", DTS)
def test_layer_training_backward_against_float64_autograd(dt):
    K, N, E, T, S = 96, 7, 3, 5, 4
    layer, idx = layer_with(E, K, N, dt).train(), make_idx(T, S, E, 6)
    x = make_x(T, S, K, dt, 8).requires_grad_(True)
    y = layer(x, idx)
    qw, sc = ext.quantize(layer.weight.detach())
    assert torch.equal(y.detach(), ext.forward(x.detach(), idx, qw, sc, layer.bias.detach()))
    y.backward(gy := torch.randn(y.shape, device=DEV).to(dt))
    live, e = (idx >= 0)[..., None].double(), idx.clamp(min=0).long()

    def grads(xd, Wd, bd, g):  # d sum(g * y) / d (x, W, bias) of the layer's definition in float64
        xd, Wd, bd = (v.clone().requires_grad_(True) for v in (xd, Wd, bd))
        yd = (torch.einsum("tsk,tsnk->tsn", xd, Wd[e]) + bd[e]) * live
        return torch.autograd.grad((yd * g).sum(), (xd, Wd, bd))

    args = (x.detach().double(), ext.dequant(qw, sc, torch.float32).double(), layer.bias.detach().double(), gy.double())
    want, absp = grads(*args), grads(*(v.abs() for v in args))  # the sums have N, P and P terms
    for got, w, a, n, what in zip((x.grad, layer.weight.grad, layer.bias.grad), want, absp, (N, T * S, T * S), ("grad_x", "grad_weight", "grad_bias")):
        F.check(got, w, a, n, dt, what)


@pytest.mark.parametrize("dt", DTS)
def test_moe_block_is_the_composition_of_its_public_pieces(dt):
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP8A16MoECuda
    from bitorch_engine.layers.qlinear.nbit.cuda.mxfp8_moe_layer import combine, swiglu
    torch.manual_seed(0)
    moe = MXFP8A16MoECuda(64, 32, 4, 2, dtype=dt).to(DEV).eval()
    x = torch.randn((9, 64), device=DEV).to(dt)
    with torch.no_grad():
        y = moe(x)
        w, idx = moe.route(x)
        h = ext.forward(x, idx, moe.gate_up.qweight, moe.gate_up.scales, moe.gate_up.bias)
        o = ext.forward(swiglu(h, moe.swiglu_limit, moe.swiglu_alpha), idx, moe.down.qweight, moe.down.scales, moe.down.bias)
    assert torch.isfinite(y).all() and torch.equal(y, combine(w, o))


@pytest.mark.parametrize("form", [0, 1])
def test_graph_replay_equals_eager(form):
    dt, (K, N, E), (T, S) = torch.float16, (2880, 33, 2), (40, 4)
    q, s, _, bias = weights(K, N, E)
    idx, x, b, e_col = make_idx(T, S, E, 2), make_x(T, S, K, dt, 5), bias.to(dt), ext.col_exp(s)
    eager = ext.forward(x, idx, q, s, b, e_col, form=form)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = ext.forward(x, idx, q, s, b, e_col, form=form)
    for i in range(3):  # several replays, each against the eager result on new data
        x.copy_(make_x(T, S, K, dt, 10 + i))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ext.forward(x, idx, q, s, b, e_col, form=form)) and not torch.equal(out, eager)
