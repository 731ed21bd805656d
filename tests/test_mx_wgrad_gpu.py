"""MX weight gradient on the MI355X (csrc/mx_wgrad.hip): gw = gy^T . x and gb = sum_m gy against a float64 product.  The shapes are the
smallest at which the kernel takes another path: a single row, a slab tail (31), two slabs (33), three (65: a last slice that is
partial at splits = 2 and a whole slab at 3); N odd (gy rows 2-byte aligned), one tile, a partial second tile; K below one tile and
a partial second tile.  The bound is the weight-only contract with M as the length (mxfp4_a4_ref.tolerance): exact products, at most one
fp32 ulp per accumulated term, one rounding to the dtype.  One collected test runs the four groups over both dtypes and output types."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
_spec = importlib.util.spec_from_file_location("mxfp4_a4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_a4_ref.py"))
_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ref)
tolerance = _ref.tolerance
from bitorch_engine.extensions import mx_grad_weight_cuda as G  # noqa: E402

# (M, N, K, splits)
CASES = [(1, 5, 32, 1), (1, 128, 160, -1), (31, 136, 32, 1), (31, 5, 160, -1), (33, 5, 32, 2), (33, 128, 160, 1), (33, 136, 160, 2),
         (65, 5, 160, 3), (65, 128, 32, 2), (65, 136, 160, 1), (65, 136, 160, 2), (65, 136, 160, 3), (65, 136, 160, -1)]


def operands(M, N, K, dt, exact):
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    if exact:  # multiples of 1/8 in [-1, 1]: every product and every partial sum is an fp32 number, in any order
        gy, x = (torch.randint(-8, 9, s, generator=g).to(dt) / 8 for s in ((M, N), (M, K)))
    else:      # standard normal data, kept in the dtype's normal range: anything below fp16's smallest normal becomes 1
        gy, x = (torch.randn(s, generator=g).to(dt) for s in ((M, N), (M, K)))
        gy, x = (torch.where(t.abs() < 2.0 ** -14, torch.ones_like(t), t) for t in (gy, x))
    return gy.to(DEV), x.to(DEV)


def exact_data_is_bit_exact_at_every_split(dt, out_fp32):
    out_dt = torch.float32 if out_fp32 else dt
    for M, N, K, S in CASES:
        gy, x = operands(M, N, K, dt, True)
        gw, gb = G.grad_weight(gy, x, out_dtype=out_dt, bias=True, splits=S)
        assert gw.dtype == out_dt and tuple(gw.shape) == (N, K) and tuple(gb.shape) == (N,)
        assert torch.equal(gw, (gy.double().t() @ x.double()).float().to(out_dt)), (dt, out_dt, M, N, K, S)
        assert torch.equal(gb, gy.double().sum(0).float().to(out_dt)), (dt, out_dt, M, N, K, S)
        assert torch.equal(G.grad_weight(gy, x, out_dtype=out_dt, splits=S), gw), (dt, out_dt, M, N, K, S)  # no bias sum, a second call: the same bits


def check(got, ref, absprod, M, dt, what):
    tol = tolerance(ref, absprod, M, dt)
    err = (got.double() - ref).abs()
    print(f"{what}: max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= tol).all(), f"{what}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def random_data_against_float64(dt, out_fp32):
    for M, N, K, S in CASES:
        gy, x = operands(M, N, K, dt, False)
        gw, gb = G.grad_weight(gy, x, out_dtype=torch.float32 if out_fp32 else dt, bias=True, splits=S)
        check(gw, gy.double().t() @ x.double(), gy.double().abs().t() @ x.double().abs(), M, dt, f"gw {(dt, out_fp32, M, N, K, S)}")
        check(gb, gy.double().sum(0), gy.double().abs().sum(0), M, dt, f"gb {(dt, out_fp32, M, N, K, S)}")


def nan_locality_zero_rows_and_alignment(dt):
    M, N, K = 65, 136, 160
    gy, x = operands(M, N, K, dt, True)
    clean_w, clean_b = G.grad_weight(gy, x, bias=True, splits=2)
    bad = gy.clone()
    bad[40, 131] = float("nan")
    gw, gb = G.grad_weight(bad, x, bias=True, splits=2)
    rows = torch.arange(N, device=DEV) != 131
    assert torch.isnan(gw[131]).all() and torch.isnan(gb[131])
    assert torch.equal(gw[rows], clean_w[rows]) and torch.equal(gb[rows], clean_b[rows])
    zw, zb = G.grad_weight(gy[:0], x[:0], bias=True)
    assert tuple(zw.shape) == (N, K) and tuple(zb.shape) == (N,) and not zw.any() and not zb.any()
    gy_t = gy.t().contiguous().t()
    x_off = torch.empty(M * K + 1, dtype=dt, device=DEV)[1:].view(M, K).copy_(x)
    assert not gy_t.is_contiguous() and x_off.data_ptr() % 16 != 0  # a transposed gy, an x view 2 bytes into its storage
    for S in (1, 2):
        w, b = G.grad_weight(gy, x, bias=True, splits=S)
        w2, b2 = G.grad_weight(gy_t, x_off, bias=True, splits=S)
        assert torch.equal(w, w2) and torch.equal(b, b2)
    gy_off = torch.empty(M * 5 + 1, dtype=dt, device=DEV)[1:].view(M, 5).copy_(gy[:, :5])
    assert gy_off.data_ptr() % 16 != 0 and torch.equal(G.grad_weight(gy_off, x), G.grad_weight(gy[:, :5].contiguous(), x))


def layer_backward_with_the_kernel(cls):
    from bitorch_engine.layers.qlinear.nbit import cuda as layers
    M, N, K, dt = 33, 136, 160, torch.float16
    g = torch.Generator().manual_seed(7)
    layer = getattr(layers, cls)(K, N, bias=True, dtype=dt, device=DEV).train()
    x0 = torch.randn((M, K), generator=g).to(dt).to(DEV)
    gy = torch.randn((M, N), generator=g).to(dt).to(DEV)
    got = {}
    for mode in ("torch", "kernel"):
        layer.grad_weight = mode
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        layer(x).backward(gy)
        got[mode] = (layer.weight.grad.clone(), layer.bias.grad.clone(), x.grad.clone())
    ref_w, abs_w = gy.double().t() @ x0.double(), gy.double().abs().t() @ x0.double().abs()
    ref_b, abs_b = gy.double().sum(0), gy.double().abs().sum(0)
    check(got["kernel"][0], ref_w, abs_w, M, dt, f"{cls} weight.grad")
    check(got["kernel"][1], ref_b, abs_b, M, dt, f"{cls} bias.grad")
    assert ((got["kernel"][0].double() - got["torch"][0].double()).abs() <= 2 * tolerance(ref_w, abs_w, M, dt)).all()
    assert ((got["kernel"][1].double() - got["torch"][1].double()).abs() <= 2 * tolerance(ref_b, abs_b, M, dt)).all()
    assert torch.equal(got["kernel"][2], got["torch"][2])


def test_mx_wgrad():
    for dt in (torch.float16, torch.bfloat16):
        for out_fp32 in (0, 1):
            print(f"--- {dt}, out_fp32 = {out_fp32}")  # shown with a failure: which pass of the loops it was
            exact_data_is_bit_exact_at_every_split(dt, out_fp32)
            random_data_against_float64(dt, out_fp32)
        nan_locality_zero_rows_and_alignment(dt)
    for cls in ("MXFP4LinearCuda", "MXFP6LinearCuda", "MXFP8LinearCuda"):
        layer_backward_with_the_kernel(cls)
