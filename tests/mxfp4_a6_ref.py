"""The MXFP4 W4A6 layer restated in torch on the CPU (INTEGRATION.md "MXFP4 W4A6 linear layer"): the activation side is that of
mxfp6_a6_ref.py (the E2M3 quantiser with the row flag, same bytes), the weight side that of mxfp4_ref.py (same bytes); the reference
product is float64 x^ . W^^T + bias with its absolute-value product.  Shared by test_mxfp4_a6_cpu.py, test_mxfp4_a6_gpu.py,
test_mx4a6_arena_gpu.py and sweeps/fuzz_mxfp4_a6.py."""
import importlib.util
import os

import torch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


a6 = _load("mxfp6_a6_ref")
mx6 = a6.mx6  # mxfp6_ref: the E2M3 codes and their 24-byte blocks
a8 = a6.a8    # mxfp4_a8_ref
mx = a6.mx    # mxfp4_ref: the weight side

quantize_act, dequant_act = a6.quantize_act, a6.dequant_act
quantize, pack, unpack, dequant = mx.quantize, mx.pack, mx.unpack, mx.dequant


def reference(xq6, xs, row_flag, qweight, scales, bias=None, device="cpu"):
    """(y float64 [M, N], absprod float64 [M, N]) = x^ . W^^T + bias and |x^| . |W^|^T + |bias|; rows with row_flag are NaN in y, and so
    are columns with a scale-255 block (the NaN rules of mxfp6_a6_ref.reference).  The products run on `device`."""
    xh = dequant_act(xq6.cpu(), xs.cpu()).to(device)
    W = mx.dequant(qweight.cpu(), scales.cpu()).to(device)
    nan_col = torch.isnan(W).any(dim=1)
    Wf = torch.nan_to_num(W, nan=0.0)
    y = xh @ Wf.t()
    a = xh.abs() @ Wf.abs().t()
    if bias is not None:
        y = y + bias.to(device).double()
        a = a + bias.to(device).double().abs()
    y[:, nan_col] = float("nan")
    y[row_flag.to(device).bool()] = float("nan")
    return y, a


PROBE_ULPS = 0.75  # profiles/mxfp4_a6_probe.txt part (c): the worst error of one instruction, in fp32 ulps of sum |products|


def tolerance(yref, absprod, K, dt):
    """eps_dt * |y| + 2 * PROBE_ULPS * 2^-23 * absprod + tiny: one rounding to dt, plus the accumulation term, twice the probe's worst
    count as in the W4A8, W6A8 and W6A6 contracts.  tools/probe/probe_mx_fp4x6.hip part (c) (profiles/mxfp4_a6_probe.txt) measured ONE
    instruction with an FP4 and an FP6 operand against float64: exact wherever all its blocks carry one scale (the products lie on a
    2^-4 grid with |p| <= 45, so every sum is an fp32 value), and at worst 0.7500 fp32 ulps of its sum |products| where the blocks
    differ in scale (16x16x128; 0.5000 in 32x32x64).  The yardstick is the instruction measured alone, not the kernels' own error."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + 2 * PROBE_ULPS * 2.0 ** -23 * absprod + tiny
