"""The MXFP6 W6A6 layer restated in torch on the CPU (INTEGRATION.md "MXFP6 W6A6 linear layer"): the activation side is the WEIGHT
quantiser of mxfp6_ref.py applied to x (same rule, same bytes) with the row flag of mxfp4_a8_ref; the reference product is float64
x^ . W^^T + bias with its absolute-value product.  Shared by test_mxfp6_a6_cpu.py, test_mxfp6_a6_gpu.py and sweeps/fuzz_mxfp6_a6.py."""
import importlib.util
import os

import torch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mx6 = _load("mxfp6_ref")
a8 = mx6.a8
mx = mx6.mx

quantize, pack, unpack, e2m3, dequant = mx6.quantize, mx6.pack, mx6.unpack, mx6.e2m3, mx6.dequant


def quantize_act(x: torch.Tensor):
    """x [M, K] -> (xq6 uint8 [M, 3K/4] packed, xs uint8 [M, K/32], row_flag uint8 [M]): mxfp6_ref.quantize + pack.  A row with a NaN or
    +-inf is flagged; its codes and scales are unspecified (here: those of the row with the non-finite values replaced by zero, the
    rule of mxfp4_a8_ref)."""
    xf = x.float()
    fin = torch.isfinite(xf)
    flag = ~fin.all(dim=1)
    clean = torch.where(fin, xf, torch.zeros((), dtype=torch.float32))
    clean = torch.where(flag[:, None], clean, xf)  # keeps -0.0 of finite rows
    c, s = mx6.quantize(clean)
    return mx6.pack(c), s, flag.to(torch.uint8)


def dequant_act(xq6: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
    """x^ [M, K] float64 (exact)."""
    return mx6.dequant(xq6, xs)


def reference(xq6, xs, row_flag, qweight, scales, bias=None, device="cpu"):
    """(y float64 [M, N], absprod float64 [M, N]) = x^ . W^^T + bias and |x^| . |W^|^T + |bias|; rows with row_flag are NaN in y, and so
    are columns with a scale-255 block.  The products run on `device`."""
    xh = dequant_act(xq6, xs).to(device)
    W = mx6.dequant(qweight, scales).to(device)
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


PROBE_ULPS = 0.9364  # profiles/mxfp6_a6_probe.txt part (c): the worst error of one instruction, in fp32 ulps of sum |products|


def tolerance(yref, absprod, K, dt):
    """eps_dt * |y| + 2 * PROBE_ULPS * 2^-23 * absprod + tiny: one rounding to dt, plus the accumulation term, twice the probe's worst
    count as in the W4A8 and W6A8 contracts.  tools/probe/probe_mx_fp6x6.hip part (c) (profiles/mxfp6_a6_probe.txt) measured ONE
    instruction with two FP6 operands against float64: exact wherever all its blocks carry one scale (the products lie on a 2^-6 grid,
    so every sum is an fp32 value), and at worst 0.9364 fp32 ulps of its sum |products| where the blocks differ in scale (16x16x128;
    0.5469 in 32x32x64).  The yardstick is the instruction measured alone, not the kernels' own error."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + 2 * PROBE_ULPS * 2.0 ** -23 * absprod + tiny
