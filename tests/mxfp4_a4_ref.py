"""The MXFP4 W4A4 layer restated in torch on the CPU (INTEGRATION.md "MXFP4 W4A4 linear layer"): the activation quantiser is the weight
quantiser of mxfp4_ref.py applied to x [M, K], plus the non-finite row rule; the reference product is float64 x^ . W^^T + bias with its
absolute-value product.  Shared by test_mxfp4_a4_cpu.py, test_mxfp4_a4_gpu.py and sweeps/fuzz_mxfp4_a4.py."""
import importlib.util
import os

import torch

_spec = importlib.util.spec_from_file_location("mxfp4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_ref.py"))
mx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mx)


def quantize_act(x: torch.Tensor):
    """x [M, K] -> (xq uint8 [M, K/2] packed, xs uint8 [M, K/32], row_flag uint8 [M]).  A row with a NaN or +-inf is flagged; its codes
    and scales are unspecified (here: those of the row with the non-finite values replaced by zero)."""
    flag = ~torch.isfinite(x.float()).all(dim=1)
    xf = torch.where(torch.isfinite(x.float()), x.float(), torch.zeros((), dtype=torch.float32))
    xf = torch.where(flag[:, None], xf, x.float())  # keeps -0.0 of finite rows
    codes, scales = mx.quantize(xf)
    return mx.pack(codes), scales, flag.to(torch.uint8)


def dequant_act(xq: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
    """x^ [M, K] float64 (exact)."""
    return mx.dequant(xq, xs)


def block_sums(xq: torch.Tensor, qweight: torch.Tensor) -> torch.Tensor:
    """[M, N, K/32] float64: the sum over each block of e2m1(x code) * e2m1(w code), without the scales."""
    one_x = torch.full((xq.shape[0], xq.shape[1] // 16), 127, dtype=torch.uint8)
    one_w = torch.full((qweight.shape[0], qweight.shape[1] // 16), 127, dtype=torch.uint8)
    a = mx.dequant(xq, one_x).reshape(xq.shape[0], 1, -1, 32)
    w = mx.dequant(qweight, one_w).reshape(1, qweight.shape[0], -1, 32)
    return (a * w).sum(-1)


def reference(xq, xs, row_flag, qweight, scales, bias=None, device="cpu"):
    """(y float64 [M, N], absprod float64 [M, N]) = x^ . W^^T + bias and |x^| . |W^|^T + |bias|; rows with row_flag are NaN in y, and so
    are columns with a scale-255 block.  The products run on `device`."""
    xh = dequant_act(xq.cpu(), xs.cpu()).to(device)
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


def tolerance(yref, absprod, K, dt):
    """The weight-only layer's contract (tests/test_mxfp4_gpu.py) on x^: one rounding to dt, an fp32 sum of exact block sums."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + (K + 2) * 2.0 ** -23 * absprod + tiny
