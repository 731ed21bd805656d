"""The MXFP8 W8A8 layer restated in torch on the CPU (INTEGRATION.md "MXFP8 W8A8 linear layer"): the activation side is that of
mxfp4_a8_ref.py (the E4M3 quantiser with the row flag, same bytes); the weight side is the same rule per block plus the NaN-block rule
(a block that holds a NaN or +-inf: scale code 255, zero bytes); the reference product is float64 x^ . W^^T + bias with its
absolute-value product.  Shared by test_mxfp8_a8_cpu.py, test_mxfp8_a8_gpu.py, test_mx8a8_arena_gpu.py and sweeps/fuzz_mxfp8_a8.py."""
import importlib.util
import os

import torch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


a8 = _load("mxfp4_a8_ref")
mx = a8.mx  # mxfp4_ref: floor_log2_f32, e8m0

quantize_act, dequant_act, e4m3 = a8.quantize_act, a8.dequant_act, a8.e4m3


def quantize(w: torch.Tensor):
    """w [N, K] (fp32 / fp16 / bf16) -> (qweight uint8 [N, K] e4m3fn bytes, scales uint8 [N, K/32]): quantize_act's rule per block of 32;
    a block that holds a NaN or +-inf gets scale code 255 and zero bytes (quantize_act zeroes the non-finite values of a flagged row
    and quantises the rest: those bytes are replaced here).  Never a NaN code."""
    N, K = w.shape
    q, s, _ = quantize_act(w)
    bad = ~torch.isfinite(w.float()).reshape(N, K // 32, 32).all(dim=-1)
    q = torch.where(bad[..., None], torch.zeros((), dtype=torch.uint8), q.reshape(N, K // 32, 32)).reshape(N, K)
    s = torch.where(bad, torch.full((), 255, dtype=torch.uint8), s)
    return q.contiguous(), s.contiguous()


def rand_w(N, K, g, lo=112, hi=124):
    """Random weights for the tests: every e4m3fn byte but the two NaN codes (0x7F -> 0x7E, 0xFF -> 0xFE), scale codes lo .. hi.  The
    default scales are those of the sibling tests (118 .. 130) moved down by 6: E4M3 reaches 448 where E2M1 stops at 6."""
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    q = torch.where((q & 0x7F) == 0x7F, q - 1, q).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


def dequant(qweight: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """W^ [N, K] float64 (exact); NaN over a block with scale code 255 and at a NaN code."""
    return dequant_act(qweight, scales)


def reference(xq, xs, row_flag, qweight, scales, bias=None, device="cpu"):
    """(y float64 [M, N], absprod float64 [M, N]) = x^ . W^^T + bias and |x^| . |W^|^T + |bias|; rows with row_flag are NaN in y, and so
    are columns with a scale-255 block or a NaN code.  The products run on `device`."""
    xh = dequant_act(xq, xs).to(device)
    W = dequant(qweight, scales).to(device)
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


PROBE_ULPS = 3688.5782  # profiles/mxfp8_a8_probe.txt part (c): the worst error of one instruction, in fp32 ulps of sum |products|


def tolerance(yref, absprod, K, dt):
    """eps_dt * |y| + 2 * PROBE_ULPS * 2^-23 * absprod + tiny: one rounding to dt, plus the accumulation term, twice the probe's worst
    count as in the W4A8, W6A8, W6A6 and W4A6 contracts.  tools/probe/probe_mx_fp8x8.hip part (c) (profiles/mxfp8_a8_probe.txt)
    measured ONE instruction with two E4M3 operands against the exact sum: it is exact on large positive products, but already on codes
    of 0.25 .. 7.5 with mixed signs under one scale, where every exact sum is an fp32 value, it errs by up to 128 fp32 ulps of its sum
    |products| (32x32x64; 64 in 16x16x128), and on codes of the whole E4M3 range (2^-9 .. 448) by up to 2763 ulps under one scale and
    3688.5782 where the blocks differ in scale (16x16x128; 3318.1198 in 32x32x64): the instruction drops low bits of the small products
    of a block, as the W4A8 probe found with one E4M3 operand.  The yardstick is the instruction measured alone, not the kernels' own
    error."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + 2 * PROBE_ULPS * 2.0 ** -23 * absprod + tiny
