"""The MXFP4 W4A8 layer restated in torch on the CPU (INTEGRATION.md "MXFP4 W4A8 linear layer"): the MXFP8 activation quantiser (the OCP
MX v1.0 rule with E4M3 elements, emax = 8) plus the non-finite row rule; the reference product is float64 x^ . W^^T + bias with its
absolute-value product.  Shared by test_mxfp4_a8_cpu.py, test_mxfp4_a8_gpu.py and sweeps/fuzz_mxfp4_a8.py."""
import importlib.util
import os

import torch

_spec = importlib.util.spec_from_file_location("mxfp4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_ref.py"))
mx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mx)

E4M3_MAX = 448.0
EMAX = 8  # floor(log2(448))


def quantize_act(x: torch.Tensor):
    """x [M, K] -> (xq uint8 [M, K] e4m3fn bytes, xs uint8 [M, K/32], row_flag uint8 [M]).  Per block of 32, in fp32: amax = max |x|;
    e = floor(log2 amax) - 8 clamped to [-127, 127]; xs = e + 127; xq = e4m3fn(clamp(x * 2^-e, -448, 448)), round to nearest even (torch's
    cast; it does not saturate, hence the clamp first), the sign kept.  An all-zero block (either zero): scale 0, all bytes 0.  A row
    with a NaN or +-inf is flagged; its codes and scales are unspecified (here: those of the row with the non-finite values replaced
    by zero)."""
    M, K = x.shape
    flag = ~torch.isfinite(x.float()).all(dim=1)
    xf = torch.where(torch.isfinite(x.float()), x.float(), torch.zeros((), dtype=torch.float32))
    xf = torch.where(flag[:, None], xf, x.float())  # keeps -0.0 of finite rows
    b = xf.reshape(M, K // 32, 32)
    amax = b.abs().amax(dim=-1)
    nz = amax > 0
    e = (mx.floor_log2_f32(torch.where(nz, amax, torch.ones_like(amax))) - EMAX).clamp(-127, 127)
    v = torch.ldexp(b, (-e)[..., None].float())  # exact: a power-of-two multiply
    codes = v.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    codes = torch.where(nz[..., None], codes, torch.zeros_like(codes))
    scales = torch.where(nz, e + 127, torch.zeros_like(e))
    return codes.reshape(M, K).contiguous(), scales.to(torch.uint8), flag.to(torch.uint8)


def e4m3(xq: torch.Tensor) -> torch.Tensor:
    """e4m3fn bytes -> float64 (exact)."""
    return xq.cpu().contiguous().view(torch.float8_e4m3fn).to(torch.float32).double()


def dequant_act(xq: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
    """x^ [M, K] float64 (exact)."""
    return e4m3(xq) * mx.e8m0(xs.cpu()).repeat_interleave(32, dim=1)


def reference(xq, xs, row_flag, qweight, scales, bias=None, device="cpu"):
    """(y float64 [M, N], absprod float64 [M, N]) = x^ . W^^T + bias and |x^| . |W^|^T + |bias|; rows with row_flag are NaN in y, and so
    are columns with a scale-255 block.  The products run on `device`."""
    xh = dequant_act(xq, xs).to(device)
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


PROBE_ULPS = 1552  # profiles/mxfp4_a8_probe.txt part (c): the worst error of one instruction, in fp32 ulps of sum |products|


def tolerance(yref, absprod, K, dt):
    """eps_dt * |y| + 2 * PROBE_ULPS * 2^-23 * absprod + tiny: one rounding to dt, plus the accumulation term.  The derived term of the
    W4A4 contract is (K + 2) * 2^-23 * absprod: at most one fp32 ulp (truncation allowed) per accumulated product on a running magnitude
    <= absprod.  tools/probe/probe_mx_a8.hip part (c) (profiles/mxfp4_a8_probe.txt) shows that ONE instruction with an E4M3 operand
    errs by more than that against float64: at worst 1552 fp32 ulps of its sum |products| in 32x32x64 (64 products, 24 ulps per
    product) and 956 in 16x16x128 (128 products), on random codes whose exact sums ARE fp32 values, so the instruction drops low bits
    of the small products of a block.  The errors of the instructions of one output add up to at most PROBE_ULPS ulps of the whole
    absprod, so the constant is twice the probe's worst count in place of K + 2; the kernels' own error is not the yardstick."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + 2 * PROBE_ULPS * 2.0 ** -23 * absprod + tiny
