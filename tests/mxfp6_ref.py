"""The MXFP6 format (OCP microscaling FP6 with E2M3 elements), its quantisation rule and the W6A8 layer restated in torch on the CPU
(INTEGRATION.md "MXFP6 W6A8 linear layer").  The activation side is mxfp4_a8_ref's (the MXFP8 quantiser, unchanged); the reference
product is float64 x^ . W^^T + bias with its absolute-value product.  Shared by test_mxfp6_a8_cpu.py, test_mxfp6_a8_gpu.py and
sweeps/fuzz_mxfp6_a8.py."""
import importlib.util
import os

import torch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


a8 = _load("mxfp4_a8_ref")
mx = a8.mx

# code & 31 -> magnitude: exponent (bias 1) in bits 4:3, mantissa in bits 2:0; exponent 0 is subnormal (m / 8)
E2M3 = torch.tensor([m / 8.0 for m in range(8)] + [(1 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)], dtype=torch.float64)
E2M3_MAX = 7.5

quantize_act = a8.quantize_act
dequant_act = a8.dequant_act


def quantize(w: torch.Tensor):
    """w [N, K] (fp32 / fp16 / bf16) -> (codes uint8 [N, K] unpacked, scales uint8 [N, K/32]).

    Per block of 32 along K, in fp32: amax = max |w|; e = floor(log2 amax) - 2 clamped to [-127, 127]; a = min(|w / 2^e|, 7.5) rounded to
    the nearest E2M3 value, ties to the even code (0.0625 -> 0, 0.1875 -> 0.25, 1.9375 -> 2), the sign bit (0x20) copied from w (so
    -0.0 and -0.03 -> 0x20).  An all-zero block: scale 0, all codes 0.  The code is linear in a on each of [0, 2], [2, 4], [4, 7.5]
    (8 a, 4 a + 8, 2 a + 16) with even offsets, so torch.round's ties-to-even on the scaled value is ties-to-even on the code."""
    N, K = w.shape
    wf = w.float().reshape(N, K // 32, 32)
    amax = wf.abs().amax(dim=-1)
    nz = amax > 0
    e = (mx.floor_log2_f32(torch.where(nz, amax, torch.ones_like(amax))) - 2).clamp(-127, 127)
    v = torch.ldexp(wf, (-e)[..., None].float())  # exact: a power-of-two multiply (w / 2^e)
    a = v.abs().clamp(max=E2M3_MAX)
    idx = torch.where(a < 2, torch.round(a * 8), torch.where(a < 4, torch.round(a * 4) + 8, torch.round(a * 2) + 16)).int()
    sign = (wf.view(torch.int32) < 0).int() * 32
    codes = torch.where(nz[..., None], idx | sign, torch.zeros_like(idx))
    scales = torch.where(nz, e + 127, torch.zeros_like(e))
    return codes.reshape(N, K).to(torch.uint8), scales.to(torch.uint8)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [N, K] -> qweight uint8 [N, 3K/4]: per block of 32, code j in bits 6 j .. 6 j + 5 of the block's little-endian 192-bit
    integer, i.e. four codes c0 .. c3 in three bytes: c0 | c1 << 6, c1 >> 2 | c2 << 4, c2 >> 4 | c3 << 2."""
    c = codes.to(torch.int32).reshape(codes.shape[0], -1, 4)
    b0 = (c[..., 0] | (c[..., 1] << 6)) & 0xFF
    b1 = ((c[..., 1] >> 2) | (c[..., 2] << 4)) & 0xFF
    b2 = ((c[..., 2] >> 4) | (c[..., 3] << 2)) & 0xFF
    return torch.stack([b0, b1, b2], dim=-1).reshape(codes.shape[0], -1).to(torch.uint8)


def unpack(qweight: torch.Tensor) -> torch.Tensor:
    b = qweight.to(torch.int32).reshape(qweight.shape[0], -1, 3)
    c0 = b[..., 0] & 63
    c1 = ((b[..., 0] >> 6) | (b[..., 1] << 2)) & 63
    c2 = ((b[..., 1] >> 4) | (b[..., 2] << 4)) & 63
    c3 = b[..., 2] >> 2
    return torch.stack([c0, c1, c2, c3], dim=-1).reshape(qweight.shape[0], -1).to(torch.uint8)


def e2m3(codes: torch.Tensor) -> torch.Tensor:
    """unpacked codes -> float64 (exact)."""
    c = codes.to(torch.int64)
    return E2M3[c & 31] * torch.where((c & 32) > 0, -1.0, 1.0).to(torch.float64)


def dequant(qweight: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """W [N, K] float64 (exact; every value is also exact in fp32), NaN in a block of scale code 255."""
    return e2m3(unpack(qweight.cpu())) * mx.e8m0(scales.cpu()).repeat_interleave(32, dim=1)


def reference(xq, xs, row_flag, qweight, scales, bias=None, device="cpu"):
    """(y float64 [M, N], absprod float64 [M, N]) = x^ . W^^T + bias and |x^| . |W^|^T + |bias|; rows with row_flag are NaN in y, and so
    are columns with a scale-255 block.  The products run on `device`."""
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


PROBE_ULPS = 1853  # profiles/mxfp6_a8_probe.txt part (c): the worst error of one instruction, in fp32 ulps of sum |products|


def tolerance(yref, absprod, K, dt):
    """eps_dt * |y| + 2 * PROBE_ULPS * 2^-23 * absprod + tiny: one rounding to dt, plus the accumulation term.  The derived term of the
    W4A4 contract is (K + 2) * 2^-23 * absprod: at most one fp32 ulp per accumulated product.  tools/probe/probe_mx_fp6.hip part (c)
    (profiles/mxfp6_a8_probe.txt) shows that ONE instruction with an FP6 and an E4M3 operand errs by more than that against float64: at
    worst 1853 fp32 ulps of its sum |products| in 32x32x64 (64 products) and 790.25 in 16x16x128 (128 products), on random codes.  The
    errors of the instructions of one output add up to at most PROBE_ULPS ulps of the whole absprod, so the constant is twice the
    probe's worst count in place of K + 2, as in the W4A8 contract; the kernels' own error is not the yardstick."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + 2 * PROBE_ULPS * 2.0 ** -23 * absprod + tiny
