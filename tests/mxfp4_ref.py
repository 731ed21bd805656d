"""The MXFP4 format and the OCP MX v1.0 quantisation rule restated in torch (INTEGRATION.md "MXFP4 linear layer"), on the CPU.  Shared
by test_mxfp4_cpu.py and test_mxfp4_gpu.py."""
import torch

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def floor_log2_f32(a: torch.Tensor) -> torch.Tensor:
    """floor(log2 a) of positive fp32 values from their bits (normal: the exponent field; subnormal: the leading mantissa bit)."""
    bits = a.float().view(torch.int32)
    ex = bits >> 23
    mant = bits & 0x7FFFFF
    top = torch.zeros_like(mant)
    for b in range(23):
        top = torch.where((mant >> b) > 0, torch.full_like(mant, b), top)
    return torch.where(ex > 0, ex - 127, top - 149)


def quantize(w: torch.Tensor):
    """w [N, K] (fp32 / fp16 / bf16) -> (codes uint8 [N, K] unpacked, scales uint8 [N, K/32]).

    Per block of 32 along K, in fp32: amax = max |w|; e = floor(log2 amax) - 2 clamped to [-127, 127]; codes = w / 2^e rounded to the
    nearest E2M1 value, ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), 6 or more
    saturating to 6, the sign bit copied from w (so -0.1 -> 0x8).  An all-zero block: scale 0, all codes 0."""
    N, K = w.shape
    wf = w.float().reshape(N, K // 32, 32)
    amax = wf.abs().amax(dim=-1)
    nz = amax > 0
    e = (floor_log2_f32(torch.where(nz, amax, torch.ones_like(amax))) - 2).clamp(-127, 127)
    v = torch.ldexp(wf, (-e)[..., None].float())  # exact: a power-of-two multiply (w / 2^e)
    a = v.abs()
    idx = ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int() + (a >= 1.75).int() + (a > 2.5).int() + (a >= 3.5).int() + (a > 5.0).int())
    sign = (wf.view(torch.int32) < 0).int() * 8
    codes = torch.where(nz[..., None], idx | sign, torch.zeros_like(idx))
    scales = torch.where(nz, e + 127, torch.zeros_like(e))
    return codes.reshape(N, K).to(torch.uint8), scales.to(torch.uint8)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [N, K] -> qweight uint8 [N, K/2]: element 2j in the low nibble of byte j, 2j + 1 in the high nibble."""
    c = codes.to(torch.int32)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)


def unpack(qweight: torch.Tensor) -> torch.Tensor:
    q = qweight.to(torch.int32)
    return torch.stack([q & 0xF, q >> 4], dim=-1).reshape(q.shape[0], -1).to(torch.uint8)


def e8m0(scales: torch.Tensor) -> torch.Tensor:
    """E8M0 codes -> float64 2^(s - 127), NaN for 255."""
    s = scales.to(torch.float64)
    return torch.where(scales == 255, torch.full_like(s, float("nan")), torch.exp2(s - 127))


def dequant(qweight: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """W [N, K] float64 (exact; every value is also exact in fp32)."""
    c = unpack(qweight.cpu()).to(torch.int64)
    v = E2M1[c & 7] * torch.where((c & 8) > 0, -1.0, 1.0).to(torch.float64)
    return v * e8m0(scales.cpu()).repeat_interleave(32, dim=1)
