"""The MXFP6 input gradient restated in float64 (INTEGRATION.md "MXFP6 input gradient"): gx = gy . W^ with W^ from mxfp6_ref.dequant, its
absolute-value product, and the contract's tolerance.  No constant of its own: the tolerance is the MXFP4 input gradient's (exact
products, an fp32 sum of N terms, one rounding).  Shared by test_mxfp6_grad_cpu.py, test_mxfp6_grad_gpu.py and sweeps/fuzz_mxfp6_grad.py."""
import importlib.util
import os

import torch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("mxfp6_ref")


def grad_reference(gy, qweight, scales, device="cpu"):
    """(gx float64 [M, K], absprod float64 [M, K]) = gy . W^ and |gy| . |W^|, W^[n, k] = e2m3(code) * 2^(scales[n, k // 32] - 127); a
    block-column that holds a scale-255 block is NaN in gx (a float product with a NaN weight).  The products run on `device`."""
    W = ref.dequant(qweight, scales).to(device)
    g = gy.to(device).double()
    nan_col = torch.isnan(W).any(dim=0)
    Wf = torch.nan_to_num(W, nan=0.0)
    gx, a = g @ Wf, g.abs() @ Wf.abs()
    gx[:, nan_col] = float("nan")
    return gx, a


def tolerance(gxref, absprod, n, dt):
    """eps_dt * |ref| + (n + 2) * 2^-23 * absprod + tiny: one rounding to dt (fp32: none beyond the sum's), at most one fp32 ulp of the
    running sum per accumulated product (products are exact: a 16-bit significand times the 4 bits of E2M3)."""
    eps = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}[dt]
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * gxref.abs() + (n + 2) * 2.0 ** -23 * absprod + tiny


def rand_mx(N, K, g, lo=119, hi=130):
    """Every code byte, scale codes lo .. hi (119 .. 130: e_blk - s <= 11, every fp16 fragment is a normal number)."""
    q = torch.randint(0, 256, (N, K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s
