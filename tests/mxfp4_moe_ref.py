"""The MXFP4 mixture-of-experts layer restated in torch / float64 (INTEGRATION.md "MXFP4 mixture-of-experts layer"), device-agnostic.
Shared by test_mxfp4_moe_cpu.py, test_mxfp4_moe_gpu.py and sweeps/fuzz_mxfp4_moe.py.  The weight format is mxfp4_ref.py's."""
import importlib.util
import os

import torch

_spec = importlib.util.spec_from_file_location("mxfp4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def dequant(qweight: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32] -> W [E, N, K] float64 (exact), on the tensors' device: mxfp4_ref.dequant's
    rule (test_mxfp4_moe_cpu.py compares the two), expert by expert so that a large stack needs no large temporaries."""
    E, N, KH = qweight.shape
    out = torch.empty((E, N, KH * 2), dtype=torch.float64, device=qweight.device)
    lut = ref.E2M1.to(qweight.device)
    for e in range(E):
        q = qweight[e].to(torch.int64)
        c = torch.stack([q & 0xF, q >> 4], dim=-1).reshape(N, KH * 2)
        v = torch.where((c & 8) > 0, -lut[c & 7], lut[c & 7])
        s = scales[e].to(torch.float64)
        s = torch.where(scales[e] == 255, torch.full_like(s, float("nan")), torch.exp2(s - 127))
        out[e] = v * s.repeat_interleave(32, dim=1)
    return out


def experts(x: torch.Tensor, idx: torch.Tensor, W: torch.Tensor, bias: torch.Tensor = None):
    """Per pair: y[t, s] = x_row . W[idx[t, s]]^T + bias[idx[t, s]] in float64, 0 for an index outside [0, E).  x [T, K] or [T, S, K],
    idx [T, S], W [E, N, K] float64 (on the device the product is to run on).  -> (y [T, S, N] float64, the same sum over absolute values)."""
    E, N, K = W.shape
    T, S = idx.shape
    dev = W.device
    xd = x.to(dev).double()
    xr = (xd if xd.dim() == 3 else xd[:, None, :].expand(T, S, K)).reshape(T * S, K)
    flat = idx.to(dev).reshape(-1).long()
    y = torch.zeros((T * S, N), dtype=torch.float64, device=dev)
    a = torch.zeros((T * S, N), dtype=torch.float64, device=dev)
    for e in range(E):
        rows = (flat == e).nonzero().reshape(-1)
        if rows.numel() == 0:
            continue
        ye, ae = xr[rows] @ W[e].t(), xr[rows].abs() @ W[e].abs().t()
        if bias is not None:
            ye, ae = ye + bias[e].to(dev).double(), ae + bias[e].to(dev).double().abs()
        y[rows], a[rows] = ye, ae
    return y.reshape(T, S, N), a.reshape(T, S, N)


def block(x, router_w, router_b, k, Wgu, bgu, Wd, bd, limit=7.0, alpha=1.702, dt=None, logits=None):
    """The MoE block.  dt None: everything in float64.  dt fp16 / bf16: the same arithmetic rounded to dt at the layer's rounding points
    (router logits, softmax weights, h, a, o, y), used to measure how far those roundings alone move the result.  The routing (top-k)
    is taken from `logits` when given, so that both versions route alike.  x [T, H]; router_w [E, H]; Wgu [E, 2I, H]; Wd [E, H, I]."""
    rnd = (lambda t: t) if dt is None else (lambda t: t.to(dt).double())
    xd = x.double()
    lg = rnd(xd @ router_w.double().t() + (0 if router_b is None else router_b.double())) if logits is None else logits.double()
    v, idx = torch.topk(lg, k, dim=-1)
    w = rnd(torch.softmax(v, dim=-1))
    h = rnd(experts(xd, idx, Wgu, bgu)[0])
    g, u = h[..., 0::2].clamp(max=limit), h[..., 1::2].clamp(min=-limit, max=limit)
    a = rnd((u + 1.0) * (g * torch.sigmoid(alpha * g)))
    o = rnd(experts(a, idx, Wd, bd)[0])
    return rnd((w[..., None] * o).sum(dim=1)), idx
