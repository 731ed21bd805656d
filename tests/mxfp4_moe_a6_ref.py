"""The MXFP4 W4A6 mixture-of-experts layer restated in torch / float64 (INTEGRATION.md "MXFP4 W4A6 mixture-of-experts layer").  It only
composes what exists: the weight side is mxfp4_ref.py per expert (quantize, pack, and mxfp4_moe_ref.dequant, as mxfp4_moe_a8_ref.py uses
it), the activation rows are mxfp6_a6_ref.quantize_act (the E2M3 quantiser with the row flag), the routed product and the block are the
MoE restatements' (mxfp4_moe_ref.experts, which takes W as float64 and does not know its format; the block of mxfp4_moe_a8_ref.py with
the FP6 activation quantiser at both projection inputs), and the tolerance is mxfp4_a6_ref.tolerance, the measured 2 * PROBE_ULPS
contract.  Shared by test_mxfp4_moe_a6_cpu.py, test_mxfp4_moe_a6_gpu.py, test_mx4a6_moe_arena_gpu.py and sweeps/fuzz_mxfp4_moe_a6.py."""
import importlib.util
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


a46 = _load("mxfp4_a6_ref")      # the W4A6 linear restatement: its tolerance is this layer's
m8 = _load("mxfp4_moe_a8_ref")   # the W4A8 expert restatement: its weight side is this layer's
a6 = a46.a6                      # mxfp6_a6_ref: the activation quantiser
m6 = a46.mx6                     # mxfp6_ref: the E2M3 codes and their 24-byte blocks (the x side)
mx = a46.mx                      # mxfp4_ref: the weight side
mref = m8.mref                   # mxfp4_moe_ref

quantize = mx.quantize
pack = mx.pack
tolerance = a46.tolerance
dequant = mref.dequant


def quantize_packed(w: torch.Tensor):
    """w float [E, N, K] -> (qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32]): mxfp4_ref.quantize and pack per expert."""
    qs, ss = [], []
    for e in range(w.shape[0]):
        codes, scales = mx.quantize(w[e])
        qs.append(mx.pack(codes))
        ss.append(scales)
    return torch.stack(qs), torch.stack(ss)


def quantize_rows(x: torch.Tensor):
    """The stored rows of x ([T, K] or [T, S, K], on any device) quantised on the CPU: (xq6 [R, 3K/4], xs [R, K/32], row_flag [R])."""
    return a6.quantize_act(x.detach().cpu().reshape(-1, x.shape[-1]))


def experts_from_codes(xq6, xs, row_flag, idx, W, bias=None):
    """Per pair, from quantised rows (R = T or T * S of them): (y [T, S, N] float64, the same sum over absolute values).  y is NaN for the
    live pairs of a flagged row and in the columns of an expert that hold a NaN (scale-255) block; a skipped slot is 0 whatever its row.
    mxfp4_moe_a8_ref.experts_from_codes with the FP6 decoder."""
    E, N, K = W.shape
    T, S = idx.shape
    dev = W.device
    xh = a6.dequant_act(xq6.cpu(), xs.cpu())
    flag = row_flag.cpu().bool()
    xh = torch.where(flag[:, None], torch.zeros((), dtype=torch.float64), xh)  # a flagged row's codes are unspecified
    per_pair = xh.shape[0] != T
    xh = xh.reshape(T, S, K) if per_pair else xh
    nan_col = torch.isnan(W).any(dim=-1)
    y, a = mref.experts(xh.to(dev), idx, torch.nan_to_num(W, nan=0.0), bias)
    flat = idx.reshape(-1).long().to(dev)
    live = (flat >= 0) & (flat < E)
    bad = torch.zeros((T * S, N), dtype=torch.bool, device=dev)
    bad[live] = nan_col[flat[live]]
    pair_flag = (flag.reshape(T, S) if per_pair else flag[:, None].expand(T, S)).reshape(-1).to(dev)
    bad |= (pair_flag & live)[:, None]
    y = torch.where(bad.reshape(T, S, N), torch.full((), float("nan"), dtype=torch.float64, device=dev), y)
    return y, a


def experts(x, idx, W, bias=None):
    """The layer from x: quantise the stored rows, then experts_from_codes."""
    return experts_from_codes(*quantize_rows(x), idx, W, bias)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """x^ float64 in x's shape: the activation quantiser and back (finite x)."""
    xq, xs, _ = quantize_rows(x)
    return a6.dequant_act(xq, xs).reshape(x.shape)


def block(x, router_w, router_b, k, Wgu, bgu, Wd, bd, limit=7.0, alpha=1.702, dt=None, logits=None):
    """mxfp4_moe_a8_ref.block with the FP6 activation quantiser where MXFP4A6MoECuda quantises: x before gate_up and a before down.
    dt None: everything else in float64; dt fp16 / bf16: rounded to dt at the layer's rounding points as well."""
    rnd = (lambda t: t) if dt is None else (lambda t: t.to(dt).double())
    xd = x.double()
    lg = rnd(xd @ router_w.double().t() + (0 if router_b is None else router_b.double())) if logits is None else logits.double()
    v, idx = torch.topk(lg, k, dim=-1)
    w = rnd(torch.softmax(v, dim=-1))
    h = rnd(mref.experts(fake_quant(xd), idx, Wgu, bgu)[0])
    g, u = h[..., 0::2].clamp(max=limit), h[..., 1::2].clamp(min=-limit, max=limit)
    a = rnd((u + 1.0) * (g * torch.sigmoid(alpha * g)))
    o = rnd(mref.experts(fake_quant(a), idx, Wd, bd)[0])
    return rnd((w[..., None] * o).sum(dim=1)), idx
