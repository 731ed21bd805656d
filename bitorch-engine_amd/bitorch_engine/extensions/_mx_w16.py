"""The forward / grad_input wrappers of the weight-only MX layers (MXFP4 and MXFP6 weights against fp16 / bf16 activations), written once:
the two linear modules, the two experts modules and the input gradients that the MXFP6 `_a8` modules define call the same four
sequences of checks, allocations and one C entry, and differ in the `bie_` symbol stem, the prefix of their messages, the function that
reads (N, K) or (E, N, K) off the weights and the col_exp / blk_exp they fill a missing e_col / e_blk with.  A module states those in a
Dense or an Experts object and keeps its own `forward` and `grad_input` definitions (names, argument names, defaults and docstrings are
the module's) as one call each.  Nothing here synchronises with the host.

_X_DT and _aligned live here and are re-exported by mxfp4_linear_cuda, where every other MX module looks for them."""
import torch

from bitorch_engine import _hip

_X_DT = (torch.float16, torch.bfloat16)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class Dense:
    """stem: `bie_<stem>_form / _linear_forward / _linear_grad_input`; prefix: the messages' (`mxfp4`); shape: (qweight, scales) -> (N, K);
    col_exp: scales -> e_col; blk_exp: scales -> e_blk."""

    def __init__(self, stem, prefix, shape, col_exp, blk_exp):
        self.stem, self.prefix, self.shape, self.col_exp, self.blk_exp = stem, prefix, shape, col_exp, blk_exp

    def entry(self, suffix):
        return getattr(_hip.lib(), f"bie_{self.stem}_{suffix}")

    def forward(self, x, qweight, scales, bias, e_col, form):
        _hip.need_gpu(x, qweight, scales, bias, e_col)
        if x.dtype not in _X_DT:
            raise RuntimeError(f"{self.prefix} linear: dtype {x.dtype} is not supported (fp16 / bf16)")
        N, K = self.shape(qweight, scales)
        if x.dim() != 2 or x.shape[1] != K:
            raise RuntimeError(f"{self.prefix} linear: x {tuple(x.shape)} does not match K={K}")
        M = x.shape[0]
        y = torch.empty((M, N), dtype=x.dtype, device=x.device)
        if M == 0:
            return y
        if form < 0:
            form = int(self.entry("form")(M, N, K, _hip.dt(x)))
        if form == 1 and e_col is None:
            e_col = self.col_exp(scales)
        if bias is not None:
            bias = bias.reshape(-1).to(dtype=x.dtype).contiguous()
        x, qweight, scales = _aligned(x), _aligned(qweight), scales.contiguous()  # held until the launch is queued
        _hip.check(self.entry("linear_forward")(_hip.ptr(x), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y), M, N, K,
                                                _hip.dt(x), int(form), _hip.stream()), f"bie_{self.stem}_linear_forward")
        return y

    def grad_input(self, gy, qweight, scales, e_blk):
        _hip.need_gpu(gy, qweight, scales, e_blk)
        if gy.dtype not in _X_DT:
            raise RuntimeError(f"{self.prefix} grad_input: dtype {gy.dtype} is not supported (fp16 / bf16)")
        N, K = self.shape(qweight, scales)
        if gy.dim() != 2 or gy.shape[1] != N:
            raise RuntimeError(f"{self.prefix} grad_input: gy {tuple(gy.shape)} does not match N={N}")
        M = gy.shape[0]
        gx = torch.empty((M, K), dtype=gy.dtype, device=gy.device)
        if M == 0:
            return gx
        if e_blk is None:
            e_blk = self.blk_exp(scales)
        elif e_blk.dtype != torch.uint8 or e_blk.numel() != K // 32:
            raise RuntimeError(f"{self.prefix} grad_input: e_blk must be uint8 [K/32 = {K // 32}]")
        gy, qweight, scales, e_blk = gy.contiguous(), _aligned(qweight), scales.contiguous(), e_blk.contiguous()  # held until the launch is queued
        _hip.check(self.entry("linear_grad_input")(_hip.ptr(gy), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_blk), _hip.ptr(gx), M, N, K,
                                                   _hip.dt(gy), _hip.stream()), f"bie_{self.stem}_linear_grad_input")
        return gx


class Experts:
    """stem: `bie_<stem>_moe_form / _moe_forward / _moe_grad_input`; prefix: the messages' (`mxfp4`); shape: (qweight, scales) -> (E, N, K);
    col_exp: scales -> e_col [E, N]; blk_exp: scales -> e_blk [E, K/32]; idx: the module's own check of idx -> (T, S), where its message
    differs from the one below.  The routing workspace is bie_mxfp4_moe_workspace_bytes' for both formats."""

    def __init__(self, stem, prefix, shape, col_exp, blk_exp, idx=None):
        self.stem, self.prefix, self.shape, self.col_exp, self.blk_exp = stem, prefix, shape, col_exp, blk_exp
        if idx is not None:
            self.idx = idx

    def entry(self, suffix):
        return getattr(_hip.lib(), f"bie_{self.stem}_moe_{suffix}")

    def idx(self, idx):
        if idx.dtype != torch.int32 or idx.dim() != 2:
            raise RuntimeError(f"{self.prefix} experts: idx must be int32 [T, S] (got {idx.dtype} {tuple(idx.shape)})")
        return idx.shape

    def forward(self, x, idx, qweight, scales, bias, e_col, form):
        _hip.need_gpu(x, idx, qweight, scales, bias, e_col)
        if x.dtype not in _X_DT:
            raise RuntimeError(f"{self.prefix} experts: dtype {x.dtype} is not supported (fp16 / bf16)")
        E, N, K = self.shape(qweight, scales)
        T, S = self.idx(idx)
        if tuple(x.shape) not in ((T, K), (T, S, K)):
            raise RuntimeError(f"{self.prefix} experts: x {tuple(x.shape)} does not match idx {tuple(idx.shape)} and K={K}")
        y = torch.empty((T, S, N), dtype=x.dtype, device=x.device)
        if T * S == 0:
            return y
        L = _hip.lib()
        if form < 0:
            form = int(self.entry("form")(T * S, E, N, K, _hip.dt(x)))
        ws = None
        if form == 1:
            if e_col is None:
                e_col = self.col_exp(scales)
            ws = torch.empty(int(L.bie_mxfp4_moe_workspace_bytes(T * S, E)), dtype=torch.uint8, device=x.device)
        if bias is not None:
            bias = bias.reshape(E, N).to(dtype=x.dtype).contiguous()
        x_per_pair = int(x.dim() == 3)
        x, idx, qweight, scales = _aligned(x), idx.contiguous(), _aligned(qweight), scales.contiguous()  # held until the launches are queued
        e_col = None if e_col is None else e_col.contiguous()
        _hip.check(self.entry("forward")(_hip.ptr(x), _hip.ptr(idx), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y),
                                         _hip.ptr(ws), T, S, E, N, K, x_per_pair, _hip.dt(x), int(form), _hip.stream()), f"bie_{self.stem}_moe_forward")
        return y

    def grad_input(self, gy, idx, qweight, scales, e_blk, out_dtype):
        _hip.need_gpu(gy, idx, qweight, scales, e_blk)
        if gy.dtype not in _X_DT:
            raise RuntimeError(f"{self.prefix} experts grad_input: dtype {gy.dtype} is not supported (fp16 / bf16)")
        if out_dtype is None:
            out_dtype = gy.dtype
        if out_dtype not in (gy.dtype, torch.float32):
            raise RuntimeError(f"{self.prefix} experts grad_input: out_dtype {out_dtype} must be gy's dtype or float32")
        E, N, K = self.shape(qweight, scales)
        T, S = self.idx(idx)
        P = T * S
        if tuple(gy.shape) not in ((T, S, N), (P, N)):
            raise RuntimeError(f"{self.prefix} experts grad_input: gy {tuple(gy.shape)} does not match idx {tuple(idx.shape)} and N={N}")
        gx = torch.empty((P, K), dtype=out_dtype, device=gy.device)
        if P == 0:
            return gx
        L = _hip.lib()
        if e_blk is None:
            e_blk = self.blk_exp(scales)
        elif e_blk.dtype != torch.uint8 or tuple(e_blk.shape) != (E, K // 32):
            raise RuntimeError(f"{self.prefix} experts grad_input: e_blk must be uint8 [E = {E}, K/32 = {K // 32}]")
        ws = torch.empty(int(L.bie_mxfp4_moe_workspace_bytes(P, E)), dtype=torch.uint8, device=gy.device)
        gy, idx, qweight, scales, e_blk = gy.contiguous(), idx.contiguous(), _aligned(qweight), scales.contiguous(), e_blk.contiguous()
        _hip.check(self.entry("grad_input")(_hip.ptr(gy), _hip.ptr(idx), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_blk), _hip.ptr(gx), _hip.ptr(ws),
                                            T, S, E, N, K, _hip.dt(gy), int(out_dtype == torch.float32), _hip.stream()), f"bie_{self.stem}_moe_grad_input")
        return gx
