"""The form / forward / gemm wrappers of the block-scaled MX layers, written once: six dense layers (W4A4, W4A6, W4A8, W6A6, W6A8, W8A8)
and five experts layers (W4A4, W4A6, W4A8, W6A6, W6A8) call the same two sequences of checks, allocations and one C entry, and differ in
the `bie_` symbol stem, the prefix of their messages, the bytes of a block of quantised activations and the function that reads (N, K)
or (E, N, K) off the weights.  A module states those in a Dense or an Experts object and keeps its own `form`, `forward` and `gemm`
definitions (names, argument names, defaults and docstrings are the module's) as one call each.  Nothing here synchronises with the host."""
import torch

from bitorch_engine import _hip
from bitorch_engine.extensions.mxfp4_linear_cuda import _X_DT, _aligned

_ROW_TEXT = {16: "K/2", 24: "3K/4", 32: "K"}


def _bias(bias, dtype):
    return None if bias is None else bias.reshape(-1).to(dtype=dtype).contiguous()


class Dense:
    """stem: `bie_<stem>_form / _workspace_bytes / _linear_forward / _gemm`; prefix: the messages' (`mxfp4 a6`); block_bytes: 16 (MXFP4),
    24 (MXFP6) or 32 (MXFP8) bytes of activation codes per block of 32; shape: (qweight, scales) -> (N, K); col_exp: scales -> e_col.
    act_shape: the MXFP4 and MXFP8 activation modules check (xq, xs) with a shape function of their own, which names a wrong dtype itself;
    the MXFP6 ones (None) spell the three shapes out.  empty_gemm: False where gemm hands M = 0 to the C entry, which refuses it."""

    def __init__(self, stem, prefix, block_bytes, shape, col_exp, act_shape=None, empty_gemm=True):
        self.stem, self.prefix, self.block_bytes, self.shape, self.col_exp = stem, prefix, block_bytes, shape, col_exp
        self.act_shape, self.empty_gemm = act_shape, empty_gemm
        self.xq = "xq6" if block_bytes == 24 else "xq"

    def entry(self, suffix):
        return getattr(_hip.lib(), f"bie_{self.stem}_{suffix}")

    def form(self, M, N, K, dtype):
        return int(self.entry("form")(M, N, K, _hip._DT[dtype]))

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
        if e_col is None:
            e_col = self.col_exp(scales)
        ws = torch.empty(int(self.entry("workspace_bytes")(M, N, K, int(form))), dtype=torch.uint8, device=x.device)
        bias = _bias(bias, x.dtype)
        x, qweight, scales = _aligned(x), _aligned(qweight), scales.contiguous()  # held until the launches are queued
        name = f"bie_{self.stem}_linear_forward"
        _hip.check(self.entry("linear_forward")(_hip.ptr(x), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y), _hip.ptr(ws),
                                                M, N, K, _hip.dt(x), int(form), _hip.stream()), name)
        return y

    def gemm(self, xq, xs, row_flag, qweight, scales, bias, e_col, dtype, form):
        _hip.need_gpu(xq, xs, row_flag, qweight, scales, bias, e_col)
        if dtype not in _X_DT:
            raise RuntimeError(f"{self.prefix} gemm: dtype {dtype} is not supported (fp16 / bf16)")
        N, K = self.shape(qweight, scales)
        M = xq.shape[0]
        shapes = f"{self.xq} {tuple(xq.shape)} / xs {tuple(xs.shape)} / row_flag {tuple(row_flag.shape)}"
        if self.act_shape is not None:
            if self.act_shape(xq, xs) != (M, K) or row_flag.dtype != torch.uint8 or tuple(row_flag.shape) != (M,):
                raise RuntimeError(f"{self.prefix} gemm: {shapes} do not match K={K}")
        elif xq.dtype != torch.uint8 or xs.dtype != torch.uint8 or tuple(xq.shape) != (M, K // 32 * self.block_bytes) or tuple(xs.shape) != (M, K // 32) \
                or row_flag.dtype != torch.uint8 or tuple(row_flag.shape) != (M,):
            raise RuntimeError(f"{self.prefix} gemm: {shapes} are not uint8 [M, {_ROW_TEXT[self.block_bytes]}] / [M, K/32] / [M] for K={K}")
        y = torch.empty((M, N), dtype=dtype, device=xq.device)
        if M == 0 and self.empty_gemm:
            return y
        if e_col is None:
            e_col = self.col_exp(scales)
        bias = _bias(bias, dtype)
        xq, xs, row_flag, qweight, scales = _aligned(xq), xs.contiguous(), row_flag.contiguous(), _aligned(qweight), scales.contiguous()
        _hip.check(self.entry("gemm")(_hip.ptr(xq), _hip.ptr(xs), _hip.ptr(row_flag), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col),
                                      _hip.ptr(bias), _hip.ptr(y), None, M, N, K, _hip._DT[dtype], int(form), _hip.stream()), f"bie_{self.stem}_gemm")
        return y


def _experts_bias(bias, E, N, dtype):
    return None if bias is None else bias.reshape(E, N).to(dtype=dtype).contiguous()


class Experts:
    """stem: `bie_<stem>_form / _workspace_bytes / _forward / _gemm`; prefix: the messages' (`mxfp4 a6`); block_bytes as for Dense;
    shape: (qweight, scales) -> (E, N, K); col_exp: scales -> e_col."""

    def __init__(self, stem, prefix, block_bytes, shape, col_exp):
        self.stem, self.prefix, self.block_bytes, self.shape, self.col_exp = stem, prefix, block_bytes, shape, col_exp
        self.xq = "xq6" if block_bytes == 24 else "xq"

    def entry(self, suffix):
        return getattr(_hip.lib(), f"bie_{self.stem}_{suffix}")

    def form(self, P, E, N, K, dtype):
        return int(self.entry("form")(P, E, N, K, _hip._DT[dtype]))

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
        if form < 0:
            form = int(self.entry("form")(T * S, E, N, K, _hip.dt(x)))
        if e_col is None:
            e_col = self.col_exp(scales)
        x_per_pair = int(x.dim() == 3)
        ws = torch.empty(int(self.entry("workspace_bytes")(T, S, E, K, x_per_pair, int(form))), dtype=torch.uint8, device=x.device)
        bias = _experts_bias(bias, E, N, x.dtype)
        x, idx, qweight, scales, e_col = _aligned(x), idx.contiguous(), _aligned(qweight), scales.contiguous(), e_col.contiguous()  # held until queued
        _hip.check(self.entry("forward")(_hip.ptr(x), _hip.ptr(idx), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col), _hip.ptr(bias), _hip.ptr(y),
                                         _hip.ptr(ws), T, S, E, N, K, x_per_pair, _hip.dt(x), int(form), _hip.stream()), f"bie_{self.stem}_forward")
        return y

    def gemm(self, xq, xs, row_flag, idx, qweight, scales, bias, e_col, dtype, form):
        _hip.need_gpu(xq, xs, row_flag, idx, qweight, scales, bias, e_col)
        if dtype not in _X_DT:
            raise RuntimeError(f"{self.prefix} experts gemm: dtype {dtype} is not supported (fp16 / bf16)")
        E, N, K = self.shape(qweight, scales)
        T, S = self.idx(idx)
        R = xq.shape[0]
        if (xq.dtype != torch.uint8 or xs.dtype != torch.uint8 or row_flag.dtype != torch.uint8 or tuple(xq.shape) != (R, K // 32 * self.block_bytes)
                or tuple(xs.shape) != (R, K // 32) or tuple(row_flag.shape) != (R,) or R not in (T, T * S)):
            rows = "uint8 [R, 3K/4] / [R, K/32] / [R], T or T * S rows" if self.block_bytes == 24 else "uint8, T or T * S rows"
            raise RuntimeError(f"{self.prefix} experts gemm: {self.xq} {tuple(xq.shape)} / xs {tuple(xs.shape)} / row_flag {tuple(row_flag.shape)} do not match "
                               f"idx {tuple(idx.shape)} and K={K} ({rows})")
        y = torch.empty((T, S, N), dtype=dtype, device=xq.device)
        if T * S == 0:
            return y
        x_per_pair = int(R != T)  # S = 1: the two readings are the same rows
        L = _hip.lib()
        if form < 0:
            form = int(self.entry("form")(T * S, E, N, K, _hip._DT[dtype]))
        if e_col is None:
            e_col = self.col_exp(scales)
        ws = torch.empty(int(L.bie_mxfp4_moe_workspace_bytes(T * S, E)), dtype=torch.uint8, device=xq.device) if form == 1 else None
        bias = _experts_bias(bias, E, N, dtype)
        xq, xs, row_flag, idx = _aligned(xq), xs.contiguous(), row_flag.contiguous(), idx.contiguous()
        qweight, scales, e_col = _aligned(qweight), scales.contiguous(), e_col.contiguous()
        _hip.check(self.entry("gemm")(_hip.ptr(xq), _hip.ptr(xs), _hip.ptr(row_flag), _hip.ptr(idx), _hip.ptr(qweight), _hip.ptr(scales), _hip.ptr(e_col),
                                      _hip.ptr(bias), _hip.ptr(y), _hip.ptr(ws), T, S, E, N, K, x_per_pair, _hip._DT[dtype], int(form), _hip.stream()),
                   f"bie_{self.stem}_gemm")
        return y
