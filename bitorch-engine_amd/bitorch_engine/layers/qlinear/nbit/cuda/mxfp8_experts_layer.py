"""MXFP8ExpertsLinearCuda: the stacked expert projection of a mixture-of-experts MLP, MXFP8 weights (OCP microscaling FP8, e4m3fn
elements, E8M0 scale per block of 32 along K) x fp16 / bf16 activations (W8A16) on the kernels of csrc/mxfp8_moe.hip.

  y[t, s] = dt( x_row . W[idx[t, s]]^T + bias[idx[t, s]] ),   W[e, n, k] = e4m3(qweight[e, n, k]) * 2^(scales[e, n, k // 32] - 127)
  x_row = x[t] for x [T, K] (every slot of a token reads the token's row) or x[t, s] for x [T, S, K];  y[t, s] = +0 for a skipped slot
  (idx outside [0, E), -1 by convention)

Products are exact, the sum is in fp32 and there is one rounding: MXFP8LinearCuda's arithmetic per expert.  qweight uint8 [E, N, K] and
scales uint8 [E, N, K/32] are MXFP8LinearCuda's format per expert; e_col is derived from scales and not saved.  A stacked MXFP4 state
dict (qweight [E, N, K/2]) and an MXFP6 one ([E, N, 3K/4]) are refused: the codes are a different format, not a different packing.

The surface is MXFP6ExpertsLinearCuda's without the grad_input constructor argument.  Training (train() with the latent weight):
re-quantised on every call, the forward runs on the kernels and the backward is the straight-through composition in torch, expert by
expert, with grad_weight = gy^T . x at the UNQUANTISED x (the weight-only rule).  Eval: the packed weight; a forward with grad enabled
is differentiable in x (and bias).  The attribute grad_input (not a constructor argument, not saved) chooses where grad_x comes from:
"torch" (the default) builds an fp32 image of every expert's W and loops over the experts on the host; "kernel" takes it from the
packed weights in one grouped call (csrc/mxfp8_grad.hip, extensions/mxfp8_grad_cuda.py: nothing is dequantised, and with frozen weights
and no bias gradient the backward has no expert loop and no host synchronisation, so it can be captured in a graph)."""
import math
import typing

import torch
from torch import nn
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from bitorch_engine.layers.qlinear.ternary.layer import TernaryWeightState

from bitorch_engine.layers.qlinear.nbit.cuda.mxfp8_layer import _checked_grad_input

mxfp8_experts_cuda = import_extension("mxfp8_experts_cuda")
mxfp8_grad_cuda = import_extension("mxfp8_grad_cuda")


class MXFP8ExpertsLinearForward(Function):
    """Forward: the W8A16 expert kernels.  Backward: MXFP6ExpertsLinearForward's straight-through composition with the MXFP8 dequant, in
    fp32, cast to the dtype, over the live pairs p of expert e:
      grad_x[row(p)] += gy[p] . W[e]        (summed over a token's slots when x is [T, K])
      grad_weight[e]  = gy[pairs of e]^T . x_rows
      grad_bias[e]    = sum gy[pairs of e]
    Skipped slots contribute nothing.  With kernel=True grad_x is one call of mxfp8_grad_cuda.experts_grad_input on the packed weights
    (fp32 rows summed over a token's slots and rounded once when x is [T, K]), and the loop runs for grad_weight / grad_bias only."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, qweight, scales, e_col, kernel=False):
        ctx.save_for_backward(x, idx, qweight, scales)
        ctx.kernel = kernel
        return mxfp8_experts_cuda.forward(x, idx, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        x, idx, qweight, scales = ctx.saved_tensors
        E, N, K = scales.shape[0], scales.shape[1], scales.shape[2] * 32
        T, S = idx.shape
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gxk = None
        if need_x and ctx.kernel:
            if x.dim() == 3:
                gxk = mxfp8_grad_cuda.experts_grad_input(gy, idx, qweight, scales).reshape(T, S, K)
            else:
                gxk = mxfp8_grad_cuda.experts_grad_input(gy, idx, qweight, scales, out_dtype=torch.float32).reshape(T, S, K).sum(1).to(gy.dtype)
            need_x = False
            if not (need_w or need_b):
                return gxk, None, None, None, None, None, None, None
        g = gy.reshape(T * S, N).float()
        flat = idx.reshape(-1).long()
        xr = (x if x.dim() == 3 else x[:, None, :].expand(T, S, K)).reshape(T * S, K).float()
        gx = torch.zeros((T * S, K), dtype=torch.float32, device=gy.device) if need_x else None
        gw = torch.zeros((E, N, K), dtype=torch.float32, device=gy.device) if need_w else None
        gb = torch.zeros((E, N), dtype=torch.float32, device=gy.device) if need_b else None
        W = mxfp8_experts_cuda.dequant(qweight, scales, torch.float32) if need_x else None
        for e in range(E):
            rows = (flat == e).nonzero().reshape(-1)
            if rows.numel() == 0:
                continue
            ge = g[rows]
            if need_x:
                gx[rows] = ge.mm(W[e])
            if need_w:
                gw[e] = ge.t().mm(xr[rows])
            if need_b:
                gb[e] = ge.sum(0)
        if need_x:
            gx = (gx.reshape(T, S, K) if x.dim() == 3 else gx.reshape(T, S, K).sum(1)).to(gy.dtype)
        elif gxk is not None:
            gx = gxk
        return gx, None, None if gw is None else gw.to(gy.dtype), None if gb is None else gb.to(gy.dtype), None, None, None, None


class MXFP8ExpertsLinearCuda(TernaryWeightState, nn.Module):
    """Float latent `weight` [E, N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_mx_weight),
    the e4m3fn codes `qweight` uint8 [E, N, K] and E8M0 `scales` uint8 [E, N, K/32] (buffers), an optional `bias` [E, N].
    K % 32 == 0, K <= 2^20; 1 <= E <= 1024; dtype fp16 or bf16.  grad_input: "torch" or "kernel", an attribute of the object only (the
    module docstring)."""

    _grad_input = "torch"

    @property
    def grad_input(self) -> str:
        return self._grad_input

    @grad_input.setter
    def grad_input(self, value: str) -> None:
        self._grad_input = _checked_grad_input(value)

    def __init__(self, num_experts: int, input_features: int, out_features: int, bias: bool = False, device: torch.device = None,
                 dtype: torch.dtype = torch.float16) -> None:
        super().__init__()
        if input_features % 32 or input_features <= 0 or input_features > (1 << 20) or out_features <= 0 or not 1 <= num_experts <= 1024:
            raise ValueError(f"mxfp8 experts need input_features % 32 == 0, 32 <= input_features <= 2^20, out_features >= 1 and "
                             f"1 <= num_experts <= 1024 (got {input_features}, {out_features}, {num_experts})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mxfp8 experts compute in fp16 or bf16 (got {dtype})")
        self.num_experts, self.input_features, self.output_features = num_experts, input_features, out_features
        self.device, self.dtype = device, dtype
        E, N, K = num_experts, out_features, input_features
        w = torch.empty((E, N, K), dtype=dtype, device=device)
        for e in range(E):
            nn.init.kaiming_uniform_(w[e], a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros((E, N), dtype=dtype, device=device)) if bias else None
        self.register_buffer("qweight", torch.zeros((E, N, K), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros((E, N, K // 32), dtype=torch.uint8, device=device))
        self.register_buffer("e_col", torch.zeros((E, N), dtype=torch.uint8, device=device), persistent=False)
        self._packed = False  # qweight / scales / e_col hold the current weight (or a loaded / set MXFP8 weight)

    def _state_device(self) -> torch.device:
        return self.qweight.device

    def prepare_params(self) -> None:
        """qweight / scales from the latent weight (kept as they are for a layer that holds only the packed weight), then e_col."""
        with torch.no_grad():
            if self.weight is not None:
                self.qweight, self.scales = mxfp8_experts_cuda.quantize(self.weight)
            self.e_col = mxfp8_experts_cuda.col_exp(self.scales)
        self._packed = True

    def set_mx_weight(self, blocks: torch.Tensor, scales: torch.Tensor) -> None:
        """Load the experts' MXFP8 weight: blocks uint8 [E, N, K] or [E, N, K/32, 32] (e4m3fn bytes), scales uint8 [E, N, K/32].  The
        latent weight is dropped, so the layer computes with exactly these values in every mode.  A tensor that holds an E4M3 NaN code
        (0x7F / 0xFF) is refused: a NaN block is spelled with scale code 255."""
        E, N, K = self.num_experts, self.output_features, self.input_features
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError("set_mx_weight: blocks and scales must be uint8")
        if tuple(blocks.shape) == (E, N, K // 32, 32):
            blocks = blocks.reshape(E, N, K)
        if tuple(blocks.shape) != (E, N, K) or tuple(scales.shape) != (E, N, K // 32):
            raise ValueError(f"set_mx_weight: blocks {tuple(blocks.shape)} / scales {tuple(scales.shape)} do not match an MXFP8 weight "
                             f"[E={E}, N={N}, K={K}] (32 bytes per block of 32)")
        nan = (blocks & 0x7F) == 0x7F
        if bool(nan.any()):
            e, n, k = (int(v) for v in nan.nonzero()[0])
            raise ValueError(f"set_mx_weight: blocks[{e}, {n}, {k}] = 0x{int(blocks[e, n, k]):02X} is an E4M3 NaN code ({int(nan.sum())} in "
                             f"all); a NaN block of an MXFP8 weight is written as scale code 255")
        dev = self.qweight.device
        self.qweight = blocks.to(dev).contiguous()
        self.scales = scales.to(dev).contiguous()
        self.weight = None
        self.prepare_params()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        q = state_dict.get(prefix + "qweight")
        E, N, K = self.num_experts, self.output_features, self.input_features
        if q is not None and tuple(q.shape) in ((E, N, K // 2), (E, N, K // 32 * 24)):
            what = "an MXFP4 weight (4-bit E2M1 codes, K/2 bytes per row)" if q.shape[2] == K // 2 else \
                "an MXFP6 weight (6-bit E2M3 codes, 3K/4 bytes per row)"
            error_msgs.append(f"{prefix}qweight {tuple(q.shape)} is {what}; MXFP8ExpertsLinearCuda holds 8-bit E4M3 codes in [E, N, K] = "
                              f"{tuple(self.qweight.shape)} and does not reinterpret it: load the latent weight, or dequantise and re-quantise")
            return
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._packed = False  # e_col is re-derived (and, with a latent weight, qweight / scales) before the next packed forward

    def forward(self, x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """x [T, K] or [T, S, K], idx int32 [T, S] (other integer types are converted) -> [T, S, N]."""
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
        if idx.dtype != torch.int32:
            idx = idx.to(torch.int32)
        training = self.training and self.weight is not None
        if training:  # re-quantised every call: the weight may have changed since the last one
            self._packed = False
            with torch.no_grad():
                qweight, scales = mxfp8_experts_cuda.quantize(self.weight)
            e_col = None  # computed by the forward where the prefill form needs it
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return mxfp8_experts_cuda.forward(x, idx, qweight, scales, self.bias, e_col)
        return MXFP8ExpertsLinearForward.apply(x, idx, self.weight if training else None, self.bias, qweight, scales, e_col,
                                               self.grad_input == "kernel")
