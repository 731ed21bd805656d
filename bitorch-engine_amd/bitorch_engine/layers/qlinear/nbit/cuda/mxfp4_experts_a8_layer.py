"""MXFP4A8ExpertsLinearCuda: the stacked expert projection of MXFP4ExpertsLinearCuda against activations quantised to MXFP8 (E4M3 elements,
E8M0 block scales) on the fly, on the kernels of csrc/mxfp4_moe_a8.hip (the block-scaled matrix instructions of gfx950 with an FP4 and
an E4M3 operand).

  x^[r, k] = e4m3(code) * 2^(sx[r, k // 32] - 127)   (the OCP MX v1.0 rule with emax = 8 per stored row of x and block of 32)
  y[t, s]  = dt( x^_row . W[idx[t, s]]^T + bias[idx[t, s]] ),  NaN for a row of x that holds NaN or +-inf, +0 for a skipped slot

Parameters, buffers, state-dict keys and set_mx_weight are MXFP4ExpertsLinearCuda's: a state dict of either class loads into the other.

Training (train() with the latent weight): re-quantised on every call, the forward runs on the kernels and the backward is the
straight-through composition in torch, expert by expert, with the QUANTISED activations in the weight gradient and the identity through
the activation quantiser in grad_x.  Eval: the packed weight; a forward with grad enabled is differentiable in x (and bias)."""
import typing

import torch
from torch.autograd import Function

from bitorch_engine.utils.safe_import import import_extension
from .mxfp4_experts_layer import MXFP4ExpertsLinearCuda

mxfp4_experts_a8_cuda = import_extension("mxfp4_experts_a8_cuda")


def experts_a8_backward(ext, K, ctx, gy, kernel=False):
    """The straight-through backward of an expert layer with MXFP8 activations; ext supplies dequant (the weight format's) and
    quantize_act / dequant_act, K is the layer's input width.  Shared by the MXFP4 and the MXFP6 expert layers.  With kernel=True
    grad_x is one call of ext.grad_input on the packed weights (e_blk from the scales of this call; fp32 rows summed over a token's
    slots and rounded once when x is [T, K]) and the expert loop runs for grad_weight / grad_bias only: with neither, nothing
    synchronises with the host."""
    x, idx, qweight, scales = ctx.saved_tensors
    E, N = qweight.shape[0], qweight.shape[1]
    T, S = idx.shape
    need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
    gxk = None
    if need_x and kernel:
        if x.dim() == 3:
            gxk = ext.grad_input(gy, idx, qweight, scales).reshape(T, S, K)
        else:
            gxk = ext.grad_input(gy, idx, qweight, scales, out_dtype=torch.float32).reshape(T, S, K).sum(1).to(gy.dtype)
        need_x = False
        if not (need_w or need_b):
            return gxk, None, None, None, None, None, None
    g = gy.reshape(T * S, N).float()
    flat = idx.reshape(-1).long()
    gx = torch.zeros((T * S, K), dtype=torch.float32, device=gy.device) if need_x else None
    gw = torch.zeros((E, N, K), dtype=torch.float32, device=gy.device) if need_w else None
    gb = torch.zeros((E, N), dtype=torch.float32, device=gy.device) if need_b else None
    W = ext.dequant(qweight, scales, torch.float32) if need_x else None
    xr = None
    if need_w:  # x^ of the stored rows, then a row per pair
        xq, xs, _ = ext.quantize_act(x.reshape(-1, K))
        xh = ext.dequant_act(xq, xs, torch.float32)
        xr = (xh.reshape(T, S, K) if x.dim() == 3 else xh[:, None, :].expand(T, S, K)).reshape(T * S, K)
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
    return gx, None, None if gw is None else gw.to(gy.dtype), None if gb is None else gb.to(gy.dtype), None, None, None


class MXFP4A8ExpertsLinearForward(Function):
    """Forward: the W4A8 expert kernels.  Backward (straight-through estimator, in fp32, cast to the dtype), over the live pairs p of expert e:
      grad_x[row(p)] += gy[p] . W[e]        (identity through the activation quantiser; summed over a token's slots when x is [T, K])
      grad_weight[e]  = gy[pairs of e]^T . x^_rows      (the quantised activations)
      grad_bias[e]    = sum gy[pairs of e]
    Skipped slots contribute nothing.  A loop over the experts in torch: not a hot path."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, qweight, scales, e_col):
        ctx.save_for_backward(x, idx, qweight, scales)
        return mxfp4_experts_a8_cuda.forward(x, idx, qweight, scales, bias, e_col)

    @staticmethod
    @typing.no_type_check
    def backward(ctx, gy):
        return experts_a8_backward(mxfp4_experts_a8_cuda, ctx.saved_tensors[2].shape[2] * 2, ctx, gy)


class MXFP4A8ExpertsLinearCuda(MXFP4ExpertsLinearCuda):
    """MXFP4ExpertsLinearCuda's state (latent `weight` [E, N, K], `qweight` uint8 [E, N, K/2], `scales` uint8 [E, N, K/32], optional `bias`
    [E, N]) with the W4A8 forward.  K % 32 == 0, K <= 2^20; 1 <= E <= 1024; dtype fp16 or bf16."""

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
                qweight, scales = mxfp4_experts_a8_cuda.quantize(self.weight)
            e_col = None  # computed by the forward
        else:
            if not self._packed:
                self.prepare_params()
            qweight, scales, e_col = self.qweight, self.scales, self.e_col
        grad = torch.is_grad_enabled() and (x.requires_grad or (training and self.weight.requires_grad)
                                            or (self.bias is not None and self.bias.requires_grad))
        if not grad:
            return mxfp4_experts_a8_cuda.forward(x, idx, qweight, scales, self.bias, e_col)
        return MXFP4A8ExpertsLinearForward.apply(x, idx, self.weight if training else None, self.bias, qweight, scales, e_col)
