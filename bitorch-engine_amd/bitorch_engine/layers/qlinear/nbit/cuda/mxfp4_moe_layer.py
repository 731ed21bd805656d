"""MXFP4MoECuda: the mixture-of-experts MLP block of gpt-oss-style models on MXFP4 expert weights ("MXFP4
mixture-of-experts layer").  For x [T, hidden] (leading dimensions are flattened), E experts, top-k slots per token:

  logits = router(x)                                     nn.Linear in the dtype
  v, idx = topk(logits, k);  w = softmax(v)              over the k kept logits, in the dtype: w [T, k]
  h = gate_up(x, idx)                                    [T, k, 2 * intermediate], gate and up interleaved: g = h[..., 0::2], u = h[..., 1::2]
  a = dt( (clamp(u, -limit, limit) + 1) * g' * sigmoid(alpha * g') ),  g' = clamp(g, max=limit)        in fp32, rounded once
  o = down(a, idx)                                       [T, k, hidden]
  y = dt( sum_s w[t, s] * o[t, s] )                      in fp32, rounded once

The two expert projections run on the kernels of csrc/mxfp4_moe.hip; the routing stays on the device, so the block can be captured in
a graph.  The activation and the combine are torch ops (fusing them into the kernels is a follow-up).

activations="mxfp4" ("MXFP4 W4A4 mixture-of-experts layer"): gate_up and down are MXFP4A4ExpertsLinearCuda, which
quantise x and a to MXFP4 per row and block of 32 and contract on the block-scaled matrix instructions (csrc/mxfp4_moe_a4.hip); the
router, the top-k softmax, the SwiGLU and the combine are the same ops.
activations="mxfp8" ("MXFP4 W4A8 mixture-of-experts layer"): gate_up and down are MXFP4A8ExpertsLinearCuda, which
quantise x and a to MXFP8 (E4M3 elements, E8M0 block scales) per row and block of 32 and contract on the same instructions with an FP4
and an E4M3 operand (csrc/mxfp4_moe_a8.hip); everything else is the same ops.  The default "dtype" is the block above, untouched.
MXFP4A6MoECuda ("MXFP4 W4A6 mixture-of-experts layer") is the same block with MXFP6 (E2M3) activations; it is a class
of its own, not a value of `activations`."""
import torch
from torch import nn

from .mxfp4_experts_layer import MXFP4ExpertsLinearCuda
from .mxfp4_experts_a4_layer import MXFP4A4ExpertsLinearCuda
from .mxfp4_experts_a8_layer import MXFP4A8ExpertsLinearCuda
from .mxfp4_experts_a6_layer import MXFP4A6ExpertsLinearCuda


def swiglu(h: torch.Tensor, limit: float, alpha: float) -> torch.Tensor:
    """The clamped SwiGLU of gpt-oss on interleaved gate / up columns: computed in fp32, rounded once to h's dtype."""
    g, u = h[..., 0::2].float(), h[..., 1::2].float()
    g = g.clamp(max=limit)
    u = u.clamp(min=-limit, max=limit)
    return ((u + 1.0) * (g * torch.sigmoid(alpha * g))).to(h.dtype)


def combine(w: torch.Tensor, o: torch.Tensor) -> torch.Tensor:
    """y[t] = dt( sum_s w[t, s] * o[t, s] ), slot by slot in fp32."""
    return (w.float()[..., None] * o.float()).sum(dim=1).to(o.dtype)


_EXPERTS = {"dtype": MXFP4ExpertsLinearCuda, "mxfp4": MXFP4A4ExpertsLinearCuda, "mxfp8": MXFP4A8ExpertsLinearCuda}


class MXFP4MoECuda(nn.Module):
    """router (nn.Linear hidden -> E), gate_up (E experts, hidden -> 2 * intermediate) and down (E experts, intermediate -> hidden).
    expert_mask (bool [E], optional): the experts this instance owns; the slots of the others are skipped (their o rows are zero), which
    is what one shard of an expert-parallel group computes before the shards' outputs are summed."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, bias: bool = True, swiglu_limit: float = 7.0,
                 swiglu_alpha: float = 1.702, device: torch.device = None, dtype: torch.dtype = torch.bfloat16, activations: str = "dtype") -> None:
        super().__init__()
        if not isinstance(activations, str) or activations not in _EXPERTS:
            raise ValueError(f"mxfp4 moe: activations must be 'dtype', 'mxfp4' or 'mxfp8' (got {activations!r})")
        if not 1 <= top_k <= min(num_experts, 32):
            raise ValueError(f"mxfp4 moe needs 1 <= top_k <= min(num_experts, 32) (got top_k={top_k}, num_experts={num_experts})")
        self.hidden, self.intermediate, self.num_experts, self.top_k = hidden, intermediate, num_experts, top_k
        self.swiglu_limit, self.swiglu_alpha, self.dtype = float(swiglu_limit), float(swiglu_alpha), dtype
        self.router = nn.Linear(hidden, num_experts, bias=bias, device=device, dtype=dtype)
        self.activations = activations
        experts = self._experts_class(activations)
        self.gate_up = experts(num_experts, hidden, 2 * intermediate, bias=bias, device=device, dtype=dtype)
        self.down = experts(num_experts, intermediate, hidden, bias=bias, device=device, dtype=dtype)
        self.register_buffer("expert_mask", None, persistent=False)

    def _experts_class(self, activations: str):
        """The class of gate_up and down (a subclass with another weight format returns its own)."""
        return _EXPERTS[activations]

    def set_expert_mask(self, mask: torch.Tensor = None) -> None:
        """bool [E]: True for the experts this instance computes (None: all of them)."""
        if mask is not None:
            if mask.dtype != torch.bool or tuple(mask.shape) != (self.num_experts,):
                raise ValueError(f"expert_mask must be bool [{self.num_experts}]")
            mask = mask.to(self.router.weight.device)
        self.expert_mask = mask

    def load_gpt_oss_experts(self, gate_up_blocks, gate_up_scales, gate_up_bias, down_blocks, down_scales, down_bias) -> None:
        """The checkpoint's expert tensors as they are: *_blocks uint8 [E, N, K/32, 16], *_scales uint8 [E, N, K/32], *_bias [E, N]
        (None for a block without bias)."""
        self._load_experts("load_gpt_oss_experts", gate_up_blocks, gate_up_scales, gate_up_bias, down_blocks, down_scales, down_bias)

    def _load_experts(self, what, gate_up_blocks, gate_up_scales, gate_up_bias, down_blocks, down_scales, down_bias) -> None:
        self.gate_up.set_mx_weight(gate_up_blocks, gate_up_scales)
        self.down.set_mx_weight(down_blocks, down_scales)
        with torch.no_grad():
            for layer, b in ((self.gate_up, gate_up_bias), (self.down, down_bias)):
                if (b is None) != (layer.bias is None):
                    raise ValueError(f"{what}: a bias is given for a block built without one (or the reverse)")
                if b is not None:
                    layer.bias.copy_(b.reshape(layer.bias.shape))

    def route(self, x: torch.Tensor):
        """x [T, hidden] -> (w [T, k] in the dtype, idx int32 [T, k]; -1 for the slots of experts outside expert_mask)."""
        v, idx = torch.topk(self.router(x), self.top_k, dim=-1)
        w = torch.softmax(v, dim=-1)
        if self.expert_mask is not None:
            idx = torch.where(self.expert_mask[idx], idx, torch.full_like(idx, -1))
        return w, idx.to(torch.int32)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.size(-1) == self.hidden, f"Weight and input tensor mismatch: {x.size(-1)} != {self.hidden}"
        lead = x.shape[:-1]
        x2 = x.reshape(-1, self.hidden)
        w, idx = self.route(x2)
        h = self.gate_up(x2, idx)
        a = swiglu(h, self.swiglu_limit, self.swiglu_alpha)
        o = self.down(a, idx)
        return combine(w, o).reshape(*lead, self.hidden)


class MXFP4A6MoECuda(MXFP4MoECuda):
    """The same block on MXFP4 expert weights with MXFP6 activations ("MXFP4 W4A6 mixture-of-experts layer"): gate_up and
    down are MXFP4A6ExpertsLinearCuda, which quantise x and a to E2M3 elements with E8M0 block scales per row and block of 32 and contract
    them with the E2M1 weight codes on the block-scaled matrix instructions with an FP4 and an FP6 operand (csrc/mxfp4_moe_a6.hip).
    Within a block a value below 1/64 of the block's power-of-two maximum becomes zero; that matters most for the SwiGLU output a that
    feeds down.  The parameters and buffers are MXFP4MoECuda's, so the blocks load each other's state_dict, and load_gpt_oss_experts is
    inherited: the checkpoint's expert tensors are taken as they are."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, bias: bool = True, swiglu_limit: float = 7.0,
                 swiglu_alpha: float = 1.702, device: torch.device = None, dtype: torch.dtype = torch.bfloat16) -> None:
        super().__init__(hidden, intermediate, num_experts, top_k, bias=bias, swiglu_limit=swiglu_limit, swiglu_alpha=swiglu_alpha, device=device,
                         dtype=dtype, activations="dtype")
        self.activations = "mxfp6"

    def _experts_class(self, activations: str):
        return MXFP4A6ExpertsLinearCuda
