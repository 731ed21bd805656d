"""MXFP8A16MoECuda: MXFP4MoECuda's mixture-of-experts MLP block (router, top-k softmax, gate_up, clamped SwiGLU, down, combine; see
mxfp4_moe_layer.py) on MXFP8 expert weights with fp16 / bf16 activations ("MXFP8 W8A16 mixture-of-experts layer"):
gate_up and down are MXFP8ExpertsLinearCuda (csrc/mxfp8_moe.hip; exact products, an fp32 sum, one rounding).  Everything else is the
same ops, inherited: the routing stays on the device, so the block can be captured in a graph."""
import torch

from .mxfp4_moe_layer import MXFP4MoECuda, combine, swiglu  # noqa: F401
from .mxfp8_experts_layer import MXFP8ExpertsLinearCuda


class MXFP8A16MoECuda(MXFP4MoECuda):
    """router (nn.Linear hidden -> E), gate_up (E experts, hidden -> 2 * intermediate) and down (E experts, intermediate -> hidden), both
    MXFP8ExpertsLinearCuda.  set_expert_mask, route and forward are MXFP4MoECuda's."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, bias: bool = True, swiglu_limit: float = 7.0,
                 swiglu_alpha: float = 1.702, device: torch.device = None, dtype: torch.dtype = torch.bfloat16) -> None:
        if not 1 <= top_k <= min(num_experts, 32):
            raise ValueError(f"mxfp8 moe needs 1 <= top_k <= min(num_experts, 32) (got top_k={top_k}, num_experts={num_experts})")
        super().__init__(hidden, intermediate, num_experts, top_k, bias=bias, swiglu_limit=swiglu_limit, swiglu_alpha=swiglu_alpha, device=device,
                         dtype=dtype, activations="dtype")

    def _experts_class(self, activations: str):
        return MXFP8ExpertsLinearCuda

    def load_mx_experts(self, gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias) -> None:
        """The experts' MXFP8 tensors: *_qweight uint8 [E, N, K] or [E, N, K/32, 32], *_scales uint8 [E, N, K/32], *_bias [E, N] (None for
        a block without bias)."""
        self._load_experts("load_mx_experts", gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias)

    def load_gpt_oss_experts(self, *args, **kwargs) -> None:
        raise TypeError("MXFP8A16MoECuda holds MXFP8 (E4M3) expert weights; a gpt-oss checkpoint's expert tensors are MXFP4 and are not "
                        "reinterpreted: use MXFP4MoECuda, or load_mx_experts with MXFP8 tensors")
