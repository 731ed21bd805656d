"""MXFP6MoECuda: MXFP4MoECuda's mixture-of-experts MLP block (router, top-k softmax, gate_up, clamped SwiGLU, down, combine; see
mxfp4_moe_layer.py) on MXFP6 expert weights with MXFP8 activations ("MXFP6 W6A8 mixture-of-experts layer"): gate_up and
down are MXFP6A8ExpertsLinearCuda, which quantise x and a to MXFP8 (E4M3 elements, E8M0 block scales) per row and block of 32 and
contract them with E2M3 weight codes on the block-scaled matrix instructions (csrc/mxfp6_moe_a8.hip).  Everything else is the same ops,
inherited: the routing stays on the device, so the block can be captured in a graph."""
import torch

from .mxfp4_moe_layer import MXFP4MoECuda, combine, swiglu  # noqa: F401
from .mxfp6_experts_a6_layer import MXFP6A6ExpertsLinearCuda
from .mxfp6_experts_a8_layer import MXFP6A8ExpertsLinearCuda
from .mxfp6_experts_layer import MXFP6ExpertsLinearCuda


class MXFP6MoECuda(MXFP4MoECuda):
    """router (nn.Linear hidden -> E), gate_up (E experts, hidden -> 2 * intermediate) and down (E experts, intermediate -> hidden), both
    MXFP6A8ExpertsLinearCuda.  set_expert_mask, route and forward are MXFP4MoECuda's."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, bias: bool = True, swiglu_limit: float = 7.0,
                 swiglu_alpha: float = 1.702, device: torch.device = None, dtype: torch.dtype = torch.bfloat16) -> None:
        if not 1 <= top_k <= min(num_experts, 32):
            raise ValueError(f"mxfp6 moe needs 1 <= top_k <= min(num_experts, 32) (got top_k={top_k}, num_experts={num_experts})")
        super().__init__(hidden, intermediate, num_experts, top_k, bias=bias, swiglu_limit=swiglu_limit, swiglu_alpha=swiglu_alpha, device=device,
                         dtype=dtype, activations="mxfp8")

    def _experts_class(self, activations: str):
        return MXFP6A8ExpertsLinearCuda

    def load_mx_experts(self, gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias) -> None:
        """The experts' MXFP6 tensors: *_qweight uint8 [E, N, 3K/4] or [E, N, K/32, 24], *_scales uint8 [E, N, K/32], *_bias [E, N] (None
        for a block without bias)."""
        self._load_experts("load_mx_experts", gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias)

    def load_gpt_oss_experts(self, *args, **kwargs) -> None:
        raise TypeError("MXFP6MoECuda holds MXFP6 (E2M3) expert weights; a gpt-oss checkpoint's expert tensors are MXFP4 and are not "
                        "reinterpreted: use MXFP4MoECuda, or load_mx_experts with MXFP6 tensors")


class MXFP6A16MoECuda(MXFP4MoECuda):
    """The same block on MXFP6 expert weights with fp16 / bf16 activations ("MXFP6 W6A16 mixture-of-experts layer"):
    gate_up and down are MXFP6ExpertsLinearCuda (csrc/mxfp6_moe.hip; exact products, an fp32 sum, one rounding).  The parameters and
    buffers are MXFP6MoECuda's, so the two blocks load each other's state_dict."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, bias: bool = True, swiglu_limit: float = 7.0,
                 swiglu_alpha: float = 1.702, device: torch.device = None, dtype: torch.dtype = torch.bfloat16) -> None:
        if not 1 <= top_k <= min(num_experts, 32):
            raise ValueError(f"mxfp6 moe needs 1 <= top_k <= min(num_experts, 32) (got top_k={top_k}, num_experts={num_experts})")
        super().__init__(hidden, intermediate, num_experts, top_k, bias=bias, swiglu_limit=swiglu_limit, swiglu_alpha=swiglu_alpha, device=device,
                         dtype=dtype, activations="dtype")

    def _experts_class(self, activations: str):
        return MXFP6ExpertsLinearCuda

    def load_mx_experts(self, gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias) -> None:
        """The experts' MXFP6 tensors: *_qweight uint8 [E, N, 3K/4] or [E, N, K/32, 24], *_scales uint8 [E, N, K/32], *_bias [E, N] (None
        for a block without bias)."""
        self._load_experts("load_mx_experts", gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias)

    def load_gpt_oss_experts(self, *args, **kwargs) -> None:
        raise TypeError("MXFP6A16MoECuda holds MXFP6 (E2M3) expert weights; a gpt-oss checkpoint's expert tensors are MXFP4 and are not "
                        "reinterpreted: use MXFP4MoECuda, or load_mx_experts with MXFP6 tensors")


class MXFP6A6MoECuda(MXFP4MoECuda):
    """The same block on MXFP6 expert weights with MXFP6 activations ("MXFP6 W6A6 mixture-of-experts layer"): gate_up and
    down are MXFP6A6ExpertsLinearCuda, which quantise x and a to E2M3 elements with E8M0 block scales per row and block of 32 and contract
    them with the E2M3 weight codes on the block-scaled matrix instructions with two FP6 operands (csrc/mxfp6_moe_a6.hip).  Within a
    block a value below 1/64 of the block's power-of-two maximum becomes zero; that matters most for the SwiGLU output a that feeds down.
    The parameters and buffers are MXFP6MoECuda's, so the two blocks load each other's state_dict."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, bias: bool = True, swiglu_limit: float = 7.0,
                 swiglu_alpha: float = 1.702, device: torch.device = None, dtype: torch.dtype = torch.bfloat16) -> None:
        if not 1 <= top_k <= min(num_experts, 32):
            raise ValueError(f"mxfp6 moe needs 1 <= top_k <= min(num_experts, 32) (got top_k={top_k}, num_experts={num_experts})")
        super().__init__(hidden, intermediate, num_experts, top_k, bias=bias, swiglu_limit=swiglu_limit, swiglu_alpha=swiglu_alpha, device=device,
                         dtype=dtype, activations="dtype")
        self.activations = "mxfp6"

    def _experts_class(self, activations: str):
        return MXFP6A6ExpertsLinearCuda

    def load_mx_experts(self, gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias) -> None:
        """The experts' MXFP6 tensors: *_qweight uint8 [E, N, 3K/4] or [E, N, K/32, 24], *_scales uint8 [E, N, K/32], *_bias [E, N] (None
        for a block without bias)."""
        self._load_experts("load_mx_experts", gate_up_qweight, gate_up_scales, gate_up_bias, down_qweight, down_scales, down_bias)

    def load_gpt_oss_experts(self, *args, **kwargs) -> None:
        raise TypeError("MXFP6A6MoECuda holds MXFP6 (E2M3) expert weights; a gpt-oss checkpoint's expert tensors are MXFP4 and are not "
                        "reinterpreted: use MXFP4MoECuda, or load_mx_experts with MXFP6 tensors")
