from .mpq_layer import MPQLinearCuda, MPQLinearCudaFunction
from .mbwq_layer import MBWQLinearCuda, MBWQLinearCudaFunction
from .utils import unpack_qweight, pack_fp_weight, make_group_map
from .mpq_list import MPQForwardList, MBWQExl2ForwardList
from .mxfp4_layer import MXFP4LinearCuda, MXFP4LinearForward
from .mxfp4_a4_layer import MXFP4A4LinearCuda, MXFP4A4LinearForward
from .mxfp4_a8_layer import MXFP4A8LinearCuda, MXFP4A8LinearForward
from .mxfp4_experts_layer import MXFP4ExpertsLinearCuda, MXFP4ExpertsLinearForward
from .mxfp4_experts_a4_layer import MXFP4A4ExpertsLinearCuda, MXFP4A4ExpertsLinearForward
from .mxfp4_experts_a8_layer import MXFP4A8ExpertsLinearCuda, MXFP4A8ExpertsLinearForward
from .mxfp4_moe_layer import MXFP4MoECuda
from .mxfp6_a8_layer import MXFP6A8LinearCuda, MXFP6A8LinearForward
from .mxfp6_experts_a8_layer import MXFP6A8ExpertsLinearCuda, MXFP6A8ExpertsLinearForward
from .mxfp6_experts_layer import MXFP6ExpertsLinearCuda, MXFP6ExpertsLinearForward
from .mxfp6_moe_layer import MXFP6MoECuda, MXFP6A16MoECuda
from .mxfp6_layer import MXFP6LinearCuda, MXFP6LinearForward
from .mxfp6_a6_layer import MXFP6A6LinearCuda, MXFP6A6LinearForward
