"""import_extension(name): same entry point as the reference's utils/safe_import.py:75-112.  The
extension objects are thin ctypes front-ends; a missing/unbuilt libbie_hip.so raises on first USE
(like the reference's ExtensionModulePlaceholder), never silently falls back."""
import importlib

KNOWN = ("q_linear_cuda", "binary_linear_cpp", "binary_linear_cuda", "binary_linear_cutlass",
         "binary_conv_cpp", "binary_conv2d_cutlass", "functions_cuda", "q_linear_cutlass", "q4_conv_cutlass",
         "ternary_linear_cuda", "ternary_conv2d_cuda", "ternary_a8_linear_cuda", "mxfp4_linear_cuda", "mxfp4_a4_linear_cuda",
         "mxfp4_experts_cuda", "mxfp4_experts_a4_cuda", "mxfp4_a8_linear_cuda", "mxfp4_experts_a8_cuda",
         "mxfp6_a8_linear_cuda", "mxfp6_experts_a8_cuda", "mxfp6_linear_cuda", "mxfp6_experts_cuda",
         "mxfp6_a6_linear_cuda", "mxfp6_experts_a6_cuda", "mxfp4_a6_linear_cuda", "mxfp4_experts_a6_cuda",
         "mxfp8_a8_linear_cuda")


class ExtensionModulePlaceholder:
    def __init__(self, name, reason):
        self._name, self._reason = name, reason

    def __getattr__(self, item):
        raise RuntimeError(f"The extension '{self._name}' is not available in the MI355X build: {self._reason}")


def import_extension(module_name: str, not_yet_implemented: bool = False):
    if module_name not in KNOWN:
        return ExtensionModulePlaceholder(module_name, "no HIP implementation (out of scope of this build)")
    return importlib.import_module(f"bitorch_engine.extensions.{module_name}")
