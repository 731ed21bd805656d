"""The MXFP6 W6A8 mixture-of-experts layer restated in torch / float64 (INTEGRATION.md "MXFP6 W6A8 mixture-of-experts layer").  It only
composes what exists: the weight side is mxfp6_ref.py per expert (quantize, pack, dequant, tolerance: the W6A8 contract with the probe's
1853 ulps), the routed product and the block are mxfp4_moe_a8_ref.py's, which take W as float64 and do not know its format.  Shared by
test_mxfp6_moe_a8_cpu.py, test_mxfp6_moe_a8_gpu.py and sweeps/fuzz_mxfp6_moe_a8.py."""
import importlib.util
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


m6 = _load("mxfp6_ref")
a8m = _load("mxfp4_moe_a8_ref")
a8 = a8m.a8
mref = a8m.mref

quantize = m6.quantize
pack = m6.pack
tolerance = m6.tolerance
quantize_rows = a8m.quantize_rows
experts_from_codes = a8m.experts_from_codes
experts = a8m.experts
fake_quant = a8m.fake_quant
block = a8m.block


def dequant(qweight: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """qweight uint8 [E, N, 3K/4], scales uint8 [E, N, K/32] -> W float64 [E, N, K] (exact), NaN in a block of scale code 255."""
    return torch.stack([m6.dequant(qweight[e], scales[e]) for e in range(qweight.shape[0])])


def quantize_packed(w: torch.Tensor):
    """float w [E, N, K] -> (qweight uint8 [E, N, 3K/4], scales uint8 [E, N, K/32]): quantize + pack per expert."""
    qs = [quantize(w[e].cpu()) for e in range(w.shape[0])]
    return torch.stack([pack(c) for c, _ in qs]), torch.stack([s for _, s in qs])
