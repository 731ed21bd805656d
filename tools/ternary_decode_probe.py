"""Kernel-level probe of the ternary decode form against BinaryLinearCuda's one-launch forward, for rocprofv3 (kernel trace or --pmc).

fp16, M = 1 and 4, 4096 x 4096 and 4096 -> 11008: three rounds over enough layers of distinct weights that one round exceeds the 256 MB
Infinity Cache (the layer sets of tools/ternary_bench.py).  Kernel times and counters come from the profiler, not from this script:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/ternary_decode_probe.py
  rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VMEM_RD --output-format csv -d DIR -o p -- python tools/ternary_decode_probe.py

Run against a lab build of the library (BIE_HIP_LIB=...) compiled with -DBIE_TERNARY_NNZ_LAB it times the decode kernel without its
per-row non-zero count, the lower bound of a count stored at pack time (profiles/ternary_decode_probe.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import ternary_bench as tb  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the probe runs on the GPU"
    from bitorch_engine.extensions import ternary_linear_cuda as tx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    for (K, N) in ((4096, 4096), (4096, 11008)):
        tl = tb.ternary_layers(K, N, torch.float16, tb.sets_for(K * N // 4), dev, gen)
        bl = tb.binary_layers(K, N, torch.float16, tb.sets_for(K * N // 8), dev, gen)
        for M in (1, 4):
            x = torch.randn((M, K), generator=gen, device=dev).half()
            with torch.no_grad():
                for _ in range(3):
                    for layer in tl:
                        tx.linear_fused(x, layer.qweight, layer.bias_a, layer.scale_a, layer.scale_w)
                    for layer in bl:
                        layer(x)
        torch.cuda.synchronize()
        del tl, bl


if __name__ == "__main__":
    main()
