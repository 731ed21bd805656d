"""Counter runs of the MXFP4 W4A4 prefill form (mxa4_quantize_kernel + mxa4_gemm_kernel) against the weight-only prefill form
(mx_gemm_kernel) at the same point.

  rocprofv3 --pmc <counters> -d DIR -o NAME --output-format csv -- python tools/mxfp4_a4_pmc.py run     the launches (fp16)
  python tools/mxfp4_a4_pmc.py summarize DIR/..._counter_collection.csv [...]                            mean per kernel and grid

Point: 4096 -> 11008 at M = 4096, 6 launches of each layer after a warm-up."""
import os
import sys

os.environ.setdefault("BIE_AUTO_GROUP", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "bitorch-engine_amd"))


def run():
    import torch
    from mxfp4_bench import mx_sets
    from bitorch_engine.extensions import mxfp4_a4_linear_cuda as a4, mxfp4_linear_cuda as mx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    K, N, M, dt = 4096, 11008, 4096, torch.float16
    (q, s, e), = mx_sets(K, N, 1, dev, gen)
    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
    with torch.no_grad():
        for _ in range(6):
            a4.forward(x, q, s, None, e, form=1)
            mx.forward(x, q, s, None, e, form=1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
    else:
        from mxfp4_pmc import summarize
        summarize(sys.argv[2:])
