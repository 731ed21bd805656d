"""Counter runs of the MXFP4 prefill form (mx_gemm_kernel) against the MPQ W4 g128 GEMM at the same points.

  rocprofv3 --pmc <counters> -d DIR -o NAME --output-format csv -- python tools/mxfp4_pmc.py run       the launches (fp16)
  python tools/mxfp4_pmc.py summarize DIR/..._counter_collection.csv [...]                              mean per kernel and grid

Points: 4096 -> 11008 at M = 4096 and M = 64 (the prefill form and the MPQ layer's own plan), 5 launches each after a warm-up."""
import csv
import os
import sys
from collections import defaultdict

os.environ.setdefault("BIE_AUTO_GROUP", "0")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bitorch-engine_amd"))


def run():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from mxfp4_bench import mx_sets, mpq_w4_layers
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    K, N, dt = 4096, 11008, torch.float16
    (q, s, e), = mx_sets(K, N, 1, dev, gen)
    mpq, = mpq_w4_layers(K, N, dt, 1, dev, gen)
    with torch.no_grad():
        for M in (4096, 64):
            x = torch.randn((M, K), generator=gen, device=dev).to(dt)
            for _ in range(6):
                mx.forward(x, q, s, None, e, form=1)
                mpq(x)
    torch.cuda.synchronize()


def summarize(paths):
    acc = defaultdict(lambda: defaultdict(list))
    for p in paths:
        for r in csv.DictReader(open(p)):
            name = r.get("Kernel_Name", "")
            if "bie::" not in name:
                continue
            key = (name.split("(")[0].replace("void ", ""), r.get("Grid_Size", ""))
            acc[key][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for (name, grid), cs in sorted(acc.items()):
        mean = {c: sum(v) / len(v) for c, v in cs.items()}
        line = f"{name} grid={grid} " + " ".join(f"{c}={mean[c]:.0f}" for c in sorted(mean))
        if "SQ_INSTS_MFMA" in mean and mean["SQ_INSTS_MFMA"]:
            if "SQ_INSTS_VALU" in mean:
                line += f" VALU/MFMA={mean['SQ_INSTS_VALU'] / mean['SQ_INSTS_MFMA']:.2f}"
            if "SQ_INSTS_LDS" in mean:
                line += f" LDS/MFMA={mean['SQ_INSTS_LDS'] / mean['SQ_INSTS_MFMA']:.2f}"
        if "SQ_WAIT_ANY" in mean and mean.get("SQ_WAVE_CYCLES"):
            line += f" WAIT_ANY/WAVE_CYCLES={mean['SQ_WAIT_ANY'] / mean['SQ_WAVE_CYCLES']:.3f}"
        if "SQ_VALU_MFMA_BUSY_CYCLES" in mean and mean.get("SQ_BUSY_CYCLES"):
            line += f" MFMA_BUSY/BUSY={mean['SQ_VALU_MFMA_BUSY_CYCLES'] / mean['SQ_BUSY_CYCLES']:.2f}"
        print(line)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "summarize":
        summarize(sys.argv[2:])
    else:
        run()
