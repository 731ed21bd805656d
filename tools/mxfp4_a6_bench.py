"""MXFP4 W4A6 linear layer (csrc/mxfp4_a6.hip) beside the MXFP4 W4A8 (csrc/mxfp4_a8.hip) and W4A4 (csrc/mxfp4_a4.hip) layers on the same
weight sets (the three layers read the same bytes), shapes and activations, the arms alternated in one process, three passes each; the
median is reported and all passes are kept, so the run-to-run spread of every arm can be read off the row.

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16:
  sweep    M in {8, 16, 24, 32, 48, 64}: both forms of the new layer forced, alternated, the activation-quantise launch included (what the
           plan's bound in mxfp4_a6.hip rests on)
  cell     M in {1, 16, 64, 256, 4096}: each layer from x in its plan's form (the quantise launch included), and the W4A6 layer's two
           launches timed apart (quant_us: bie_mxfp6_quantize_act alone; gemm_us: the contraction from quantised activations); for
           M >= 256 TFLOP/s and the share of the 10 PF block-scaled FP4 x FP6 peak, below that the share of 8 TB/s over the bytes the
           layer must move (weights + scales + x + y); a6_over_a8 / a6_over_a4 are the ratios of the layers' times (below 1: W4A6 ahead)
Timing: as tools/mxfp4_bench.py (graph-captured rounds over enough weight sets to exceed the 256 MB Infinity Cache, HIP events).

  python tools/mxfp4_a6_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp4_a6_bench.jsonl)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402
from mxfp4_bench import SHAPES, mx_sets, sets_for  # noqa: E402
from mxfp6_a8_bench import CELLS, FP6_PEAK, HBM, SWEEP, alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 1 and M = 4096 at 4096 -> 11008, fp16, no sweep (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp4_a6_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp4_a6_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_a4_linear_cuda as a4, mxfp4_a6_linear_cuda as a6, mxfp4_a8_linear_cuda as a8
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp4_a6_bench.jsonl"), "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    shapes = ((4096, 11008),) if a.quick else SHAPES
    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    for K, N in shapes:
        for dt in dts:
            dname = str(dt).replace("torch.", "")
            sets = mx_sets(K, N, sets_for(N * K // 32 * 17), dev, gen)  # one list of weight sets for the three arms: the same bytes
            with torch.no_grad():
                if not a.quick:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        arms = {"decode": [(lambda q=q, s=s, e=e: a6.forward(x, q, s, None, e, form=0)) for q, s, e in sets],
                                "prefill": [(lambda q=q, s=s, e=e: a6.forward(x, q, s, None, e, form=1)) for q, s, e in sets]}
                        t = alternate(arms, 240)
                        emit({"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": a6.form(M, N, K, dt),
                              "decode_us": round(statistics.median(t["decode"]), 2), "prefill_us": round(statistics.median(t["prefill"]), 2),
                              "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}})
                for M in ((1, 4096) if a.quick else CELLS):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    xq, xs, flag = a6.quantize_act(x)
                    n = min(len(sets), 4 if M >= 256 else len(sets))
                    calls = 40 if M >= 256 else 120 if M >= 64 else 240
                    arms = {"a6": [(lambda q=q, s=s, e=e: a6.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "a8": [(lambda q=q, s=s, e=e: a8.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "a4": [(lambda q=q, s=s, e=e: a4.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "a6_gemm": [(lambda q=q, s=s, e=e: a6.gemm(xq, xs, flag, q, s, None, e, dtype=dt)) for q, s, e in sets[:n]],
                            "a6_quant": [lambda: a6.quantize_act(x)]}
                    t = alternate(arms, calls)
                    us = {k: statistics.median(v) for k, v in t.items()}
                    row = {"part": "cell", "dtype": dname, "K": K, "N": N, "M": M, "a6_form": a6.form(M, N, K, dt), "a8_form": a8.form(M, N, K, dt),
                           "a4_form": a4.form(M, N, K, dt), "a6_us": round(us["a6"], 2), "a8_us": round(us["a8"], 2), "a4_us": round(us["a4"], 2),
                           "quant_us": round(us["a6_quant"], 2), "gemm_us": round(us["a6_gemm"], 2),
                           "a6_over_a8": round(us["a6"] / us["a8"], 3), "a6_over_a4": round(us["a6"] / us["a4"], 3),
                           "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}}
                    if M >= 256:
                        fl = 2.0 * M * K * N
                        row.update(bound="matrix", tflops=round(fl / us["a6"] * 1e-6, 1), peak_share=round(fl / FP6_PEAK / (us["a6"] * 1e-6), 4))
                    else:
                        byts = N * K // 32 * 17 + 2 * M * K + 2 * M * N
                        row.update(bound="bytes", hbm_share=round(byts / HBM / (us["a6"] * 1e-6), 3))
                    emit(row)
            del sets
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
