"""MXFP6 W6A8 linear layer (csrc/mxfp6_a8.hip) beside the MXFP4 W4A8 layer (csrc/mxfp4_a8.hip) on the same shapes and activations, the
arms alternated in one process, three passes each; the median is reported and all passes are kept, so the run-to-run spread of every arm
can be read off the row.

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16:
  sweep    M in {8, 16, 24, 32, 48, 64}: both forms of the new layer forced, alternated, the activation-quantise launch included (what the
           plan's bound in mxfp6_a8.hip rests on)
  cell     M in {1, 16, 64, 256, 4096}: each layer from x in its plan's form (the quantise launch included); for M >= 256 TFLOP/s and the
           share of the 10 PF block-scaled FP6 peak, below that the share of 8 TB/s over the bytes the layer must move (weights + scales
           + x + y); w6_over_w4 beside the ratio of weight bytes read, (24 + 1) / (16 + 1) per block
Timing: as tools/mxfp4_bench.py (graph-captured rounds over enough weight sets to exceed the 256 MB Infinity Cache, HIP events).

  python tools/mxfp6_a8_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp6_a8_bench.jsonl)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402
from mxfp4_bench import SHAPES, mx_sets, sets_for, time_graph  # noqa: E402

HBM = 8.0e12
FP6_PEAK = 10.0e15
CELLS = (1, 16, 64, 256, 4096)
SWEEP = (8, 16, 24, 32, 48, 64)
PASSES = 3


def mx6_sets(K, N, n, dev, gen):
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as w6
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (N, K // 32 * 24), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, w6.col_exp(s)))
    return out


def alternate(arms, calls):
    """{name: [us of each pass]} with the arms alternated pass by pass."""
    t = {k: [] for k in arms}
    for _ in range(PASSES):
        for k, fns in arms.items():
            t[k].append(time_graph(fns, calls))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 1 and M = 4096 at 4096 -> 11008, fp16, no sweep (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp6_a8_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp6_a8_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as w4, mxfp6_a8_linear_cuda as w6
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp6_a8_bench.jsonl"), "w")

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
            n_sets = sets_for(N * K // 2 + N * K // 32)  # as many sets on either arm; the W4 sets alone exceed the cache
            sets6 = mx6_sets(K, N, n_sets, dev, gen)
            sets4 = mx_sets(K, N, n_sets, dev, gen)
            with torch.no_grad():
                if not a.quick:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        arms = {"decode": [(lambda q=q, s=s, e=e: w6.forward(x, q, s, None, e, form=0)) for q, s, e in sets6],
                                "prefill": [(lambda q=q, s=s, e=e: w6.forward(x, q, s, None, e, form=1)) for q, s, e in sets6]}
                        t = alternate(arms, 240)
                        emit({"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": w6.form(M, N, K, dt),
                              "decode_us": round(statistics.median(t["decode"]), 2), "prefill_us": round(statistics.median(t["prefill"]), 2),
                              "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}})
                for M in ((1, 4096) if a.quick else CELLS):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    n = min(n_sets, 4 if M >= 256 else n_sets)
                    calls = 40 if M >= 256 else 120 if M >= 64 else 240
                    arms = {"w6": [(lambda q=q, s=s, e=e: w6.forward(x, q, s, None, e)) for q, s, e in sets6[:n]],
                            "w4": [(lambda q=q, s=s, e=e: w4.forward(x, q, s, None, e)) for q, s, e in sets4[:n]]}
                    t = alternate(arms, calls)
                    us = {k: statistics.median(v) for k, v in t.items()}
                    row = {"part": "cell", "dtype": dname, "K": K, "N": N, "M": M, "w6_form": w6.form(M, N, K, dt), "w4_form": w4.form(M, N, K, dt),
                           "w6_us": round(us["w6"], 2), "w4_us": round(us["w4"], 2), "w6_over_w4": round(us["w6"] / us["w4"], 3),
                           "weight_bytes_ratio": round(25 / 17, 3), "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}}
                    if M >= 256:
                        fl = 2.0 * M * K * N
                        row.update(bound="matrix", tflops=round(fl / us["w6"] * 1e-6, 1), peak_share=round(fl / FP6_PEAK / (us["w6"] * 1e-6), 4))
                    else:
                        byts = N * K // 32 * 25 + 2 * M * K + 2 * M * N
                        row.update(bound="bytes", hbm_share=round(byts / HBM / (us["w6"] * 1e-6), 3))
                    emit(row)
            del sets6, sets4
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
