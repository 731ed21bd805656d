"""MXFP4 W4A8 linear layer (csrc/mxfp4_a8.hip) beside the W4A4 layer (csrc/mxfp4_a4.hip) and the MXFP4 weight-only layer (csrc/mxfp4.hip)
on the same shapes and weight bytes, the three arms alternated in one process (a8, a4, w4, a8, a4, w4; the mean of the two passes is
reported, both passes are kept, so the run-to-run spread of every arm can be read off the row).

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16:
  sweep    M in {8, 16, 24, 32, 48, 64}: both forms of the new layer forced, twice, the activation-quantise launch included (what the
           plan's bound in mxfp4_a8.hip rests on)
  cell     M in {1, 16, 64, 512, 4096}: each layer from x in its plan's form (the quantise launches of a8 and a4 included); for M >= 512
           TFLOP/s and the share of the 5 PF block-scaled FP8 peak, below that the share of 8 TB/s over the bytes the layer must move
           (weights + scales + x + y)
Timing: as tools/mxfp4_bench.py (graph-captured rounds over enough weight sets to exceed the 256 MB Infinity Cache, HIP events).

  python tools/mxfp4_a8_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp4_a8_bench.jsonl)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402
from mxfp4_bench import SHAPES, mx_sets, sets_for, time_graph  # noqa: E402

HBM = 8.0e12
FP8_PEAK = 5.0e15
CELLS = (1, 16, 64, 512, 4096)
SWEEP = (8, 16, 24, 32, 48, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 1 and M = 4096 at 4096 -> 11008, fp16, no sweep (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp4_a8_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp4_a8_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_a4_linear_cuda as a4, mxfp4_a8_linear_cuda as a8, mxfp4_linear_cuda as mx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp4_a8_bench.jsonl"), "w")

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
            sets = mx_sets(K, N, sets_for(N * K // 2 + N * K // 32), dev, gen)
            with torch.no_grad():
                if not a.quick:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        row = {"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": a8.form(M, N, K, dt)}
                        for name, form in (("decode_us", 0), ("prefill_us", 1), ("decode_us_2", 0), ("prefill_us_2", 1)):
                            row[name] = round(time_graph([(lambda q=q, s=s, e=e: a8.forward(x, q, s, None, e, form=form)) for q, s, e in sets]), 2)
                        emit(row)
                for M in ((1, 4096) if a.quick else CELLS):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    n = min(len(sets), 4 if M >= 512 else len(sets))
                    calls = 40 if M >= 512 else 120 if M >= 64 else 240
                    arms = {"a8": [(lambda q=q, s=s, e=e: a8.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "a4": [(lambda q=q, s=s, e=e: a4.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "w4": [(lambda q=q, s=s, e=e: mx.forward(x, q, s, None, e)) for q, s, e in sets[:n]]}
                    t = {k: [] for k in arms}
                    for _ in range(2):
                        for k, fns in arms.items():
                            t[k].append(time_graph(fns, calls))
                    us = {k: sum(v) / len(v) for k, v in t.items()}
                    row = {"part": "cell", "dtype": dname, "K": K, "N": N, "M": M, "a8_form": a8.form(M, N, K, dt), "a4_form": a4.form(M, N, K, dt),
                           "w4_form": mx.form(M, N, K, dt), "a8_us": round(us["a8"], 2), "a4_us": round(us["a4"], 2), "w4_us": round(us["w4"], 2),
                           "a8_over_a4": round(us["a8"] / us["a4"], 3), "a8_over_w4": round(us["a8"] / us["w4"], 3),
                           "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}}
                    if M >= 512:
                        fl = 2.0 * M * K * N
                        row.update(bound="matrix", tflops=round(fl / us["a8"] * 1e-6, 1), peak_share=round(fl / FP8_PEAK / (us["a8"] * 1e-6), 4))
                    else:
                        byts = N * K // 2 + N * K // 32 + 2 * M * K + 2 * M * N
                        row.update(bound="bytes", hbm_share=round(byts / HBM / (us["a8"] * 1e-6), 3))
                    emit(row)
            del sets
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
