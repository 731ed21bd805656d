"""MXFP4 W4A4 linear layer (csrc/mxfp4_a4.hip) against the MXFP4 weight-only layer (csrc/mxfp4.hip) and the lone MPQ W4A16 g128 layer on the
same shapes, the three arms alternated in one process (new, weight-only, MPQ, new, weight-only, MPQ; the mean of the two passes is
reported, both passes are kept).

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16:
  cell     M in {1, 4, 8, 16, 64, 256, 1024, 4096}: the new layer from x (its activation-quantise launch included, the plan's form), the
           weight-only layer (its plan's form) and MPQ; for M >= 256 TFLOP/s and the share of the 10 PF FP4 peak, below that the share of
           8 TB/s over the bytes the layer must move (weights + scales + x + y)
  sweep    M in {8, 16, 24, 32, 48, 64}: both forms of the new layer forced (what the plan's bound in mxfp4_a4.hip rests on)
Timing: as tools/mxfp4_bench.py (graph-captured rounds over enough weight sets to exceed the 256 MB Infinity Cache, HIP events).

  python tools/mxfp4_a4_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp4_a4_bench.jsonl)"""
import argparse
import json
import os
import sys

os.environ.setdefault("BIE_AUTO_GROUP", "0")  # the lone MPQ forward
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402
from mxfp4_bench import SHAPES, mpq_w4_layers, mx_sets, sets_for, time_graph  # noqa: E402

HBM = 8.0e12
FP4_PEAK = 10.0e15
CELLS = (1, 4, 8, 16, 64, 256, 1024, 4096)
SWEEP = (8, 16, 24, 32, 48, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 1 and M = 4096 at 4096 -> 11008, fp16 (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp4_a4_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp4_a4_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_a4_linear_cuda as a4, mxfp4_linear_cuda as mx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp4_a4_bench.jsonl"), "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")

    shapes = ((4096, 11008),) if a.quick else SHAPES
    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    for K, N in shapes:
        for dt in dts:
            dname = str(dt).replace("torch.", "")
            sets = mx_sets(K, N, sets_for(N * K // 2 + N * K // 32), dev, gen)
            mpq = mpq_w4_layers(K, N, dt, sets_for(N * K // 2 + N * K // 16), dev, gen)
            with torch.no_grad():
                for M in ((1, 4096) if a.quick else CELLS):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    n = min(len(sets), 4 if M >= 1024 else len(sets))
                    calls = 40 if M >= 1024 else 120 if M >= 64 else 240
                    arms = {"a4": [(lambda q=q, s=s, e=e: a4.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "w4": [(lambda q=q, s=s, e=e: mx.forward(x, q, s, None, e)) for q, s, e in sets[:n]],
                            "mpq": [(lambda l=l: l(x)) for l in mpq[:n]]}
                    t = {k: [] for k in arms}
                    for _ in range(2):
                        for k, fns in arms.items():
                            t[k].append(time_graph(fns, calls))
                    us = {k: sum(v) / len(v) for k, v in t.items()}
                    row = {"part": "cell", "dtype": dname, "K": K, "N": N, "M": M, "a4_form": a4.form(M, N, K, dt), "w4_form": mx.form(M, N, K, dt),
                           "a4_us": round(us["a4"], 2), "w4_us": round(us["w4"], 2), "mpq_w4g128_us": round(us["mpq"], 2),
                           "a4_over_w4": round(us["a4"] / us["w4"], 3), "a4_over_mpq": round(us["a4"] / us["mpq"], 3),
                           "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}}
                    if M >= 256:
                        fl = 2.0 * M * K * N
                        row.update(bound="matrix", tflops=round(fl / us["a4"] * 1e-6, 1), peak_share=round(fl / FP4_PEAK / (us["a4"] * 1e-6), 4))
                    else:
                        byts = N * K // 2 + N * K // 32 + 2 * M * K + 2 * M * N
                        row.update(bound="bytes", hbm_share=round(byts / HBM / (us["a4"] * 1e-6), 3))
                    emit(row)
                if not a.quick:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        row = {"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": a4.form(M, N, K, dt)}
                        for name, form in (("decode_us", 0), ("prefill_us", 1), ("decode_us_2", 0), ("prefill_us_2", 1)):
                            row[name] = round(time_graph([(lambda q=q, s=s, e=e: a4.forward(x, q, s, None, e, form=form)) for q, s, e in sets]), 2)
                        emit(row)
            del sets, mpq
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
