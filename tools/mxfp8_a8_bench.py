"""MXFP8 W8A8 linear layer (csrc/mxfp8_a8.hip) beside the MXFP4 W4A8 (csrc/mxfp4_a8.hip) and MXFP6 W6A8 (csrc/mxfp6_a8.hip) layers on the
same latent weights (each layer quantises them to its own format), shapes and activations, the arms alternated in one process, three
passes each; the median is reported and all passes are kept, so the run-to-run spread of every arm can be read off the row.  The three
layers pay the same matrix cycles (every pair has an E4M3 operand); what differs is the weight stream: 33 / 32 bytes per weight here,
against 17 / 32 (W4A8: 1.94 x fewer) and 25 / 32 (W6A8: 1.32 x fewer).

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16:
  sweep    M in {8, 16, 24, 32, 48, 64}: both forms of the new layer forced, alternated, the activation-quantise launch included (what the
           plan's bound in mxfp8_a8.hip rests on)
  cell     M in {1, 16, 64, 256, 4096}: each layer from x in its plan's form (the quantise launch included), and the W8A8 layer's two
           launches timed apart (quant_us: bie_mxfp8_quantize_act alone; gemm_us: the contraction from quantised activations); for
           M >= 256 TFLOP/s and the share of the 5 PF block-scaled FP8 peak, below that the share of 8 TB/s over the bytes the layer
           must move (weights + scales + x + y); w8_over_w4 / w8_over_w6 are the ratios of the layers' times (above 1: W8A8 behind),
           bytes_w8_over_w4 / bytes_w8_over_w6 the ratios of those byte counts
The "tile" rows of profiles/mxfp8_a8_bench.jsonl (M = 4096: 128 x 128 at 64 k per stage, which ships, against 128 x 64 at 128 k per
stage and 64 x 64 tiles everywhere) were taken with the same timing from a build that still held the two losing instances; they are
kept in the profile and cannot be re-measured from this source.
Timing: as tools/mxfp4_bench.py (graph-captured rounds over enough weight sets to exceed the 256 MB Infinity Cache, HIP events).

  python tools/mxfp8_a8_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp8_a8_bench.jsonl)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))

FP8_PEAK = 5.0e15


def latent_sets(K, N, n, dt, dev, gen):
    """n latent weights, each quantised by the three layers' own quantisers: [(w8, w6, w4)] of (qweight, scales, e_col)."""
    import torch
    from bitorch_engine.extensions import mxfp4_linear_cuda as w4, mxfp6_a8_linear_cuda as w6, mxfp8_a8_linear_cuda as w8
    out = []
    for _ in range(n):
        w = (torch.randn((N, K), generator=gen, device=dev) * 0.02).to(dt)
        trio = []
        for m in (w8, w6, w4):
            q, s = m.quantize(w)
            trio.append((q, s, w4.col_exp(s)))
        out.append(tuple(trio))
        del w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 1 and M = 4096 at 4096 -> 11008, fp16, no sweep (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp8_a8_bench.jsonl")
    a = ap.parse_args()
    import torch
    from mxfp4_bench import SHAPES, sets_for
    from mxfp6_a8_bench import CELLS, HBM, SWEEP, alternate
    assert torch.cuda.is_available(), "mxfp8_a8_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as a4, mxfp6_a8_linear_cuda as a6, mxfp8_a8_linear_cuda as a8
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp8_a8_bench.jsonl"), "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def med(t):
        return {k: statistics.median(v) for k, v in t.items()}

    shapes = ((4096, 11008),) if a.quick else SHAPES
    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    for K, N in shapes:
        for dt in dts:
            dname = str(dt).replace("torch.", "")
            # as many sets as keep the smallest format (W4: 17 bytes per 32 weights) beyond the Infinity Cache
            sets = latent_sets(K, N, sets_for(N * K // 32 * 17), dt, dev, gen)
            with torch.no_grad():
                if not a.quick:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        arms = {"decode": [(lambda q=q, s=s, e=e: a8.forward(x, q, s, None, e, form=0)) for (q, s, e), _, _ in sets],
                                "prefill": [(lambda q=q, s=s, e=e: a8.forward(x, q, s, None, e, form=1)) for (q, s, e), _, _ in sets]}
                        t = alternate(arms, 240)
                        emit({"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": a8.form(M, N, K, dt),
                              "decode_us": round(statistics.median(t["decode"]), 2), "prefill_us": round(statistics.median(t["prefill"]), 2),
                              "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}})
                for M in ((1, 4096) if a.quick else CELLS):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    xq, xs, flag = a8.quantize_act(x)
                    n = min(len(sets), 4 if M >= 256 else len(sets))
                    calls = 40 if M >= 256 else 120 if M >= 64 else 240
                    arms = {"w8": [(lambda q=q, s=s, e=e: a8.forward(x, q, s, None, e)) for (q, s, e), _, _ in sets[:n]],
                            "w6": [(lambda q=q, s=s, e=e: a6.forward(x, q, s, None, e)) for _, (q, s, e), _ in sets[:n]],
                            "w4": [(lambda q=q, s=s, e=e: a4.forward(x, q, s, None, e)) for _, _, (q, s, e) in sets[:n]],
                            "w8_gemm": [(lambda q=q, s=s, e=e: a8.gemm(xq, xs, flag, q, s, None, e, dtype=dt)) for (q, s, e), _, _ in sets[:n]],
                            "w8_quant": [lambda: a8.quantize_act(x)]}
                    t = alternate(arms, calls)
                    us = med(t)
                    act = 2 * M * K + 2 * M * N
                    b8, b6, b4 = (N * K // 32 * c + act for c in (33, 25, 17))
                    row = {"part": "cell", "dtype": dname, "K": K, "N": N, "M": M, "w8_form": a8.form(M, N, K, dt), "w6_form": a6.form(M, N, K, dt),
                           "w4_form": a4.form(M, N, K, dt), "w8_us": round(us["w8"], 2), "w6_us": round(us["w6"], 2), "w4_us": round(us["w4"], 2),
                           "quant_us": round(us["w8_quant"], 2), "gemm_us": round(us["w8_gemm"], 2),
                           "w8_over_w4": round(us["w8"] / us["w4"], 3), "w8_over_w6": round(us["w8"] / us["w6"], 3),
                           "bytes_w8_over_w4": round(b8 / b4, 3), "bytes_w8_over_w6": round(b8 / b6, 3),
                           "passes_us": {k: [round(v, 2) for v in vs] for k, vs in t.items()}}
                    if M >= 256:
                        fl = 2.0 * M * K * N
                        row.update(bound="matrix", tflops=round(fl / us["w8"] * 1e-6, 1), peak_share=round(fl / FP8_PEAK / (us["w8"] * 1e-6), 4))
                    else:
                        row.update(bound="bytes", hbm_share=round(b8 / HBM / (us["w8"] * 1e-6), 3))
                    emit(row)
            del sets
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
