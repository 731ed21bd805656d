"""MXFP8 weight-only linear layer (W8A16, csrc/mxfp8.hip): the plan sweep and the figures beside the library's other routes, in one process.

Shapes 4096 x 4096, 4096 -> 11008, 11008 -> 4096 and 2880 -> 5760, fp16 and bf16:
  sweep    M = 1 .. 32, 40, 48, 56, 64: both forms of the layer where they exist (what the plan's bound in mxfp8.hip rests on)
  beside   M in {1, 16, 64, 4096}, every layer under its own plan, on weights quantised from the same latent matrices: MXFP8LinearCuda;
           MXFP8A8LinearCuda (its quantise launch included); MXFP6LinearCuda; and the route without this layer, bie_mx8_dequant to the
           dtype followed by torch.matmul.  The M = 1 row carries the GB/s over the qweight + scales bytes.
Timing is tools/mxfp6_bench.py's: the calls of `reps` rounds over enough weight sets that one round exceeds the 256 MB Infinity Cache are
captured in one HIP graph; a measurement is the median of REPLAYS replays, with the fastest and slowest beside it.

  python tools/mxfp8_bench.py [--part sweep,beside] [--shape I ...] [--dtype f16,bf16] [--m M ...] [--out DIR]
one JSON line per measurement on stdout (and appended to DIR/mxfp8_bench.jsonl)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402
from mxfp6_bench import SHAPES, SWEEP, put, sets_for, time_graph  # noqa: E402

DTS = {"f16": torch.float16, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="sweep,beside")
    ap.add_argument("--shape", type=int, nargs="*", default=None, help="indices into SHAPES (default: all)")
    ap.add_argument("--dtype", default="f16,bf16")
    ap.add_argument("--m", type=int, nargs="*", default=None, help="the sweep's M (default: SWEEP)")
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mxfp8_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp8_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine import _hip
    from bitorch_engine.extensions import mxfp6_linear_cuda as mx6, mxfp8_a8_linear_cuda as mx8a8, mxfp8_linear_cuda as mx8
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    parts = set(a.part.split(","))
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp8_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    fake = 1 << 20
    bound = 0  # the decode form's largest M: form 0 is refused beyond it, before the NULL x is found
    while bound < 4096 and _hip.lib().bie_mx8_linear_forward(None, fake, fake, fake, None, fake, bound + 1, 8, 64, 0, 0, None) == -1:
        bound += 1
    for K, N in [SHAPES[i] for i in (a.shape if a.shape is not None else range(len(SHAPES)))]:
        wbytes = N * K + N * K // 32
        for dname in a.dtype.split(","):
            dt = DTS[dname]
            s8, s6 = [], []
            for _ in range(sets_for(wbytes)):  # one latent matrix per set, quantised to both formats
                w = (torch.randn((N, K), generator=gen, device=dev) * 0.05).to(dt)
                q, s = mx8.quantize(w)
                s8.append((q, s, mx8.col_exp(s)))
                q, s = mx6.quantize(w)
                s6.append((q, s, mx6.col_exp(s)))
                del w
            with torch.no_grad():
                if "sweep" in parts:
                    for M in (a.m or SWEEP):
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        row = {"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": mx8.form(M, N, K, dt)}
                        if M <= bound:
                            put(row, "decode", time_graph([(lambda q=q, s=s: mx8.forward(x, q, s, None, None, form=0)) for q, s, e in s8]))
                        put(row, "prefill", time_graph([(lambda q=q, s=s, e=e: mx8.forward(x, q, s, None, e, form=1)) for q, s, e in s8]))
                        emit(row)
                if "beside" in parts:
                    for M in (1, 16, 64, 4096):
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        n = min(len(s8), 4 if M >= 1024 else len(s8))
                        calls = 16 if M >= 1024 else 96
                        row = {"part": "beside", "dtype": dname, "K": K, "N": N, "M": M, "form": mx8.form(M, N, K, dt)}
                        us = put(row, "mxfp8", time_graph([(lambda q=q, s=s, e=e: mx8.forward(x, q, s, None, e)) for q, s, e in s8[:n]], calls))
                        u8 = put(row, "mxfp8_a8", time_graph([(lambda q=q, s=s, e=e: mx8a8.forward(x, q, s, None, e)) for q, s, e in s8[:n]], calls))
                        u6 = put(row, "mxfp6", time_graph([(lambda q=q, s=s, e=e: mx6.forward(x, q, s, None, e)) for q, s, e in s6[:n]], calls))
                        ud = put(row, "dequant_matmul", time_graph(
                            [(lambda q=q, s=s: torch.matmul(x, mx8.dequant(q, s, dt).t())) for q, s, e in s8[:n]], calls))
                        if M == 1:
                            row["mxfp8_gbps"], row["mxfp8_a8_gbps"] = round(wbytes / us * 1e-3, 1), round(wbytes / u8 * 1e-3, 1)
                        row["over_mxfp8_a8"], row["over_mxfp6"], row["over_dequant_matmul"] = round(us / u8, 3), round(us / u6, 3), round(us / ud, 3)
                        emit(row)
            del s8, s6
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
