"""MXFP6 weight-only linear layer (W6A16, csrc/mxfp6.hip) against the library's other microscaling layers on the same shapes, in one process.

Shapes 4096 x 4096, 4096 -> 11008, 11008 -> 4096 and 2880 -> 5760, fp16 and bf16:
  sweep    M = 1 .. 32, 40, 48, 56, 64: both forms of the new layer where they exist (what the plan's bound in mxfp6.hip rests on)
  decode   M in {1, 4, 16}: the decode form (forced), the GB/s over the qweight + scales bytes, MXFP4LinearCuda's decode form and
           MXFP6A8LinearCuda's decode form (quantiser included) on the same shape
  prefill  M in {256, 4096}: the prefill form (forced) and TFLOP/s; MXFP4LinearCuda's and MXFP6A8LinearCuda's prefill forms, and
           bie_mxfp6_dequant to the dtype followed by torch.nn.functional.linear (the path without this layer)
Timing: the calls of `reps` rounds over enough weight sets that one round exceeds the 256 MB Infinity Cache are captured in one HIP graph;
HIP events around each of REPLAYS replays give device time without the host's launch floor.  A measurement is the median replay, with
the fastest and slowest beside it.

  python tools/mxfp6_bench.py [--part sweep,decode,prefill] [--shape I ...] [--quick] [--out DIR]
one JSON line per measurement on stdout (and appended to DIR/mxfp6_bench.jsonl)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402

MFMA_PEAK = 2.5e15
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096), (2880, 5760))
SWEEP = tuple(range(1, 33)) + (40, 48, 56, 64)
REPLAYS = 7


def sets_for(nbytes, cap=48):
    return max(2, min(cap, -(-512 * 2 ** 20 // nbytes)))


def time_graph(fns, calls=96):
    """(median, fastest, slowest) device microseconds per call of `fns` called round-robin, over REPLAYS replays of one captured graph."""
    reps = max(1, calls // len(fns))
    for f in fns:
        f()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in fns:
            f()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            for f in fns:
                f()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / (reps * len(fns)))
    del g
    return statistics.median(us), min(us), max(us)


def put(row, key, t):
    row[key + "_us"], row[key + "_min"], row[key + "_max"] = round(t[0], 2), round(t[1], 2), round(t[2], 2)
    return t[0]


def rand_sets(K, N, n, dev, gen, bytes_per_row):
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx4
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (N, bytes_per_row), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, mx4.col_exp(s)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="sweep,decode,prefill")
    ap.add_argument("--shape", type=int, nargs="*", default=None, help="indices into SHAPES (default: all)")
    ap.add_argument("--quick", action="store_true", help="fp16 only, decode M = 1 and prefill M = 4096, no sweep (for a profiler run)")
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mxfp6_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp6_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx4, mxfp6_a8_linear_cuda as mx6a8, mxfp6_linear_cuda as mx6
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    parts = set(a.part.split(",")) - ({"sweep"} if a.quick else set())
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp6_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    bound = 0  # the decode form's largest M, from the host-side check
    while bound < 4096 and _decode_exists(bound + 1):
        bound += 1
    shapes = [SHAPES[i] for i in (a.shape if a.shape is not None else range(len(SHAPES)))]
    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    for K, N in shapes:
        wbytes6, wbytes4 = N * K * 3 // 4 + N * K // 32, N * K // 2 + N * K // 32
        for dt in dts:
            dname = str(dt).replace("torch.", "")
            s6 = rand_sets(K, N, sets_for(wbytes6), dev, gen, K // 32 * 24)
            s4 = rand_sets(K, N, sets_for(wbytes4), dev, gen, K // 2)
            with torch.no_grad():
                if "decode" in parts:
                    for M in ((1,) if a.quick else (1, 4, 16)):
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        row = {"part": "decode", "dtype": dname, "K": K, "N": N, "M": M}
                        us = put(row, "mxfp6", time_graph([(lambda q=q, s=s: mx6.forward(x, q, s, None, None, form=0)) for q, s, e in s6]))
                        u4 = put(row, "mxfp4", time_graph([(lambda q=q, s=s: mx4.forward(x, q, s, None, None, form=0)) for q, s, e in s4]))
                        put(row, "mxfp6_a8", time_graph([(lambda q=q, s=s, e=e: mx6a8.forward(x, q, s, None, e, form=0)) for q, s, e in s6]))
                        row["mxfp6_gbps"], row["mxfp4_gbps"] = round(wbytes6 / us * 1e-3, 1), round(wbytes4 / u4 * 1e-3, 1)
                        row["mxfp6_over_mxfp4"] = round(us / u4, 3)
                        emit(row)
                if "prefill" in parts:
                    for M in ((4096,) if a.quick else (256, 4096)):
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        n = min(len(s6), 4 if M >= 1024 else 16)
                        calls = 16 if M >= 1024 else 48
                        row = {"part": "prefill", "dtype": dname, "K": K, "N": N, "M": M}
                        us = put(row, "mxfp6", time_graph([(lambda q=q, s=s, e=e: mx6.forward(x, q, s, None, e, form=1)) for q, s, e in s6[:n]], calls))
                        u4 = put(row, "mxfp4", time_graph([(lambda q=q, s=s, e=e: mx4.forward(x, q, s, None, e, form=1)) for q, s, e in s4[:n]], calls))
                        u8 = put(row, "mxfp6_a8", time_graph([(lambda q=q, s=s, e=e: mx6a8.forward(x, q, s, None, e, form=1)) for q, s, e in s6[:n]], calls))
                        ud = put(row, "dequant_linear", time_graph(
                            [(lambda q=q, s=s: torch.nn.functional.linear(x, mx6.dequant(q, s, dt))) for q, s, e in s6[:n]], calls))
                        row["mxfp6_tflops"] = round(2.0 * M * K * N / us * 1e-6, 1)
                        row["peak_share"] = round(2.0 * M * K * N / MFMA_PEAK / (us * 1e-6), 3)
                        row["over_mxfp4"], row["over_mxfp6_a8"], row["over_dequant_linear"] = round(us / u4, 3), round(us / u8, 3), round(us / ud, 3)
                        emit(row)
                if "sweep" in parts:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        row = {"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": mx6.form(M, N, K, dt)}
                        if M <= bound:
                            put(row, "decode", time_graph([(lambda q=q, s=s: mx6.forward(x, q, s, None, None, form=0)) for q, s, e in s6]))
                        put(row, "prefill", time_graph([(lambda q=q, s=s, e=e: mx6.forward(x, q, s, None, e, form=1)) for q, s, e in s6]))
                        emit(row)
            del s6, s4
            torch.cuda.empty_cache()
    if sink:
        sink.close()


def _decode_exists(M):
    """Whether bie_mxfp6_linear_forward takes form 0 at M: asked with a NULL x, so the call ends in the host-side checks either way."""
    from bitorch_engine import _hip
    fake = 1 << 20
    return _hip.lib().bie_mxfp6_linear_forward(None, fake, fake, fake, None, fake, M, 8, 64, 0, 0, None) == -1


if __name__ == "__main__":
    main()
