"""MXFP4 linear layer (csrc/mxfp4.hip) against the lone MPQ W4A16 g128 layer (bie_mpq_forward, sibling grouping off) on the same shapes,
in one process.

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16:
  decode   M in {1, 4, 8, 16}: the decode form (forced) and MPQ W4 g128; us and the HBM share (bytes = N*K/2 + N*K/32 + x + y over 8 TB/s)
  prefill  M in {64, 256, 1024, 4096}: the prefill form (forced) and MPQ (its own plan); TFLOP/s and the share of the 2.5 PF bf16/fp16 peak
  sweep    M = 1 .. 16, 20, 24, 32, 48, 64: both forms of the new layer where they exist (what the plan's bound in mxfp4.hip rests on)
Timing: the calls of `reps` rounds over enough weight sets that one round exceeds the 256 MB Infinity Cache are captured in one HIP graph;
HIP events around its replay give device time without the host's launch floor.

  python tools/mxfp4_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp4_bench.jsonl)"""
import argparse
import copy
import json
import os
import sys

os.environ.setdefault("BIE_AUTO_GROUP", "0")  # the lone MPQ forward
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402

HBM = 8.0e12
MFMA_PEAK = 2.5e15
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))
SWEEP = tuple(range(1, 17)) + (20, 24, 32, 48, 64)


def sets_for(nbytes, cap=48):
    return max(2, min(cap, -(-512 * 2 ** 20 // nbytes)))


def time_graph(fns, calls=240):
    """Mean device microseconds per call of `fns` called round-robin, replayed from one captured graph."""
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * len(fns))
    del g
    return us


def mx_sets(K, N, n, dev, gen):
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (N, K // 2), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, mx.col_exp(s)))
    return out


def mpq_w4_layers(K, N, dt, n, dev, gen):
    from bitorch_engine.layers.qlinear.nbit.cuda import MPQLinearCuda
    proto = MPQLinearCuda(K, N, w_bit=4, dtype=dt, group_size=128, dq_group_size=32, use_gba_quant=True, asym=False)
    proto.qweight.data = torch.zeros(proto.qweight.shape, dtype=torch.int32)
    proto.prepare_params()
    proto.to(dev).eval()
    out = []
    for _ in range(n):
        layer = copy.deepcopy(proto)
        layer.qweight.data = torch.randint(-2 ** 31, 2 ** 31 - 1, layer.qweight.shape, generator=gen, device=dev, dtype=torch.int32)
        layer.scales = (torch.rand(layer.scales.shape, generator=gen, device=dev) * 0.01 + 0.005).to(dt)
        layer.zeros = (layer.scales.float() * 7.5).to(dt)
        out.append(layer)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="decode M = 1 and prefill M = 4096 at 4096 -> 11008, fp16 (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp4_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp4_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp4_bench.jsonl"), "w")

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
                for M in ((1,) if a.quick else (1, 4, 8, 16)):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    us = time_graph([(lambda q=q, s=s, e=e: mx.forward(x, q, s, None, e, form=0)) for q, s, e in sets])
                    ref = time_graph([(lambda l=l: l(x)) for l in mpq])
                    byts = N * K // 2 + N * K // 32 + 2 * M * K + 2 * M * N
                    emit({"part": "decode", "dtype": dname, "K": K, "N": N, "M": M, "mxfp4_us": round(us, 2), "mpq_w4g128_us": round(ref, 2),
                          "ratio": round(us / ref, 3), "hbm_share": round(byts / HBM / (us * 1e-6), 3)})
                for M in ((4096,) if a.quick else (64, 256, 1024, 4096)):
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    n = min(len(sets), 4 if M >= 1024 else len(sets))
                    us = time_graph([(lambda q=q, s=s, e=e: mx.forward(x, q, s, None, e, form=1)) for q, s, e in sets[:n]], 40 if M >= 1024 else 120)
                    ref = time_graph([(lambda l=l: l(x)) for l in mpq[:n]], 40 if M >= 1024 else 120)
                    fl = 2.0 * M * K * N
                    emit({"part": "prefill", "dtype": dname, "K": K, "N": N, "M": M, "mxfp4_us": round(us, 2), "mpq_w4g128_us": round(ref, 2),
                          "ratio": round(us / ref, 3), "tflops": round(fl / us * 1e-6, 1), "peak_share": round(fl / MFMA_PEAK / (us * 1e-6), 3)})
                if not a.quick:
                    for M in SWEEP:
                        x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                        row = {"part": "sweep", "dtype": dname, "K": K, "N": N, "M": M, "plan": mx.form(M, N, K, dt)}
                        if M <= 16:
                            row["decode_us"] = round(time_graph([(lambda q=q, s=s, e=e: mx.forward(x, q, s, None, e, form=0)) for q, s, e in sets]), 2)
                        row["prefill_us"] = round(time_graph([(lambda q=q, s=s, e=e: mx.forward(x, q, s, None, e, form=1)) for q, s, e in sets]), 2)
                        emit(row)
            del sets, mpq
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
