"""Ternary W1.58A8 linear layer (TernaryA8LinearCuda, eval) against its yardsticks on the same shapes, in one process: W8A8 q8_forward
(bie_q8_gemm on int8 operands already quantised), the MPQ W2A16 layer and the binary-activation TernaryLinearCuda.

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16, M in {1, 2, 4, 8, 16, 32, 64, 128, 512, 4096}.  Timing: HIP events
around a loop of calls after warm-up, rotating over enough weight sets that one round exceeds the 256 MB Infinity Cache (small-M numbers
are HBM numbers).  For M <= 8 a second line times the two forms of the new layer directly (decode: linear_fused; GEMM: quantise + GEMM),
which is what the decode bound of bie_ternary_a8_fused_ok rests on.  Event times at small M sit on the host's launch floor: kernel times
come from a separate `rocprofv3 --kernel-trace --stats` run of `--quick`.  Roofline: bytes = 2*N*K/8 + alpha + x + y over the 8 TB/s
HBM peak; the I8 matrix peak is taken as 5.0e15 op/s (2x BF16 per clock).

  python tools/ternary_a8_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/ternary_a8_bench.jsonl)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402
from ternary_bench import HBM, SHAPES, sets_for, time_region, ternary_layers, mpq_w2_layers  # noqa: E402

I8_PEAK = 5.0e15
ROWS = (1, 2, 4, 8, 16, 32, 64, 128, 512, 4096)


def a8_layers(K, N, dt, n, dev, gen):
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryA8LinearCuda
    out = []
    for _ in range(n):
        layer = TernaryA8LinearCuda(K, N, dtype=dt, device=dev)
        t = torch.randint(-1, 2, (N, K), generator=gen, device=dev, dtype=torch.int8)
        layer.set_ternary_weight(t, torch.rand(N, generator=gen, device=dev) * 0.05)
        out.append(layer.eval())
    return out


def q8_sets(K, N, dt, n, dev, gen):
    from bitorch_engine.extensions import q_linear_cutlass as qc
    ws = [torch.randint(-127, 128, (N, K), generator=gen, device=dev, dtype=torch.int8) for _ in range(n)]
    return [(lambda x, w=w: qc.q8_forward(x, w, False, 0.01, 0.02)) for w in ws]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the two headline points only (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/ternary_a8_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ternary_a8_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import ternary_a8_linear_cuda as ax
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "ternary_a8_bench.jsonl"), "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")

    if a.quick:  # decode M = 1 at 4096 -> 11008 and prefill M = 4096 at 4096^2, new layer and the two yardsticks the targets name
        plan = [((4096, 11008), (1,)), ((4096, 4096), (4096,))]
        dts = (torch.float16,)
    else:
        plan = [(s, ROWS) for s in SHAPES]
        dts = (torch.float16, torch.bfloat16)
    for (K, N), rows in plan:
        for dt in dts:
            dname = str(dt).replace("torch.", "")
            kinds = [("ternary_a8", a8_layers, K * N // 4), ("ternary_binary_act", ternary_layers, K * N // 4),
                     ("mpq_w2a16", mpq_w2_layers, K * N // 4), ("w8a8_q8_forward", None, K * N)]
            for kind, make, wbytes in kinds:
                n = sets_for(wbytes)
                if make is None:
                    fns_of = q8_sets(K, N, dt, n, dev, gen)
                else:
                    layers = make(K, N, dt, n, dev, gen)
                    fns_of = [(lambda x, l=l: l(x)) for l in layers]
                for M in rows:
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    if make is None:
                        x = torch.randint(-127, 128, (M, K), generator=gen, device=dev, dtype=torch.int8)
                    fns = [(lambda f=f: f(x)) for f in fns_of]
                    with torch.no_grad():
                        us = time_region(fns, max(2, min(50, int(2e4 // (len(fns) * (1 + M // 16))))))
                    ysz = 4 if make is None else x.element_size()
                    byts = wbytes + N * x.element_size() + M * K * x.element_size() + M * N * ysz
                    emit({"layer": kind, "dtype": dname, "K": K, "N": N, "M": M, "us": round(us, 2), "roofline": round(byts / HBM / (us * 1e-6), 3),
                          "i8_peak": round(2.0 * M * K * N / I8_PEAK / (us * 1e-6), 3)})
                del fns_of
                torch.cuda.empty_cache()
            if a.quick:
                continue
            al = a8_layers(K, N, dt, sets_for(K * N // 4), dev, gen)
            for M in (1, 2, 3, 4, 5, 8):
                if not ax.fused_ok(M, N, K):
                    continue
                x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                with torch.no_grad():
                    dec = time_region([(lambda l=l: ax.linear_fused(x, l.qweight, l.scale_w)) for l in al], 20)
                    gm = time_region([(lambda l=l: ax.linear_gemm(x, l.qweight, l.scale_w)) for l in al], 20)
                emit({"forms": "ternary_a8", "dtype": dname, "K": K, "N": N, "M": M, "decode_us": round(dec, 2), "gemm_us": round(gm, 2)})
            del al
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
