"""Ternary linear layer forward (TernaryLinearCuda, eval) against BinaryLinearCuda and the MPQ W2A16 layer on the same shapes, in one process.

Shapes 4096 x 4096, 4096 -> 11008 and 11008 -> 4096, fp16 and bf16, M in {1, 4, 16, 64, 256, 4096}.  Timing: HIP events around a loop of
module forwards after warm-up, one synchronise per region; the forwards rotate over enough layer instances (distinct weights) that the
weights of one round exceed the 256 MB Infinity Cache, so small-M numbers are HBM numbers.  A second table times the ternary layer's two
forms directly (decode: bie_ternary_linear_fused, matrix pipe: bie_ternary_linear_layer_fp4 on a prebuilt weight image) for the rows the
decode form covers (M <= 4, the bound of bie_ternary_linear_fused_ok; profiles/ternary_bench_16rows.jsonl holds the run that set it, with a
16-row decode instance).  Event times of these Python-level calls sit on the host's launch floor at small M: kernel times come from
rocprofv3 (profiles/ternary_kernel_stats.csv, and tools/ternary_decode_probe.py for the decode form).  Roofline: bytes = K*N/4 (two bits per ternary
weight) + x + y over the 8 TB/s HBM peak.

  python tools/ternary_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/ternary_bench.jsonl)"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
import torch  # noqa: E402

HBM = 8.0e12
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))
ROWS = (1, 4, 16, 64, 256, 4096)


def sets_for(nbytes, cap=64):
    return max(2, min(cap, -(-512 * 2 ** 20 // nbytes)))


def time_region(fns, reps):
    """Mean microseconds per call of the functions in `fns` called round-robin, after one warm-up round."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for f in fns:
            f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(fns))


def ternary_layers(K, N, dt, n, dev, gen):
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryLinearCuda
    out = []
    for _ in range(n):
        layer = TernaryLinearCuda(K, N, dtype=dt, device=dev)
        t = torch.randint(-1, 2, (N, K), generator=gen, device=dev, dtype=torch.int8)
        layer.set_ternary_weight(t, torch.rand(N, generator=gen, device=dev) * 0.05)
        with torch.no_grad():
            layer.bias_a.normal_(0, 0.1, generator=gen)
            layer.scale_a.fill_(0.05)
        out.append(layer.eval())
    return out


def binary_layers(K, N, dt, n, dev, gen):
    from bitorch_engine.layers.qlinear.binary.cuda import BinaryLinearCuda
    proto = BinaryLinearCuda(K, N, dtype=dt)
    proto.weight = None
    proto.to(dev).eval()
    out = []
    for _ in range(n):
        layer = copy.deepcopy(proto)
        layer.qweight = torch.nn.Parameter(torch.randint(0, 256, (N * K // 8,), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8),
                                           requires_grad=False)
        with torch.no_grad():
            layer.bias_a.normal_(0, 0.1, generator=gen)
            layer.scale_a.fill_(0.05)
            layer.scale_w.fill_(0.01)
        out.append(layer)
    return out


def mpq_w2_layers(K, N, dt, n, dev, gen):
    from bitorch_engine.layers.qlinear.nbit.cuda import MPQLinearCuda
    proto = MPQLinearCuda(K, N, w_bit=2, dtype=dt, group_size=128, dq_group_size=32, use_gba_quant=True, asym=False)
    proto.qweight.data = torch.zeros(proto.qweight.shape, dtype=torch.int32)
    proto.prepare_params()
    proto.to(dev).eval()
    out = []
    for _ in range(n):
        layer = copy.deepcopy(proto)
        layer.qweight.data = torch.randint(-2 ** 31, 2 ** 31 - 1, layer.qweight.shape, generator=gen, device=dev, dtype=torch.int32)
        layer.scales = (torch.rand(layer.scales.shape, generator=gen, device=dev) * 0.01 + 0.005).to(dt)
        layer.zeros = (layer.scales.float() * 1.5).to(dt)
        out.append(layer)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one shape, one dtype, fewer rows (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/ternary_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ternary_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import ternary_linear_cuda as tx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "ternary_bench.jsonl"), "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")

    shapes = SHAPES[1:2] if a.quick else SHAPES
    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    rows = (1, 16, 4096) if a.quick else ROWS
    kinds = (("ternary", ternary_layers, lambda K, N: K * N // 4), ("binary", binary_layers, lambda K, N: K * N // 8),
             ("mpq_w2a16", mpq_w2_layers, lambda K, N: K * N // 4))
    for (K, N) in shapes:
        for dt in dts:
            dname = str(dt).replace("torch.", "")
            for kind, make, wbytes in kinds:
                layers = make(K, N, dt, sets_for(wbytes(K, N)), dev, gen)
                for M in rows:
                    x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                    fns = [(lambda l=l: l(x)) for l in layers]
                    with torch.no_grad():
                        us = time_region(fns, max(2, min(50, int(2e4 // (len(fns) * (1 + M // 16))))))
                    byts = wbytes(K, N) + M * K * x.element_size() + M * N * x.element_size()
                    emit({"layer": kind, "dtype": dname, "K": K, "N": N, "M": M, "us": round(us, 2), "GB/s": round(byts / us / 1e3, 1),
                          "roofline": round(byts / HBM / (us * 1e-6), 3), "TOP/s": round(2.0 * M * K * N / us / 1e6, 1)})
                del layers
                torch.cuda.empty_cache()
            # the two forms of the ternary layer, called directly, where both exist
            tl = ternary_layers(K, N, dt, sets_for(K * N // 4), dev, gen)
            imgs = [tx.fp4_image(l.qweight) for l in tl]
            for M in (1, 2, 3, 4):
                x = torch.randn((M, K), generator=gen, device=dev).to(dt)
                with torch.no_grad():
                    dec = time_region([(lambda l=l: tx.linear_fused(x, l.qweight, l.bias_a, l.scale_a, l.scale_w)) for l in tl], 20)
                    mp = time_region([(lambda l=l, i=i: tx.linear_fp4(x, l.qweight, l.bias_a, l.scale_a, l.scale_w, wimage=i)) for l, i in zip(tl, imgs)], 20)
                emit({"forms": "ternary", "dtype": dname, "K": K, "N": N, "M": M, "decode_us": round(dec, 2), "matrix_pipe_us": round(mp, 2),
                      "decode_roofline": round((K * N // 4 + M * (K + N) * x.element_size()) / HBM / (dec * 1e-6), 3)})
            del tl, imgs
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
