"""MXFP8 input gradient (csrc/mxfp8_grad.hip) against two arms, in one process: time and peak bytes.

  (i)  the "torch" path of the same layers' backward (the backward before the kernel existed, still the layers' default): an fp32 image
       of W and mm;
  (ii) the MXFP6 input gradient (mxfp6_a8_linear_cuda.grad_input / mxfp6_experts_a8_cuda.grad_input) on an FP6 weight of the same shape
       and scales: the MFMA count is the same; that kernel stages a 16-bit image in 32-n stages, this one packed units in 64-n stages.

  dense    (K, N) = (4096, 4096), (4096, 11008), (2880, 5760), M in {128, 1024, 4096}: grad_x of MXFP8LinearCuda's backward
           kernel  blk_exp(scales) + grad_input(gy, qweight, scales, e_blk)
           torch   gy.float().mm(dequant(qweight, scales, float32)).to(dtype)
  experts  E = 32, 2880 -> 5760 and 2880 -> 2880, top-4, T = 1024, x [T, K]: grad_x of MXFP8ExpertsLinearCuda's backward
           kernel  experts_blk_exp + experts_grad_input(..., out_dtype=float32), the sum over a token's slots, one rounding
           torch   dequant of all [E, N, K] to fp32 and the loop over the experts (a host synchronisation per expert)
Timing: the calls of `reps` rounds over weight sets that together exceed the 256 MB Infinity Cache are captured in one HIP graph; HIP
events around each of five replays give device time without the host's launch floor, and the median is kept.  The experts' torch path
synchronises with the host and cannot be captured: it is timed eagerly between HIP events, host stalls included (timing = "eager").
Peak bytes: torch.cuda.max_memory_allocated over one eager call, above what was allocated before it.

  python tools/mxfp8_grad_bench.py [--quick] [--part dense|experts] [--out DIR]   one JSON line per measurement on stdout (and
                                                                                 DIR/mxfp8_grad_bench.jsonl, appended)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402

DENSE = ((4096, 4096), (4096, 11008), (2880, 5760))  # (K, N)
EXPERTS = ((2880, 5760), (2880, 2880))
E, TOP, T = 32, 4, 1024


def time_graph(fns, calls):
    """Median over five replays of the mean device microseconds per call of `fns`, called round-robin inside one captured graph."""
    reps = max(1, calls // len(fns))
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            for f in fns:
                f()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / (reps * len(fns)))
    del g
    return statistics.median(us)


def time_eager(fns):
    for f in fns[:1]:
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for f in fns:
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(fns)


def peak_bytes(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def experts_torch(gy, idx, q, s):
    """grad_x of MXFP8ExpertsLinearForward.backward with grad_input = "torch" (need_x alone, x [T, K])."""
    from bitorch_engine.extensions import mxfp8_experts_cuda as ex
    En, N, K = q.shape[0], q.shape[1], s.shape[2] * 32
    P = idx.numel()
    g = gy.reshape(P, N).float()
    flat = idx.reshape(-1).long()
    gx = torch.zeros((P, K), dtype=torch.float32, device=gy.device)
    W = ex.dequant(q, s, torch.float32)
    for e in range(En):
        rows = (flat == e).nonzero().reshape(-1)
        if rows.numel() == 0:
            continue
        gx[rows] = g[rows].mm(W[e])
    return gx.reshape(idx.shape[0], idx.shape[1], K).sum(1).to(gy.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one dense and one experts point, fp16")
    ap.add_argument("--part", default="all", choices=("all", "dense", "experts"))
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mxfp8_grad_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp8_grad_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as mx6, mxfp6_experts_a8_cuda as ex6
    from bitorch_engine.extensions import mxfp8_experts_cuda as ex8, mxfp8_grad_cuda as g8, mxfp8_linear_cuda as mx8
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp8_grad_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def u8(lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)

    def codes(*shape):  # every E4M3 byte but the NaN codes
        q = u8(0, 256, *shape)
        return torch.where((q & 0x7F) == 0x7F, q - 1, q)

    def nsets(nbytes):
        return max(2, min(12, -(-320 * 2 ** 20 // nbytes)))

    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    with torch.no_grad():
        for K, N in (() if a.part == "experts" else DENSE[:1] if a.quick else DENSE):
            packed = N * K + N * K // 32
            sets = [(codes(N, K), u8(124, 130, N, K // 32)) for _ in range(nsets(packed))]
            sets6 = [(u8(0, 256, N, K // 32 * 24), s) for _, s in sets]
            for dt in dts:
                for M in ((1024,) if a.quick else (128, 1024, 4096)):
                    gy = torch.randn((M, N), generator=gen, device=dev).to(dt)
                    n = min(len(sets), 4 if M >= 1024 else len(sets))
                    calls = 8 if M >= 4096 else 16 if M >= 1024 else 48
                    kern = [(lambda q=q, s=s: g8.grad_input(gy, q, s, g8.blk_exp(s))) for q, s in sets[:n]]
                    fp6 = [(lambda q=q, s=s: mx6.grad_input(gy, q, s, mx6.blk_exp(s))) for q, s in sets6[:n]]
                    tor = [(lambda q=q, s=s: gy.float().mm(mx8.dequant(q, s, torch.float32)).to(dt)) for q, s in sets[:n]]
                    k_us, t_us, f_us = time_graph(kern, calls), time_graph(tor, calls), time_graph(fp6, calls)
                    emit({"part": "dense", "dtype": str(dt).replace("torch.", ""), "K": K, "N": N, "M": M, "kernel_us": round(k_us, 2),
                          "torch_us": round(t_us, 2), "mxfp6_us": round(f_us, 2), "ratio_torch": round(k_us / t_us, 3),
                          "ratio_mxfp6": round(k_us / f_us, 3), "kernel_tflops": round(2.0 * M * K * N / k_us * 1e-6, 1),
                          "kernel_peak_bytes": peak_bytes(kern[0]), "torch_peak_bytes": peak_bytes(tor[0]), "packed_bytes": packed})
            del sets, sets6
            torch.cuda.empty_cache()
        for K, N in (() if a.part == "dense" else EXPERTS[:1] if a.quick else EXPERTS):
            packed = E * (N * K + N * K // 32)
            sets = [(codes(E, N, K), u8(124, 130, E, N, K // 32)) for _ in range(2)]
            sets6 = [(u8(0, 256, E, N, K // 32 * 24), s) for _, s in sets]
            for dt in dts:
                gy = torch.randn((T, TOP, N), generator=gen, device=dev).to(dt)
                idx = torch.stack([torch.randperm(E, generator=gen, device=dev)[:TOP] for _ in range(T)]).to(torch.int32)
                kern = [(lambda q=q, s=s: g8.experts_grad_input(gy, idx, q, s, g8.experts_blk_exp(s), out_dtype=torch.float32)
                         .reshape(T, TOP, K).sum(1).to(dt)) for q, s in sets]
                fp6 = [(lambda q=q, s=s: ex6.grad_input(gy, idx, q, s, ex6.blk_exp(s), out_dtype=torch.float32).reshape(T, TOP, K).sum(1).to(dt))
                       for q, s in sets6]
                tor = [(lambda q=q, s=s: experts_torch(gy, idx, q, s)) for q, s in sets]
                k_us, f_us, t_us = time_graph(kern, 8), time_graph(fp6, 8), time_eager(tor)
                emit({"part": "experts", "dtype": str(dt).replace("torch.", ""), "E": E, "K": K, "N": N, "T": T, "S": TOP, "kernel_us": round(k_us, 2),
                      "torch_us": round(t_us, 2), "torch_timing": "eager", "mxfp6_us": round(f_us, 2), "ratio_torch": round(k_us / t_us, 3),
                      "ratio_mxfp6": round(k_us / f_us, 3), "kernel_tflops": round(2.0 * T * TOP * K * N / k_us * 1e-6, 1),
                      "kernel_peak_bytes": peak_bytes(kern[0]), "torch_peak_bytes": peak_bytes(tor[0]), "packed_bytes": packed})
            del sets, sets6
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
