"""MXFP6 input gradient (csrc/mxfp6_grad.hip) against two arms, in one process: time and peak bytes.

  (a) the "torch" path of the same layers' backward (the parent commit's backward, unchanged);
  (b) the MXFP4 input gradient (mxfp4_linear_cuda.grad_input / mxfp4_experts_cuda.grad_input) on an FP4 weight of the same shape: the MFMA
      count is the same, so at M = 4096 this ratio should be near 1.0; the excess is the 16-bit LDS image and the 32-n stage.

  dense    (K, N) = (4096, 4096), (4096, 11008), (11008, 4096), M in {256, 1024, 4096}: grad_x of MXFP6A8LinearCuda's backward
           kernel  blk_exp(scales) + grad_input(gy, qweight, scales, e_blk)
           torch   gy.float().mm(dequant(qweight, scales, float32)).to(dtype)
  experts  E = 32, 2880 -> 5760 and 2880 -> 2880, top-4, T in {256, 4096}, x [T, K]: grad_x of MXFP6A8ExpertsLinearCuda's backward
           kernel  blk_exp + grad_input(..., out_dtype=float32), the sum over a token's slots, one rounding
           torch   dequant of all [E, N, K] to fp32 and the loop over the experts (a host synchronisation per expert)
The columns restate the lines of the layers' backward, so that they can be called without an autograd graph.
Timing: the calls of `reps` rounds over enough weight sets that one round exceeds the 256 MB Infinity Cache are captured in one HIP graph;
HIP events around its replay give device time without the host's launch floor.  The experts' torch path synchronises with the host and
cannot be captured: it is timed eagerly between HIP events, host stalls included (its row says timing = "eager").
Peak bytes: torch.cuda.max_memory_allocated over one eager call, above what was allocated before it.

  python tools/mxfp6_grad_bench.py [--quick] [--part dense|experts] [--out DIR]   one JSON line per measurement on stdout (and
                                                                                 DIR/mxfp6_grad_bench.jsonl, appended)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402

MFMA_PEAK = 2.5e15
DENSE = ((4096, 4096), (4096, 11008), (11008, 4096))  # (K, N)
EXPERTS = ((2880, 5760), (2880, 2880))
E, TOP = 32, 4


def sets_for(nbytes, cap=48):
    return max(2, min(cap, -(-512 * 2 ** 20 // nbytes)))


def time_graph(fns, calls=96):
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


def time_eager(fns, reps=2):
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
    """grad_x of experts_a8_backward with grad_input="torch" (need_x alone, x [T, K])."""
    from bitorch_engine.extensions import mxfp6_experts_a8_cuda as ex
    En, N, K = q.shape[0], q.shape[1], s.shape[2] * 32
    T, S = idx.shape
    g = gy.reshape(T * S, N).float()
    flat = idx.reshape(-1).long()
    gx = torch.zeros((T * S, K), dtype=torch.float32, device=gy.device)
    W = ex.dequant(q, s, torch.float32)
    for e in range(En):
        rows = (flat == e).nonzero().reshape(-1)
        if rows.numel() == 0:
            continue
        gx[rows] = g[rows].mm(W[e])
    return gx.reshape(T, S, K).sum(1).to(gy.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one dense and one experts point, fp16 (for a profiler run)")
    ap.add_argument("--part", default="all", choices=("all", "dense", "experts"))
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mxfp6_grad_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp6_grad_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_experts_cuda as ex4, mxfp4_linear_cuda as mx4
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as mx, mxfp6_experts_a8_cuda as ex
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp6_grad_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def u8(lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)

    dts = (torch.float16,) if a.quick else (torch.float16, torch.bfloat16)
    with torch.no_grad():
        for K, N in (() if a.part == "experts" else DENSE[1:2] if a.quick else DENSE):
            packed = N * K // 32 * 24 + N * K // 32
            ns = sets_for(packed)
            sets = [(u8(0, 256, N, K // 32 * 24), u8(119, 131, N, K // 32)) for _ in range(ns)]
            sets4 = [(u8(0, 256, N, K // 2), s) for _, s in sets]
            for dt in dts:
                for M in ((1024,) if a.quick else (256, 1024, 4096)):
                    gy = torch.randn((M, N), generator=gen, device=dev).to(dt)
                    n = min(len(sets), 4 if M >= 1024 else len(sets))
                    calls = 24 if M >= 4096 else 48 if M >= 1024 else 96
                    kern = [(lambda q=q, s=s: mx.grad_input(gy, q, s, mx.blk_exp(s))) for q, s in sets[:n]]
                    fp4 = [(lambda q=q, s=s: mx4.grad_input(gy, q, s, mx4.blk_exp(s))) for q, s in sets4[:n]]
                    tor = [(lambda q=q, s=s: gy.float().mm(mx.dequant(q, s, torch.float32)).to(dt)) for q, s in sets[:n]]
                    k_us, t_us, f_us = time_graph(kern, calls), time_graph(tor, calls), time_graph(fp4, calls)
                    fl = 2.0 * M * K * N
                    emit({"part": "dense", "dtype": str(dt).replace("torch.", ""), "K": K, "N": N, "M": M, "kernel_us": round(k_us, 2),
                          "torch_us": round(t_us, 2), "mxfp4_us": round(f_us, 2), "ratio_torch": round(k_us / t_us, 3),
                          "ratio_mxfp4": round(k_us / f_us, 3), "kernel_tflops": round(fl / k_us * 1e-6, 1),
                          "kernel_peak_share": round(fl / MFMA_PEAK / (k_us * 1e-6), 3), "kernel_peak_bytes": peak_bytes(kern[0]),
                          "torch_peak_bytes": peak_bytes(tor[0]), "packed_bytes": packed})
            del sets, sets4
            torch.cuda.empty_cache()
        for K, N in (() if a.part == "dense" else EXPERTS[:1] if a.quick else EXPERTS):
            packed = E * (N * K // 32 * 24 + N * K // 32)
            ns = sets_for(packed)
            sets = [(u8(0, 256, E, N, K // 32 * 24), u8(119, 131, E, N, K // 32)) for _ in range(ns)]
            sets4 = [(u8(0, 256, E, N, K // 2), s) for _, s in sets]
            for dt in dts:
                for T in ((256,) if a.quick else (256, 4096)):
                    gy = torch.randn((T, TOP, N), generator=gen, device=dev).to(dt)
                    idx = torch.stack([torch.randperm(E, generator=gen, device=dev)[:TOP] for _ in range(T)]).to(torch.int32)
                    kern = [(lambda q=q, s=s: ex.grad_input(gy, idx, q, s, ex.blk_exp(s), out_dtype=torch.float32).reshape(T, TOP, K).sum(1).to(dt))
                            for q, s in sets]
                    fp4 = [(lambda q=q, s=s: ex4.grad_input(gy, idx, q, s, ex4.blk_exp(s), out_dtype=torch.float32).reshape(T, TOP, K).sum(1).to(dt))
                           for q, s in sets4]
                    tor = [(lambda q=q, s=s: experts_torch(gy, idx, q, s)) for q, s in sets]
                    calls = 24 if T >= 4096 else 48
                    k_us, f_us, t_us = time_graph(kern, calls), time_graph(fp4, calls), time_eager(tor, 1)
                    fl = 2.0 * T * TOP * K * N
                    emit({"part": "experts", "dtype": str(dt).replace("torch.", ""), "E": E, "K": K, "N": N, "T": T, "S": TOP, "kernel_us": round(k_us, 2),
                          "torch_us": round(t_us, 2), "torch_timing": "eager", "mxfp4_us": round(f_us, 2), "ratio_torch": round(k_us / t_us, 3),
                          "ratio_mxfp4": round(k_us / f_us, 3), "kernel_tflops": round(fl / k_us * 1e-6, 1),
                          "kernel_peak_bytes": peak_bytes(kern[0]), "torch_peak_bytes": peak_bytes(tor[0]), "packed_bytes": packed})
            del sets, sets4
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
