"""MX weight gradient (csrc/mx_wgrad.hip) against the layers' torch path, and the sweep over the split count behind the plan rule.

  llama   (N, K) = (4096, 4096), (11008, 4096), (4096, 11008), M in {512, 2048, 8192}, fp16 and bf16, with the bias gradient:
          kernel  mx_grad_weight_cuda.grad_weight(gy, x, bias=True)            (the plan's splits)
          torch   gy.float().t().mm(x.float()).to(dt) and gy.float().sum(0).to(dt)   (the backward's default)
  sweep   shapes with few 128 x 128 tiles, M in {2048, 8192}, fp16, splits forced to 1, 2, 4, ... : the time of each and the plan's choice
Timing: HIP events around `reps` back-to-back calls on one stream (every call is far longer than a launch), the two arms alternating,
the median of five rounds.  Inputs rotate over copies that together exceed the 256 MB Infinity Cache.

  python tools/mx_wgrad_bench.py [--quick] [--part llama|sweep] [--out DIR]     one JSON line per measurement on stdout (and
                                                                                DIR/mx_wgrad_bench.jsonl, appended)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
import torch  # noqa: E402

LLAMA = ((4096, 4096), (11008, 4096), (4096, 11008))  # (N, K)
SWEEP = ((128, 128), (512, 512), (1024, 1024), (2048, 1024), (2048, 2048), (4096, 4096))


def time_arms(arms, reps):
    """arms: lists of callables (one list per arm, a callable per input copy).  Median over five rounds of the mean microseconds per call."""
    us = [[] for _ in arms]
    for fns in arms:
        for f in fns:
            f()
    torch.cuda.synchronize()
    for _ in range(5):
        for i, fns in enumerate(arms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(reps):
                fns[r % len(fns)]()
            e1.record()
            e1.synchronize()
            us[i].append(e0.elapsed_time(e1) * 1e3 / reps)
    return [statistics.median(u) for u in us]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one llama point and one sweep shape, fp16")
    ap.add_argument("--part", default="all", choices=("all", "llama", "sweep"))
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mx_wgrad_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mx_wgrad_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mx_grad_weight_cuda as G
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mx_wgrad_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def inputs(M, N, K, dt):
        n = max(2, min(8, -(-320 * 2 ** 20 // (2 * M * (N + K)))))
        return [(torch.randn((M, N), generator=gen, device=dev).to(dt), torch.randn((M, K), generator=gen, device=dev).to(dt)) for _ in range(n)]

    def reps_for(M, N, K):
        return max(4, min(200, int(2e13 / (2.0 * M * N * K))))

    with torch.no_grad():
        for N, K in (() if a.part == "sweep" else LLAMA[:1] if a.quick else LLAMA):
            for dt in ((torch.float16,) if a.quick else (torch.float16, torch.bfloat16)):
                for M in ((2048,) if a.quick else (512, 2048, 8192)):
                    sets = inputs(M, N, K, dt)
                    kern = [(lambda gy=gy, x=x: G.grad_weight(gy, x, bias=True)) for gy, x in sets]
                    tor = [(lambda gy=gy, x=x: (gy.float().t().mm(x.float()).to(dt), gy.float().sum(0).to(dt))) for gy, x in sets]
                    k_us, t_us = time_arms([kern, tor], reps_for(M, N, K))
                    emit({"part": "llama", "dtype": str(dt).replace("torch.", ""), "N": N, "K": K, "M": M, "splits": G.plan_splits(M, N, K),
                          "kernel_us": round(k_us, 2), "torch_us": round(t_us, 2), "ratio_torch": round(k_us / t_us, 3),
                          "kernel_tflops": round(2.0 * M * K * N / k_us * 1e-6, 1)})
                    del sets, kern, tor
                    torch.cuda.empty_cache()
        for N, K in (() if a.part == "llama" else SWEEP[2:3] if a.quick else SWEEP):
            for M in ((2048,) if a.quick else (2048, 8192)):
                dt = torch.float16
                sets = inputs(M, N, K, dt)
                cand = [s for s in (1, 2, 4, 8, 16, 32, 64) if s <= (M + 31) // 32 and s * ((N + 127) // 128) * ((K + 127) // 128) <= 4096]
                arms = [[(lambda gy=gy, x=x, s=s: G.grad_weight(gy, x, bias=True, splits=s)) for gy, x in sets] for s in cand]
                us = time_arms(arms, reps_for(M, N, K))
                emit({"part": "sweep", "dtype": "float16", "N": N, "K": K, "M": M, "tiles": ((N + 127) // 128) * ((K + 127) // 128),
                      "plan": G.plan_splits(M, N, K), "us_by_splits": {str(s): round(u, 2) for s, u in zip(cand, us)}})
                del sets, arms
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
