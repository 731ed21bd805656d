"""MXFP4 mixture-of-experts expert GEMM (csrc/mxfp4_moe.hip) against the only route the library had before it: a loop over the experts
around mxfp4_linear_cuda.forward with the routing read on the host (idx.cpu(), gather, call, scatter), in one process.

gpt-oss-20b's two expert projections (E = 32, top-4; 2880 -> 5760 with x per token, 2880 -> 2880 with x per pair), fp16 and bf16:
  accept   T in {1, 16, 256, 4096}: the new path (its own plan) and the loop, both timed eagerly with events (the loop synchronises
           with the host, so it cannot be captured), the median of the rounds; the ratio new / loop; the new path's graph time as well.
           T = 1: GB/s over the qweight + scales bytes of the S selected experts and the share of 8 TB/s; T = 4096: TFLOP/s over 2 P N K.
  sweep    P in {1, 2, 4, ..., 256} pairs, both forms (forced), graph time; also at E = 128 (2880 -> 5760): what the plan's bound in
           mxfp4_moe.hip rests on.
Every call of a round uses another routing and the rounds alternate between weight stacks, so that the experts a round reads exceed the
256 MB Infinity Cache where the stacks do (decode numbers are HBM numbers).

  python tools/mxfp4_moe_bench.py [--quick] [--out DIR]     one JSON line per measurement on stdout (and DIR/mxfp4_moe_bench.jsonl)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mxfp4_bench import time_graph  # noqa: E402

HBM = 8.0e12
PROJ = (("gate_up", 2880, 5760, 0), ("down", 2880, 2880, 1))  # name, K, N, x_per_pair
SWEEP_P = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def stacks(E, N, K, n, dev, gen):
    from bitorch_engine.extensions import mxfp4_experts_cuda as moe
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (E, N, K // 2), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (E, N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, moe.col_exp(s)))
    return out


def routings(T, S, E, n, dev, gen):
    """n routings of T tokens: the top-S of uniform random logits (distinct experts per token), int32 [T, S]."""
    return [torch.rand((T, E), generator=gen, device=dev).topk(S, dim=-1).indices.to(torch.int32) for _ in range(n)]


def loop_forward(mx, x, idx, q, s, e_col, N):
    """The route of the library before the expert kernels: the routing read on the host, one mxfp4_linear_cuda.forward per expert."""
    T, S = idx.shape
    K = q.shape[2] * 2
    flat = idx.reshape(-1).cpu()
    xr = (x if x.dim() == 3 else x[:, None, :].expand(T, S, K)).reshape(T * S, K)
    y = torch.zeros((T * S, N), dtype=x.dtype, device=x.device)
    for e in flat.unique().tolist():
        if 0 <= e < q.shape[0]:
            sel = (flat == e).nonzero().reshape(-1).to(x.device)
            y[sel] = mx.forward(xr[sel].contiguous(), q[e], s[e], None, e_col[e])
    return y.reshape(T, S, N)


def time_eager(fns, rounds=7):
    """Median over the rounds of the mean microseconds per call, events around each round of eager calls."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for f in fns:
            f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / len(fns))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="accept rows T = 1 and T = 4096 of gate_up in bf16 only (for a profiler run)")
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp4_moe_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mxfp4_moe_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_experts_cuda as moe
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp4_moe_bench.jsonl"), "w")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")

    def x_for(T, S, K, xpp, dt):
        return torch.randn((T, S, K) if xpp else (T, K), generator=gen, device=dev).to(dt)

    E, S = 32, 4
    dts = (torch.bfloat16,) if a.quick else (torch.float16, torch.bfloat16)
    with torch.no_grad():
        for name, K, N, xpp in (PROJ[:1] if a.quick else PROJ):
            st = stacks(E, N, K, 2, dev, gen)
            for dt in dts:
                dname = str(dt).replace("torch.", "")
                for T in ((1, 4096) if a.quick else (1, 16, 256, 4096)):
                    P, n = T * S, 16 if T <= 16 else 4
                    x, idxs = x_for(T, S, K, xpp, dt), routings(T, S, E, n, dev, gen)
                    new = [(lambda i=i, w=st[j % 2]: moe.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)]
                    old = [(lambda i=i, w=st[j % 2]: loop_forward(mx, x, i, w[0], w[1], w[2], N)) for j, i in enumerate(idxs)]
                    new_us, loop_us = time_eager(new), time_eager(old)
                    graph_us = time_graph(new, 240 if T <= 16 else 24)
                    row = {"part": "accept", "proj": name, "dtype": dname, "E": E, "S": S, "K": K, "N": N, "T": T, "form": moe.form(P, E, N, K, dt),
                           "new_us": round(new_us, 2), "loop_us": round(loop_us, 2), "ratio": round(new_us / loop_us, 3), "new_graph_us": round(graph_us, 2)}
                    if T == 1:
                        gbs = S * (N * K // 2 + N * K // 32) / (graph_us * 1e-6) / 1e9
                        row.update(gbs=round(gbs, 1), hbm_share=round(gbs * 1e9 / HBM, 3))
                    if T == 4096:
                        row.update(tflops=round(2.0 * P * N * K / graph_us * 1e-6, 1))
                    emit(row)
            del st
            torch.cuda.empty_cache()
        if not a.quick:
            for E, (name, K, N, xpp) in ((32, PROJ[0]), (32, PROJ[1]), (128, PROJ[0])):
                st = stacks(E, N, K, 2 if E == 32 else 1, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for P in SWEEP_P:
                        T, Sp = (1, P) if P < S else (P // S, S)
                        x, idxs = x_for(T, Sp, K, xpp, dt), routings(T, Sp, E, 16, dev, gen)
                        row = {"part": "sweep", "proj": name, "dtype": dname, "E": E, "S": Sp, "K": K, "N": N, "P": P, "plan": moe.form(P, E, N, K, dt)}
                        for form, key in ((0, "decode_us"), (1, "grouped_us")):
                            fns = [(lambda i=i, w=st[j % len(st)]: moe.forward(x, i, w[0], w[1], None, w[2], form=form)) for j, i in enumerate(idxs)]
                            row[key] = round(time_graph(fns, 96), 2)
                        emit(row)
                del st
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
