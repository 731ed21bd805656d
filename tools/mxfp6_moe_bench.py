"""MXFP6 W6A16 mixture-of-experts expert GEMM (csrc/mxfp6_moe.hip) in one process, everything that is timed captured in one graph and
replayed 7 times (the median, with the fastest and slowest replay beside it; tools/mxfp6_bench.py's time_graph).  Every call of a
round uses another routing and the rounds alternate between weight stacks, so that the experts a round reads exceed the 256 MB Infinity
Cache where the stacks do (decode numbers are HBM numbers).  gpt-oss-20b's two expert projections (2880 -> 5760 with x per token,
2880 -> 2880 with x per pair):

  sweep    P in {1, 2, 4, ..., 256} pairs, both forms (forced), at E = 32 on both projections and at E = 128 on 2880 -> 5760, fp16 and bf16:
           what the plan's bounds in mxfp6_moe.hip rest on
  decode   P in {4, 16, 64} (T = P / 4 tokens, top-4 of E = 32): microseconds and GB/s over the touched experts' qweight + scales bytes,
           beside the MXFP4 experts (mxfp4_experts_cuda) and the W6A8 experts (mxfp6_experts_a8_cuda, its activation quantiser included)
  prefill  T in {256, 4096}, S = 4: microseconds and TFLOP/s over 2 P N K, beside the same two, and beside the route without this layer:
           dequant of the stack to the dtype plus a per-expert torch loop with the routing read on the host (timed eagerly with events:
           it synchronises with the host and cannot be captured)
  pmc      a few calls of the grouped form alone (T = 4096, 2880 -> 5760, fp16) for a counter run of rocprofv3

  python tools/mxfp6_moe_bench.py [--part sweep,decode,prefill] [--out DIR]    one JSON line per measurement on stdout (and appended to
                                                                               DIR/mxfp6_moe_bench.jsonl)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mxfp6_bench import put, time_graph  # noqa: E402

PROJ = (("gate_up", 2880, 5760, 0), ("down", 2880, 2880, 1))  # name, K, N, x_per_pair
SWEEP_P = (1, 2, 4, 8, 16, 32, 64, 128, 256)
S = 4


def stacks6(E, N, K, n, dev, gen):
    from bitorch_engine.extensions import mxfp6_experts_cuda as moe
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (E, N, K // 32 * 24), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (E, N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, moe.col_exp(s)))
    return out


def stacks4(E, N, K, n, dev, gen):
    from bitorch_engine.extensions import mxfp4_experts_cuda as moe4
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (E, N, K // 2), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (E, N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, moe4.col_exp(s)))
    return out


def routings(T, Sl, E, n, dev, gen):
    """n routings of T tokens: the top-Sl of uniform random logits (distinct experts per token), int32 [T, Sl]."""
    return [torch.rand((T, E), generator=gen, device=dev).topk(Sl, dim=-1).indices.to(torch.int32) for _ in range(n)]


def touched(idxs, E):
    """Mean number of distinct experts a call reads."""
    return statistics.mean(int(i.reshape(-1).unique().numel()) for i in idxs)


def loop_forward(moe, x, idx, q, s, N, dt):
    """The route without the layer: a dtype image of every expert, the routing read on the host, one torch matmul per expert."""
    T, Sl = idx.shape
    W = moe.dequant(q, s, dt)
    K = W.shape[2]
    flat = idx.reshape(-1).cpu()
    xr = (x if x.dim() == 3 else x[:, None, :].expand(T, Sl, K)).reshape(T * Sl, K)
    y = torch.zeros((T * Sl, N), dtype=dt, device=x.device)
    for e in flat.unique().tolist():
        if 0 <= e < q.shape[0]:
            sel = (flat == e).nonzero().reshape(-1).to(x.device)
            y[sel] = xr[sel] @ W[e].t()
    return y.reshape(T, Sl, N)


def time_eager(fns, rounds=7):
    """(median, fastest, slowest) over the rounds of the mean microseconds per call, events around each round of eager calls."""
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
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="sweep,decode,prefill")
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mxfp6_moe_bench.jsonl")
    a = ap.parse_args()
    parts = a.part.split(",")
    assert torch.cuda.is_available(), "mxfp6_moe_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_experts_cuda as moe4
    from bitorch_engine.extensions import mxfp6_experts_a8_cuda as moe68
    from bitorch_engine.extensions import mxfp6_experts_cuda as moe
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp6_moe_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def x_for(T, Sl, K, xpp, dt):
        return torch.randn((T, Sl, K) if xpp else (T, K), generator=gen, device=dev).to(dt)

    dts = (torch.float16, torch.bfloat16)
    with torch.no_grad():
        if "pmc" in parts:
            name, K, N, xpp = PROJ[0]
            st = stacks6(32, N, K, 1, dev, gen)[0]
            x, idx = x_for(4096, S, K, xpp, torch.float16), routings(4096, S, 32, 1, dev, gen)[0]
            for _ in range(3):
                moe.forward(x, idx, st[0], st[1], None, st[2], form=1)
            torch.cuda.synchronize()
            counts = torch.bincount(idx.reshape(-1).long(), minlength=32)
            emit({"part": "pmc", "proj": name, "dtype": "float16", "E": 32, "S": S, "K": K, "N": N, "T": 4096, "calls": 3,
                  "row_tiles": int(((counts + 127) // 128).sum()), "col_tiles": (N + 127) // 128, "stages": (K + 63) // 64,
                  "grid": (4096 * S // 128 + 32 + 1) * ((N + 127) // 128)})
        if "sweep" in parts:
            for E, (name, K, N, xpp) in ((32, PROJ[0]), (32, PROJ[1]), (128, PROJ[0])):
                st = stacks6(E, N, K, 2 if E == 32 else 1, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for P in SWEEP_P:
                        T, Sp = (1, P) if P < S else (P // S, S)
                        x, idxs = x_for(T, Sp, K, xpp, dt), routings(T, Sp, E, 16, dev, gen)
                        row = {"part": "sweep", "proj": name, "dtype": dname, "E": E, "S": Sp, "K": K, "N": N, "P": P, "plan": moe.form(P, E, N, K, dt)}
                        for form, key in ((0, "decode"), (1, "grouped")):
                            fns = [(lambda i=i, w=st[j % len(st)]: moe.forward(x, i, w[0], w[1], None, w[2], form=form)) for j, i in enumerate(idxs)]
                            put(row, key, time_graph(fns, 96))
                        emit(row)
                del st
                torch.cuda.empty_cache()
        for part, Ts in (("decode", (1, 4, 16)), ("prefill", (256, 4096))):
            if part not in parts:
                continue
            E = 32
            for name, K, N, xpp in PROJ:
                st6, st4 = stacks6(E, N, K, 2, dev, gen), stacks4(E, N, K, 2, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for T in Ts:
                        P, n = T * S, 16 if part == "decode" else 4
                        x, idxs = x_for(T, S, K, xpp, dt), routings(T, S, E, n, dev, gen)
                        calls = 96 if part == "decode" else 16
                        row = {"part": part, "proj": name, "dtype": dname, "E": E, "S": S, "K": K, "N": N, "T": T, "P": P, "form": moe.form(P, E, N, K, dt),
                               "form_w4": moe4.form(P, E, N, K, dt), "form_w6a8": moe68.form(P, E, N, K, dt)}
                        put(row, "w6a16", time_graph([(lambda i=i, w=st6[j % 2]: moe.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)], calls))
                        put(row, "w4a16", time_graph([(lambda i=i, w=st4[j % 2]: moe4.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)], calls))
                        put(row, "w6a8", time_graph([(lambda i=i, w=st6[j % 2]: moe68.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)], calls))
                        if part == "decode":
                            n_e = touched(idxs, E)
                            row["experts_touched"] = round(n_e, 2)
                            row["w6a16_gbs"] = round(n_e * (N * K * 3 // 4 + N * K // 32) / (row["w6a16_us"] * 1e-6) / 1e9, 1)
                            row["w4a16_gbs"] = round(n_e * (N * K // 2 + N * K // 32) / (row["w4a16_us"] * 1e-6) / 1e9, 1)
                            row["w6a8_gbs"] = round(n_e * (N * K * 3 // 4 + N * K // 32) / (row["w6a8_us"] * 1e-6) / 1e9, 1)
                        else:
                            put(row, "dequant_loop", time_eager([(lambda i=i, w=st6[j % 2]: loop_forward(moe, x, i, w[0], w[1], N, dt)) for j, i in enumerate(idxs)], 3))
                            for k in ("w6a16", "w4a16", "w6a8", "dequant_loop"):
                                row[k + "_tflops"] = round(2.0 * P * N * K / row[k + "_us"] * 1e-6, 1)
                        emit(row)
                del st6, st4
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
