"""MXFP8 W8A16 mixture-of-experts expert GEMM (csrc/mxfp8_moe.hip) in one process, everything that is timed captured in one graph and
replayed 7 times (the median, with the fastest and slowest replay and their spread in per cent of the median beside it;
tools/mxfp6_bench.py's time_graph).  Every call of a round uses another routing and the rounds alternate between weight stacks, so that
the experts a round reads exceed the 256 MB Infinity Cache where the stacks do (decode numbers are HBM numbers).  The shapes, routings
and the dequant + loop route are tools/mxfp6_moe_bench.py's: gpt-oss-20b's two expert projections (2880 -> 5760 with x per token,
2880 -> 2880 with x per pair):

  sweep    P in {1, 2, 4, ..., 1024} pairs (up to the decode form's last P), both forms (forced), at E = 32 on both projections and at
           E = 128 on 2880 -> 5760, fp16 and bf16: what the plan's bounds in mxfp8_moe.hip rest on
  compare  P in {4, 16, 64} (T = P / 4 tokens) and T in {256, 4096}, top-4 of E = 32, the plan's form: microseconds beside the MXFP6
           experts (mxfp6_experts_cuda; 3/4 of the weight bytes) and beside the route without this layer: dequant of the stack to the
           dtype plus a per-expert torch loop with the routing read on the host (timed eagerly with events: it synchronises with the
           host and cannot be captured); GB/s over the touched experts' qweight + scales bytes up to P = 64, TFLOP/s over 2 P N K beyond

  python tools/mxfp8_moe_bench.py [--part sweep,compare] [--out DIR]    one JSON line per measurement on stdout (and appended to
                                                                        DIR/mxfp8_moe_bench.jsonl)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mxfp6_bench import time_graph  # noqa: E402
from mxfp6_moe_bench import PROJ, S, loop_forward, routings, stacks6, time_eager, touched  # noqa: E402

SWEEP_P = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)


def put(row, key, t):
    """median, fastest, slowest, and slowest - fastest in per cent of the median"""
    row[key + "_us"], row[key + "_min"], row[key + "_max"] = round(t[0], 2), round(t[1], 2), round(t[2], 2)
    row[key + "_spread_pct"] = round(100.0 * (t[2] - t[1]) / t[0], 1)


def stacks8(E, N, K, n, dev, gen):
    from bitorch_engine.extensions import mxfp8_experts_cuda as moe
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (E, N, K), generator=gen, device=dev, dtype=torch.int32)
        q = torch.where((q & 0x7F) == 0x7F, q - 1, q).to(torch.uint8)  # no E4M3 NaN code
        s = torch.randint(118, 131, (E, N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        out.append((q, s, moe.col_exp(s)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="sweep,compare")
    ap.add_argument("--out", default=None, help="also append the lines to DIR/mxfp8_moe_bench.jsonl")
    a = ap.parse_args()
    parts = a.part.split(",")
    assert torch.cuda.is_available(), "mxfp8_moe_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp6_experts_cuda as moe6
    from bitorch_engine.extensions import mxfp8_experts_cuda as moe
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp8_moe_bench.jsonl"), "a")

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
        if "sweep" in parts:
            for E, (name, K, N, xpp) in ((32, PROJ[0]), (32, PROJ[1]), (128, PROJ[0])):
                st = stacks8(E, N, K, 2 if E == 32 else 1, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for P in SWEEP_P:
                        T, Sp = (1, P) if P < S else (P // S, S)
                        n = 16 if P <= 64 else 4
                        x, idxs = x_for(T, Sp, K, xpp, dt), routings(T, Sp, E, n, dev, gen)
                        row = {"part": "sweep", "proj": name, "dtype": dname, "E": E, "S": Sp, "K": K, "N": N, "P": P, "plan": moe.form(P, E, N, K, dt)}
                        for form, key in ((0, "decode"), (1, "grouped")):
                            fns = [(lambda i=i, w=st[j % len(st)]: moe.forward(x, i, w[0], w[1], None, w[2], form=form)) for j, i in enumerate(idxs)]
                            put(row, key, time_graph(fns, 96 if P <= 64 else 16))
                        emit(row)
                del st
                torch.cuda.empty_cache()
        if "compare" in parts:
            E = 32
            for name, K, N, xpp in PROJ:
                st8, st6 = stacks8(E, N, K, 2, dev, gen), stacks6(E, N, K, 2, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for T in (1, 4, 16, 256, 4096):
                        P, small = T * S, T <= 16
                        n, calls = (16, 96) if small else (4, 16)
                        x, idxs = x_for(T, S, K, xpp, dt), routings(T, S, E, n, dev, gen)
                        row = {"part": "compare", "proj": name, "dtype": dname, "E": E, "S": S, "K": K, "N": N, "T": T, "P": P,
                               "form": moe.form(P, E, N, K, dt), "form_w6": moe6.form(P, E, N, K, dt)}
                        put(row, "w8a16", time_graph([(lambda i=i, w=st8[j % 2]: moe.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)], calls))
                        put(row, "w6a16", time_graph([(lambda i=i, w=st6[j % 2]: moe6.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)], calls))
                        put(row, "dequant_loop", time_eager([(lambda i=i, w=st8[j % 2]: loop_forward(moe, x, i, w[0], w[1], N, dt)) for j, i in enumerate(idxs[:4])], 3))
                        row["w8_over_w6"] = round(row["w8a16_us"] / row["w6a16_us"], 3)
                        row["w8_over_loop"] = round(row["w8a16_us"] / row["dequant_loop_us"], 4)
                        if small:
                            n_e = touched(idxs, E)
                            row["experts_touched"] = round(n_e, 2)
                            row["w8a16_gbs"] = round(n_e * (N * K + N * K // 32) / (row["w8a16_us"] * 1e-6) / 1e9, 1)
                            row["w6a16_gbs"] = round(n_e * (N * K * 3 // 4 + N * K // 32) / (row["w6a16_us"] * 1e-6) / 1e9, 1)
                        else:
                            for k in ("w8a16", "w6a16", "dequant_loop"):
                                row[k + "_tflops"] = round(2.0 * P * N * K / row[k + "_us"] * 1e-6, 1)
                        emit(row)
                del st8, st6
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
