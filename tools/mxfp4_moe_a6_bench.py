"""MXFP4 W4A6 expert GEMM (csrc/mxfp4_moe_a6.hip) against the MXFP4 W4A8 and W4A4 expert GEMMs (csrc/mxfp4_moe_a8.hip,
csrc/mxfp4_moe_a4.hip; mxfp4_experts_a8_cuda.forward, mxfp4_experts_a4_cuda.forward) in one process: the same weights, routings and
activations; only the activation format differs.  The method is tools/mxfp6_moe_a6_bench.py's.

gpt-oss-20b's two expert projections (top-4; 2880 -> 5760 with x per token, 2880 -> 2880 with x per pair), fp16 and bf16:
  tile     T in {64, 256, 4096} at E = 32 and E = 128: the grouped form on 128 x 128 tiles against 128 x 64 tiles (BIE_MXFP4_MOE_A6_WN = 2 / 1
           under BIE_TUNING; the knob is read when the graph is captured).  What the shipped tile width rests on.
  sweep    P in {1, 2, 4, ..., 1024} pairs, both forms of the new path (forced), at E = 32 and E = 128, both projections: what the plan's
           bound in mxfp4_moe_a6.hip rests on.
  accept   T in {1, 16, 256, 4096} at E = 32: the new path under its own plan, the activation quantiser included, beside the W4A8 and
           the W4A4 paths under their own plans.  Each arm is one captured graph; the three graphs are replayed alternately, round by
           round; the medians over the rounds, their ratios, and the spread (max - min) / median of each arm across the rounds.
           T = 1: GB/s over the MXFP4 qweight + scales bytes of the S selected experts; T = 4096: TFLOP/s over 2 P N K.
Every call of a round uses another routing and the calls alternate between weight stacks, so that the experts a round reads exceed the
256 MB Infinity Cache where the stacks do (decode numbers are HBM numbers).

  python tools/mxfp4_moe_a6_bench.py [--quick] [--part tile|sweep|accept|all] [--out DIR]
one JSON line per measurement on stdout (and DIR/mxfp4_moe_a6_bench.jsonl); --quick = the accept rows alone."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mxfp4_moe_a8_bench import SWEEP_P, alternate, capture  # noqa: E402
from mxfp4_moe_bench import PROJ, routings, stacks  # noqa: E402

WN_KNOB = "BIE_MXFP4_MOE_A6_WN"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the accept rows alone")
    ap.add_argument("--part", default="all", choices=("tile", "sweep", "accept", "all"))
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp4_moe_a6_bench.jsonl")
    a = ap.parse_args()
    parts = ("accept",) if a.quick else ("tile", "sweep", "accept") if a.part == "all" else (a.part,)
    if "tile" in parts:
        os.environ["BIE_TUNING"] = "1"  # read once, at the library's first call: the tile knob is then re-read on every call
    assert torch.cuda.is_available(), "mxfp4_moe_a6_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp4_experts_a6_cuda as a6
    from bitorch_engine.extensions import mxfp4_experts_a8_cuda as a8  # the comparison arms: W4A8 and W4A4 on the same weights
    from bitorch_engine.extensions import mxfp4_experts_a4_cuda as a4
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp4_moe_a6_bench.jsonl"), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def x_for(T, S, K, xpp, dt):
        return torch.randn((T, S, K) if xpp else (T, K), generator=gen, device=dev).to(dt)

    dts = (torch.float16, torch.bfloat16)
    with torch.no_grad():
        if "tile" in parts:
            S = 4
            for E in (32, 128):
                for name, K, N, xpp in PROJ:
                    st = stacks(E, N, K, 2 if E == 32 else 1, dev, gen)
                    for dt in dts:
                        dname = str(dt).replace("torch.", "")
                        for T in (64, 256, 4096):
                            P = T * S
                            x, idxs = x_for(T, S, K, xpp, dt), routings(T, S, E, 4, dev, gen)
                            fns = [(lambda i=i, w=st[j % len(st)]: a6.forward(x, i, w[0], w[1], None, w[2], form=1)) for j, i in enumerate(idxs)]
                            arms = []
                            for wn in (2, 1):
                                os.environ[WN_KNOB] = str(wn)
                                arms.append(capture(fns, 24))
                            del os.environ[WN_KNOB]
                            t2, t1 = alternate(arms, 9)
                            u2, u1 = statistics.median(t2), statistics.median(t1)
                            emit({"part": "tile", "proj": name, "dtype": dname, "E": E, "S": S, "K": K, "N": N, "T": T, "t128x128_us": round(u2, 2),
                                  "t128x64_us": round(u1, 2), "ratio": round(u2 / u1, 3), "spread128": round((max(t2) - min(t2)) / u2, 3),
                                  "spread64": round((max(t1) - min(t1)) / u1, 3), "tflops128": round(2.0 * P * N * K / u2 * 1e-6, 1)})
                    del st
                    torch.cuda.empty_cache()
        if "sweep" in parts:
            S = 4
            for E in (32, 128):
                for name, K, N, xpp in PROJ:
                    st = stacks(E, N, K, 2 if E == 32 else 1, dev, gen)
                    for dt in dts:
                        dname = str(dt).replace("torch.", "")
                        for P in SWEEP_P:
                            T, Sp = (1, P) if P < S else (P // S, S)
                            x, idxs = x_for(T, Sp, K, xpp, dt), routings(T, Sp, E, 8, dev, gen)
                            row = {"part": "sweep", "proj": name, "dtype": dname, "E": E, "S": Sp, "K": K, "N": N, "P": P, "plan": a6.form(P, E, N, K, dt)}
                            arms = [capture([(lambda i=i, w=st[j % len(st)]: a6.forward(x, i, w[0], w[1], None, w[2], form=form)) for j, i in enumerate(idxs)], 48)
                                    for form in (0, 1)]
                            t0, t1 = alternate(arms, 5)
                            row.update(decode_us=round(statistics.median(t0), 2), grouped_us=round(statistics.median(t1), 2))
                            emit(row)
                    del st
                    torch.cuda.empty_cache()
        if "accept" in parts:
            E, S = 32, 4
            for name, K, N, xpp in PROJ:
                st = stacks(E, N, K, 2, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for T in (1, 16, 256, 4096):
                        P, n = T * S, 16 if T <= 16 else 4
                        x, idxs = x_for(T, S, K, xpp, dt), routings(T, S, E, n, dev, gen)
                        new = [(lambda i=i, w=st[j % 2]: a6.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)]
                        old8 = [(lambda i=i, w=st[j % 2]: a8.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)]
                        old4 = [(lambda i=i, w=st[j % 2]: a4.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)]
                        calls = 240 if T <= 16 else 24
                        t_new, t_8, t_4 = alternate([capture(new, calls), capture(old8, calls), capture(old4, calls)])
                        new_us, us8, us4 = statistics.median(t_new), statistics.median(t_8), statistics.median(t_4)
                        row = {"part": "accept", "proj": name, "dtype": dname, "E": E, "S": S, "K": K, "N": N, "T": T, "form": a6.form(P, E, N, K, dt),
                               "w4a8_form": a8.form(P, E, N, K, dt), "w4a4_form": a4.form(P, E, N, K, dt), "w4a6_us": round(new_us, 2),
                               "w4a8_us": round(us8, 2), "w4a4_us": round(us4, 2), "ratio_a8": round(new_us / us8, 3), "ratio_a4": round(new_us / us4, 3),
                               "w4a8_spread": round((max(t_8) - min(t_8)) / us8, 3), "w4a4_spread": round((max(t_4) - min(t_4)) / us4, 3),
                               "w4a6_spread": round((max(t_new) - min(t_new)) / new_us, 3)}
                        if T == 1:
                            row.update(gbs=round(S * (N * K // 2 + N * K // 32) / (new_us * 1e-6) / 1e9, 1))
                        if T == 4096:
                            row.update(tflops=round(2.0 * P * N * K / new_us * 1e-6, 1), w4a8_tflops=round(2.0 * P * N * K / us8 * 1e-6, 1),
                                       w4a4_tflops=round(2.0 * P * N * K / us4 * 1e-6, 1))
                        emit(row)
                del st
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
