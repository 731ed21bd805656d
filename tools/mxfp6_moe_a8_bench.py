"""MXFP6 W6A8 expert GEMM (csrc/mxfp6_moe_a8.hip) against the MXFP4 W4A8 expert GEMM (csrc/mxfp4_moe_a8.hip,
mxfp4_experts_a8_cuda.forward) in one process: the same shapes, routings and activations, 1.5 x the weight bytes.

gpt-oss-20b's two expert projections (E = 32, top-4; 2880 -> 5760 with x per token, 2880 -> 2880 with x per pair), fp16 and bf16:
  accept   T in {1, 16, 256, 4096}: the new path under its own plan, the activation quantiser included, and the W4A8 path under
           its own plan.  Each arm is one captured graph; the two graphs are replayed alternately, round by round; the medians over the
           rounds, their ratio, and the spread (max - min) / median of the W4A8 arm across the rounds as the noise figure.
           T = 1: GB/s over the MXFP6 qweight + scales bytes of the S selected experts; T = 4096: TFLOP/s over 2 P N K.
  sweep    P in {1, 2, 4, ..., 1024} pairs, both forms of the new path (forced), at E = 32 and E = 128, both projections: what the plan's
           bound in mxfp6_moe_a8.hip rests on.
  strip    the decode form at P in {1, 4, 16, 64} with strips of 16, 32 and 64 columns (BIE_MXFP6_MOE_A8_STRIP under BIE_TUNING).
Every call of a round uses another routing and the calls alternate between weight stacks, so that the experts a round reads exceed the
256 MB Infinity Cache where the stacks do (decode numbers are HBM numbers).

  python tools/mxfp6_moe_a8_bench.py [--quick] [--part accept|sweep|strip|all] [--out DIR]
one JSON line per measurement on stdout (and DIR/mxfp6_moe_a8_bench.jsonl); --quick = the accept rows alone."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "bitorch-engine_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mxfp4_moe_a8_bench import alternate, capture  # noqa: E402
from mxfp4_moe_bench import PROJ, routings  # noqa: E402

SWEEP_P = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)


def stacks(E, N, K, n, dev, gen, fp4=False):
    """n random weight stacks (qweight, scales, e_col): MXFP6 [E, N, 3K/4], and with fp4 the MXFP4 stack [E, N, K/2] under the same
    scales appended as a fourth member."""
    from bitorch_engine.extensions import mxfp6_experts_a8_cuda as a6
    out = []
    for _ in range(n):
        q = torch.randint(0, 256, (E, N, K // 32 * 24), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        s = torch.randint(118, 131, (E, N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        q4 = torch.randint(0, 256, (E, N, K // 2), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8) if fp4 else None
        out.append((q, s, a6.col_exp(s), q4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the accept rows alone")
    ap.add_argument("--part", default="all", choices=("accept", "sweep", "strip", "all"))
    ap.add_argument("--out", default=None, help="also write the lines to DIR/mxfp6_moe_a8_bench.jsonl")
    a = ap.parse_args()
    parts = ("accept",) if a.quick else ("accept", "sweep", "strip") if a.part == "all" else (a.part,)
    if "strip" in parts:
        os.environ["BIE_TUNING"] = "1"  # read once, at the library's first call: the strip knob is then re-read on every call
    assert torch.cuda.is_available(), "mxfp6_moe_a8_bench.py measures on the GPU; there is no CPU fallback"
    from bitorch_engine.extensions import mxfp6_experts_a8_cuda as a8
    from bitorch_engine.extensions import mxfp4_experts_a8_cuda as w4  # the comparison arm: W4A8
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = None
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        sink = open(os.path.join(a.out, "mxfp6_moe_a8_bench.jsonl"), "a")

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
        if "accept" in parts:
            E, S = 32, 4
            for name, K, N, xpp in PROJ:
                st = stacks(E, N, K, 2, dev, gen, fp4=True)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for T in (1, 16, 256, 4096):
                        P, n = T * S, 16 if T <= 16 else 4
                        x, idxs = x_for(T, S, K, xpp, dt), routings(T, S, E, n, dev, gen)
                        new = [(lambda i=i, w=st[j % 2]: a8.forward(x, i, w[0], w[1], None, w[2])) for j, i in enumerate(idxs)]
                        old = [(lambda i=i, w=st[j % 2]: w4.forward(x, i, w[3], w[1], None, w[2])) for j, i in enumerate(idxs)]
                        calls = 240 if T <= 16 else 24
                        t_new, t_old = alternate([capture(new, calls), capture(old, calls)])
                        new_us, old_us = statistics.median(t_new), statistics.median(t_old)
                        row = {"part": "accept", "proj": name, "dtype": dname, "E": E, "S": S, "K": K, "N": N, "T": T, "form": a8.form(P, E, N, K, dt),
                               "w4a8_form": w4.form(P, E, N, K, dt), "w6a8_us": round(new_us, 2), "w4a8_us": round(old_us, 2),
                               "ratio": round(new_us / old_us, 3), "noise": round((max(t_old) - min(t_old)) / old_us, 3),
                               "w6a8_spread": round((max(t_new) - min(t_new)) / new_us, 3)}
                        if T == 1:
                            row.update(gbs=round(S * (N * K // 32 * 24 + N * K // 32) / (new_us * 1e-6) / 1e9, 1))
                        if T == 4096:
                            row.update(tflops=round(2.0 * P * N * K / new_us * 1e-6, 1), w4a8_tflops=round(2.0 * P * N * K / old_us * 1e-6, 1))
                        emit(row)
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
                            row = {"part": "sweep", "proj": name, "dtype": dname, "E": E, "S": Sp, "K": K, "N": N, "P": P, "plan": a8.form(P, E, N, K, dt)}
                            arms = [capture([(lambda i=i, w=st[j % len(st)]: a8.forward(x, i, w[0], w[1], None, w[2], form=form)) for j, i in enumerate(idxs)], 48)
                                    for form in (0, 1)]
                            t0, t1 = alternate(arms, 5)
                            row.update(decode_us=round(statistics.median(t0), 2), grouped_us=round(statistics.median(t1), 2))
                            emit(row)
                    del st
                    torch.cuda.empty_cache()
        if "strip" in parts:
            E, S = 32, 4
            for name, K, N, xpp in PROJ:
                st = stacks(E, N, K, 2, dev, gen)
                for dt in dts:
                    dname = str(dt).replace("torch.", "")
                    for P in (1, 4, 16, 64):
                        T, Sp = (1, P) if P < S else (P // S, S)
                        x, idxs = x_for(T, Sp, K, xpp, dt), routings(T, Sp, E, 16, dev, gen)
                        fns = [(lambda i=i, w=st[j % 2]: a8.forward(x, i, w[0], w[1], None, w[2], form=0)) for j, i in enumerate(idxs)]
                        arms = []
                        for strip in (1, 2, 4):
                            os.environ["BIE_MXFP6_MOE_A8_STRIP"] = str(strip)
                            arms.append(capture(fns, 96))
                        del os.environ["BIE_MXFP6_MOE_A8_STRIP"]
                        ts = alternate(arms, 5)
                        emit({"part": "strip", "proj": name, "dtype": dname, "E": E, "K": K, "N": N, "P": P,
                              **{f"cols{16 * c}_us": round(statistics.median(t), 2) for c, t in zip((1, 2, 4), ts)}})
                del st
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
