#!/usr/bin/env python
"""Kernel time and host cost of the weight-only MX layers (MXFP4 / MXFP6 weights x fp16 / bf16: linear, experts, input gradients), one
build of the library against another.

  python tools/mx_w16_ab.py NEW_LIB PARENT_LIB > profiles/mx_w16_ab.txt

The method is that of tools/mx_host_launch_ab.py (its docstring gives the reasons): every figure comes from a fresh child process
(BIE_HIP_LIB selects the library; two libraries are never loaded in one process); three arms are run in turn for ROUNDS rounds: the new
library, the parent, and the parent once more; `spread` is the range of the parent's 2 x ROUNDS round figures, and a cell passes when
median(new) - median(parent) <= spread.  Exit status 1 when a cell does not.

Kernel cells (us per call): CALLS calls captured in one graph, HIP events around its replay, the median of REPLAYS replays; one set of
weights per cell, random code bytes and scale codes 118 .. 130.  On 4096 x 4096 and 2880 -> 5760 (E = 32, S = 4 for the experts), fp16
and bf16: the dense decode form at every row instance (M = 1, 2, 4, 8, 16, and 32 for MXFP6), the routed decode form at P = 1, 4, 64,
the dense and the grouped prefill form at 512 rows / pairs, the dense input gradient at M = 512 and the grouped one at P = 512 with gx in
the dtype and in fp32.
Host cells (us per call): the eight forward / grad_input C entries at host-bound shapes (dense M = 1, 96 -> 130; experts T = 1, S = 4,
E = 3, 96 -> 33; fp16, the plan's form), HOST_CALLS eager calls on the host clock, one synchronise at the end."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, REPLAYS, HOST_CALLS, HOST_WARMUP, ROUNDS = 32, 5, 2000, 200, 3
SHAPES = ((4096, 4096), (2880, 5760))  # K, N
E, S = 32, 4
FORMATS = (("mxfp4", 4, (1, 2, 4, 8, 16)), ("mxfp6", 6, (1, 2, 4, 8, 16, 32)))  # name, bits per code, decode row instances
ROWS = 512


def child():
    import importlib
    import torch
    sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
    from bitorch_engine import _hip
    L, dev = _hip.lib(), "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}

    def ext(name):
        return importlib.import_module("bitorch_engine.extensions." + name)

    def graph_us(f):
        f()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f()
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(CALLS):
                f()
        gr.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(REPLAYS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / CALLS)
        del gr
        return statistics.median(us)

    def rand_u8(shape, lo=0, hi=256):
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32, device=dev).to(torch.uint8)

    def normal(shape, dt):
        return torch.randn(shape, generator=g, device=dev, dtype=torch.float32).to(dt)

    for fmt, bits, decode_rows in FORMATS:
        lin, exp = ext(fmt + "_linear_cuda"), ext(fmt + "_experts_cuda")
        for K, N in SHAPES:
            q, s = rand_u8((E, N, K * bits // 8)), rand_u8((E, N, K // 32), 118, 131)
            e_col, e_blk = exp.col_exp(s), exp.blk_exp(s)
            for dt, dname in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
                tag = f"{fmt} {K}x{N} {dname}"
                x = normal((ROWS, K), dt)
                gy = normal((ROWS, N), dt)
                for M in decode_rows:
                    out[f"{tag} dense decode M={M}"] = graph_us(lambda: lin.forward(x[:M], q[0], s[0], None, e_col[0], form=0))
                out[f"{tag} dense prefill M={ROWS}"] = graph_us(lambda: lin.forward(x, q[0], s[0], None, e_col[0], form=1))
                out[f"{tag} dense grad_input M={ROWS}"] = graph_us(lambda: lin.grad_input(gy, q[0], s[0], e_blk[0]))
                idx = torch.randint(0, E, (ROWS // S, S), generator=g, dtype=torch.int32, device=dev)
                for P in (1, 4, 64):
                    T = max(1, P // S)
                    ip = idx[:T, :P // T].contiguous()
                    out[f"{tag} routed decode P={P}"] = graph_us(lambda: exp.forward(x[:T], ip, q, s, None, e_col, form=0))
                out[f"{tag} grouped prefill P={ROWS}"] = graph_us(lambda: exp.forward(x[:ROWS // S], idx, q, s, None, e_col, form=1))
                for odt, oname in ((None, "dtype"), (torch.float32, "fp32")):
                    out[f"{tag} grouped grad_input P={ROWS} gx {oname}"] = graph_us(lambda: exp.grad_input(gy, idx, q, s, e_blk, out_dtype=odt))
            del q, s

    # host cost of the eight C entries
    st = _hip.stream()

    def clock(name, f, args):
        for _ in range(HOST_WARMUP):
            rc = f(*args)
        assert rc == 0, (name, L.bie_last_error())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(HOST_CALLS):
            f(*args)
        torch.cuda.synchronize()
        out["host " + name] = (time.perf_counter() - t0) / HOST_CALLS * 1e6

    ptr = _hip.ptr
    for fmt, bits, _ in FORMATS:
        M, K, N = 1, 96, 130
        x, gy = normal((M, K), torch.half), normal((M, N), torch.half)
        q, s = rand_u8((N, K * bits // 8)), rand_u8((N, K // 32), 118, 131)
        ecol, eblk = ext("mxfp4_linear_cuda").col_exp(s), ext("mxfp4_linear_cuda").blk_exp(s)
        y, gx = torch.empty((M, N), dtype=torch.half, device=dev), torch.empty((M, K), dtype=torch.half, device=dev)
        clock(f"bie_{fmt}_linear_forward", getattr(L, f"bie_{fmt}_linear_forward"), (ptr(x), ptr(q), ptr(s), ptr(ecol), None, ptr(y), M, N, K, 0, -1, st))
        clock(f"bie_{fmt}_linear_grad_input", getattr(L, f"bie_{fmt}_linear_grad_input"), (ptr(gy), ptr(q), ptr(s), ptr(eblk), ptr(gx), M, N, K, 0, st))
        T, S_, E_, K, N = 1, 4, 3, 96, 33
        x, gy = normal((T, K), torch.half), normal((T * S_, N), torch.half)
        idx = torch.tensor([[0, 2, 1, 2]], dtype=torch.int32, device=dev)
        q, s = rand_u8((E_, N, K * bits // 8)), rand_u8((E_, N, K // 32), 118, 131)
        ecol, eblk = ext("mxfp4_experts_cuda").col_exp(s), ext("mxfp4_experts_cuda").blk_exp(s)
        y, gx = torch.empty((T, S_, N), dtype=torch.half, device=dev), torch.empty((T * S_, K), dtype=torch.half, device=dev)
        ws = torch.empty(int(L.bie_mxfp4_moe_workspace_bytes(T * S_, E_)), dtype=torch.uint8, device=dev)
        clock(f"bie_{fmt}_moe_forward", getattr(L, f"bie_{fmt}_moe_forward"),
              (ptr(x), ptr(idx), ptr(q), ptr(s), ptr(ecol), None, ptr(y), ptr(ws), T, S_, E_, N, K, 0, 0, -1, st))
        clock(f"bie_{fmt}_moe_grad_input", getattr(L, f"bie_{fmt}_moe_grad_input"),
              (ptr(gy), ptr(idx), ptr(q), ptr(s), ptr(eblk), ptr(gx), ptr(ws), T, S_, E_, N, K, 0, 0, st))
    print("AB " + json.dumps(out))


def main(new_lib, parent_lib):
    arms = {"new": new_lib, "parent": parent_lib, "parent2": parent_lib}
    figures = {a: [] for a in arms}
    for r in range(ROUNDS):
        for arm, lib in arms.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=400,
                               env=dict(os.environ, BIE_HIP_LIB=os.path.abspath(lib)))
            if p.returncode != 0:
                print(f"round {r} arm {arm}: exit {p.returncode}\n{p.stderr[-3000:]}", file=sys.stderr)
                sys.exit(2)  # nothing more is started after a child that failed
            figures[arm].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("AB ")][-1][3:]))
            print(f"# round {r} arm {arm} done", file=sys.stderr, flush=True)
    print(f"# us per call.  Kernel cells: {CALLS} calls in one graph, median of {REPLAYS} replays; host cells: {HOST_CALLS} eager calls, host clock.  "
          f"{ROUNDS} rounds per arm, arms alternated, a fresh process each")
    print(f"# {'cell':58s} {'new':>9s} {'parent':>9s} {'parent2':>9s} {'new-parent':>10s} {'spread':>8s}  verdict   rounds new | parent | parent2")
    bad = 0
    for name in figures["new"][0]:
        rounds = {a: [f[name] for f in figures[a]] for a in arms}
        med = {a: statistics.median(v) for a, v in rounds.items()}
        both = rounds["parent"] + rounds["parent2"]
        spread, delta = max(both) - min(both), med["new"] - med["parent"]
        ok = delta <= spread
        bad += not ok
        print(f"  {name:58s} {med['new']:9.3f} {med['parent']:9.3f} {med['parent2']:9.3f} {delta:+10.3f} {spread:8.3f}  {'pass' if ok else 'SLOWER'}     "
              + " | ".join(" ".join(f"{v:.3f}" for v in rounds[a]) for a in arms))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main(sys.argv[1], sys.argv[2]))
