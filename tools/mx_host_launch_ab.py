#!/usr/bin/env python
"""Host cost per call of the eleven block-scaled MX forward entries (six dense, five grouped), one build of the library against another.

  python tools/mx_host_launch_ab.py NEW_LIB PARENT_LIB > profiles/mx_host_launch_ab.txt

The kernels and grids of the two builds being the same, what can differ is the enqueue path.  So the shapes are host-bound (dense: M = 1,
96 -> 130; experts: T = 1, S = 4, E = 3, 96 -> 33; the plan's form, fp16, no bias) and a figure is the host clock around 2000 back-to-back
eager calls of the C entry, ended by one device synchronise, in microseconds per call.  Every figure comes from a fresh child process
(BIE_HIP_LIB selects the library; two libraries are never loaded in one process).  Three arms are run in turn for ROUNDS rounds: the new
library, the parent, and the parent once more.

Per entry: `new` and `parent` are the medians of the new arm's and of the first parent arm's rounds; `parent2` is the second parent arm's
median.  The spread of the parent against itself is taken as the range (largest minus smallest) of the parent's 2 x ROUNDS round figures:
a single difference of two medians is one draw of the noise and is below the other arm's with probability about 1/4 per entry even
when nothing changed, so with eleven entries it would fail a build that is identical; the range is the widest disagreement the parent
shows with itself in the same run.  An entry passes when new - parent <= spread.  Exit status 1 when an entry does not."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, WARMUP, ROUNDS = 2000, 200, 5
# (extension module, C symbol stem)
DENSE = (("mxfp4_a4_linear_cuda", "bie_mxfp4_a4"), ("mxfp4_a6_linear_cuda", "bie_mx4a6"), ("mxfp4_a8_linear_cuda", "bie_mxfp4_a8"),
         ("mxfp6_a6_linear_cuda", "bie_mxfp6_a6"), ("mxfp6_a8_linear_cuda", "bie_mxfp6_a8"), ("mxfp8_a8_linear_cuda", "bie_mx8a8"))
GROUPED = (("mxfp4_experts_a4_cuda", "bie_mxfp4_moe_a4"), ("mxfp4_experts_a6_cuda", "bie_mx4a6_moe"), ("mxfp4_experts_a8_cuda", "bie_mxfp4_moe_a8"),
           ("mxfp6_experts_a6_cuda", "bie_mxfp6_moe_a6"), ("mxfp6_experts_a8_cuda", "bie_mxfp6_moe_a8"))


def child():
    import importlib
    import torch
    sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
    from bitorch_engine import _hip
    L, dev, g = _hip.lib(), "cuda", torch.Generator().manual_seed(0)
    st = _hip.stream()
    out = {}

    def clock(name, f, args):
        for _ in range(WARMUP):
            rc = f(*args)
        assert rc == 0, (name, L.bie_last_error())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            f(*args)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / CALLS * 1e6

    M, K, N = 1, 96, 130
    x = torch.randn((M, K), generator=g).half().to(dev)
    for mod, stem in DENSE:
        e = importlib.import_module("bitorch_engine.extensions." + mod)
        qw, sc = e.quantize(torch.randn((N, K), generator=g).to(dev))
        ecol, y = e.col_exp(sc), torch.empty((M, N), dtype=torch.half, device=dev)
        ws = torch.empty(int(getattr(L, stem + "_workspace_bytes")(M, N, K, -1)), dtype=torch.uint8, device=dev)
        clock(stem + "_linear_forward", getattr(L, stem + "_linear_forward"),
              (_hip.ptr(x), _hip.ptr(qw), _hip.ptr(sc), _hip.ptr(ecol), None, _hip.ptr(y), _hip.ptr(ws), M, N, K, 0, -1, st))
    T, S, E, K, N = 1, 4, 3, 96, 33
    x = torch.randn((T, K), generator=g).half().to(dev)
    idx = torch.tensor([[0, 2, 1, 2]], dtype=torch.int32, device=dev)
    for mod, stem in GROUPED:
        e = importlib.import_module("bitorch_engine.extensions." + mod)
        qw, sc = e.quantize(torch.randn((E, N, K), generator=g).to(dev))
        ecol, y = e.col_exp(sc), torch.empty((T, S, N), dtype=torch.half, device=dev)
        ws = torch.empty(int(getattr(L, stem + "_workspace_bytes")(T, S, E, K, 0, -1)), dtype=torch.uint8, device=dev)
        clock(stem + "_forward", getattr(L, stem + "_forward"),
              (_hip.ptr(x), _hip.ptr(idx), _hip.ptr(qw), _hip.ptr(sc), _hip.ptr(ecol), None, _hip.ptr(y), _hip.ptr(ws), T, S, E, N, K, 0, 0, -1, st))
    print("AB " + json.dumps(out))


def main(new_lib, parent_lib):
    arms = {"new": new_lib, "parent": parent_lib, "parent2": parent_lib}
    figures = {a: [] for a in arms}
    for r in range(ROUNDS):
        for arm, lib in arms.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, BIE_HIP_LIB=os.path.abspath(lib)))
            if p.returncode != 0:
                print(f"round {r} arm {arm}: exit {p.returncode}\n{p.stderr[-3000:]}", file=sys.stderr)
                sys.exit(2)  # nothing more is started after a child that failed
            figures[arm].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("AB ")][-1][3:]))
    print(f"# us per call: {CALLS} eager calls, host clock, one synchronise at the end; {ROUNDS} rounds per arm, arms alternated, a fresh process each")
    print(f"# {'entry':34s} {'new':>8s} {'parent':>8s} {'parent2':>8s} {'new-parent':>10s} {'spread':>8s}  verdict   rounds new | parent | parent2")
    bad = 0
    for name in figures["new"][0]:
        rounds = {a: [f[name] for f in figures[a]] for a in arms}
        med = {a: statistics.median(v) for a, v in rounds.items()}
        both = rounds["parent"] + rounds["parent2"]
        spread, delta = max(both) - min(both), med["new"] - med["parent"]
        ok = delta <= spread
        bad += not ok
        print(f"  {name:34s} {med['new']:8.3f} {med['parent']:8.3f} {med['parent2']:8.3f} {delta:+10.3f} {spread:8.3f}  {'pass' if ok else 'SLOWER'}     "
              + " | ".join(" ".join(f"{v:.3f}" for v in rounds[a]) for a in arms))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main(sys.argv[1], sys.argv[2]))
