#!/usr/bin/env python3
"""Ternary conv2d forms against the binary conv, graph-timed (bench.capture / bench.time_graph, as tools/conv_ab.py), in one process.

Geometries: the ResNet-18 stages (64@56^2, 128@28^2, 256@14^2, 512@7^2 3x3 stride 1; the three 3x3 stride-2 transitions and the three 1x1
stride-2 downsamples), B in {1, 8, 32, 128}, fp16 and bf16, seeded inputs and trits.  Per point every ternary form that can run it is timed
through its C entry -- VALU one-launch (bie_ternary_conv2d_forward_fused), matrix-pipe one-launch (bie_ternary_conv2d_forward_mfma), the
general path (unfold + the ternary linear) -- and so is the binary conv: its dispatch (binary_conv_cpp.forward) and its two one-launch
forms.  The ternary one-launch forms are timed twice: `tern_valu` / `tern_mfma` store the layer's y in the dtype (three roundings per
value), `tern_valu_f32` / `tern_mfma_f32` store the raw D as fp32 (y_f32, no scales) -- the same output bytes and the same single
fp32 store per value as the binary one-launch forms, which always write fp32 y.  The forms alternate over ROUNDS rounds; a row holds
the median of each.  `plan` is what bie_ternary_conv2d_form picks.  The
VALU / matrix-pipe bound (TERN_CONV_VALU_MAX_PIXELS in csrc/binary_conv_fused.hip) is read off these rows.

The binary one-launch forms are re-timed on the shapes of profiles/r06_conv_ab.txt (fp32) in the same run ("retime" rows); with
--baseline-lib PATH (a libbie_hip.so built from an earlier commit) the same forms of that library are timed alternating with this one.

  python tools/ternary_conv_bench.py [--quick] [--out DIR] [--baseline-lib PATH]      -> DIR/ternary_conv_bench.jsonl (default profiles/)
  python tools/ternary_conv_bench.py --stage C,H,OC,k,stride,pad --batch B --dtype bfloat16 --forms tern_mfma,bin_mfma --out DIR
      one point and only the named forms, no re-time rows: for a per-shape kernel trace (rocprofv3 --kernel-trace --stats -- ...)"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import capture, time_graph  # noqa: E402

ROUNDS, REPS = 3, 20
STAGES = [  # (C, H, OC, k, stride, pad)
    (64, 56, 64, 3, 1, 1), (128, 28, 128, 3, 1, 1), (256, 14, 256, 3, 1, 1), (512, 7, 512, 3, 1, 1),
    (64, 56, 128, 3, 2, 1), (128, 28, 256, 3, 2, 1), (256, 14, 512, 3, 2, 1),
    (64, 56, 128, 1, 2, 0), (128, 28, 256, 1, 2, 0), (256, 14, 512, 1, 2, 0)]
R06 = [(1, 512, 7, 512, 3, 1), (8, 512, 7, 512, 3, 1), (32, 512, 7, 512, 3, 1), (128, 512, 7, 512, 3, 1), (512, 512, 7, 512, 3, 1),
       (32, 256, 14, 256, 3, 1), (32, 128, 28, 128, 3, 1), (32, 256, 14, 512, 3, 2), (32, 256, 14, 512, 1, 2)]


def timed(fns):
    """{name: median us} over ROUNDS rounds of the graph-captured functions, alternating in each round."""
    graphs = {n: capture(lambda st, f=f: f()) for n, f in fns.items()}
    res = {n: [] for n in fns}
    for _ in range(ROUNDS):
        for n, g in graphs.items():
            res[n].append(time_graph(g, REPS))
    return {n: round(statistics.median(v), 2) for n, v in res.items()}


def binary_forms(L, x, wp, B, C, H, OC, k, st, pad, y):
    """The binary conv's one-launch forms through the C entries of library L (None where the geometry is outside a form)."""
    from bitorch_engine.extensions import _binary_common as bc
    from bitorch_engine import _hip
    out = {}
    if L.bie_binary_conv2d_fused_ok(B, C, H, H, OC, k, st, pad, 1):
        wl = bc.conv_weight_lanes(wp, OC, C, k)
        out["valu"] = lambda: _hip.check(L.bie_binary_conv2d_forward_fused(x.data_ptr(), wl.data_ptr(), y.data_ptr(), B, C, H, H, OC, k, st, pad, 1, 1.0,
                                                                           _hip.dt(x), torch.cuda.current_stream().cuda_stream), "binary fused")
    if L.bie_binary_conv2d_mfma_ok(B, C, H, H, OC, k, st, pad, 1):
        wi = bc.conv_weight_fp4_image(wp, OC, C, k)
        out["mfma"] = lambda: _hip.check(L.bie_binary_conv2d_forward_mfma(x.data_ptr(), wi.data_ptr(), y.data_ptr(), B, C, H, H, OC, k, st, pad, 1, 1.0,
                                                                          _hip.dt(x), torch.cuda.current_stream().cuda_stream), "binary mfma")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B in {1, 32} and fp16 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--stage", default=None, help="C,H,OC,k,stride,pad: this geometry only")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--dtype", default=None, choices=("float16", "bfloat16"))
    ap.add_argument("--forms", default=None, help="comma-separated names of the forms to time (default: all)")
    args = ap.parse_args()
    from bitorch_engine import _hip
    from bitorch_engine.extensions import ternary_conv2d_cuda as tc, binary_conv_cpp
    from bitorch_engine.extensions._binary_common import pack_rows
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ternary_conv_bench.jsonl")
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    batches = (1, 32) if args.quick else (1, 8, 32, 128)
    dts = (torch.float16,) if args.quick else (torch.float16, torch.bfloat16)
    stages = STAGES
    if args.stage:
        stages = [tuple(int(v) for v in args.stage.split(","))]
    if args.batch:
        batches = (args.batch,)
    if args.dtype:
        dts = (getattr(torch, args.dtype),)
    keep = set(args.forms.split(",")) if args.forms else None
    for (C, H, OC, k, st, pad) in stages:
        t = (torch.randint(0, 3, (OC, C, k, k), generator=g) - 1).to(torch.int8)
        q = tc.w_pack(t.to(dev))
        lanes = tc.weight_lanes(q, C, k) if C % 128 == 0 else None  # the VALU form's lane images need four K quarters of whole words
        img = tc.weight_fp4_image(q, C, k)
        wp = pack_rows(torch.randn((OC, C * k * k), generator=g).to(dev)).contiguous()
        OH, OW = tc.out_size(H, H, k, st, pad, 1)
        for B in batches:
            for dt in dts:
                x = torch.randn((B, C, H, H), generator=g).to(dt).to(dev)
                sa = torch.tensor(0.5, dtype=dt, device=dev)
                alpha = (torch.rand(OC, generator=g) * 0.1).to(dt).to(dev)
                plan = tc.form(B, C, H, H, OC, k, st, pad, 1)
                fns = {"tern_general": lambda: tc.conv_general(x, q, k, st, pad, 1, sa, alpha)}
                if lanes is not None:
                    try:
                        tc.conv_fused(x, q, k, st, pad, 1, sa, alpha, lanes=lanes)
                        fns["tern_valu"] = lambda: tc.conv_fused(x, q, k, st, pad, 1, sa, alpha, lanes=lanes)
                        fns["tern_valu_f32"] = lambda: tc.conv_fused(x, q, k, st, pad, 1, raw=True, lanes=lanes)
                    except RuntimeError:
                        pass
                try:
                    tc.conv_mfma(x, q, k, st, pad, 1, sa, alpha, wimage=img)
                    fns["tern_mfma"] = lambda: tc.conv_mfma(x, q, k, st, pad, 1, sa, alpha, wimage=img)
                    fns["tern_mfma_f32"] = lambda: tc.conv_mfma(x, q, k, st, pad, 1, raw=True, wimage=img)
                except RuntimeError:
                    pass
                yb = torch.empty((B, OC, OH, OW), dtype=torch.float32, device=dev)
                for n, f in binary_forms(L, x, wp, B, C, H, OC, k, st, pad, yb).items():
                    fns["bin_" + n] = f
                fns["bin_dispatch"] = lambda: binary_conv_cpp.forward(x, wp, OC, B * OH * OW, C * k * k, k, st, pad, 1, OH)
                if keep is not None:
                    fns = {n: f for n, f in fns.items() if n in keep}
                r = {"B": B, "C": C, "H": H, "OC": OC, "k": k, "stride": st, "dtype": str(dt).split(".")[-1], "pixels": B * OH * OW, "plan": plan}
                r.update(timed(fns))
                emit(r)
    # the binary one-launch forms on the r06 shapes (fp32), this library against the baseline library when one is given
    base = None
    if args.baseline_lib:
        import copy
        raw = ctypes.CDLL(args.baseline_lib)
        base = copy.copy(L)
        for name in ("bie_binary_conv2d_fused_ok", "bie_binary_conv2d_mfma_ok", "bie_binary_conv2d_forward_fused", "bie_binary_conv2d_forward_mfma"):
            fn = getattr(raw, name)
            fn.restype, fn.argtypes = _hip.SIGNATURES[name]
            setattr(base, name, fn)
        raw.bie_status_init()
    for (B, C, H, OC, k, st) in ([] if args.stage else R06):
        pad = 1 if k == 3 else 0
        x = torch.randn((B, C, H, H), generator=g).to(dev)
        wp = pack_rows(torch.randn((OC, C * k * k), generator=g).to(dev)).contiguous()
        OH, OW = tc.out_size(H, H, k, st, pad, 1)
        y = torch.empty((B, OC, OH, OW), dtype=torch.float32, device=dev)
        fns = {"bin_" + n: f for n, f in binary_forms(L, x, wp, B, C, H, OC, k, st, pad, y).items()}
        if base is not None:
            y0 = torch.empty_like(y)
            for n, f in binary_forms(base, x, wp, B, C, H, OC, k, st, pad, y0).items():
                fns["baseline_bin_" + n] = f
            for n in ("valu", "mfma"):
                if "bin_" + n in fns:
                    fns["bin_" + n]()
                    fns["baseline_bin_" + n]()
                    torch.cuda.synchronize()
                    assert torch.equal(y, y0), f"binary {n} form differs from the baseline library"
        r = {"retime": "r06_conv_ab", "B": B, "C": C, "H": H, "OC": OC, "k": k, "stride": st, "dtype": "float32"}
        r.update(timed(fns))
        emit(r)
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
