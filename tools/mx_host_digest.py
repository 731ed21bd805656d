#!/usr/bin/env python
"""One line per host-side answer of the MX layers' C entry points: the block-scaled layers (six dense: W4A4, W4A6, W4A8, W6A6, W6A8, W8A8;
five grouped: W4A4, W4A6, W4A8, W6A6, W6A8 experts), then the weight-only layers (MXFP4 and MXFP6 x fp16 / bf16: linear, experts and
their input gradients).  No GPU is needed: every call is a host function or fails its entry check before any
device call.  Two builds of the library have the same plans, workspace sizes, return codes and error texts exactly when their listings
are equal line for line.

  python tools/mx_host_digest.py > new.txt;  BIE_HIP_LIB=/path/to/other/libbie_hip.so python tools/mx_host_digest.py > old.txt;  diff old.txt new.txt

Lines: every *_form (dense at M = 0 .. 130, grouped at P x E below) with the layer's FORM knob unset, 0 and 1 under BIE_TUNING; every
*_workspace_bytes over a grid that crosses each stated limit; and the return code and bie_last_error text of every forward and gemm
entry under one broken argument at a time: K, M / T, N, S, E, x_per_pair, dtype, form, the decode form past its row or pair bound, each
NULL pointer and each misaligned pointer.  The weight-only lines follow those (so the block-scaled listing stays as recorded): the four
*_form functions under their knobs unset, 0 and 1, bie_mxfp4_moe_workspace_bytes, and the refusals of the four forward entries, the four
grad_input entries and bie_mxfp4_blk_exp."""
import os
import sys

os.environ["BIE_TUNING"] = "1"  # read once, at the library's first call: the FORM knobs are then re-read on every call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))

# (symbol stem of the layer's entries, its FORM knob)
DENSE = (("bie_mxfp4_a4", "BIE_MXFP4_A4_FORM"), ("bie_mx4a6", "BIE_MXFP4_A6_FORM"), ("bie_mxfp4_a8", "BIE_MXFP4_A8_FORM"),
         ("bie_mxfp6_a6", "BIE_MXFP6_A6_FORM"), ("bie_mxfp6_a8", "BIE_MXFP6_A8_FORM"), ("bie_mx8a8", "BIE_MXFP8_A8_FORM"))
GROUPED = (("bie_mxfp4_moe_a4", "BIE_MXFP4_MOE_A4_FORM"), ("bie_mx4a6_moe", "BIE_MXFP4_MOE_A6_FORM"), ("bie_mxfp4_moe_a8", "BIE_MXFP4_MOE_A8_FORM"),
           ("bie_mxfp6_moe_a6", "BIE_MXFP6_MOE_A6_FORM"), ("bie_mxfp6_moe_a8", "BIE_MXFP6_MOE_A8_FORM"))
PAIRS = (0, 1, 31, 32, 33, 64, 65, 128, 129, 1024, 1025)
EXPERTS = (1, 32, 127, 128, 256)
KS = (0, 32, 48, 64, 2880, 1 << 20, (1 << 20) + 32)
ROWS = (0, 1, 17, (1 << 31) - 1, 1 << 31)
FAKE = 1 << 20  # a pointer value that no call below dereferences


def knob(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def forms(L):
    for stem, name in DENSE:
        for v in (None, "0", "1"):
            knob(name, v)
            print(f"{stem}_form {name}={v}", *[getattr(L, stem + "_form")(M, 8, 64, M & 1) for M in range(131)])
        knob(name, None)
    for stem, name in GROUPED:
        for v in (None, "0", "1"):
            knob(name, v)
            for E in EXPERTS:
                print(f"{stem}_form {name}={v} E={E}", *[getattr(L, stem + "_form")(P, E, 8, 64, P & 1) for P in PAIRS])
        knob(name, None)


def workspaces(L):
    for stem, _ in DENSE:
        f = getattr(L, stem + "_workspace_bytes")
        for K in KS:
            for form in (-1, 0, 1):
                print(f"{stem}_workspace_bytes K={K} form={form}", *[f(M, 8, K, form) for M in ROWS])
    for stem, _ in GROUPED:
        f = getattr(L, stem + "_workspace_bytes")
        for K in KS:
            for S in (1, 4, 32, 33):
                for E in (1, 32, 1024, 1025):
                    for xpp in (0, 1, 2):
                        for form in (-2, -1, 0, 1, 2):
                            print(f"{stem}_workspace_bytes K={K} S={S} E={E} x_per_pair={xpp} form={form}", *[f(T, S, E, K, xpp, form) for T in ROWS])


def refusals(L, name, ptrs, align, ints, broken):
    """ptrs: the pointer arguments of a valid call (None: an optional one); align: index -> required alignment in bytes; ints: the valid
    integer arguments by name, in order; broken: (name or names, values) replacements, one at a time."""
    f = getattr(L, name)

    def call(tag, p, i):
        rc = f(*p, *i.values(), None)
        assert rc != 0, (name, tag)  # a case that passed its check would launch
        print(f"{name} {tag} rc={rc} {L.bie_last_error().decode()}")

    for key, values in broken:
        for v in values:
            i = dict(ints)
            change = dict(zip(key, v)) if isinstance(key, tuple) else {key: v}
            i.update(change)
            call(",".join(f"{k}={x}" for k, x in change.items()), ptrs, i)
    for n in range(len(ptrs)):
        if ptrs[n] is not None:
            call(f"NULL[{n}]", [None if m == n else p for m, p in enumerate(ptrs)], ints)
        for off in (1, 2, 4, 8):
            if off < align.get(n, 1):
                call(f"misaligned[{n}]+{off}", [FAKE + off if m == n else p for m, p in enumerate(ptrs)], ints)


def entries(L):
    dense_broken = (("K", (0, 48, (1 << 20) + 32, -32)), ("M", (0, -1, 1 << 31)), ("N", (0, 1 << 31)), ("dtype", (-1, 2, 3)), ("form", (-2, 2)),
                    (("M", "form"), ((65, 0), (4096, 0))), (("M", "K"), ((1 << 21, 1 << 20),)), (("M", "N"), ((1 << 21, 1 << 20),)))
    for stem, _ in DENSE:
        ints = dict(M=1, N=8, K=64, dtype=0, form=-1)
        # x, qweight, scales, e_col, bias, y, workspace
        refusals(L, stem + "_linear_forward", [FAKE] * 4 + [None, FAKE, FAKE], {0: 16, 1: 16, 4: 2, 5: 16, 6: 16}, ints, dense_broken)
        # xq, xs, row_flag, qweight, scales, e_col, bias, y, workspace (ignored)
        refusals(L, stem + "_gemm", [FAKE] * 6 + [None, FAKE, None], {0: 16, 3: 16, 6: 2, 7: 16}, ints, dense_broken)
    grouped_broken = (("K", (0, 48, (1 << 20) + 32)), ("T", (0, -1, (1 << 22) + 1)), ("S", (0, 33)), ("E", (0, 1025)), ("N", (0, (1 << 31) - 127, 1 << 31)),
                      ("x_per_pair", (-1, 2)), ("dtype", (-1, 2)), ("form", (-2, 2)), (("T", "S"), ((1 << 22, 2),)),
                      (("T", "S", "form"), ((1025, 1, 0), (257, 4, 0))), (("E", "N"), ((1024, 1 << 21),)), (("T", "S", "N"), ((1 << 22, 1, 1 << 18),)),
                      (("T", "S", "K"), ((1 << 22, 1, 1 << 18),)))
    for stem, _ in GROUPED:
        ints = dict(T=1, S=4, E=3, N=8, K=64, x_per_pair=0, dtype=0, form=1)  # form 1: the workspace is needed
        # x, idx, qweight, scales, e_col, bias, y, workspace
        refusals(L, stem + "_forward", [FAKE] * 5 + [None, FAKE, FAKE], {0: 16, 1: 4, 2: 16, 5: 2, 6: 16, 7: 16}, ints, grouped_broken)
        # xq, xs, row_flag, idx, qweight, scales, e_col, bias, y, workspace
        refusals(L, stem + "_gemm", [FAKE] * 7 + [None, FAKE, FAKE], {0: 16, 3: 4, 4: 16, 7: 2, 8: 16, 9: 16}, ints, grouped_broken)
        # the decode form past the one-launch K needs the workspace too
        ints.update(form=0, K=1 << 16)
        rc = getattr(L, stem + "_forward")(*([FAKE] * 5 + [None, FAKE, None]), *ints.values(), None)
        assert rc != 0
        print(f"{stem}_forward decode K=65536 NULL workspace rc={rc} {L.bie_last_error().decode()}")


def weight_only(L):
    for fmt in ("mxfp4", "mxfp6"):
        name = f"BIE_{fmt.upper()}_FORM"
        for v in (None, "0", "1"):
            knob(name, v)
            print(f"bie_{fmt}_form {name}={v}", *[getattr(L, f"bie_{fmt}_form")(M, 8, 64, M & 1) for M in range(131)])
        knob(name, None)
    for fmt in ("mxfp4", "mxfp6"):
        name = f"BIE_{fmt.upper()}_MOE_FORM"
        for v in (None, "0", "1"):
            knob(name, v)
            for E in EXPERTS:
                print(f"bie_{fmt}_moe_form {name}={v} E={E}", *[getattr(L, f"bie_{fmt}_moe_form")(P, E, 8, 64, P & 1) for P in PAIRS])
        knob(name, None)
    for E in (0, 1, 32, 1024, 1025):
        print(f"bie_mxfp4_moe_workspace_bytes E={E}", *[L.bie_mxfp4_moe_workspace_bytes(P, E) for P in (0, 1, 127, 128, 129, 4096, 1 << 22, (1 << 22) + 1)])
    shape = (("K", (0, 48, (1 << 20) + 32, -32)), ("N", (0, 1 << 31)))
    dense = shape + (("M", (0, -1, 1 << 31)), ("dtype", (-1, 2, 3)), (("M", "K"), ((1 << 21, 1 << 20),)), (("M", "N"), ((1 << 21, 1 << 20),)))
    routed = shape + (("T", (0, -1, (1 << 22) + 1)), ("S", (0, 33)), ("E", (0, 1025)), ("dtype", (-1, 2)), (("T", "S"), ((1 << 22, 2),)),
                      (("E", "N"), ((1024, 1 << 21),)), (("T", "S", "N"), ((1 << 22, 1, 1 << 18),)))
    for fmt in ("mxfp4", "mxfp6"):
        # x, qweight, scales, e_col, bias, y; form 1: e_col is needed
        refusals(L, f"bie_{fmt}_linear_forward", [FAKE] * 4 + [None, FAKE], {0: 16, 1: 16, 4: 2, 5: 2}, dict(M=1, N=8, K=64, dtype=0, form=1),
                 dense + (("form", (-2, 2)), (("M", "form"), ((33, 0), (65, 0), (4096, 0)))))
        # x, idx, qweight, scales, e_col, bias, y, workspace; form 1: e_col and the workspace are needed
        refusals(L, f"bie_{fmt}_moe_forward", [FAKE] * 5 + [None, FAKE, FAKE], {0: 16, 1: 4, 2: 16, 5: 2, 6: 2, 7: 16},
                 dict(T=1, S=4, E=3, N=8, K=64, x_per_pair=0, dtype=0, form=1),
                 routed + (("N", ((1 << 31) - 127,)), ("x_per_pair", (-1, 2)), ("form", (-2, 2)), (("T", "S", "form"), ((1025, 1, 0), (257, 4, 0)))))
        # gy, qweight, scales, e_blk, gx
        refusals(L, f"bie_{fmt}_linear_grad_input", [FAKE] * 5, {0: 2, 1: 16, 4: 16}, dict(M=1, N=8, K=64, dtype=0), dense)
        # gy, idx, qweight, scales, e_blk, gx, workspace
        refusals(L, f"bie_{fmt}_moe_grad_input", [FAKE] * 7, {0: 2, 1: 4, 2: 16, 5: 16, 6: 16}, dict(T=1, S=4, E=3, N=8, K=64, dtype=0, out_fp32=0),
                 routed + (("out_fp32", (-1, 2)),))
    # scales, e_blk
    refusals(L, "bie_mxfp4_blk_exp", [FAKE] * 2, {}, dict(rows=8, K=64, groups=1),
             (("rows", (0, 1 << 31)), ("K", (0, 48, (1 << 20) + 32)), ("groups", (0, 1025)), (("groups", "rows"), ((1024, 1 << 21),))))


def main():
    from bitorch_engine import _hip
    L = _hip.lib()
    forms(L)
    workspaces(L)
    entries(L)
    weight_only(L)


if __name__ == "__main__":
    main()
