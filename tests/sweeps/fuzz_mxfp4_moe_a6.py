#!/usr/bin/env python3
"""Randomised sweep of the MXFP4 W4A6 expert GEMM (csrc/mxfp4_moe_a6.hip) against the restatement (mxfp4_moe_a6_ref.py): the sweep of
fuzz_mxfp6_moe_a6.py on the new entries.  E, S, T, K and N at the plan's, the decode form's (P = 1024, K = 16384 and the K just past it)
and the tiles' edges, skewed routing with skipped shares of 0 .. 100 %, both dtypes, both x_per_pair values, special values, the grouped
form on either tile width (BIE_MXFP4_MOE_A6_WN, drawn per case and re-read per call under BIE_TUNING), each configuration on every form
that accepts it:

  normal   Gaussian x and random weights: every form within mxfp4_a6_ref.tolerance of the float64 product per pair, NaN exactly where
           the restatement has it, skipped slots exactly +0; forward bit-identical to quantize_act + gemm (in the decode form up to
           K = 16384 that pins the in-LDS quantiser to bie_mxfp6_quantize_act)
  special  normal, with NaN / +-inf planted in rows of x and scale-255 blocks in the weights
  exact    x a fixed point of the quantiser under ONE scale code (a 4 per block, the rest multiples of 0.5 up to 3.5), weight scale code 127
           everywhere, integer bias, K <= 256 (exact_case of tests/test_mxfp4_moe_a6_gpu.py: an instruction whose blocks carry one scale is
           exact, products are multiples of 2^-4 and sums of 256 stay exact in fp32): every form bit-identical to the float64 product
           rounded once; a larger K drawn with this mode runs as normal

draw(rng) returns a plain configuration and forms_of(cfg) the forms it runs (host predicates only).  A refusal (RuntimeError with the
library's message) is counted as skipped; a wrong value, an unexpected NaN or a crash is a finding.
    usage: python tests/sweeps/fuzz_mxfp4_moe_a6.py [cases=300] [seed=1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("BIE_TUNING", "1")  # read once, at the library's first call: the tile-width knob is then re-read on every call
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mxfp4_moe_a6_ref as aref  # noqa: E402

DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
FORMS = ("decode", "grouped")
DECODE_PAIRS, ONE_K = 1024, 16384
WN_KNOB = "BIE_MXFP4_MOE_A6_WN"  # the grouped form's column tile: 2 = 128 x 128, 1 = 128 x 64
E_SET = [1, 2, 3, 8, 32, 33, 128]
S_SET = [1, 2, 4, 8]
P_SET = [1, 2, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 640, 1023, 1024, 1025, 1300, 3000]  # pairs: the plan's and the tiles' edges
K_SET = [32, 64, 96, 128, 160, 256, 1056, 2880]
K_EDGE = [ONE_K - 32, ONE_K, ONE_K + 32]  # the one-launch decode form's bound
MODES = ("normal", "normal", "special", "exact")


def draw(rng):
    S = int(rng.choice(S_SET))
    T = max(1, int(rng.choice(P_SET)) // S + int(rng.integers(0, 2)))
    u = rng.random()
    N = int(rng.integers(1, 71)) if u < 0.5 else max(1, 128 * int(rng.integers(1, 4)) + int(rng.integers(-1, 2)))
    E, K = int(rng.choice(E_SET)), int(rng.choice(K_SET))
    if rng.random() < 0.1:  # the K bound: a short stack and few pairs keep the case small
        K, E, N, T = int(rng.choice(K_EDGE)), min(E, 3), min(N, 40), min(T, 24)
    return dict(E=E, S=S, T=T, N=N, K=K, dt=str(rng.choice(list(DTS))), mode=str(rng.choice(MODES)),
                xpp=int(rng.integers(0, 2)), bias=bool(rng.integers(0, 2)), skew=float(rng.choice([0.0, 1.2, 3.0])),
                skip=float(rng.choice([0.0, 0.0, 0.3, 0.9, 1.0])), seed=int(rng.integers(0, 2 ** 31)), wn=int(rng.integers(1, 3)))


def forms_of(c):
    return (["decode"] if c["T"] * c["S"] <= DECODE_PAIRS else []) + ["grouped"]


def routing(c, g):
    """Zipf-skewed experts (exponent `skew`, 0 = uniform), a share `skip` of the slots replaced by out-of-range indices."""
    E, P = c["E"], c["T"] * c["S"]
    prob = 1.0 / torch.arange(1, E + 1, dtype=torch.float64) ** c["skew"]
    idx = torch.multinomial(prob / prob.sum(), P, replacement=True, generator=g).to(torch.int32)
    bad = torch.tensor([-1, E, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    skipped = torch.rand(P, generator=g) < c["skip"]
    idx[skipped] = bad[torch.randint(0, 4, (int(skipped.sum()),), generator=g)]
    return idx.reshape(c["T"], c["S"])


def run_case(c):
    from bitorch_engine.extensions import mxfp4_experts_a6_cuda as ext
    g = torch.Generator().manual_seed(c["seed"])
    E, S, T, N, K, dt, mode = c["E"], c["S"], c["T"], c["N"], c["K"], DTS[c["dt"]], c["mode"]
    exact = mode == "exact" and K <= 256
    lo, hi = (127, 127) if exact else (118, 130)
    q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    shape = (T, S, K) if c["xpp"] else (T, K)
    if exact:
        x = torch.randint(-7, 8, shape, generator=g).float() * 0.5
        x[..., 0::32] = 4.0
    else:
        x = torch.randn(shape, generator=g) * 0.5
    if mode == "special":
        rows = x.reshape(-1, K)
        for r in torch.randint(0, rows.shape[0], (max(1, rows.shape[0] // 8),), generator=g).tolist():
            rows[r, int(torch.randint(0, K, (1,), generator=g))] = [float("nan"), float("inf"), float("-inf")][r % 3]
        s[int(torch.randint(0, E, (1,), generator=g)), int(torch.randint(0, N, (1,), generator=g)), int(torch.randint(0, K // 32, (1,), generator=g))] = 255
    x = x.to(dt)
    bias = None
    if c["bias"]:
        bias = (torch.randint(-8, 9, (E, N), generator=g) if exact else torch.randn((E, N), generator=g)).to(dt).to(DEV)
    idx = routing(c, g)
    live = ((idx >= 0) & (idx < E)).to(DEV)
    q, s = q.to(DEV), s.to(DEV)
    yref, a = aref.experts(x, idx, aref.dequant(q, s).to(DEV), bias)
    nan = torch.isnan(yref)
    if mode != "special":
        assert not nan.any()
    tol = aref.tolerance(yref, a, K, dt)
    xd, idxd = x.to(DEV), idx.to(DEV)
    xq, xs, flag = ext.quantize_act(xd.reshape(-1, K))
    forms = forms_of(c)
    outs = {}
    old = os.environ.get(WN_KNOB)
    os.environ[WN_KNOB] = str(c["wn"])
    try:
        _run_forms(c, ext, forms, outs, xd, idxd, q, s, bias, xq, xs, flag, yref, nan, live, tol, exact, dt)
    finally:
        if old is None:
            os.environ.pop(WN_KNOB, None)
        else:
            os.environ[WN_KNOB] = old
    return forms


def _run_forms(c, ext, forms, outs, xd, idxd, q, s, bias, xq, xs, flag, yref, nan, live, tol, exact, dt):
    T, S, N = c["T"], c["S"], c["N"]
    for f in forms:
        y = ext.forward(xd, idxd, q, s, bias, form=FORMS.index(f))
        assert y.dtype == dt and y.shape == (T, S, N)
        assert torch.equal(torch.isnan(y), nan), f"{f}: NaN pattern differs"
        assert torch.isfinite(y[~nan]).all(), f"{f}: non-finite output"
        assert (y[~live] == 0).all() and not torch.signbit(y[~live]).any(), f"{f}: a skipped slot is not +0"
        if exact:
            assert torch.equal(y, yref.to(dt)), f"{f}: not bit-exact on exact data"
        else:
            err = (y.double() - yref).abs()[~nan]
            assert (err <= tol[~nan]).all(), f"{f}: max err {err.max().item()} (tol there {tol[~nan].flatten()[err.argmax()].item()})"
        y2 = ext.gemm(xq, xs, flag, idxd, q, s, bias, dtype=dt, form=FORMS.index(f))
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), f"{f}: forward differs from quantize_act + gemm"
        outs[f] = y
    y = ext.forward(xd, idxd, q, s, bias)  # the plan's own choice is one of the forms above
    assert any(torch.equal(y.view(torch.int16), o.view(torch.int16)) for o in outs.values()), "the planned form differs from every forced one"


def run(cases=300, seed=1):
    rng = np.random.default_rng(seed)
    ok, bad, refused, forms, edge, bound, widths = 0, [], {}, {f: 0 for f in FORMS}, 0, 0, {1: 0, 2: 0}
    for _ in range(cases):
        c = draw(rng)
        try:
            got = run_case(c)
            torch.cuda.synchronize()
        except RuntimeError as err:
            if " failed with status " not in str(err):
                raise  # not a refusal of the library's (a device error, say): the sweep ends here
            key = str(err)[:100]
            refused[key] = refused.get(key, 0) + 1
            continue
        except AssertionError as err:
            bad.append(f"{c}: {str(err)[:300]}")
            continue
        ok += 1
        edge += c["K"] in K_EDGE
        bound += c["K"] == ONE_K
        widths[c["wn"]] += "grouped" in got
        for f in got:
            forms[f] += 1
    return {"cases": cases, "seed": seed, "ok": ok, "bad": bad, "refused": refused, "forms": forms, "k_edge_cases": edge, "k_bound_cases": bound,
            "tile_widths": {"128x64": widths[1], "128x128": widths[2]}}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 300, int(sys.argv[2]) if len(sys.argv) > 2 else 1), indent=1))
