#!/usr/bin/env python3
"""Randomised sweep of the MXFP4 mixture-of-experts expert GEMM (csrc/mxfp4_moe.hip) against the restatement (mxfp4_moe_ref.py): E, S,
T, K and N at the form and tile boundaries, skewed routing with skipped slots, both dtypes, both x_per_pair values, each configuration
on every form that accepts it:

  normal   Gaussian x and random weights: every form within the MXFP4 linear contract's tolerance of the float64 product per pair,
           skipped slots exactly zero
  exact    integer x, scale codes 125 .. 129, integer bias: every form bit-identical to the float64 product rounded once

draw(rng) returns a plain configuration and forms_of(cfg) the forms it runs (host predicates only).  A refusal (RuntimeError with the
library's message) is counted as skipped; a wrong value, an unexpected NaN or a crash is a finding.
    usage: python tests/sweeps/fuzz_mxfp4_moe.py [cases=300] [seed=1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mxfp4_moe_ref as mref  # noqa: E402

DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
FORMS = ("decode", "grouped")
DECODE_PAIRS = 1024
E_SET = [1, 2, 3, 8, 32, 33, 128]
S_SET = [1, 2, 4, 8]
P_SET = [1, 2, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 640, 1023, 1024, 1025, 1300, 3000]  # pairs: the plan's and the tiles' edges
K_SET = [32, 64, 96, 128, 160, 256, 1056, 2880]
MODES = ("normal", "normal", "exact")


def draw(rng):
    S = int(rng.choice(S_SET))
    T = max(1, int(rng.choice(P_SET)) // S + int(rng.integers(0, 2)))
    u = rng.random()
    N = int(rng.integers(1, 71)) if u < 0.5 else max(1, 128 * int(rng.integers(1, 4)) + int(rng.integers(-1, 2)))
    return dict(E=int(rng.choice(E_SET)), S=S, T=T, N=N, K=int(rng.choice(K_SET)), dt=str(rng.choice(list(DTS))), mode=str(rng.choice(MODES)),
                xpp=int(rng.integers(0, 2)), bias=bool(rng.integers(0, 2)), skew=float(rng.choice([0.0, 1.2, 3.0])),
                skip=float(rng.choice([0.0, 0.0, 0.3, 1.0])), seed=int(rng.integers(0, 2 ** 31)))


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
    from bitorch_engine.extensions import mxfp4_experts_cuda as ext
    g = torch.Generator().manual_seed(c["seed"])
    E, S, T, N, K, dt, exact = c["E"], c["S"], c["T"], c["N"], c["K"], DTS[c["dt"]], c["mode"] == "exact"
    lo, hi = (125, 129) if exact else (118, 130)
    q = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    s = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    shape = (T, S, K) if c["xpp"] else (T, K)
    x = (torch.randint(-2, 3, shape, generator=g) if exact else torch.randn(shape, generator=g) * 0.5).to(dt).to(DEV)
    bias = None
    if c["bias"]:
        bias = (torch.randint(-8, 9, (E, N), generator=g) if exact else torch.randn((E, N), generator=g)).to(dt).to(DEV)
    idx = routing(c, g)
    live = ((idx >= 0) & (idx < E)).to(DEV)
    yref, a = mref.experts(x, idx, mref.dequant(q, s), bias)
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tol = eps * yref.abs() + (K + 2) * 2.0 ** -23 * a + (2.0 ** -24 if dt == torch.float16 else 1e-38)
    forms = forms_of(c)
    outs = {}
    for f in forms:
        y = ext.forward(x, idx.to(DEV), q, s, bias, form=FORMS.index(f))
        assert y.dtype == dt and y.shape == (T, S, N)
        assert torch.isfinite(y).all(), f"{f}: non-finite output"
        assert (y[~live] == 0).all(), f"{f}: a skipped slot is not zero"
        if exact:
            assert torch.equal(y, yref.to(dt)), f"{f}: not bit-exact on exact data"
        else:
            err = (y.double() - yref).abs()
            assert (err <= tol).all(), f"{f}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"
        outs[f] = y
    y = ext.forward(x, idx.to(DEV), q, s, bias)  # the plan's own choice is one of the forms above
    assert any(torch.equal(y, o) for o in outs.values()), "the planned form differs from every forced one"
    return forms


def run(cases=300, seed=1):
    rng = np.random.default_rng(seed)
    ok, bad, refused, forms = 0, [], {}, {f: 0 for f in FORMS}
    for _ in range(cases):
        c = draw(rng)
        try:
            got = run_case(c)
            torch.cuda.synchronize()
        except RuntimeError as err:
            key = str(err)[:100]
            refused[key] = refused.get(key, 0) + 1
            continue
        except AssertionError as err:
            bad.append(f"{c}: {str(err)[:300]}")
            continue
        ok += 1
        for f in got:
            forms[f] += 1
    return {"cases": cases, "seed": seed, "ok": ok, "bad": bad, "refused": refused, "forms": forms}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 300, int(sys.argv[2]) if len(sys.argv) > 2 else 1), indent=1))
