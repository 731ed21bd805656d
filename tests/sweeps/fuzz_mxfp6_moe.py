#!/usr/bin/env python3
"""Randomised sweep of the MXFP6 W6A16 mixture-of-experts expert GEMM (csrc/mxfp6_moe.hip) against the restatement (mxfp4_moe_ref.experts
on mxfp6_ref.dequant of the stacked weights): E, S, T, K and N at the form and tile boundaries, skewed routing with skipped slots, both
dtypes, both x_per_pair values, each configuration on every form that accepts it:

  normal     Gaussian x and random weights: every form within the weight-only contract's tolerance of the float64 product per pair,
             skipped slots exactly +0
  exact      integer x, scale codes 125 .. 129, integer bias, K <= 4128: every form bit-identical to the float64 product rounded once
  nonfinite  one stored row of x holds a NaN or an inf: the pairs of the other rows equal the run without it, on every form

draw(rng) returns a plain configuration and forms_of(cfg) the forms it runs (host predicates only), so a CPU test can see what a seed
covers.  Only a RuntimeError that carries the library's refusal text (an argument check of the C entry or of the extension) counts as
refused; any other RuntimeError ends the run at once and is reported under "fatal", so nothing more is started on the device after a
fault.  A wrong value or an unexpected NaN is a finding.
    usage: python tests/sweeps/fuzz_mxfp6_moe.py [cases=300] [seed=1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests", "sweeps"), os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fuzz_mxfp6 as F6  # noqa: E402
import mxfp4_moe_ref as mref  # noqa: E402
import mxfp6_ref as m6  # noqa: E402

DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
# decode128 / 64 / 32: the routed decode form's threads per column group (chosen from K / 32); grouped: the routing kernel and the tile GEMM
FORMS = ("decode128", "decode64", "decode32", "grouped")
DECODE_PAIRS = 1024
S_SET = [1, 2, 3, 4, 8]
P_SET = [1, 2, 7, 64, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1300]  # pairs: around 1, the decode form's bound, the row tile's edges
K_SET = F6.K_SET
MODES = ("normal", "normal", "exact", "nonfinite")
MAX_W, MAX_Y = 1 << 22, 1 << 20  # E * N * K and P * N: the float64 reference stays well under a second
REFUSAL = ("failed with status -1:", "failed with status -2:", "mxfp6 experts:")


def draw(rng):
    S = int(rng.choice(S_SET))
    T = max(1, int(rng.choice(P_SET)) // S + int(rng.integers(0, 2)))
    E = int(rng.integers(1, 41))
    K = int(rng.choice(K_SET))
    N = int(rng.integers(1, 71)) if rng.random() < 0.5 else max(1, 16 * int(rng.integers(1, 20)) + int(rng.integers(-1, 2)))
    N = max(1, min(N, MAX_W // (E * K), MAX_Y // (T * S)))
    return dict(E=E, S=S, T=T, N=N, K=K, dt=str(rng.choice(list(DTS))), mode=str(rng.choice(MODES)), xpp=int(rng.integers(0, 2)),
                bias=bool(rng.integers(0, 2)), skew=float(rng.choice([0.0, 1.2, 3.0])), skip=float(rng.choice([0.0, 0.0, 0.3, 1.0])),
                seed=int(rng.integers(0, 2 ** 31)))


def k_of(c):
    return min(c["K"], 4128) if c["mode"] == "exact" else c["K"]  # exact: every partial sum below 2^18 in multiples of 2^-5


def forms_of(c):
    return ([f"decode{F6.decode_group(k_of(c))}"] if c["T"] * c["S"] <= DECODE_PAIRS else []) + ["grouped"]


def routing(c, g):
    """Zipf-skewed experts (exponent `skew`, 0 = uniform), a share `skip` of the slots replaced by out-of-range indices."""
    E, P = c["E"], c["T"] * c["S"]
    prob = 1.0 / torch.arange(1, E + 1, dtype=torch.float64) ** c["skew"]
    idx = torch.multinomial(prob / prob.sum(), P, replacement=True, generator=g).to(torch.int32)
    bad = torch.tensor([-1, E, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    skipped = torch.rand(P, generator=g) < c["skip"]
    idx[skipped] = bad[torch.randint(0, 4, (int(skipped.sum()),), generator=g)]
    return idx.reshape(c["T"], c["S"])


def dequant(q, s):
    """mxfp6_ref.dequant per expert, float64 [E, N, K] on the device the product runs on."""
    return torch.stack([m6.dequant(q[e], s[e]) for e in range(q.shape[0])]).to(DEV)


def run_case(c):
    from bitorch_engine.extensions import mxfp6_experts_cuda as ext
    g = torch.Generator().manual_seed(c["seed"])
    E, S, T, N, K, dt, mode = c["E"], c["S"], c["T"], c["N"], k_of(c), DTS[c["dt"]], c["mode"]
    exact = mode == "exact"
    lo, hi = (125, 129) if exact else (118, 130)
    q = torch.randint(0, 256, (E, N, K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    shape = (T, S, K) if c["xpp"] else (T, K)
    x = (torch.randint(-2, 3, shape, generator=g) if exact else torch.randn(shape, generator=g) * 0.5).to(dt)
    bias = None
    if c["bias"]:
        bias = (torch.randint(-8, 9, (E, N), generator=g) if exact else torch.randn((E, N), generator=g)).to(dt).to(DEV)
    idx = routing(c, g)
    live = ((idx >= 0) & (idx < E)).to(DEV)
    yref, a = mref.experts(x, idx, dequant(q, s), bias)
    tol = F6.tolerance(yref, a, K, dt)
    qd, sd, xd, idxd = q.to(DEV), s.to(DEV), x.to(DEV), idx.to(DEV)
    forms = forms_of(c)
    fid = {f: (0 if f.startswith("decode") else 1) for f in forms}
    outs = {}
    for f in forms:
        y = ext.forward(xd, idxd, qd, sd, bias, form=fid[f])
        assert y.dtype == dt and y.shape == (T, S, N)
        assert torch.isfinite(y).all(), f"{f}: non-finite output"
        assert (y[~live] == 0).all() and not torch.signbit(y[~live]).any(), f"{f}: a skipped slot is not +0"
        if exact:
            assert torch.equal(y, yref.to(dt)), f"{f}: not bit-exact on exact data"
        else:
            err = (y.double() - yref).abs()
            assert (err <= tol).all(), f"{f}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"
        outs[f] = y
    if mode == "nonfinite":
        flat = x.reshape(-1, K).clone()
        row = int(torch.randint(0, flat.shape[0], (1,), generator=g))
        flat[row, int(torch.randint(0, K, (1,), generator=g))] = [float("nan"), float("inf"), float("-inf")][c["seed"] % 3]
        hit = torch.zeros(flat.shape[0], dtype=torch.bool)
        hit[row] = True
        hit = (hit.reshape(T, S) if c["xpp"] else hit[:, None].expand(T, S)).to(DEV)
        for f in forms:
            y = ext.forward(flat.reshape(shape).to(DEV), idxd, qd, sd, bias, form=fid[f])
            assert not torch.isfinite(y[hit & live]).any(), f"{f}: the non-finite value did not reach its pairs"
            assert (y[hit & ~live] == 0).all(), f"{f}: a skipped slot of the non-finite row is not zero"
            assert torch.equal(y[~hit], outs[f][~hit]), f"{f}: a non-finite row changed other pairs"
    y = ext.forward(xd, idxd, qd, sd, bias)  # the plan's own choice is one of the forms above
    assert any(torch.equal(y, o) for o in outs.values()), "the planned form differs from every forced one"
    return forms


def run(cases=300, seed=1):
    rng = np.random.default_rng(seed)
    ok, bad, refused, fatal, forms = 0, [], {}, None, {f: 0 for f in FORMS}
    for _ in range(cases):
        c = draw(rng)
        try:
            got = run_case(c)
            torch.cuda.synchronize()
        except RuntimeError as err:
            if not any(t in str(err) for t in REFUSAL):  # not an argument refusal: nothing more is started on the device
                fatal = f"{c}: {str(err)[:300]}"
                break
            key = str(err)[:100]
            refused[key] = refused.get(key, 0) + 1
            continue
        except AssertionError as err:
            bad.append(f"{c}: {str(err)[:300]}")
            continue
        ok += 1
        for f in got:
            forms[f] += 1
    return {"cases": cases, "seed": seed, "ok": ok, "bad": bad, "refused": refused, "fatal": fatal, "forms": forms}


if __name__ == "__main__":
    r = run(int(sys.argv[1]) if len(sys.argv) > 1 else 300, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    print(json.dumps(r, indent=1))
    sys.exit(1 if r["fatal"] or r["bad"] else 0)
