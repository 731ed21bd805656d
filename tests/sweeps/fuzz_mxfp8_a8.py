#!/usr/bin/env python3
"""Randomised sweep of the MXFP8 W8A8 linear layer (MXFP8A8LinearCuda's kernels) around its form boundaries, each configuration on every
form that accepts it, against the references of the fixed-shape tests (test_mxfp8_a8_gpu.py, mxfp8_a8_ref.py):

  normal   Gaussian x and random weights: the activation quantiser bit-exact, every form within the contract tolerance of the float64
           product of x^ and W^
  exact    the E4M3 codes of the integers -7 .. 7 on both sides under scales 2^-1 .. 2^1 through gemm(): every form bit-identical to
           the float64 product
  nonfinite  one row of x holds a NaN or an inf: that row of y is NaN on every form, the others equal the run without it

draw(rng) returns a plain configuration and forms_of(cfg) the forms it runs (host predicates only), so a CPU test can see what a seed
covers.  A refusal (RuntimeError with the library's message) is counted as skipped; a wrong value, an unexpected NaN or a crash is a
finding.    usage: python tests/sweeps/fuzz_mxfp8_a8.py [cases=200] [seed=1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mxfp8_a8_ref as ref  # noqa: E402

DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
# decode16 / 32 / 64: the decode form's row instances; prefill64 / prefill128: the prefill form's 64 x 64 and 128 x 128 tiles
FORMS = ("decode16", "decode32", "decode64", "prefill64", "prefill128")
DECODE_ROWS = 64
M_SET = [1, 2, 3, 5, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128, 129, 257, 300, 1000]
K_SET = [32, 64, 96, 128, 160, 224, 256, 288, 1024, 1056, 2048, 4096, 4128, 11008]
MODES = ("normal", "normal", "exact", "nonfinite")


def draw(rng):
    M = int(rng.choice(M_SET))
    K = int(rng.choice(K_SET))
    u = rng.random()
    if u < 0.2:   # enough 128 x 128 tiles for the prefill form's wide instance
        M = int(rng.choice([2048, 3000, 4096]))
        N = 128 * int(rng.integers(16, 33)) + int(rng.integers(-1, 2)) * int(rng.integers(0, 4))
        K = int(rng.choice([32, 96, 128, 160, 1056]))
    elif u < 0.6:
        N = int(rng.integers(1, 71))
    else:
        N = max(1, 16 * int(rng.integers(1, 80)) + int(rng.integers(-1, 2)))
    return dict(M=M, N=N, K=K, dt=str(rng.choice(list(DTS))), mode=str(rng.choice(MODES)), bias=bool(rng.integers(0, 2)),
                seed=int(rng.integers(0, 2 ** 31)))


def _cdiv(a, b):
    return (a + b - 1) // b


def forms_of(c):
    """The forms a configuration runs: the decode instance of its M (M <= 64) and the prefill tile the launcher picks for (M, N)."""
    M, N = c["M"], c["N"]
    out = []
    if M <= DECODE_ROWS:
        out.append("decode16" if M <= 16 else "decode32" if M <= 32 else "decode64")
    out.append("prefill128" if _cdiv(M, 128) * _cdiv(N, 128) >= 512 else "prefill64")
    return out


def _ext():
    from bitorch_engine.extensions import mxfp8_a8_linear_cuda
    return mxfp8_a8_linear_cuda


def run_case(c):
    ext = _ext()
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, dt, mode = c["M"], c["N"], c["K"], DTS[c["dt"]], c["mode"]
    forms = forms_of(c)
    fid = {f: (0 if f.startswith("decode") else 1) for f in forms}
    if mode == "exact":  # integer codes |m| <= 7 and scales 2^-1 .. 2^1 on both sides: every product is a multiple of 2^-2 and every
        K = min(K, 1056)  # partial sum stays below 1056 * 49 * 4 < 2^18: 20 bits, exact in fp32
        q = torch.randint(-7, 8, (N, K), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
        s = torch.randint(126, 129, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
        xq = torch.randint(-7, 8, (M, K), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
        xs = torch.randint(126, 129, (M, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
        flag = torch.zeros(M, dtype=torch.uint8)
        bias = torch.randint(-8, 9, (N,), generator=g).to(dt) if c["bias"] else None
        yref, _ = ref.reference(xq, xs, flag, q, s, bias, DEV)
        for f in forms:
            y = ext.gemm(xq.to(DEV), xs.to(DEV), flag.to(DEV), q.to(DEV), s.to(DEV), None if bias is None else bias.to(DEV), dtype=dt, form=fid[f])
            assert torch.equal(y, yref.to(dt)), f"{f}: not bit-exact on exact data"
        return forms
    q, s = ref.rand_w(N, K, g)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    bias = (torch.randn(N, generator=g)).to(dt) if c["bias"] else None
    bd = None if bias is None else bias.to(DEV)
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext.col_exp(sd)
    xq, xs, flag = ref.quantize_act(x)
    gq, gs, gf = ext.quantize_act(x.to(DEV))
    assert torch.equal(gq.cpu(), xq) and torch.equal(gs.cpu(), xs) and torch.equal(gf.cpu(), flag), "quantize_act differs from the restatement"
    yref, a = ref.reference(xq, xs, flag, q, s, bias, DEV)
    tol = ref.tolerance(yref, a, K, dt)
    outs = {}
    for f in forms:
        y = ext.forward(x.to(DEV), qd, sd, bd, e, form=fid[f])
        assert y.dtype == dt and y.shape == (M, N)
        assert torch.isfinite(y).all(), f"{f}: non-finite output"
        err = (y.double() - yref).abs()
        assert (err <= tol).all(), f"{f}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"
        outs[f] = y
    if mode == "nonfinite":
        row = int(torch.randint(0, M, (1,), generator=g))
        pos = int(torch.randint(0, K, (1,), generator=g))
        xb = x.clone()
        xb[row, pos] = [float("nan"), float("inf"), float("-inf")][c["seed"] % 3]
        keep = torch.ones(M, dtype=torch.bool)
        keep[row] = False
        for f in forms:
            y = ext.forward(xb.to(DEV), qd, sd, bd, e, form=fid[f])
            assert torch.isnan(y[row]).all(), f"{f}: the non-finite row is not NaN"
            assert torch.equal(y[keep], outs[f][keep]), f"{f}: a non-finite row changed its neighbours"
    y = ext.forward(x.to(DEV), qd, sd, bd)  # the plan's own choice is one of the forms above
    assert any(torch.equal(y, o) for o in outs.values()), "the planned form differs from every forced one"
    return forms


def run(cases=200, seed=1):
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
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1), indent=1))
