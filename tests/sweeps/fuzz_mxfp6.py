#!/usr/bin/env python3
"""Randomised sweep of the MXFP6 weight-only linear layer (MXFP6LinearCuda's kernels, csrc/mxfp6.hip) around its form boundaries, each
configuration on every form that accepts it, against the check of the fixed-shape tests (test_mxfp6_gpu.py): the float64 product of x
with mxfp6_ref.dequant, within eps * |y| + (K + 2) * 2^-23 * sum |x W| + tiny (exact products, an fp32 sum, one rounding).

  normal     Gaussian x and random weights: every form within the tolerance
  exact      integer x, scale codes 125 .. 129, integer bias: every form bit-identical to the float64 product
  nonfinite  one row of x holds a NaN or an inf: the other rows equal the run without it, on every form

The helpers rand_mx / ref_y / check / decode_bound are shared with test_mxfp6_gpu.py.  draw(rng) returns a plain configuration and
forms_of(cfg, b) the forms it runs (b = the decode form's largest M), so a CPU test can see what a seed covers.  A refusal (RuntimeError
with the library's message) is counted as skipped; a wrong value, an unexpected NaN or a crash is a finding.
usage: python tests/sweeps/fuzz_mxfp6.py [cases=200] [seed=1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mxfp6_ref as ref  # noqa: E402

DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
# decode128 / 64 / 32: the decode form's threads per column group (chosen from K / 32); prefill: the 128 x 128 tile GEMM
FORMS = ("decode128", "decode64", "decode32", "prefill")
M_SET = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 48, 64, 65, 127, 128, 129, 257, 300, 1000]
K_SET = [32, 64, 96, 160, 288, 1056, 1920, 2048, 2880, 4096, 4128, 6144, 11008]
MODES = ("normal", "normal", "exact", "nonfinite")


def decode_bound() -> int:
    """The largest M the decode form takes: bie_mxfp6_linear_forward refuses form 0 beyond it, before any launch."""
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20
    b = 0
    while L.bie_mxfp6_linear_forward(None, fake, fake, fake, None, fake, b + 1, 8, 64, 0, 0, None) == -1:  # -1: the NULL x, found after the form check
        b += 1
        assert b < 4096
    return b


def plan_bound() -> int:
    """The largest M at which the plan takes the decode form (BIE_MXFP6_FORM unset)."""
    from bitorch_engine import _hip
    L = _hip.lib()
    b = 0
    while L.bie_mxfp6_form(b + 1, 4096, 4096, 0) == 0:
        b += 1
        assert b < 4096
    return b


def decode_group(K: int) -> int:
    """mx6_decode_group of csrc/mxfp6.hip: the largest of 128, 64, 32 threads per column group whose last pass wastes at most an eighth."""
    KB = K // 32
    for g in (128, 64):
        if -(-KB // g) * g * 8 <= KB * 9:
            return g
    return 32


def rand_mx(N, K, g, lo=118, hi=130):
    q = torch.randint(0, 256, (N, K // 32 * 24), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(lo, hi + 1, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


def ref_y(x, W, bias=None):
    """float64 x . W^T (+ bias) on the GPU, with the absolute-value product the tolerance scales with."""
    xd, Wd = x.to(DEV).double(), W.to(DEV)
    y = xd @ Wd.t()
    a = xd.abs() @ Wd.abs().t()
    if bias is not None:
        y = y + bias.to(DEV).double()
        a = a + bias.to(DEV).double().abs()
    return y, a


def tolerance(yref, absprod, K, dt):
    """tests/test_mxfp4_gpu.py::check's: exact products, an fp32 sum, one rounding to dt."""
    eps = 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7
    tiny = 2.0 ** -24 if dt == torch.float16 else 1e-38
    return eps * yref.abs() + (K + 2) * 2.0 ** -23 * absprod + tiny


def check(y, yref, absprod, K, dt, what=""):
    tol = tolerance(yref, absprod, K, dt)
    err = (y.double() - yref).abs()
    assert torch.isfinite(y).all(), f"{what}: non-finite output"
    assert (err <= tol).all(), f"{what}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def draw(rng):
    M = int(rng.choice(M_SET))
    K = int(rng.choice(K_SET))
    u = rng.random()
    if u < 0.5:
        N = int(rng.integers(1, 71))
    else:
        N = max(1, 16 * int(rng.integers(1, 40)) + int(rng.integers(-1, 2)))
    return dict(M=M, N=N, K=K, dt=str(rng.choice(list(DTS))), mode=str(rng.choice(MODES)), bias=bool(rng.integers(0, 2)),
                seed=int(rng.integers(0, 2 ** 31)))


def forms_of(c, b):
    out = []
    if c["M"] <= b:
        out.append(f"decode{decode_group(c['K'])}")
    out.append("prefill")
    return out


def _ext():
    from bitorch_engine.extensions import mxfp6_linear_cuda
    return mxfp6_linear_cuda


def run_case(c, b):
    ext = _ext()
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, dt, mode = c["M"], c["N"], c["K"], DTS[c["dt"]], c["mode"]
    forms = forms_of(c, b)
    fid = {f: (0 if f.startswith("decode") else 1) for f in forms}
    if mode == "exact":  # K <= 4128: every partial sum a multiple of 2^-5 (E2M3's 2^-3 under 2^-2) below 4128 * 2 * 7.5 * 4 < 2^18: 23
        K = min(K, 4128)  # bits, exact in fp32
        q, s = rand_mx(N, K, g, 125, 129)
        x = torch.randint(-2, 3, (M, K), generator=g).to(dt)
        bias = torch.randint(-8, 9, (N,), generator=g).to(dt) if c["bias"] else None
        yref, _ = ref_y(x, ref.dequant(q, s), bias)
        for f in forms:
            y = ext.forward(x.to(DEV), q.to(DEV), s.to(DEV), None if bias is None else bias.to(DEV), form=fid[f])
            assert torch.equal(y, yref.to(dt)), f"{f}: not bit-exact on exact data"
        return forms
    q, s = rand_mx(N, K, g)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    bias = (torch.randn(N, generator=g)).to(dt) if c["bias"] else None
    bd = None if bias is None else bias.to(DEV)
    qd, sd = q.to(DEV), s.to(DEV)
    e = ext.col_exp(sd)
    yref, a = ref_y(x, ref.dequant(q, s), bias)
    outs = {}
    for f in forms:
        y = ext.forward(x.to(DEV), qd, sd, bd, e if fid[f] else None, form=fid[f])
        assert y.dtype == dt and y.shape == (M, N)
        check(y, yref, a, K, dt, f)
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
            assert not torch.isfinite(y[row]).all(), f"{f}: the non-finite value did not reach its row"
            assert torch.equal(y[keep], outs[f][keep]), f"{f}: a non-finite row changed its neighbours"
    y = ext.forward(x.to(DEV), qd, sd, bd)  # the plan's own choice is one of the forms above
    assert any(torch.equal(y, o) for o in outs.values()), "the planned form differs from every forced one"
    return forms


def run(cases=200, seed=1):
    rng = np.random.default_rng(seed)
    b = decode_bound()
    ok, bad, refused, forms = 0, [], {}, {f: 0 for f in FORMS}
    for _ in range(cases):
        c = draw(rng)
        try:
            got = run_case(c, b)
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
    return {"cases": cases, "seed": seed, "decode_bound": b, "ok": ok, "bad": bad, "refused": refused, "forms": forms}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1), indent=1))
