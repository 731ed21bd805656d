#!/usr/bin/env python3
"""Randomised sweep of the MXFP6 input gradient (csrc/mxfp6_grad.hip), dense and grouped, around the edges of its tile (128 rows x 128 k,
stages of 32 n), against the references of the fixed-shape tests (test_mxfp6_grad_gpu.py, mxfp6_grad_ref.py):

  normal   Gaussian gy and random codes, scale codes 119 .. 130: within the contract tolerance of the float64 product (the grouped form
           in fp32 and in the dtype), skipped rows +0
  exact    integer gy in [-2, 2], scale codes 125 .. 129, N <= 4096: bit-identical to the float64 product rounded once and to the torch
           composition gy.float().mm(dequant)
  nan      one scale code set to 255: its block-column (of its expert) is NaN, every other element keeps its bits

draw(rng, small) returns a plain configuration; small=True bounds the shapes for the suite's slice.  A wrong value, an unexpected NaN or
a RuntimeError is a finding: no configuration drawn here is one the library refuses.
usage: python tests/sweeps/fuzz_mxfp6_grad.py [cases=300] [seed=1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mxfp6_grad_ref as gref  # noqa: E402

ref = gref.ref
DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
KINDS = ("dense", "grouped")
MODES = ("normal", "normal", "exact", "nan")
M_SET = [1, 2, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000]
K_SET = [32, 64, 96, 128, 160, 224, 256, 288, 1056, 2048, 4128]
N_EDGE = [1, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]


def draw(rng, small=False):
    kind = str(rng.choice(KINDS))
    K = int(rng.choice(K_SET[:8] if small else K_SET))
    N = int(rng.choice(N_EDGE)) if rng.random() < 0.6 else int(rng.integers(1, 300 if small else 1500))
    c = dict(kind=kind, K=K, N=N, dt=str(rng.choice(list(DTS))), mode=str(rng.choice(MODES)), seed=int(rng.integers(0, 2 ** 31)))
    if kind == "dense":
        c["M"] = int(rng.choice(M_SET[:13] if small else M_SET))
    else:
        c["E"] = int(rng.choice([1, 2, 3, 8]))
        c["S"] = int(rng.choice([1, 2, 4]))
        c["T"] = int(rng.choice([1, 5, 32, 33, 64, 65, 100] if small else [1, 5, 32, 33, 64, 65, 100, 257, 600]))
        if small:
            c["N"] = min(c["N"], 130)
    return c


def _lin():
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda
    return mxfp6_a8_linear_cuda


def _ext():
    from bitorch_engine.extensions import mxfp6_experts_a8_cuda
    return mxfp6_experts_a8_cuda


def _within(y, yref, a, n, dt, what):
    tol = gref.tolerance(yref, a, n, dt)
    err = (y.double() - yref).abs()
    assert torch.isfinite(y).all(), f"{what}: non-finite output"
    assert (err <= tol).all(), f"{what}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"


def run_dense(c, g):
    lin = _lin()
    M, N, K, dt, mode = c["M"], c["N"], c["K"], DTS[c["dt"]], c["mode"]
    lo, hi = (125, 129) if mode == "exact" else (119, 130)
    q, s = gref.rand_mx(N, K, g, lo, hi)
    qd, sd = q.to(DEV), s.to(DEV)
    if mode == "exact":
        gy = torch.randint(-2, 3, (M, N), generator=g).to(dt).to(DEV)
        gx = lin.grad_input(gy, qd, sd)
        assert torch.equal(gx, (gy.double() @ ref.dequant(q, s).to(DEV)).to(dt)), "dense: not bit-exact on exact data"
        assert torch.equal(gx, gy.float().mm(lin.dequant(qd, sd, torch.float32)).to(dt)), "dense: differs from the torch composition"
        return
    gy = (torch.randn((M, N), generator=g) * 0.5).to(dt).to(DEV)
    gx = lin.grad_input(gy, qd, sd)
    assert gx.dtype == dt and gx.shape == (M, K)
    gxref, a = gref.grad_reference(gy, q, s, DEV)
    _within(gx, gxref, a, N, dt, "dense")
    if mode == "nan":
        n, kb = int(torch.randint(0, N, (1,), generator=g)), int(torch.randint(0, K // 32, (1,), generator=g))
        s2 = s.clone()
        s2[n, kb] = 255
        bad = lin.grad_input(gy, qd, s2.to(DEV))
        keep = torch.ones(K, dtype=torch.bool, device=DEV)
        keep[32 * kb:32 * kb + 32] = False
        assert torch.isnan(bad[:, ~keep]).all(), "dense: the NaN block-column is not NaN"
        assert torch.equal(bad[:, keep], gx[:, keep]), "dense: a NaN block changed other columns"


def run_grouped(c, g):
    ext = _ext()
    T, S, E, N, K, dt, mode = c["T"], c["S"], c["E"], c["N"], c["K"], DTS[c["dt"]], c["mode"]
    P = T * S
    lo, hi = (125, 129) if mode == "exact" else (119, 130)
    q, s = gref.rand_mx(E * N, K, g, lo, hi)
    q, s = q.reshape(E, N, -1), s.reshape(E, N, -1)
    qd, sd = q.to(DEV), s.to(DEV)
    idx = torch.randint(-1, E + 1, (T, S), generator=g, dtype=torch.int32)  # -1 and E: skipped slots
    flat = idx.reshape(-1).long()
    live = (flat >= 0) & (flat < E)
    W = torch.stack([ref.dequant(q[e], s[e]) for e in range(E)]).to(DEV)
    We = W[flat.clamp(0, E - 1).to(DEV)]
    lv = live.to(DEV)
    if mode == "exact":
        gy = torch.randint(-2, 3, (P, N), generator=g).to(dt).to(DEV)
    else:
        gy = (torch.randn((P, N), generator=g) * 0.5).to(dt).to(DEV)
    gl = gy.double() * lv.double()[:, None]
    gxref, a = torch.einsum("pn,pnk->pk", gl, We), torch.einsum("pn,pnk->pk", gl.abs(), We.abs())
    gx = ext.grad_input(gy, idx.to(DEV), qd, sd)
    g32 = ext.grad_input(gy.reshape(T, S, N), idx.to(DEV), qd, sd, out_dtype=torch.float32)
    assert gx.dtype == dt and g32.dtype == torch.float32 and gx.shape == g32.shape == (P, K)
    assert (gx[~lv].view(torch.int16) == 0).all() and (g32[~lv].view(torch.int32) == 0).all(), "grouped: a skipped row is not +0"
    if mode == "exact":
        assert torch.equal(gx, gxref.to(dt)) and torch.equal(g32, gxref.float()), "grouped: not bit-exact on exact data"
        return
    _within(gx, gxref, a, N, dt, "grouped")
    _within(g32, gxref, a, N, torch.float32, "grouped fp32")
    if mode == "nan":
        e, n, kb = (int(torch.randint(0, hi_, (1,), generator=g)) for hi_ in (E, N, K // 32))
        s2 = s.clone()
        s2[e, n, kb] = 255
        bad = ext.grad_input(gy, idx.to(DEV), qd, s2.to(DEV))
        hit = torch.zeros((P, K), dtype=torch.bool, device=DEV)
        hit[(flat == e).to(DEV), 32 * kb:32 * kb + 32] = True
        assert torch.isnan(bad[hit]).all(), "grouped: the NaN block-column of the expert is not NaN"
        assert torch.equal(bad[~hit], gx[~hit]), "grouped: a NaN block changed other elements"


def run(cases=300, seed=1, small=False):
    rng = np.random.default_rng(seed)
    ok, bad, kinds = 0, [], {k: 0 for k in KINDS}
    for _ in range(cases):
        c = draw(rng, small)
        try:
            (run_dense if c["kind"] == "dense" else run_grouped)(c, torch.Generator().manual_seed(c["seed"]))
            torch.cuda.synchronize()
        except (AssertionError, RuntimeError) as err:
            bad.append(f"{c}: {type(err).__name__}: {str(err)[:300]}")
            if isinstance(err, RuntimeError):  # a device error: nothing more is started on the GPU
                break
            continue
        ok += 1
        kinds[c["kind"]] += 1
    return {"cases": cases, "seed": seed, "small": small, "ok": ok, "bad": bad, "kinds": kinds}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 300, int(sys.argv[2]) if len(sys.argv) > 2 else 1), indent=1))
