#!/usr/bin/env python3
"""Randomised sweeps of the ternary linear (tern), ternary conv2d (tconv), ternary W1.58A8 linear (ta8) and MXFP4 linear (mx) kernels at
their form boundaries, each configuration on every form that accepts it, against the high-precision references of the fixed-shape tests
(test_ternary_gpu.py, test_ternary_conv_gpu.py, test_ternary_a8_gpu.py, test_mxfp4_gpu.py, mxfp4_ref.py):

  tern   raw D bit-exact against the float64 product on both forms, y bit-exact against dt(dt(dt(D) * scale_a) * alpha), the decode and
         matrix-pipe forms bit-identical; tie-heavy inputs (x + bias_a cancelling exactly), +-0, NaN and +-inf
  ta8    q and r equal to the torch restatement, the raw int32 D exact, y bit-exact, the decode / GEMM / raw outputs in agreement; all-zero
         rows, one dominant value, fp16 subnormals, bf16 extremes, wide per-row spreads; K at each decode instance's LDS bound and past it
  tconv  every form that can run the geometry gives D and y bit-exact and identical to the others, and the chosen form is one of them
  mx     both forms (where M <= 16) within the contract tolerance; on exact data bit-identical to each other and to the float64 product

draw(op, rng) returns a plain configuration and forms_of(op, cfg) the forms it runs (host predicates only), so a CPU test can see what a
seed covers.  A refusal (RuntimeError with the library's message) is fine; a wrong value, an unexpected NaN or a crash is a finding.
   usage: python tests/sweeps/fuzz_ternary_mx.py [cases=60 per operator] [seed=1]"""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "bitorch-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import test_mxfp4_gpu as MX  # noqa: E402
import test_ternary_a8_gpu as TA  # noqa: E402
import test_ternary_conv_gpu as TC  # noqa: E402
import test_ternary_gpu as TG  # noqa: E402

DEV = "cuda"
OPS = ("tern", "tconv", "ta8", "mx")
DTS = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
# every form each op has; forms_of() names the ones a configuration runs.  "decode_wide": the decode form with N > 16384, where a
# workgroup walks more than one 16-column sweep (cols = ceil(ceil(N / 1024) / 16) * 16 > 16)
FORMS = {"tern": ("decode", "decode_wide", "mfma"),
         "ta8": ("decode1", "decode2", "decode4", "decode8", "decode_wide", "gemm128", "gemm256"),
         "tconv": ("general", "valu", "mfma"),
         "mx": ("decode1", "decode2", "decode4", "decode8", "decode16", "prefill")}
TERN_K_MAX = 131040   # the decode form's LDS bound at 4 rows (ternary.hip)
TA8_K_MAX = {1: 64512, 2: 32256, 4: 16128, 8: 8064}   # R * K <= 64512 (ternary_a8.hip)
M_SET = [1, 2, 3, 4, 5, 8, 16, 17, 31, 33, 64, 65, 128, 257, 300, 1000]


def _lib():
    from bitorch_engine import _hip
    return _hip.lib()


def _n(rng, small_m):
    u = rng.random()
    if small_m and u < 0.15:
        return int(rng.choice([16385, 17000, 20000, 28672, 32000]))
    if u < 0.5:
        return int(rng.integers(1, 71))
    return max(1, 16 * int(rng.integers(1, 80)) + int(rng.integers(-1, 2)))


def draw(op, rng):
    """One random configuration of `op` (a dict of plain values)."""
    seed = int(rng.integers(1 << 30))
    if op == "tern":
        M = int(rng.choice(M_SET))
        N = _n(rng, M <= 5)
        u = rng.random()
        if u < 0.1 and M <= 5 and N <= 70:
            K = int(rng.choice([TERN_K_MAX - 32, TERN_K_MAX, TERN_K_MAX + 32]))
        elif N > 16384 or M >= 128:
            K = 32 * int(rng.integers(1, 33))
        else:
            K = 32 * int(rng.integers(1, 129))
        return dict(op=op, M=M, N=N, K=K, dt=str(rng.choice(list(DTS))), x=str(rng.choice(["normal", "ties", "zeros", "nonfinite"])),
                    bias=bool(rng.random() < 0.8), seed=seed)
    if op == "ta8":
        u = rng.random()
        if u < 0.12:  # the 256 x 256 GEMM instance and its neighbours: ceil(M/256) * ceil(N/256) around 192
            M = int(rng.choice([1000, 1500, 2048, 3000]))
            t_m = -(-M // 256)
            N = 256 * (-(-192 // t_m) + int(rng.integers(-1, 2))) + int(rng.integers(-3, 4))
            K = 32 * int(rng.integers(1, 5))
        else:
            M = int(rng.choice(M_SET))
            N = _n(rng, M <= 8)
            R = 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8
            if M <= 8 and N <= 70 and rng.random() < 0.3:
                K = min(65536, TA8_K_MAX[R] + 32 * int(rng.choice([-1, 0, 0, 1, 1])))
            elif N > 16384 or M >= 1000:
                K = 32 * int(rng.integers(1, 33))
            elif rng.random() < 0.1 and M <= 64 and N <= 70:
                K = 32 * int(rng.integers(1, 2049))  # up to 65536
            else:
                K = 32 * int(rng.integers(1, 129))
        return dict(op=op, M=M, N=N, K=K, dt=str(rng.choice(list(DTS))), seed=seed,
                    rows=[str(rng.choice(["normal", "zero", "dominant", "subnormal", "extreme", "spread"])) for _ in range(min(M, 6))])
    if op == "tconv":
        while True:
            C = int(rng.choice([64, 128, 256, 512])) if rng.random() < 0.6 else 32 * int(rng.integers(1, 18))
            k = int(rng.choice([1, 3, 3, 5]))
            st, pad, dil = int(rng.choice([1, 1, 2, 3])), int(rng.integers(0, 3)), int(rng.choice([1, 1, 1, 2]))
            ow = int(rng.choice([int(rng.integers(1, 40)), 64 + int(rng.integers(-2, 3)), 128 + int(rng.integers(-2, 3))]))
            W = (ow - 1) * st + dil * (k - 1) + 1 - 2 * pad + int(rng.integers(0, st))
            if W < 1:
                continue
            B = int(rng.integers(1, 3)) if ow > 40 else int(rng.integers(1, 9))
            H = int(rng.integers(1, 7)) if ow > 40 else int(rng.integers(1, 20))
            OC = int(rng.choice([1, 16, 31, 64, 65, 100, 128, 130]))
            OH = (H + 2 * pad - dil * (k - 1) - 1) // st + 1
            if H + 2 * pad < dil * (k - 1) + 1 or OH < 1 or B * OH * ow * OC * C * k * k > 1.5e8:
                continue
            return dict(op=op, B=B, C=C, H=H, W=W, OC=OC, k=k, st=st, pad=pad, dil=dil, dt=str(rng.choice(list(DTS))), seed=seed)
    if op == "mx":
        u = rng.random()
        M = int(rng.integers(1, 17)) if u < 0.6 else int(rng.choice([17, 31, 33, 100, 129, 200, 300]))
        w = 4 if rng.random() < 0.5 else 8
        N = w * int(rng.integers(0, 130)) + int(rng.integers(1, w + 1))
        K = 32 * (int(rng.integers(1, 130)) if rng.random() < 0.85 else int(rng.integers(130, 300)))
        return dict(op=op, M=M, N=N, K=K, dt=str(rng.choice(["f16", "bf16"])), scales=str(rng.choice(["narrow", "wide", "exact"])),
                    bias=bool(rng.random() < 0.5), seed=seed)
    raise ValueError(op)


def _ta8_r(M):
    return 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8


TCONV_FORMS = {0: "general", 1: "valu", 2: "mfma"}


def forms_of(op, c):
    """The forms configuration c runs, from the library's host predicates (no GPU needed)."""
    L = _lib()
    if op == "tern":
        f = ["mfma"]
        if L.bie_ternary_linear_fused_ok(c["M"], c["N"], c["K"]):
            f.append("decode_wide" if c["N"] > 16384 else "decode")
        return f
    if op == "ta8":
        M, N = c["M"], c["N"]
        f = ["gemm256" if -(-M // 256) * -(-N // 256) >= 192 else "gemm128"]
        if L.bie_ternary_a8_fused_ok(M, N, c["K"]):
            f.append(f"decode{_ta8_r(M)}")
            if N > 16384:
                f.append("decode_wide")
        return f
    if op == "tconv":  # the general path always runs; bie_ternary_conv2d_form's choice is the one-launch form the layer takes
        f = TCONV_FORMS[L.bie_ternary_conv2d_form(c["B"], c["C"], c["H"], c["W"], c["OC"], c["k"], c["st"], c["pad"], c["dil"])]
        return sorted({"general", f})
    if op == "mx":
        M = c["M"]
        f = ["prefill"]
        if M <= 16:
            f.append(f"decode{next(r for r in (1, 2, 4, 8, 16) if M <= r)}")
        return f
    raise ValueError(op)


# ---- tern --------------------------------------------------------------------------------------------------------------------------
def _tern_inputs(c, g):
    M, K, dt = c["M"], c["K"], DTS[c["dt"]]
    if c["x"] == "ties":  # small integers: x + bias_a is exactly zero at about one position in seven, and at chosen ones of row 0
        x = torch.randint(-3, 4, (M, K), generator=g).to(dt)
        bias = torch.randint(-3, 4, (K,), generator=g).to(dt)
        at = torch.rand(K, generator=g) < 0.3
        bias[at] = -x[0, at]
    else:
        x = torch.randn((M, K), generator=g).to(dt)
        bias = (torch.randn(K, generator=g) * 0.2).to(dt)
        if c["x"] == "zeros":
            x.view(-1)[::3] = 0.0
            x.view(-1)[1::5] = -0.0
            bias[::2] = 0.0
        elif c["x"] == "nonfinite":
            n = x.numel()
            for v in (float("nan"), float("inf"), float("-inf")):
                x.view(-1)[torch.randint(0, n, (max(1, n // 97),), generator=g)] = v
    if not c["bias"]:
        bias.zero_()
    return x, bias


def run_tern(c):
    ext = TG.ext()
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, dt = c["M"], c["N"], c["K"], DTS[c["dt"]]
    t = TG.rand_trits(N, K, g)
    q = ext.w_pack(t.to(DEV))
    x, bias = _tern_inputs(c, g)
    sa = torch.tensor(float(torch.rand(1, generator=g)) * 0.1 + 0.01).to(dt)
    alpha = (torch.rand(N, generator=g) * 0.1).to(dt)
    xd, bd = x.to(DEV), (bias.to(DEV) if c["bias"] else None)
    want_D = TG.ref_D(TG.signs(xd, bias.to(DEV)).to(DEV), t.to(DEV)).cpu()
    layer = types.SimpleNamespace(bias_a=bias, scale_a=sa, scale_w=alpha)
    want_y = TG._ref_layer(x, layer, t, dt)
    forms = forms_of("tern", c)
    ys = {}
    D = ext.linear_fp4(xd.float(), q, None if bd is None else bd.float())
    assert torch.equal(D.cpu().double(), want_D), "matrix-pipe raw D"
    ys["mfma"] = ext.linear_fp4(xd, q, bd, sa.to(DEV), alpha.to(DEV))
    if any(f.startswith("decode") for f in forms):
        D = ext.linear_fused(xd, q, bd, raw=True)
        assert torch.equal(D.cpu().double(), want_D), "decode raw D"
        ys["decode"] = ext.linear_fused(xd, q, bd, sa.to(DEV), alpha.to(DEV))
    for f, y in ys.items():
        assert y.dtype == dt and torch.equal(y.cpu(), want_y), f"{f} y"
    y = ext.layer_forward(xd, bd, q, sa.to(DEV), alpha.to(DEV), cache=False)
    assert torch.equal(y.cpu(), want_y), "layer_forward y"
    return forms


# ---- ta8 ---------------------------------------------------------------------------------------------------------------------------
def _ta8_x(c, g):
    M, K, dt = c["M"], c["K"], DTS[c["dt"]]
    x = torch.randn((M, K), generator=g) * torch.rand((M, 1), generator=g) * 4
    big = 65504.0 if dt == torch.float16 else 3.3895e38
    for m, kind in enumerate(c["rows"]):
        if kind == "zero":
            x[m] = 0.0
        elif kind == "dominant":
            x[m] *= 1e-3
            x[m, int(torch.randint(0, K, (1,), generator=g))] = float(torch.randn(1, generator=g)) * 50
        elif kind == "subnormal":  # fp16 subnormals (2^-24 .. 2^-14), exact in every dtype
            x[m] = torch.randint(-1023, 1024, (K,), generator=g).float() * 2.0 ** -24
        elif kind == "extreme":  # the dtype's largest finite magnitudes next to its smallest normals
            x[m] = torch.where(torch.rand(K, generator=g) < 0.5, torch.finfo(dt).tiny, -torch.finfo(dt).tiny)
            x[m, 0], x[m, K // 2] = big, -big
        elif kind == "spread":  # magnitudes over 2^-20 .. 2^12 within the row
            x[m] = torch.randn(K, generator=g) * torch.exp2(torch.randint(-20, 13, (K,), generator=g).float())
    return x.to(dt)


def run_ta8(c):
    ext = TA.ext()
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, dt = c["M"], c["N"], c["K"], DTS[c["dt"]]
    t = TA.rand_trits(N, K, g)
    qw = ext.w_pack(t.to(DEV))
    x = _ta8_x(c, g).to(DEV)
    alpha = (torch.rand(N, generator=g) * 0.05 + 0.001).to(dt)
    rq, rr = TA.ref_quant(x)
    q, r = ext.quantize(x)
    assert torch.equal(q.cpu(), rq), "q"
    assert torch.equal(r.cpu(), rr), "r"
    want_D = TA.ref_D(rq, t)
    want_y = TA.ref_y(want_D, rr, alpha, dt)
    forms = forms_of("ta8", c)
    assert torch.equal(ext.linear_gemm(x, qw, raw=True).cpu().long(), want_D), "GEMM raw D"
    assert torch.equal(ext.linear_gemm(x, qw, alpha.to(DEV)).cpu(), want_y), "GEMM y"
    if any(f.startswith("decode") for f in forms):
        assert torch.equal(ext.linear_fused(x, qw, raw=True).cpu().long(), want_D), "decode raw D"
        assert torch.equal(ext.linear_fused(x, qw, alpha.to(DEV)).cpu(), want_y), "decode y"
    assert torch.equal(ext.layer_forward(x, qw, alpha.to(DEV)).cpu(), want_y), "layer_forward y"
    return forms


# ---- tconv -------------------------------------------------------------------------------------------------------------------------
def run_tconv(c):
    ext = TC.ext()
    g = torch.Generator().manual_seed(c["seed"])
    B, C, H, W, OC, k, st, pad, dil = (c[n] for n in ("B", "C", "H", "W", "OC", "k", "st", "pad", "dil"))
    dt = DTS[c["dt"]]
    x = TC.special_input((B, C, H, W), g).to(dt)
    t = TC.rand_trits((OC, C, k, k), g, float(torch.rand(1, generator=g)))
    q = ext.w_pack(t.to(DEV))
    alpha = (torch.rand(OC, generator=g) * 0.1).to(dt)
    sa = torch.tensor(0.37, dtype=dt)
    want = TC.ref_D(x.float(), t, st, pad, dil)
    want_y = TC.ref_layer(want, sa, alpha, dt)
    raw = TC.all_forms(x.to(DEV), q, k, st, pad, dil, raw=True)
    ys = TC.all_forms(x.to(DEV), q, k, st, pad, dil, scale_a=sa.to(DEV), alpha=alpha.to(DEV))
    assert raw.keys() == ys.keys()
    for f, D in raw.items():  # every form against the reference is also every form against every other
        assert torch.equal(D.cpu().double(), want), f"{TCONV_FORMS[f]} raw D"
        assert ys[f].dtype == dt and torch.equal(ys[f].cpu(), want_y), f"{TCONV_FORMS[f]} y"
    chosen = ext.form(B, C, H, W, OC, k, st, pad, dil)
    assert chosen in raw, f"form() chose {chosen}, which does not run"
    assert torch.equal(ext.forward(x.to(DEV), q, k, st, pad, dil).cpu().double(), want), "the dispatch's D"
    return sorted(TCONV_FORMS[f] for f in raw)


# ---- mx ----------------------------------------------------------------------------------------------------------------------------
def run_mx(c):
    ext = MX.ext()
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, dt = c["M"], c["N"], c["K"], DTS[c["dt"]]
    mode = c["scales"]
    if mode == "exact":  # every partial sum a multiple of 2^-3 below 2^21: exact in fp32 in any order
        K = min(K, 8192)
        qw, s = MX.rand_mx(N, K, g, 125, 129)
        x = torch.randint(-2, 3, (M, K), generator=g).to(dt)
        bias = torch.randint(-8, 9, (N,), generator=g).to(dt) if c["bias"] else None
    elif mode == "wide":  # per column a range of scale codes inside 103 .. 143 (2^-24 .. 2^16)
        qw = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
        lo = torch.randint(103, 144, (N, 1), generator=g)
        hi = torch.minimum(lo + torch.randint(0, 41, (N, 1), generator=g), torch.tensor(143))
        s = (lo + (torch.rand((N, K // 32), generator=g) * (hi - lo + 1)).floor().long()).clamp(103, 143).to(torch.uint8)
        x = (torch.randn((M, K), generator=g) * 2.0 ** -12).to(dt)
        bias = (torch.randn(N, generator=g)).to(dt) if c["bias"] else None
    else:
        qw, s = MX.rand_mx(N, K, g)
        x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
        bias = (torch.randn(N, generator=g)).to(dt) if c["bias"] else None
    W = MX.ref.dequant(qw, s)
    yref, a = MX.ref_y(x, W, bias)
    qd, sd = qw.to(DEV), s.to(DEV)
    e = ext.col_exp(sd)
    colmax = MX.ref.e8m0(e.cpu()).to(DEV)
    forms = forms_of("mx", c)
    outs = {}
    for f in forms:
        form = 1 if f == "prefill" else 0
        y = ext.forward(x.to(DEV), qd, sd, None if bias is None else bias.to(DEV), e, form=form)
        assert y.dtype == dt and y.shape == (M, N)
        outs[f] = y
        if mode == "exact":
            assert torch.equal(y, yref.to(dt)), f"{f}: not bit-exact on exact data"
            continue
        rebias = x.to(DEV).double().abs().sum(1, keepdim=True) * colmax[None, :] * 2.0 ** -24 if form == 1 and dt == torch.float16 else 0.0
        eps, tiny = (2.0 ** -10, 2.0 ** -24) if dt == torch.float16 else (2.0 ** -7, 1e-38)
        tol = eps * yref.abs() + (K + 2) * 2.0 ** -23 * a + rebias + tiny
        assert torch.isfinite(y).all(), f"{f}: non-finite output"
        err = (y.double() - yref).abs()
        assert (err <= tol).all(), f"{f}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"
    y = ext.forward(x.to(DEV), qd, sd, None if bias is None else bias.to(DEV))  # the plan's own choice is one of the forms above
    assert any(torch.equal(y, o) for o in outs.values()), "the planned form differs from every forced one"
    return forms


RUN = {"tern": run_tern, "ta8": run_ta8, "tconv": run_tconv, "mx": run_mx}


def run(cases=60, seed=1, ops=OPS):
    rng = np.random.default_rng(seed)
    res = {}
    for op in ops:
        ok, bad, refused, forms = 0, [], {}, {f: 0 for f in FORMS[op]}
        for _ in range(cases):
            c = draw(op, rng)
            try:
                got = RUN[op](c)
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
        res[op] = {"ok": ok, "bad": bad, "refused": refused, "forms": forms}
    return {"cases_per_op": cases, "seed": seed, "ops": res}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 1), indent=1))
