"""MXFP6 W6A8 linear layer, the parts that need no GPU: properties of the torch restatement (the E2M3 code table, ties, saturation, signs,
idempotence, pack / unpack), its error against the MXFP4 restatement's on weights and on the layer's product, the new entries in the
header, the ctypes table and the library, host-side argument validation of every new entry, the form plan / workspace size, the
layer's constructor, export and checkpoint rules, the fuzz generator's draws and the compiler's resource report for csrc/mxfp6_a8.hip."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import mxfp6_ref as ref  # noqa: E402

mx4 = ref.mx        # mxfp4_ref
a8 = ref.a8         # mxfp4_a8_ref

NEW = ("bie_mxfp6_quantize", "bie_mxfp6_dequant", "bie_mxfp6_a8_form", "bie_mxfp6_a8_workspace_bytes", "bie_mxfp6_a8_linear_forward",
       "bie_mxfp6_a8_gemm")
BENCH_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))  # (K, N)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_code_table_has_exactly_the_32_e2m3_magnitudes():
    want = ([0.125 * i for i in range(8)] + [1 + 0.125 * i for i in range(8)] + [2 + 0.25 * i for i in range(8)] + [4 + 0.5 * i for i in range(8)])
    assert ref.E2M3.tolist() == want and len(set(want)) == 32 and max(want) == ref.E2M3_MAX == 7.5
    assert torch.equal(ref.e2m3(torch.arange(32, 64, dtype=torch.uint8)), -ref.E2M3)
    assert torch.isfinite(ref.e2m3(torch.arange(64, dtype=torch.uint8))).all()  # no Inf / NaN code


def _block(vals, amax):
    """One block of 32: vals, then the block maximum, zeros behind."""
    w = torch.zeros((1, 32))
    w[0, :len(vals)] = torch.tensor(vals)
    w[0, 31] = amax
    return w


def test_ties_saturation_and_signs():
    # amax 4 * 2^t -> e = t, scale code t + 127: at t = 0 the scaled magnitudes are the values themselves
    for t in (0, -9, 6):
        s = 2.0 ** t
        vals = [0.0625, 0.1875, 1.9375, 0.3125, 1.0625, 2.125, 2.375, 3.875, 0.06, 0.07, -0.0, -0.03, -1.9375, 3.9, -0.1875]
        want = [0, 2, 16, 2, 8, 16, 18, 24, 0, 1, 0x20, 0x20, 0x30, 24, 0x22]
        c, sc = ref.quantize(_block([v * s for v in vals], 4.0 * s))
        assert sc.item() == t + 127 and c[0, 31].item() == 24
        assert c[0, :len(vals)].tolist() == want, (t, c[0, :len(vals)].tolist())
        # saturation: a block maximum in (7.5, 8) keeps e = t and clamps: 7.74, 7.8 (and the midpoint 7.75 to the absent 8) give 7.5
        for big in (7.74, 7.75, 7.8, 7.99):
            c, sc = ref.quantize(_block([-big * s, 4.25 * s, 4.75 * s], big * s))
            assert sc.item() == t + 127 and c[0, 31].item() == 31 and c[0, :3].tolist() == [0x3F, 24, 26], (t, big)
    for z in (0.0, -0.0):  # both zeros: scale code 0 and zero codes, hence 24 zero bytes
        c, sc = ref.quantize(torch.full((2, 64), z))
        assert not sc.any() and not c.any() and not ref.pack(c).any() and ref.pack(c).shape == (2, 48)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_rule_is_idempotent_and_pack_round_trips(dt):
    g = torch.Generator().manual_seed(3)
    for N, K in ((8, 4096), (33, 96), (3, 32)):
        w = (torch.randn((N, K), generator=g) * torch.exp2(torch.randint(-10, 10, (N, 1), generator=g).float())).to(dt)
        c, s = ref.quantize(w)
        q = ref.pack(c)
        assert q.shape == (N, 3 * K // 4) and torch.equal(ref.unpack(q), c) and (c < 64).all()
        W = ref.dequant(q, s)
        assert torch.equal(W.float().double(), W)
        if dt != torch.float16:  # W^ is a value of the dtype (not of fp16 in general: 0.125 * 2^e can lie below its smallest subnormal)
            assert torch.equal(W.to(dt).double(), W)
        c2, s2 = ref.quantize(W.float())
        assert torch.equal(c2, c) and torch.equal(s2, s)
    # every byte pattern is a weight: unpack . pack is the identity on codes, pack . unpack on bytes
    q = torch.randint(0, 256, (5, 72), generator=g, dtype=torch.uint8)
    assert torch.equal(ref.pack(ref.unpack(q)), q)
    # code j sits in bits 6 j .. 6 j + 5 of the block's little-endian 192-bit integer
    c = torch.zeros((1, 32), dtype=torch.uint8)
    for j in (0, 1, 5, 10, 21, 31):
        c.zero_()
        c[0, j] = 0x2B
        assert int.from_bytes(bytes(ref.pack(c)[0].tolist()), "little") == 0x2B << (6 * j)


def test_weight_error_is_less_than_half_of_mxfp4():
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        w = torch.randn((256, 4096), generator=g)
        wd = w.double()
        c6, s6 = ref.quantize(w)
        e6 = (ref.dequant(ref.pack(c6), s6) - wd).norm() / wd.norm()
        c4, s4 = mx4.quantize(w)
        e4 = (mx4.dequant(mx4.pack(c4), s4) - wd).norm() / wd.norm()
        print(f"seed {seed}: relative weight error mxfp6 {e6.item():.4f}, mxfp4 {e4.item():.4f}, ratio {(e6 / e4).item():.3f}")
        assert e6 < 0.5 * e4


def test_w6a8_product_is_closer_to_the_float_product_than_w4a8():
    """Expected ratio about 0.34: sqrt(0.028^2 + 0.029^2) against sqrt(0.115^2 + 0.029^2)."""
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((64, 4096), generator=g).half()
        w = torch.randn((256, 4096), generator=g)
        exact = x.double() @ w.double().t()
        xq, xs, flag = ref.quantize_act(x)
        c6, s6 = ref.quantize(w)
        y6, _ = ref.reference(xq, xs, flag, ref.pack(c6), s6)
        c4, s4 = mx4.quantize(w)
        y4, _ = a8.reference(xq, xs, flag, mx4.pack(c4), s4)
        e6, e4 = (y6 - exact).norm() / exact.norm(), (y4 - exact).norm() / exact.norm()
        print(f"seed {seed}: relative Frobenius error w6a8 {e6.item():.4f}, w4a8 {e4.item():.4f}, ratio {(e6 / e4).item():.3f}")
        assert e6 < 0.5 * e4


def test_reference_nan_rules():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 64), generator=g).half()
    x[1, 3], x[3, 63] = float("inf"), float("nan")
    xq, xs, flag = ref.quantize_act(x)
    c, s = ref.quantize(torch.randn((3, 64), generator=g))
    s[2, 1] = 255
    y, a = ref.reference(xq, xs, flag, ref.pack(c), s)
    assert torch.isnan(y[1]).all() and torch.isnan(y[3]).all() and torch.isnan(y[:, 2]).all()
    assert torch.isfinite(y[0, :2]).all() and torch.isfinite(y[2, :2]).all() and torch.isfinite(a).all()
    assert ref.PROBE_ULPS == 1853 and "mxfp6_a8_probe.txt" in ref.tolerance.__doc__
    probe = open(os.path.join(ROOT, "profiles", "mxfp6_a8_probe.txt")).read()
    assert "worst accumulation error of one instruction 1853.0000" in probe


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert "bie_mxfp6_a8_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as w4a8, mxfp4_linear_cuda as w4, mxfp6_a8_linear_cuda as w6
    assert w6.quantize_act is w4a8.quantize_act and w6.dequant_act is w4a8.dequant_act and w6.col_exp is w4.col_exp  # re-used, not copied
    assert w6.quantize is not w4.quantize and w6.dequant is not w4.dequant
    assert all(callable(getattr(w6, n)) for n in ("quantize", "dequant", "form", "forward", "gemm"))


def test_argument_validation_of_every_new_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    for name in ("bie_mxfp6_quantize", "bie_mxfp6_dequant"):
        Q = getattr(L, name)
        assert Q(fake, fake, fake, 4, 48, 0, None) == -1
        assert name.encode() in L.bie_last_error() and b"K=48" in L.bie_last_error()
        assert Q(fake, fake, fake, 4, 0, 0, None) == -1
        assert Q(fake, fake, fake, 4, (1 << 20) + 32, 0, None) == -1
        assert Q(fake, fake, fake, 0, 64, 0, None) == -1
        assert Q(fake, fake, fake, 4, 64, 3, None) == -2     # dtype
        assert Q(fake, fake, fake, 4, 64, -1, None) == -2
        for i in range(3):
            a = [fake, fake, fake]
            a[i] = None
            assert Q(*a, 4, 64, 2, None) == -1, (name, i)
    assert L.bie_mxfp6_quantize(fake + 2, fake, fake, 4, 64, 0, None) == -1   # w 4-byte aligned
    assert L.bie_mxfp6_quantize(fake, fake + 8, fake, 4, 64, 0, None) == -1   # qweight 16-byte aligned
    assert L.bie_mxfp6_dequant(fake + 8, fake, fake, 4, 64, 0, None) == -1
    assert L.bie_mxfp6_dequant(fake, fake, fake + 2, 4, 64, 0, None) == -1
    F = L.bie_mxfp6_a8_linear_forward
    ok = [fake, fake, fake, fake, None, fake, fake]
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert F(*ok, 1, 8, 0, 0, -1, None) == -1       # K range
    assert F(*ok, 1, 8, (1 << 20) + 32, 0, -1, None) == -1
    assert F(*ok, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(*ok, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(*ok, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(*ok, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(*ok, 65, 8, 64, 0, 0, None) == -2      # the decode form takes M <= 64
    assert b"bie_mxfp6_a8_linear_forward" in L.bie_last_error() and b"M=65" in L.bie_last_error()
    for i in (0, 1, 2, 3, 5, 6):                     # x, qweight, scales, e_col, y, workspace
        a = list(ok)
        a[i] = None
        assert F(*a, 1, 8, 64, 0, -1, None) == -1, i
    for i in (0, 1, 5, 6):                           # alignment of x, qweight, y, workspace
        a = list(ok)
        a[i] = fake + 8
        assert F(*a, 1, 8, 64, 0, -1, None) == -1, i
    a = list(ok)
    a[4] = fake + 1                                  # bias alignment
    assert F(*a, 1, 8, 64, 0, -1, None) == -1
    G = L.bie_mxfp6_a8_gemm
    okg = [fake, fake, fake, fake, fake, fake, None, fake, None]
    assert G(*okg, 1, 8, 48, 1, -1, None) == -1
    assert G(*okg, 0, 8, 64, 1, -1, None) == -1
    assert G(*okg, 1, 8, 64, 2, -1, None) == -2
    assert G(*okg, 1, 8, 64, 1, -2, None) == -1
    assert G(*okg, 65, 8, 64, 1, 0, None) == -2
    assert b"bie_mxfp6_a8_gemm" in L.bie_last_error()
    for i in (0, 1, 2, 3, 4, 5, 7):                  # xq, xs, row_flag, qweight, scales, e_col, y
        a = list(okg)
        a[i] = None
        assert G(*a, 1, 8, 64, 1, -1, None) == -1, i
    for i in (0, 3, 7):
        a = list(okg)
        a[i] = fake + 8
        assert G(*a, 1, 8, 64, 1, -1, None) == -1, i


def test_form_and_workspace_are_host_functions_and_total():
    from bitorch_engine import _hip
    L = _hip.lib()
    shapes = [(K, N) for K, N in BENCH_SHAPES] + [(32, 1), (96, 7), (1 << 20, 3)]
    for K, N in shapes:
        for dt in (0, 1):
            fs = [L.bie_mxfp6_a8_form(M, N, K, dt) for M in range(1, 8193)]
            assert set(fs) == {0, 1} and fs == sorted(fs), (K, N)   # decode below one bound, prefill above it: monotone
            assert all(f == 1 for f in fs[64:])                      # never the decode form where it is refused
        for M in (1, 2, 16, 17, 64, 65, 1000, 8192):
            for form in (-1, 0, 1):
                b = L.bie_mxfp6_a8_workspace_bytes(M, N, K, form)
                need = M * K + M * (K // 32) + M
                assert need <= b <= need + 32 and b % 16 == 0
                assert b == L.bie_mxfp4_a8_workspace_bytes(M, N, K, form)  # the W4A8 layout
    assert L.bie_mxfp6_a8_workspace_bytes(0, 8, 64, -1) == 0
    assert L.bie_mxfp6_a8_workspace_bytes(4, 8, 48, -1) == 0


def test_form_knob_forces_either_form_where_it_is_legal():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mxfp6_a8_form(M, N, K, d) for M in (1, 64, 65, 4096) for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (32, 1)) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP6_A8_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 32
    assert out["0"] == ["0"] * 16 + ["1"] * 16  # the decode form exists for M <= 64 only


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------
def test_layer_is_exported_and_keeps_its_own_checkpoint_shapes():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A8LinearCuda, MXFP4LinearCuda, MXFP6A8LinearCuda, MXFP6A8LinearForward  # noqa: F401
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp6_a8_linear_cuda" in KNOWN
    assert not issubclass(MXFP6A8LinearCuda, MXFP4LinearCuda)
    layer = MXFP6A8LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP6A8LinearCuda(64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.qweight.shape == (8, 48) and layer.scales.shape == (8, 2) and layer.e_col.shape == (8,)
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP6A8LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP6A8LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):  # an MXFP4 block tensor is not an MXFP6 one
        layer.set_mx_weight(torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((8, 48), dtype=torch.int8), torch.zeros((8, 2), dtype=torch.uint8))
    # its own state dict loads; a qweight-only one drops the latent weight
    other = MXFP6A8LinearCuda(64, 8)
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.weight, layer.weight)
    sd = {k: v for k, v in layer.state_dict().items() if k != "weight"}
    other.load_state_dict(sd)
    assert other.weight is None and set(other.state_dict()) == {"qweight", "scales"}
    # an MXFP4 state dict is refused with a message that says why, and nothing is loaded
    for cls in (MXFP4LinearCuda, MXFP4A8LinearCuda):
        before = {k: v.clone() for k, v in layer.state_dict().items()}
        with pytest.raises(RuntimeError, match="MXFP4 weight"):
            layer.load_state_dict(cls(64, 8).state_dict())
        assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())
    with pytest.raises(RuntimeError):  # and the other way round, by torch's own shape check
        MXFP4LinearCuda(64, 8).load_state_dict(layer.state_dict())


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as w6
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A8LinearCuda
    q, s = torch.zeros((8, 48), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        w6.forward(torch.zeros((1, 64), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        w6.quantize(torch.zeros((8, 64)))
    with pytest.raises(RuntimeError):
        w6.dequant(q, s)
    with pytest.raises(RuntimeError):
        w6.gemm(torch.zeros((1, 64), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), q, s)
    with pytest.raises(RuntimeError):
        MXFP6A8LinearCuda(64, 8).eval()(torch.zeros((1, 64), dtype=torch.half))


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the layer's host checks and every form is drawn."""
    import fuzz_mxfp6_a8 as F
    import test_mxfp6_a8_fuzz_gpu as S
    from bitorch_engine import _hip
    L = _hip.lib()
    rng = np.random.default_rng(S.SEED)
    seen = {f: 0 for f in F.FORMS}
    fake = 1 << 20
    for _ in range(S.CASES):
        c = F.draw(rng)
        M, N, K = c["M"], c["N"], c["K"]
        assert K % 32 == 0 and 32 <= K <= (1 << 20) and N >= 1 and M >= 1 and c["dt"] in F.DTS
        assert M * N <= 4096 * 4224 and M * K <= 4096 * 11008  # the float64 reference stays small
        fs = F.forms_of(c)
        for f in fs:
            seen[f] += 1
            form = 0 if f.startswith("decode") else 1
            rc = L.bie_mxfp6_a8_linear_forward(None, fake, fake, fake, None, fake, fake, M, N, K, 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
    assert all(n > 0 for n in seen.values()), seen


def test_mxfp6_a8_kernels_do_not_spill():
    """Every kernel of mxfp6_a8.hip compiles without warnings and with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp6_a8.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-Wall", "-Wno-unused-function"]
    p = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning" not in p.stderr, p.stderr[-2000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    assert sum("mx6_quantize_kernel" in n for n in seen) == 3, list(seen)
    assert sum("mx6_dequant_kernel" in n for n in seen) == 3, list(seen)
    assert sum("mx6a8_decode_kernel" in n for n in seen) == 6, list(seen)
    assert sum("mx6a8_gemm_kernel" in n for n in seen) == 4, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp6_a8 kernel spills: {seen}"
