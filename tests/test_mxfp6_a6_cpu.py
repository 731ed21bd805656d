"""MXFP6 W6A6 linear layer, the parts that need no GPU: properties of the restated activation quantiser (mxfp6_a6_ref.py), the probe's
figure, the new entries in the header, the ctypes table and the library, host-side argument validation of every new entry, the form
plan / workspace size, the accuracy statement against the W6A8 and W4A4 restatements, the range caveat, the layer's export and
checkpoint rules, the fuzz generator's draws and the compiler's resource report for csrc/mxfp6_a6.hip."""
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
import mxfp6_a6_ref as ref  # noqa: E402

mx6 = ref.mx6       # mxfp6_ref
a8 = ref.a8         # mxfp4_a8_ref
mx4 = ref.mx        # mxfp4_ref

NEW = ("bie_mxfp6_quantize_act", "bie_mxfp6_a6_form", "bie_mxfp6_a6_workspace_bytes", "bie_mxfp6_a6_linear_forward", "bie_mxfp6_a6_gemm")
BENCH_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))  # (K, N)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def _row(vals, amax):
    """One block of 32: vals, then the block maximum, zeros behind."""
    x = torch.zeros((1, 32))
    x[0, :len(vals)] = torch.tensor(vals)
    x[0, 31] = amax
    return x


def _codes(x):
    q, s, f = ref.quantize_act(x)
    return ref.unpack(q), s, f


def test_quantize_act_ties_saturation_signs_and_zero_blocks():
    for t in (0, -9, 6):
        sc = 2.0 ** t
        c, s, f = _codes(_row([0.0625 * sc, 0.1875 * sc, 1.9375 * sc, -0.0, -0.03 * sc], 4.0 * sc))
        assert s.item() == t + 127 and not f.any()
        assert c[0, :5].tolist() == [0, 2, 16, 0x20, 0x20] and c[0, 31].item() == 24  # 0.0625 -> 0, 0.1875 -> 0.25, 1.9375 -> 2, -0.0 -> 0x20
        for big in (7.74, 7.75, 7.8, 7.99):  # saturation at 7.5: a block maximum in (7.5, 8) keeps e = t
            c, s, _ = _codes(_row([-big * sc, 4.25 * sc], big * sc))
            assert s.item() == t + 127 and c[0, 31].item() == 31 and c[0, :2].tolist() == [0x3F, 24]
    for z in (0.0, -0.0):  # an all-zero block: scale code 0 and 24 zero bytes
        q, s, f = ref.quantize_act(torch.full((2, 64), z))
        assert q.shape == (2, 48) and not q.any() and not s.any() and not f.any()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_quantize_act_is_idempotent_on_x_hat_and_is_the_weight_rule(dt):
    g = torch.Generator().manual_seed(2)
    for M, K in ((8, 4096), (33, 96), (3, 32)):
        x = (torch.randn((M, K), generator=g) * torch.exp2(torch.randint(-6, 6, (M, 1), generator=g).float())).to(dt)
        q, s, f = ref.quantize_act(x)
        c, s0 = mx6.quantize(x)
        assert torch.equal(q, mx6.pack(c)) and torch.equal(s, s0) and not f.any()
        xh = ref.dequant_act(q, s)
        q2, s2, _ = ref.quantize_act(xh.float())
        assert torch.equal(q2, q) and torch.equal(s2, s)


def test_row_flag_rule_and_reference_nan_rules():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 64), generator=g).half()
    clean = ref.quantize_act(x)
    x[1, 3], x[3, 63] = float("inf"), float("nan")
    xq, xs, flag = ref.quantize_act(x)
    assert flag.tolist() == [0, 1, 0, 1]
    assert torch.equal(xq[[0, 2]], clean[0][[0, 2]]) and torch.equal(xs[[0, 2]], clean[1][[0, 2]])
    c, s = mx6.quantize(torch.randn((3, 64), generator=g))
    s[2, 1] = 255
    y, a = ref.reference(xq, xs, flag, ref.pack(c), s)
    assert torch.isnan(y[1]).all() and torch.isnan(y[3]).all() and torch.isnan(y[:, 2]).all()
    assert torch.isfinite(y[0, :2]).all() and torch.isfinite(y[2, :2]).all() and torch.isfinite(a).all()


def test_probe_figure_is_the_one_in_the_profile():
    probe = open(os.path.join(ROOT, "profiles", "mxfp6_a6_probe.txt")).read()
    m = re.search(r"worst accumulation error of one instruction ([0-9.]+)", probe)
    assert m and float(m.group(1)) == ref.PROBE_ULPS and f"worst accumulation error of one instruction {ref.PROBE_ULPS:.4f}" in probe
    assert "mxfp6_a6_probe.txt" in ref.tolerance.__doc__
    assert probe.count("B field map and C/D map: as expected") == 2 and probe.count("scale map: as expected") == 2
    worst = max(float(v) for v in re.findall(r"largest \|D - exact\| = ([0-9.]+)", probe))
    assert worst == ref.PROBE_ULPS  # the worst count over both shapes and every data mode


# ---- the accuracy statement and the range caveat ---------------------------------------------------------------------------------------------
def test_w6a6_is_as_accurate_as_w6a8_on_gaussian_data_and_twice_as_accurate_as_w4a4():
    a4 = ref._load("mxfp4_a4_ref")
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((64, 4096), generator=g).half()
        w = torch.randn((256, 4096), generator=g)
        exact = x.double() @ w.double().t()
        c6, s6 = mx6.quantize(w)
        y66, _ = ref.reference(*ref.quantize_act(x), ref.pack(c6), s6)
        y68, _ = mx6.reference(*a8.quantize_act(x), mx6.pack(c6), s6)
        c4, s4 = mx4.quantize(w)
        y44, _ = a4.reference(*a4.quantize_act(x), mx4.pack(c4), s4)
        e66, e68, e44 = ((y - exact).norm() / exact.norm() for y in (y66, y68, y44))
        print(f"seed {seed}: relative Frobenius error w6a6 {e66.item():.4f}, w6a8 {e68.item():.4f}, w4a4 {e44.item():.4f}; "
              f"w6a6 / w6a8 {(e66 / e68).item():.3f}, w6a6 / w4a4 {(e66 / e44).item():.3f}")
        assert e66 < 1.25 * e68 and e66 < 0.5 * e44


def test_range_caveat_one_64th_of_the_block_maximum_is_lost_by_e2m3_and_kept_by_e4m3():
    for t in (0, -5, 7):
        sc = 2.0 ** t
        x = _row([sc / 64, -sc / 64], sc).half()  # the block's power-of-two maximum and 1/64 of it
        xh6 = ref.dequant_act(*ref.quantize_act(x)[:2])
        q8, s8, _ = a8.quantize_act(x)
        xh8 = a8.dequant_act(q8, s8)
        assert xh6[0, 31] == sc and xh8[0, 31] == sc
        assert xh6[0, 0] == 0 and xh6[0, 1] == 0                  # 2^-6 of the maximum is half of E2M3's smallest step: the tie goes to the even code 0
        assert xh8[0, 0] == sc / 64 and xh8[0, 1] == -sc / 64     # E4M3 holds it exactly


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert "bie_mxfp6_a6_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300
    from bitorch_engine.extensions import mxfp4_linear_cuda as w4, mxfp6_a6_linear_cuda as w66, mxfp6_a8_linear_cuda as w68
    assert w66.quantize is w68.quantize and w66.dequant is w68.dequant and w66.col_exp is w4.col_exp  # re-used, not copied
    assert w66.blk_exp is w4.blk_exp and w66.grad_input is w68.grad_input and w66.dequant_act is w66.dequant
    assert w66.quantize_act is not w68.quantize_act and w66.forward is not w68.forward and w66.gemm is not w68.gemm and w66.form is not w68.form
    assert all(callable(getattr(w66, n)) for n in ("quantize_act", "form", "forward", "gemm"))


def test_argument_validation_of_every_new_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    Q = L.bie_mxfp6_quantize_act
    okq = [fake, fake, fake, fake]
    assert Q(*okq, 4, 48, 0, None) == -1
    assert b"bie_mxfp6_quantize_act" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert Q(*okq, 4, 0, 0, None) == -1
    assert Q(*okq, 4, (1 << 20) + 32, 0, None) == -1
    assert Q(*okq, 0, 64, 0, None) == -1
    assert Q(*okq, 4, 64, 2, None) == -2      # fp32 x
    assert Q(*okq, 4, 64, -1, None) == -2
    for i in range(4):
        a = list(okq)
        a[i] = None
        assert Q(*a, 4, 64, 0, None) == -1, i
    for i in (0, 1):                          # x and xq6 16-byte aligned
        a = list(okq)
        a[i] = fake + 8
        assert Q(*a, 4, 64, 0, None) == -1, i
    F = L.bie_mxfp6_a6_linear_forward
    ok = [fake, fake, fake, fake, None, fake, fake]
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert F(*ok, 1, 8, 0, 0, -1, None) == -1       # K range
    assert F(*ok, 1, 8, (1 << 20) + 32, 0, -1, None) == -1
    assert F(*ok, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(*ok, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(*ok, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(*ok, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(*ok, 1, 8, 64, 0, -2, None) == -1
    assert F(*ok, 65, 8, 64, 0, 0, None) == -2      # the decode form takes M <= 64
    assert b"bie_mxfp6_a6_linear_forward" in L.bie_last_error() and b"M=65" in L.bie_last_error()
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
    G = L.bie_mxfp6_a6_gemm
    okg = [fake, fake, fake, fake, fake, fake, None, fake, None]
    assert G(*okg, 1, 8, 48, 1, -1, None) == -1
    assert G(*okg, 1, 8, 0, 1, -1, None) == -1
    assert G(*okg, 0, 8, 64, 1, -1, None) == -1
    assert G(*okg, 1, 0, 64, 1, -1, None) == -1
    assert G(*okg, 1, 8, 64, 2, -1, None) == -2
    assert G(*okg, 1, 8, 64, 1, -2, None) == -1
    assert G(*okg, 1, 8, 64, 1, 2, None) == -1
    assert G(*okg, 65, 8, 64, 1, 0, None) == -2
    assert b"bie_mxfp6_a6_gemm" in L.bie_last_error() and b"M=65" in L.bie_last_error()
    for i in (0, 1, 2, 3, 4, 5, 7):                  # xq6, xs, row_flag, qweight, scales, e_col, y
        a = list(okg)
        a[i] = None
        assert G(*a, 1, 8, 64, 1, -1, None) == -1, i
    for i in (0, 3, 7):
        a = list(okg)
        a[i] = fake + 8
        assert G(*a, 1, 8, 64, 1, -1, None) == -1, i
    a = list(okg)
    a[6] = fake + 1
    assert G(*a, 1, 8, 64, 1, -1, None) == -1


def test_form_and_workspace_are_host_functions_and_total():
    from bitorch_engine import _hip
    L = _hip.lib()
    shapes = [(K, N) for K, N in BENCH_SHAPES] + [(32, 1), (96, 7), (1 << 20, 3)]
    for K, N in shapes:
        for dt in (0, 1):
            fs = [L.bie_mxfp6_a6_form(M, N, K, dt) for M in range(1, 8193)]
            assert set(fs) == {0, 1} and fs == sorted(fs), (K, N)   # decode below one bound, prefill above it: monotone
            assert all(f == 1 for f in fs[64:])                      # never the decode form where it is refused
        for M in (1, 2, 16, 17, 64, 65, 1000, 8192):
            for form in (-1, 0, 1):
                b = L.bie_mxfp6_a6_workspace_bytes(M, N, K, form)
                need = M * (3 * K // 4) + M * (K // 32) + M        # xq6, xs, row_flag
                assert need <= b < need + 16 and b % 16 == 0
    assert L.bie_mxfp6_a6_workspace_bytes(0, 8, 64, -1) == 0
    assert L.bie_mxfp6_a6_workspace_bytes(4, 8, 48, -1) == 0


def test_form_knob_forces_either_form_where_it_is_legal():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mxfp6_a6_form(M, N, K, d) for M in (1, 64, 65, 4096) for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (32, 1)) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP6_A6_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 32
    assert out["0"] == ["0"] * 16 + ["1"] * 16  # the decode form exists for M <= 64 only


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------
def test_layer_is_exported_and_shares_the_mxfp6_checkpoint():
    from bitorch_engine.layers.qlinear.nbit.cuda import (MXFP4A8LinearCuda, MXFP4LinearCuda, MXFP6A6LinearCuda, MXFP6A6LinearForward,  # noqa: F401
                                                         MXFP6A8LinearCuda, MXFP6LinearCuda)
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp6_a6_linear_cuda" in KNOWN
    assert not issubclass(MXFP6A6LinearCuda, MXFP4LinearCuda)
    layer = MXFP6A6LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP6A6LinearCuda(64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.qweight.shape == (8, 48) and layer.scales.shape == (8, 2) and layer.e_col.shape == (8,)
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP6A6LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP6A6LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        MXFP6A6LinearCuda(64, 8, grad_input="fast")
    with pytest.raises(ValueError):  # an MXFP4 block tensor is not an MXFP6 one
        layer.set_mx_weight(torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    # the three MXFP6 linear layers load each other's state dicts, latent and packed
    for cls in (MXFP6A8LinearCuda, MXFP6LinearCuda, MXFP6A6LinearCuda):
        other = cls(64, 8)
        other.load_state_dict(layer.state_dict())
        assert torch.equal(other.weight, layer.weight)
        back = MXFP6A6LinearCuda(64, 8)
        back.load_state_dict(other.state_dict())
        assert torch.equal(back.weight, layer.weight)
        sd = {k: v for k, v in other.state_dict().items() if k != "weight"}
        back.load_state_dict(sd)
        assert back.weight is None and set(back.state_dict()) == {"qweight", "scales"}
    # an MXFP4 state dict is refused with a message that says why, and nothing is loaded
    for cls in (MXFP4LinearCuda, MXFP4A8LinearCuda):
        before = {k: v.clone() for k, v in layer.state_dict().items()}
        with pytest.raises(RuntimeError, match="MXFP4 weight.*MXFP6A6LinearCuda"):
            layer.load_state_dict(cls(64, 8).state_dict())
        assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp6_a6_linear_cuda as w66
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A6LinearCuda
    q, s = torch.zeros((8, 48), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        w66.forward(torch.zeros((1, 64), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        w66.quantize_act(torch.zeros((1, 64), dtype=torch.half))
    with pytest.raises(RuntimeError):
        w66.gemm(torch.zeros((1, 48), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), q, s)
    with pytest.raises(RuntimeError):
        MXFP6A6LinearCuda(64, 8).eval()(torch.zeros((1, 64), dtype=torch.half))


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the layer's host checks and every form is drawn."""
    import fuzz_mxfp6_a6 as F
    import test_mxfp6_a6_fuzz_gpu as S
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
        for f in F.forms_of(c):
            seen[f] += 1
            form = 0 if f.startswith("decode") else 1
            rc = L.bie_mxfp6_a6_linear_forward(None, fake, fake, fake, None, fake, fake, M, N, K, 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
    assert all(n > 0 for n in seen.values()), seen


def test_mxfp6_a6_kernels_do_not_spill():
    """Every kernel of mxfp6_a6.hip compiles without warnings and with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp6_a6.hip")
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
    assert sum("mx6a6_quantize_kernel" in n for n in seen) == 2, list(seen)
    assert sum("mx6a6_decode_kernel" in n for n in seen) == 6, list(seen)
    assert sum("mx6a6_gemm_kernel" in n for n in seen) == 4, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp6_a6 kernel spills: {seen}"
