"""MXFP4 W4A6 linear layer, the parts that need no GPU: the probe's figure and maps, the new entries in the header, the ctypes table and
the library, host-side argument validation of every new entry, the form plan / workspace size, the accuracy statement against the W4A8
and W4A4 restatements, the range caveat, the layer's export and checkpoint rules, the fuzz generator's draws, the layout of every arena
case of test_mx4a6_arena_gpu.py and the compiler's resource report for csrc/mxfp4_a6.hip."""
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
import mxfp4_a6_ref as ref  # noqa: E402

a6 = ref.a6         # mxfp6_a6_ref
a8 = ref.a8         # mxfp4_a8_ref
mx4 = ref.mx        # mxfp4_ref

NEW = ("bie_mx4a6_form", "bie_mx4a6_workspace_bytes", "bie_mx4a6_linear_forward", "bie_mx4a6_gemm")
BENCH_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))  # (K, N)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_shares_the_activation_side_of_w6a6_and_the_weight_side_of_mxfp4():
    assert ref.quantize_act is a6.quantize_act and ref.dequant_act is a6.dequant_act
    assert ref.quantize is mx4.quantize and ref.pack is mx4.pack and ref.dequant is mx4.dequant
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 64), generator=g).half()
    x[1, 3], x[3, 63] = float("inf"), float("nan")
    xq, xs, flag = ref.quantize_act(x)
    assert flag.tolist() == [0, 1, 0, 1] and xq.shape == (4, 48)
    c, s = mx4.quantize(torch.randn((3, 64), generator=g))
    s[2, 1] = 255
    b = torch.randn(3, generator=g)
    y, a = ref.reference(xq, xs, flag, ref.pack(c), s, b)
    assert torch.isnan(y[1]).all() and torch.isnan(y[3]).all() and torch.isnan(y[:, 2]).all()
    assert torch.isfinite(y[0, :2]).all() and torch.isfinite(y[2, :2]).all() and torch.isfinite(a).all()
    xh, W = ref.dequant_act(xq, xs), ref.dequant(ref.pack(c), s)
    assert torch.equal(y[0, :2], xh[0] @ W[:2].t() + b[:2].double())


def test_probe_figure_is_the_one_in_the_profile_and_the_maps_are_stated():
    probe = open(os.path.join(ROOT, "profiles", "mxfp4_a6_probe.txt")).read()
    m = re.search(r"worst accumulation error of one instruction ([0-9.]+)", probe)
    assert m and float(m.group(1)) == ref.PROBE_ULPS and f"worst accumulation error of one instruction {ref.PROBE_ULPS:.4f}" in probe
    assert "mxfp4_a6_probe.txt" in ref.tolerance.__doc__
    assert "A = FP4 E2M1 (cbsz 4), B = FP6 E2M3 (blgp 2)" in probe
    assert probe.count("B field map and C/D map: as expected") == 2 and probe.count("A field map: as expected") == 2
    assert probe.count("scale map: as expected") == 2 and "field order, lane map and scale map as assumed" in probe
    worst = max(float(v) for v in re.findall(r"largest \|D - exact\| = ([0-9.]+)", probe))
    assert worst == ref.PROBE_ULPS  # the worst count over both shapes and every data mode
    one_scale = re.findall(r"scales 2\^0: (\d+) of \d+ exact sums are not fp32 values; largest \|D - exact\| = ([0-9.]+)", probe)
    assert len(one_scale) == 4 and all(int(n) == 0 and float(e) == 0.0 for n, e in one_scale)  # exact under one scale, both shapes


# ---- the accuracy statement and the range caveat ---------------------------------------------------------------------------------------------
def test_w4a6_is_as_accurate_as_w4a8_on_gaussian_data_and_a_quarter_of_w4a4s_activation_error():
    """The distance of the restated product to x . W^^T (the same MXFP4 weights, unquantised x): the activation error alone."""
    a4 = ref._load("mxfp4_a4_ref")
    for seed in (0, 1, 2):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((64, 4096), generator=g).half()
        w = torch.randn((256, 4096), generator=g)
        c4, s4 = mx4.quantize(w)
        qw = mx4.pack(c4)
        w16 = x.double() @ mx4.dequant(qw, s4).t()
        y46, _ = ref.reference(*ref.quantize_act(x), qw, s4)
        y48, _ = a8.reference(*a8.quantize_act(x), qw, s4)
        y44, _ = a4.reference(*a4.quantize_act(x), qw, s4)
        e46, e48, e44 = ((y - w16).norm() / w16.norm() for y in (y46, y48, y44))
        print(f"seed {seed}: distance to the W4A16 product w4a6 {e46.item():.4f}, w4a8 {e48.item():.4f}, w4a4 {e44.item():.4f}; "
              f"w4a6 / w4a8 {(e46 / e48).item():.3f}, w4a6 / w4a4 {(e46 / e44).item():.3f}")
        assert e46 < 1.25 * e48 and e46 < 0.5 * e44


def test_range_caveat_one_64th_of_the_block_maximum_is_lost_by_e2m3_and_kept_by_e4m3():
    for t in (0, -5, 7):
        sc = 2.0 ** t
        x = torch.zeros((1, 32))
        x[0, 0], x[0, 1], x[0, 31] = sc / 64, -sc / 64, sc  # the block's power-of-two maximum and 1/64 of it
        x = x.half()
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
    assert "bie_mx4a6_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300
    from bitorch_engine.extensions import mxfp4_a6_linear_cuda as w46, mxfp4_a8_linear_cuda as w48, mxfp4_linear_cuda as w4, mxfp6_a6_linear_cuda as w66
    for n in ("quantize", "dequant", "col_exp", "blk_exp", "grad_input"):  # re-used, not copied
        assert getattr(w46, n) is getattr(w4, n), n
    assert w46.quantize_act is w66.quantize_act and w46.dequant_act is w66.dequant_act
    for other in (w4, w48, w66):
        assert w46.forward is not other.forward and w46.form is not other.form
    assert w46.gemm is not w48.gemm and w46.gemm is not w66.gemm
    assert all(callable(getattr(w46, n)) for n in ("quantize_act", "form", "forward", "gemm"))
    src = open(w46.__file__).read()
    assert "matmul" not in src and ".mm(" not in src and " @ " not in src  # no torch product in the shim, no fallback


def test_argument_validation_of_every_new_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    F = L.bie_mx4a6_linear_forward
    ok = [fake, fake, fake, fake, None, fake, fake]
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert b"bie_mx4a6_linear_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert F(*ok, 1, 8, 0, 0, -1, None) == -1       # K range
    assert F(*ok, 1, 8, (1 << 20) + 32, 0, -1, None) == -1
    assert F(*ok, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(*ok, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(*ok, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(*ok, 1, 8, 64, -1, -1, None) == -2
    assert F(*ok, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(*ok, 1, 8, 64, 0, -2, None) == -1
    assert F(*ok, 65, 8, 64, 0, 0, None) == -2      # the decode form takes M <= 64
    assert b"bie_mx4a6_linear_forward" in L.bie_last_error() and b"M=65" in L.bie_last_error()
    for i in (0, 1, 2, 3, 5, 6):                     # x, qweight, scales, e_col, y, workspace
        a = list(ok)
        a[i] = None
        assert F(*a, 1, 8, 64, 0, -1, None) == -1, i
        assert b"NULL tensor pointer" in L.bie_last_error()
    for i in (0, 1, 5, 6):                           # alignment of x, qweight, y, workspace
        a = list(ok)
        a[i] = fake + 8
        assert F(*a, 1, 8, 64, 0, -1, None) == -1, i
    a = list(ok)
    a[4] = fake + 1                                  # bias alignment
    assert F(*a, 1, 8, 64, 0, -1, None) == -1
    G = L.bie_mx4a6_gemm
    okg = [fake, fake, fake, fake, fake, fake, None, fake, None]
    assert G(*okg, 1, 8, 48, 1, -1, None) == -1
    assert G(*okg, 1, 8, 0, 1, -1, None) == -1
    assert G(*okg, 1, 8, (1 << 20) + 32, 1, -1, None) == -1
    assert G(*okg, 0, 8, 64, 1, -1, None) == -1
    assert G(*okg, 1, 0, 64, 1, -1, None) == -1
    assert G(*okg, 1, 8, 64, 2, -1, None) == -2
    assert G(*okg, 1, 8, 64, 1, -2, None) == -1
    assert G(*okg, 1, 8, 64, 1, 2, None) == -1
    assert G(*okg, 65, 8, 64, 1, 0, None) == -2
    assert b"bie_mx4a6_gemm" in L.bie_last_error() and b"M=65" in L.bie_last_error()
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
            fs = [L.bie_mx4a6_form(M, N, K, dt) for M in range(1, 8193)]
            assert set(fs) == {0, 1} and fs == sorted(fs), (K, N)   # decode below one bound, prefill above it: monotone
            assert all(f == 1 for f in fs[64:])                      # never the decode form where it is refused
        for M in (1, 2, 16, 17, 64, 65, 1000, 8192):
            for form in (-1, 0, 1):
                b = L.bie_mx4a6_workspace_bytes(M, N, K, form)
                need = M * (3 * K // 4) + M * (K // 32) + M        # xq6, xs, row_flag
                assert need <= b < need + 16 and b % 16 == 0
                assert b == L.bie_mxfp6_a6_workspace_bytes(M, N, K, form)  # the W6A6 layout
    assert L.bie_mx4a6_workspace_bytes(0, 8, 64, -1) == 0
    assert L.bie_mx4a6_workspace_bytes(4, 8, 48, -1) == 0


def test_form_knob_forces_either_form_where_it_is_legal():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mx4a6_form(M, N, K, d) for M in (1, 64, 65, 4096) for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (32, 1)) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP4_A6_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 32
    assert out["0"] == ["0"] * 16 + ["1"] * 16  # the decode form exists for M <= 64 only


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------
def test_layer_is_exported_and_shares_the_mxfp4_checkpoint():
    from bitorch_engine.layers.qlinear.nbit.cuda import (MXFP4A4LinearCuda, MXFP4A6LinearCuda, MXFP4A6LinearForward, MXFP4A8LinearCuda,  # noqa: F401
                                                         MXFP4LinearCuda, MXFP6A6LinearCuda, MXFP6LinearCuda)
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp4_a6_linear_cuda" in KNOWN
    assert issubclass(MXFP4A6LinearCuda, MXFP4LinearCuda) and not issubclass(MXFP4A6LinearCuda, (MXFP4A8LinearCuda, MXFP4A4LinearCuda))
    layer = MXFP4A6LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP4A6LinearCuda(64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.qweight.shape == (8, 32) and layer.scales.shape == (8, 2) and layer.e_col.shape == (8,)
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP4A6LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP4A6LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        MXFP4A6LinearCuda(64, 8, grad_input="fast")
    with pytest.raises(ValueError):  # an MXFP6 block tensor is not an MXFP4 one
        layer.set_mx_weight(torch.zeros((8, 48), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    # the four MXFP4 linear layers load each other's state dicts, latent and packed
    for cls in (MXFP4LinearCuda, MXFP4A4LinearCuda, MXFP4A8LinearCuda, MXFP4A6LinearCuda):
        other = cls(64, 8)
        other.load_state_dict(layer.state_dict())
        assert torch.equal(other.weight, layer.weight)
        back = MXFP4A6LinearCuda(64, 8)
        back.load_state_dict(other.state_dict())
        assert torch.equal(back.weight, layer.weight)
        sd = {k: v for k, v in other.state_dict().items() if k != "weight"}
        back.load_state_dict(sd)
        assert back.weight is None and set(back.state_dict()) == {"qweight", "scales"}
    # an MXFP6 state dict is refused with a message that says why, and nothing is loaded
    for cls in (MXFP6LinearCuda, MXFP6A6LinearCuda):
        before = {k: v.clone() for k, v in layer.state_dict().items()}
        with pytest.raises(RuntimeError, match="MXFP6 weight.*MXFP4A6LinearCuda"):
            layer.load_state_dict(cls(64, 8).state_dict())
        assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp4_a6_linear_cuda as w46
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A6LinearCuda
    q, s = torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        w46.forward(torch.zeros((1, 64), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        w46.quantize_act(torch.zeros((1, 64), dtype=torch.half))
    with pytest.raises(RuntimeError):
        w46.gemm(torch.zeros((1, 48), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), q, s)
    with pytest.raises(RuntimeError):
        MXFP4A6LinearCuda(64, 8).eval()(torch.zeros((1, 64), dtype=torch.half))


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the layer's host checks and every form is drawn."""
    import fuzz_mxfp4_a6 as F
    import test_mxfp4_a6_fuzz_gpu as S
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
            rc = L.bie_mx4a6_linear_forward(None, fake, fake, fake, None, fake, fake, M, N, K, 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
    assert all(n > 0 for n in seen.values()), seen


def test_layout_of_every_arena_case():
    """test_abi_contract_cpu.py::assert_layout's conditions on the cases of test_mx4a6_arena_gpu.py: exactly the stated alignment, guards
    that do not overlap, a workspace of exactly the size function's bytes."""
    import abi_arena as A
    import test_mx4a6_arena_gpu as T
    for entry in T.ENTRIES:
        grid = T.grid(entry)
        assert len(grid) == 2 * 2 * 3 * (3 * 2 + 2) and grid[-1][5] and grid[-1][6] == 1 and not grid[0][5]
        assert {(c[1], c[6]) for c in grid} == {(1, 0), (1, 1), (17, 0), (17, 1), (64, 0), (64, 1), (65, 1), (130, 1)}
        for args in grid:
            c = T.mx4a6_case(*args)
            assert c.entry == entry
            lay, total = A.layout(c.ops)
            prev_end, prev_guard = 0, 0
            for o in c.ops:
                off, n = lay[o.name]
                assert n == o.nbytes and o.guard >= A.GUARD_MIN and o.guard >= 128 * o.row_bytes
                assert off % (2 * o.align) == o.align, (c.id, o.name, off, o.align)
                assert off - prev_end >= prev_guard + o.guard, (c.id, o.name)
                prev_end, prev_guard = off + n, o.guard
            assert total - prev_end >= prev_guard and total % A.TIGHT_ALIGN == 0
            align = {o.name: o.align for o in c.ops}
            want = {"qweight": 16, "scales": 1, "e_col": 1, "y": 16}
            want.update({"xq6": 16, "xs": 1, "row_flag": 1} if entry.endswith("gemm") else {"x": 16, "workspace": 16})
            if args[5]:
                want["bias"] = 2
            assert align == want, c.id
            if entry.endswith("forward"):
                ws = [o for o in c.ops if o.kind == "ws"]
                assert len(ws) == 1 and ws[0].nbytes == getattr(A.lib(), c.ws[0])(*c.ws[1]) > 0, c.id
            else:
                assert c.ws is None and not any(o.kind == "ws" for o in c.ops)
            assert sum(o.kind == "out" for o in c.ops) == 1


def test_mxfp4_a6_kernels_do_not_spill():
    """Every kernel of mxfp4_a6.hip compiles without warnings and with ScratchSize 0: 6 decode and 4 GEMM instances."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp4_a6.hip")
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
    assert sum("mx4a6_decode_kernel" in n for n in seen) == 6, list(seen)
    assert sum("mx4a6_gemm_kernel" in n for n in seen) == 4, list(seen)
    assert len(seen) == 10, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp4_a6 kernel spills: {seen}"
