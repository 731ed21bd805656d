"""MXFP8 W8A8 linear layer, the parts that need no GPU: the restatement's rules, the probe's figure and maps, the new entries in the
header, the ctypes table and the library, host-side argument validation of every new entry, the form plan / workspace size, the accuracy
statement against the MXFP6 restatement and the range statement, the layer's export, checkpoint rules and refusals, the fuzz generator's
draws, the layout of every arena case of test_mx8a8_arena_gpu.py and the compiler's resource report for csrc/mxfp8_a8.hip."""
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
import mxfp8_a8_ref as ref  # noqa: E402

a8 = ref.a8                       # mxfp4_a8_ref
mx6 = ref._load("mxfp6_ref")

NEW = ("bie_mx8_quantize", "bie_mx8_dequant", "bie_mx8a8_form", "bie_mx8a8_workspace_bytes", "bie_mx8a8_linear_forward", "bie_mx8a8_gemm")
BENCH_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))  # (K, N)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_rules_flags_nan_block_idempotence_and_the_activation_bytes():
    assert ref.quantize_act is a8.quantize_act and ref.dequant_act is a8.dequant_act and ref.e4m3 is a8.e4m3
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 64), generator=g).half()
    x[1, 3], x[3, 63] = float("inf"), float("nan")
    xq, xs, flag = ref.quantize_act(x)
    assert flag.tolist() == [0, 1, 0, 1] and xq.shape == (4, 64)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        w = (torch.randn((6, 96), generator=g) * 3).to(dt)
        q, s = ref.quantize(w)
        assert q.shape == (6, 96) and s.shape == (6, 3) and not ((q & 0x7F) == 0x7F).any()
        W = ref.dequant(q, s)
        q2, s2 = ref.quantize(W.float())                                # idempotent on W^
        assert torch.equal(q2, q) and torch.equal(s2, s)
        if dt != torch.float32:                                          # on finite 16-bit rows: the activation quantiser's bytes
            aq, as_, af = ref.quantize_act(w)
            assert not af.any() and torch.equal(aq, q) and torch.equal(as_, s)
        wb = w.clone()
        wb[2, 40], wb[4, 0], wb[5, 95] = float("nan"), float("inf"), float("-inf")
        qb, sb = ref.quantize(wb)                                        # the NaN-block rule: scale 255, zero bytes, nothing else moves
        assert sb[2, 1] == 255 and sb[4, 0] == 255 and sb[5, 2] == 255 and (sb == 255).sum() == 3
        assert not qb[2, 32:64].any() and not qb[4, :32].any() and not qb[5, 64:].any()
        same = sb != 255
        assert torch.equal(sb[same], s[same]) and torch.equal(qb.reshape(6, 3, 32)[same], q.reshape(6, 3, 32)[same])
        assert torch.isnan(ref.dequant(qb, sb)[2, 32:64]).all() and torch.isfinite(ref.dequant(qb, sb)[2, :32]).all()
    z = torch.zeros((1, 64))
    z[0, 1::2] = -0.0
    q, s = ref.quantize(z)
    assert not q.any() and not s.any()                                   # an all-zero block: scale 0 and zero bytes
    c, s = ref.rand_w(3, 64, g)
    s[2, 1] = 255
    b = torch.randn(3, generator=g)
    y, a = ref.reference(xq, xs, flag, c, s, b)
    assert torch.isnan(y[1]).all() and torch.isnan(y[3]).all() and torch.isnan(y[:, 2]).all()
    assert torch.isfinite(y[0, :2]).all() and torch.isfinite(y[2, :2]).all() and torch.isfinite(a).all()
    xh, W = ref.dequant_act(xq, xs), ref.dequant(c, s)
    assert torch.equal(y[0, :2], xh[0] @ W[:2].t() + b[:2].double())
    c[0, 5] = 0x7F                                                       # a NaN code: its column is NaN (probe part (d))
    y, _ = ref.reference(xq, xs, flag, c, s, b)
    assert torch.isnan(y[:, 0]).all() and torch.isfinite(y[0, 1]) and torch.isfinite(y[2, 1])


def test_probe_figure_is_the_one_in_the_profile_and_the_maps_are_stated():
    probe = open(os.path.join(ROOT, "profiles", "mxfp8_a8_probe.txt")).read()
    m = re.search(r"worst accumulation error of one instruction ([0-9.]+)", probe)
    assert m and float(m.group(1)) == ref.PROBE_ULPS and f"worst accumulation error of one instruction {ref.PROBE_ULPS:.4f}" in probe
    assert "mxfp8_a8_probe.txt" in ref.tolerance.__doc__ and f"{ref.PROBE_ULPS:.4f}" in ref.tolerance.__doc__
    assert "A = FP8 E4M3 (cbsz 0), B = FP8 E4M3 (blgp 0)" in probe
    assert probe.count("B byte map and C/D map: as expected") == 2 and probe.count("A byte map and C/D map: as expected") == 2
    assert probe.count("scale map: as expected") == 2 and "byte pairing, block map and scale map as assumed" in probe
    # part (b): bytes 0 .. 15 of lane group g in k-block g / 2, bytes 16 .. 31 in k-block G / 2 + g / 2, on A and on B, both shapes
    rows = re.findall(r"^  lane group (\d):((?: \d)+)$", probe, flags=re.M)
    assert len(rows) == 2 * (2 + 4)
    for i, (g, vals) in enumerate(rows):
        G = 2 if i < 4 else 4
        v = [int(t) for t in vals.split()]
        assert v == [int(g) // 2] * 16 + [G // 2 + int(g) // 2] * 16, (i, g, v)
    worst = max(float(v) for v in re.findall(r"largest \|D - exact\| = ([0-9.]+)", probe))
    assert worst == ref.PROBE_ULPS  # the worst count over both shapes and every data mode
    # part (d): a NaN code makes its whole row / column NaN whatever the partner holds, and nothing else
    d = re.findall(r"^\(d\) .*: (\d+) of the (\d+) outputs of that (?:row|column) are NaN; of the other (\d+), (\d+) are NaN and (\d+) are the exact sum$", probe, flags=re.M)
    assert len(d) == 16 and all(a == b and c == e and n == "0" for a, b, c, n, e in d)
    hdr = open(os.path.join(ROOT, "include", "bie_hip.h")).read()
    assert "A NaN code (0x7F / 0xFF) inside qweight makes y[:, n] NaN" in hdr


# ---- the accuracy statement and the range statement -------------------------------------------------------------------------------------------
def test_mxfp8_weights_are_not_closer_to_gaussian_rows_than_mxfp6():
    """The relative error of the quantised weight, 256 x 4096 Gaussian rows, seeds 0 .. 2: MXFP8 within 10 % of MXFP6 (measured: 0.0293
    against 0.0284, 3 % behind: both carry three mantissa bits and the E4M3 rule saturates block maxima in (448, 512) * 2^e)."""
    e8, e6 = [], []
    for seed in (0, 1, 2):
        g = torch.Generator().manual_seed(seed)
        w = torch.randn((256, 4096), generator=g)
        q8, s8 = ref.quantize(w)
        c6, s6 = mx6.quantize(w)
        e8.append(((ref.dequant(q8, s8) - w.double()).norm() / w.double().norm()).item())
        e6.append(((mx6.dequant(mx6.pack(c6), s6) - w.double()).norm() / w.double().norm()).item())
        print(f"seed {seed}: relative weight error mxfp8 {e8[-1]:.4f}, mxfp6 {e6[-1]:.4f}, ratio {e8[-1] / e6[-1]:.3f}")
        assert 0.9 * e6[-1] < e8[-1] < 1.1 * e6[-1]
    assert abs(sum(e8) / 3 - 0.0293) < 5e-4 and abs(sum(e6) / 3 - 0.0284) < 5e-4  # the figures in README / INTEGRATION


def test_range_statement_two_to_the_minus_nine_of_the_block_maximum_survives_e4m3_and_is_zero_in_e2m3():
    for t in (0, -5, 7):
        sc = 2.0 ** t
        w = torch.zeros((1, 32))
        w[0, 0], w[0, 1], w[0, 2], w[0, 31] = sc * 2.0 ** -9, -sc * 2.0 ** -9, sc / 64, sc  # the block's power-of-two maximum
        q8, s8 = ref.quantize(w)
        W8 = ref.dequant(q8, s8)
        c6, s6 = mx6.quantize(w)
        W6 = mx6.dequant(mx6.pack(c6), s6)
        assert W8[0, 31] == sc and W6[0, 31] == sc
        assert W8[0, 0] == sc * 2.0 ** -9 and W8[0, 1] == -sc * 2.0 ** -9 and W8[0, 2] == sc / 64  # E4M3 holds them exactly
        assert W6[0, 0] == 0 and W6[0, 1] == 0 and W6[0, 2] == 0        # E2M3 stops at 1/64 (half its smallest step: the tie goes to 0)


def test_discriminating_shares_are_the_ones_written_in_the_gpu_test():
    """The shares of test_mxfp8_a8_gpu.py::test_the_layer_is_w8a8_and_not_w6a8_or_w4a8, recomputed from the restatements alone on the
    small shapes of its list; every share is at least 0.5 and the bounds are less than half of the smallest."""
    import test_mxfp8_a8_gpu as T
    assert min(T.SHARES_W6A8) >= 0.5 and min(T.SHARES_W4A8) >= 0.5
    assert T.OUTSIDE_W6A8 < 0.5 * min(T.SHARES_W6A8) and T.OUTSIDE_W4A8 < 0.5 * min(T.SHARES_W4A8)
    i = 0
    for M, K, N in T.DISCRIMINATING:
        for dt in T.DTS:
            if M * K * N <= 64 * 1024 * 128:
                w, x = T.discriminating_case(M, K, N, dt)
                (r88, r68, r48), *_ = T.restated(w, x, dt)
                for (r, a), tolf, want in ((r68, mx6.tolerance, T.SHARES_W6A8[i]), (r48, a8.tolerance, T.SHARES_W4A8[i])):
                    got = ((r88[0] - r).abs() > tolf(r, a, K, dt)).double().mean().item()
                    assert abs(got - want) < 6e-4, (M, K, N, dt, got, want)
            i += 1


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
        assert not re.match(r"bie_(ternary|mxfp)", name)  # the table of tests/abi_arena.py lists those prefixes; these go to test_mx8a8_arena_gpu.py
    assert "bie_mx8a8_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as w48, mxfp4_linear_cuda as w4, mxfp6_a8_linear_cuda as w68, mxfp8_a8_linear_cuda as w88
    assert w88.col_exp is w4.col_exp                                      # re-used, not copied
    assert w88.quantize_act is w48.quantize_act and w88.dequant_act is w48.dequant_act
    for other in (w4, w48, w68):
        assert w88.forward is not other.forward and w88.form is not other.form and w88.quantize is not other.quantize
        assert w88.dequant is not other.dequant
    assert w88.gemm is not w48.gemm and w88.gemm is not w68.gemm
    assert all(callable(getattr(w88, n)) for n in ("quantize", "dequant", "form", "forward", "gemm"))
    assert not hasattr(w88, "grad_input")
    src = open(w88.__file__).read()
    assert "matmul" not in src and ".mm(" not in src and " @ " not in src  # no torch product in the shim, no fallback


def test_argument_validation_of_every_new_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    F = L.bie_mx8a8_linear_forward
    ok = [fake, fake, fake, fake, None, fake, fake]
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert b"bie_mx8a8_linear_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert F(*ok, 1, 8, 0, 0, -1, None) == -1       # K range
    assert F(*ok, 1, 8, (1 << 20) + 32, 0, -1, None) == -1
    assert F(*ok, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(*ok, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(*ok, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(*ok, 1, 8, 64, -1, -1, None) == -2
    assert F(*ok, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(*ok, 1, 8, 64, 0, -2, None) == -1
    assert F(*ok, 65, 8, 64, 0, 0, None) == -2      # the decode form takes M <= 64
    assert b"bie_mx8a8_linear_forward" in L.bie_last_error() and b"M=65" in L.bie_last_error()
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
    G = L.bie_mx8a8_gemm
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
    assert b"bie_mx8a8_gemm" in L.bie_last_error() and b"M=65" in L.bie_last_error()
    for i in (0, 1, 2, 3, 4, 5, 7):                  # xq, xs, row_flag, qweight, scales, e_col, y
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
    for name in ("bie_mx8_quantize", "bie_mx8_dequant"):  # (w, qweight, scales) / (qweight, scales, w): the codes of bie_mxfp6_quantize
        Q = getattr(L, name)
        okq = [fake, fake, fake]
        wi, qi = (0, 1) if name.endswith("quantize") else (2, 0)
        assert Q(*okq, 8, 48, 0, None) == -1 and name.encode() in L.bie_last_error()
        assert Q(*okq, 8, 0, 0, None) == -1 and Q(*okq, 8, (1 << 20) + 32, 0, None) == -1
        assert Q(*okq, 0, 64, 0, None) == -1
        assert Q(*okq, 8, 64, 3, None) == -2 and Q(*okq, 8, 64, -1, None) == -2
        for i in range(3):
            a = list(okq)
            a[i] = None
            assert Q(*a, 8, 64, 2, None) == -1 and b"NULL pointer" in L.bie_last_error()
        a = list(okq)
        a[wi] = fake + 2                             # w 4-byte aligned
        assert Q(*a, 8, 64, 2, None) == -1
        a = list(okq)
        a[qi] = fake + 8                             # qweight 16-byte aligned
        assert Q(*a, 8, 64, 2, None) == -1


def test_form_and_workspace_are_host_functions_and_total():
    from bitorch_engine import _hip
    L = _hip.lib()
    shapes = [(K, N) for K, N in BENCH_SHAPES] + [(32, 1), (96, 7), (1 << 20, 3)]
    for K, N in shapes:
        for dt in (0, 1):
            fs = [L.bie_mx8a8_form(M, N, K, dt) for M in range(1, 8193)]
            assert set(fs) == {0, 1} and fs == sorted(fs), (K, N)   # decode below one bound, prefill above it: monotone
            assert all(f == 1 for f in fs[64:])                      # never the decode form where it is refused
        for M in (1, 2, 16, 17, 64, 65, 1000, 8192):
            for form in (-1, 0, 1):
                b = L.bie_mx8a8_workspace_bytes(M, N, K, form)
                need = M * K + M * (K // 32) + M                   # xq, xs, row_flag
                assert need <= b < need + 16 and b % 16 == 0
                assert b == L.bie_mxfp4_a8_workspace_bytes(M, N, K, form)  # the W4A8 layout and value
    assert L.bie_mx8a8_workspace_bytes(0, 8, 64, -1) == 0
    assert L.bie_mx8a8_workspace_bytes(4, 8, 48, -1) == 0
    assert L.bie_mx8a8_workspace_bytes(4, 8, (1 << 20) + 32, -1) == 0


def test_form_knob_forces_either_form_where_it_is_legal():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mx8a8_form(M, N, K, d) for M in (1, 64, 65, 4096) for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (32, 1)) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP8_A8_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 32
    assert out["0"] == ["0"] * 16 + ["1"] * 16  # the decode form exists for M <= 64 only


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------
def test_layer_is_exported_and_its_checkpoint_rules_and_refusals():
    from bitorch_engine.layers.qlinear.nbit.cuda import (MXFP4A8LinearCuda, MXFP4LinearCuda, MXFP6A6LinearCuda, MXFP6A8LinearCuda, MXFP6LinearCuda,  # noqa: F401
                                                         MXFP8A8LinearCuda, MXFP8A8LinearForward)
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp8_a8_linear_cuda" in KNOWN
    assert not issubclass(MXFP8A8LinearCuda, (MXFP6A8LinearCuda, MXFP4LinearCuda))
    layer = MXFP8A8LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP8A8LinearCuda(64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.qweight.shape == (8, 64) and layer.scales.shape == (8, 2) and layer.e_col.shape == (8,)
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP8A8LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP8A8LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        MXFP8A8LinearCuda(64, 8, grad_input="fast")
    with pytest.raises(ValueError, match="no packed-weight input gradient exists for MXFP8"):
        MXFP8A8LinearCuda(64, 8, grad_input="kernel")
    assert MXFP8A8LinearCuda(64, 8, grad_input="torch").grad_input == "torch"
    for blocks in (torch.zeros((8, 48), dtype=torch.uint8), torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2, 24), dtype=torch.uint8)):
        with pytest.raises(ValueError):  # an MXFP6 or MXFP4 block tensor is not an MXFP8 one
            layer.set_mx_weight(blocks, torch.zeros((8, 2), dtype=torch.uint8))
    # a NaN code is refused with a message that says where, before anything is loaded
    for code in (0x7F, 0xFF):
        q = torch.zeros((8, 64), dtype=torch.uint8)
        q[5, 33] = code
        before = {k: v.clone() for k, v in layer.state_dict().items()}
        with pytest.raises(ValueError, match=rf"blocks\[5, 33\] = 0x{code:02X} is an E4M3 NaN code"):
            layer.set_mx_weight(q, torch.zeros((8, 2), dtype=torch.uint8))
        with pytest.raises(ValueError, match=r"blocks\[5, 33\]"):
            layer.set_mx_weight(q.reshape(8, 2, 32), torch.zeros((8, 2), dtype=torch.uint8))
        assert layer.weight is not None and all(torch.equal(before[k], v) for k, v in layer.state_dict().items())
    # latent and packed checkpoints between two MXFP8 layers
    other = MXFP8A8LinearCuda(64, 8)
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.weight, layer.weight)
    sd = {k: v for k, v in layer.state_dict().items() if k != "weight"}
    other.load_state_dict(sd)
    assert other.weight is None and set(other.state_dict()) == {"qweight", "scales"}
    # an MXFP4 and an MXFP6 state dict are refused with a message that names the format, and nothing is loaded
    for cls, what in ((MXFP4LinearCuda, "MXFP4 weight"), (MXFP4A8LinearCuda, "MXFP4 weight"), (MXFP6LinearCuda, "MXFP6 weight"),
                      (MXFP6A8LinearCuda, "MXFP6 weight"), (MXFP6A6LinearCuda, "MXFP6 weight")):
        before = {k: v.clone() for k, v in layer.state_dict().items()}
        with pytest.raises(RuntimeError, match=what + ".*MXFP8A8LinearCuda"):
            layer.load_state_dict(cls(64, 8).state_dict())
        assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp8_a8_linear_cuda as w88
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP8A8LinearCuda
    q, s = torch.zeros((8, 64), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        w88.forward(torch.zeros((1, 64), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        w88.quantize(torch.zeros((8, 64)))
    with pytest.raises(RuntimeError):
        w88.dequant(q, s)
    with pytest.raises(RuntimeError):
        w88.gemm(torch.zeros((1, 64), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), q, s)
    with pytest.raises(RuntimeError):
        MXFP8A8LinearCuda(64, 8).eval()(torch.zeros((1, 64), dtype=torch.half))


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the layer's host checks and every form is drawn."""
    import fuzz_mxfp8_a8 as F
    import test_mxfp8_a8_fuzz_gpu as S
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
            rc = L.bie_mx8a8_linear_forward(None, fake, fake, fake, None, fake, fake, M, N, K, 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
    assert all(n > 0 for n in seen.values()), seen


def test_layout_of_every_arena_case():
    """test_abi_contract_cpu.py::assert_layout's conditions on the cases of test_mx8a8_arena_gpu.py: exactly the stated alignment, guards
    that do not overlap, a workspace of exactly the size function's bytes."""
    import abi_arena as A
    import test_mx8a8_arena_gpu as T
    for entry in T.ENTRIES:
        grid = T.grid(entry)
        assert len(grid) == 2 * 2 * 3 * (3 * 2 + 2) and grid[-1][5] and grid[-1][6] == 1 and not grid[0][5]
        assert {(c[1], c[6]) for c in grid} == {(1, 0), (1, 1), (17, 0), (17, 1), (64, 0), (64, 1), (65, 1), (130, 1)}
        for args in grid:
            c = T.mx8a8_case(*args)
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
            want.update({"xq": 16, "xs": 1, "row_flag": 1} if entry.endswith("gemm") else {"x": 16, "workspace": 16})
            if args[5]:
                want["bias"] = 2
            assert align == want, c.id
            if entry.endswith("forward"):
                ws = [o for o in c.ops if o.kind == "ws"]
                assert len(ws) == 1 and ws[0].nbytes == getattr(A.lib(), c.ws[0])(*c.ws[1]) > 0, c.id
            else:
                assert c.ws is None and not any(o.kind == "ws" for o in c.ops)
            assert sum(o.kind == "out" for o in c.ops) == 1


def test_mxfp8_a8_kernels_do_not_spill():
    """Every kernel of mxfp8_a8.hip compiles without warnings and with ScratchSize 0: 3 quantise, 3 dequant, 6 decode and 4 GEMM instances."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp8_a8.hip")
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
    assert sum("mx8_quantize_kernel" in n for n in seen) == 3, list(seen)
    assert sum("mx8_dequant_kernel" in n for n in seen) == 3, list(seen)
    assert sum("mx8a8_decode_kernel" in n for n in seen) == 6, list(seen)
    assert sum("mx8a8_gemm_kernel" in n for n in seen) == 4, list(seen)
    assert len(seen) == 16, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp8_a8 kernel spills: {seen}"
    text = open(src).read()
    assert text.count("__global__") == 4  # quantise, dequant, decode, GEMM: the templates behind the 16 instances
