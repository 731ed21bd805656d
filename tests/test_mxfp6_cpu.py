"""MXFP6 weight-only linear layer (W6A16), the parts that need no GPU: the new entries in the header, the ctypes table and the library,
the re-exports, host-side argument validation, the form plan and its knob, the layer's constructor, export and checkpoint rules (the
keys and shapes of MXFP6A8LinearCuda), the fuzz generator's draws and the compiler's resource report for csrc/mxfp6.hip."""
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

NEW = ("bie_mxfp6_form", "bie_mxfp6_linear_forward")
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096), (2880, 5760), (32, 1), (96, 7), (1 << 20, 3))  # (K, N)


def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert "bie_mxfp6_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300


def test_re_exports_are_the_same_objects():
    from bitorch_engine.extensions import mxfp4_linear_cuda as w4, mxfp6_a8_linear_cuda as w6a8, mxfp6_linear_cuda as w6
    from bitorch_engine.utils.safe_import import KNOWN, import_extension
    assert "mxfp6_linear_cuda" in KNOWN and import_extension("mxfp6_linear_cuda") is w6
    assert w6.quantize is w6a8.quantize and w6.dequant is w6a8.dequant and w6.grad_input is w6a8.grad_input
    assert w6.col_exp is w4.col_exp and w6.blk_exp is w4.blk_exp
    assert w6.forward is not w6a8.forward and w6.form is not w6a8.form and callable(w6.forward) and callable(w6.form)


def _decode_bound():
    import fuzz_mxfp6 as F
    return F.decode_bound()


def test_argument_validation_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    b = _decode_bound()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    F = L.bie_mxfp6_linear_forward
    ok = [fake, fake, fake, fake, None, fake]  # x, qweight, scales, e_col, bias, y
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert b"bie_mxfp6_linear_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert F(*ok, 1, 8, 0, 0, -1, None) == -1       # K range
    assert F(*ok, 1, 8, (1 << 20) + 32, 0, -1, None) == -1
    assert F(*ok, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(*ok, 1 << 31, 8, 64, 0, 1, None) == -1
    assert F(*ok, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(*ok, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(*ok, 1, 8, 64, -1, -1, None) == -2
    assert F(*ok, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(*ok, 1, 8, 64, 0, -2, None) == -1
    assert F(*ok, b + 1, 8, 64, 0, 0, None) == -2   # form 0 beyond the decode bound
    assert b"bie_mxfp6_linear_forward" in L.bie_last_error() and f"M={b + 1}".encode() in L.bie_last_error()
    for i in (0, 1, 2, 5):                           # x, qweight, scales, y
        for form, M in ((0, 1), (1, 1), (-1, 1), (-1, b + 1)):
            a = list(ok)
            a[i] = None
            assert F(*a, M, 8, 64, 0, form, None) == -1, (i, form, M)
            assert b"NULL tensor pointer" in L.bie_last_error()
    a = list(ok)
    a[3] = None                                      # e_col: the prefill form needs it, the decode form does not look at it
    assert F(*a, 1, 8, 64, 0, 1, None) == -1 and b"e_col" in L.bie_last_error()
    assert F(*a, b + 1, 8, 64, 1, -1, None) == -1 and b"e_col" in L.bie_last_error()
    for i in (0, 1):                                 # alignment of x and qweight
        a = list(ok)
        a[i] = fake + 8
        assert F(*a, 1, 8, 64, 0, -1, None) == -1 and b"aligned" in L.bie_last_error(), i
    for i in (4, 5):                                 # bias and y: 2 bytes
        a = list(ok)
        a[i] = fake + 1
        assert F(*a, 1, 8, 64, 0, -1, None) == -1 and b"aligned" in L.bie_last_error(), i


def test_form_is_a_total_host_function_and_never_picks_a_missing_decode_form():
    from bitorch_engine import _hip
    L = _hip.lib()
    b = _decode_bound()
    assert b >= 1
    for K, N in SHAPES:
        for dt in (0, 1):
            fs = [L.bie_mxfp6_form(M, N, K, dt) for M in range(1, 2049)] + [L.bie_mxfp6_form(M, N, K, dt) for M in (4096, 1 << 20)]
            assert set(fs) == {0, 1} and fs == sorted(fs), (K, N)   # decode below one bound, prefill above it: monotone
            assert all(f == 1 for f in fs[b:])                       # never the decode form where it is refused


def test_form_knob_forces_either_form_where_it_is_legal():
    b = _decode_bound()
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            f"print(*[L.bie_mxfp6_form(M, N, K, d) for M in (1, {b}, {b + 1}, 4096) for K, N in ((4096, 4096), (4096, 11008), (2880, 5760), (32, 1)) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP6_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 32
    assert out["0"] == ["0"] * 16 + ["1"] * 16  # form 0 only where the decode form exists


def test_layer_is_exported_and_has_the_w6a8_checkpoint_keys_and_shapes():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda, MXFP6A8LinearCuda, MXFP6LinearCuda, MXFP6LinearForward  # noqa: F401
    layer = MXFP6LinearCuda(64, 8)
    for bias in (False, True):
        mine, theirs = MXFP6LinearCuda(64, 8, bias=bias).state_dict(), MXFP6A8LinearCuda(64, 8, bias=bias).state_dict()
        assert list(mine) == list(theirs)
        assert all(mine[k].shape == theirs[k].shape and mine[k].dtype == theirs[k].dtype for k in mine)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert layer.qweight.shape == (8, 48) and layer.scales.shape == (8, 2) and layer.e_col.shape == (8,)
    assert "e_col" not in layer.state_dict()
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP6LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP6LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        MXFP6LinearCuda(64, 8, grad_input="hip")
    assert MXFP6LinearCuda(64, 8, grad_input="kernel").grad_input == "kernel"
    with pytest.raises(ValueError):  # an MXFP4 block tensor is not an MXFP6 one
        layer.set_mx_weight(torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((8, 48), dtype=torch.int8), torch.zeros((8, 2), dtype=torch.uint8))
    # the two MXFP6 layers load each other's state dict, with and without the latent weight
    a8 = MXFP6A8LinearCuda(64, 8)
    a8.load_state_dict(layer.state_dict())
    assert torch.equal(a8.weight, layer.weight)
    other = MXFP6LinearCuda(64, 8)
    other.load_state_dict(a8.state_dict())
    assert torch.equal(other.weight, layer.weight)
    sd = {k: v for k, v in a8.state_dict().items() if k != "weight"}
    other.load_state_dict(sd)
    assert other.weight is None and set(other.state_dict()) == {"qweight", "scales"}
    # an MXFP4 state dict is refused with a message that says why, and nothing is loaded
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    with pytest.raises(RuntimeError, match="MXFP4 weight"):
        layer.load_state_dict(MXFP4LinearCuda(64, 8).state_dict())
    assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp6_linear_cuda as w6
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6LinearCuda
    q, s = torch.zeros((8, 48), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        w6.forward(torch.zeros((1, 64), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        MXFP6LinearCuda(64, 8).eval()(torch.zeros((1, 64), dtype=torch.half))


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the layer's host checks and every form is drawn."""
    import fuzz_mxfp6 as F
    import test_mxfp6_fuzz_gpu as S
    from bitorch_engine import _hip
    L = _hip.lib()
    b = F.decode_bound()
    rng = np.random.default_rng(S.SEED)
    seen = {f: 0 for f in F.FORMS}
    fake = 1 << 20
    for _ in range(S.CASES):
        c = F.draw(rng)
        M, N, K = c["M"], c["N"], c["K"]
        assert K % 32 == 0 and 32 <= K <= (1 << 20) and N >= 1 and M >= 1 and c["dt"] in F.DTS
        assert M * N <= 1000 * 640 and N * K <= 640 * 11008  # the float64 reference stays small
        for f in F.forms_of(c, b):
            seen[f] += 1
            form = 0 if f.startswith("decode") else 1
            rc = L.bie_mxfp6_linear_forward(None, fake, fake, fake, None, fake, M, N, K, 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
    assert all(n > 0 for n in seen.values()), seen


def test_mxfp6_kernels_do_not_spill():
    """Every kernel of mxfp6.hip compiles without warnings and with ScratchSize 0, and the prefill tile's static LDS is at most 64 KiB."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp6.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-Wall", "-Wno-unused-function"]
    p = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning" not in p.stderr, p.stderr[-2000:]
    scratch, lds, name = {}, {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    assert sum("mx6_decode_kernel" in n for n in scratch) >= 2, list(scratch)
    assert sum("mx6_gemm_kernel" in n for n in scratch) == 2, list(scratch)
    assert all(v == 0 for v in scratch.values()), f"an mxfp6 kernel spills: {scratch}"
    assert all(v <= 65536 for v in lds.values()), lds
