"""MXFP6 input gradient, the parts that need no GPU: the new entries in the header, the ctypes table and the library, host-side argument
validation of both entries, the layers' grad_input keyword, host-tensor refusal of the extension functions, the float64 restatement
against a plain loop, and the compiler's resource report for csrc/mxfp6_grad.hip."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("mxfp6_grad_ref", os.path.join(HERE, "mxfp6_grad_ref.py"))
gref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gref)

NEW = ("bie_mxfp6_linear_grad_input", "bie_mxfp6_moe_grad_input")


def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
        assert name not in _hip._HOST_ONLY
    assert L.bie_version() == 300
    from bitorch_engine.extensions import mxfp4_experts_cuda, mxfp4_linear_cuda
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as w6, mxfp6_experts_a8_cuda as ex
    assert all(callable(getattr(m, n)) for m in (w6, ex) for n in ("blk_exp", "grad_input"))
    assert w6.blk_exp is mxfp4_linear_cuda.blk_exp and ex.blk_exp is mxfp4_experts_cuda.blk_exp  # re-exported, as col_exp is


def test_argument_validation_of_both_entries_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    G = L.bie_mxfp6_linear_grad_input
    ok = [fake, fake, fake, fake, fake]                  # gy, qweight, scales, e_blk, gx
    assert G(*ok, 1, 8, 48, 0, None) == -1               # K % 32
    assert b"bie_mxfp6_linear_grad_input" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert G(*ok, 1, 8, 0, 0, None) == -1
    assert G(*ok, 1, 8, (1 << 20) + 32, 0, None) == -1   # K <= 2^20
    assert G(*ok, 0, 8, 64, 0, None) == -1               # M
    assert G(*ok, 1 << 31, 8, 64, 0, None) == -1
    assert G(*ok, 1, 0, 64, 0, None) == -1               # N
    assert G(*ok, 1, 8, 64, 2, None) == -2               # fp32
    assert G(*ok, 1, 8, 64, 3, None) == -2
    for i in range(5):
        a = list(ok)
        a[i] = None
        assert G(*a, 1, 8, 64, 0, None) == -1, i
    for i in (1, 4):                                     # alignment of qweight, gx
        a = list(ok)
        a[i] = fake + 8
        assert G(*a, 1, 8, 64, 0, None) == -1, i
    a = list(ok)
    a[0] = fake + 1                                      # gy is 2-byte data
    assert G(*a, 1, 8, 64, 0, None) == -1
    a[0] = fake + 2                                      # ... and needs no more than that: reaches the NULL check
    a[4] = None
    assert G(*a, 1, 7, 64, 0, None) == -1 and b"NULL" in L.bie_last_error()

    X = L.bie_mxfp6_moe_grad_input
    okx = [fake] * 7                                     # gy, idx, qweight, scales, e_blk, gx, workspace
    assert X(*okx, 4, 2, 3, 8, 48, 0, 0, None) == -1     # K % 32
    assert b"bie_mxfp6_moe_grad_input" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert X(*okx, 4, 2, 3, 8, (1 << 20) + 32, 0, 0, None) == -1
    assert X(*okx, 4, 2, 3, 0, 64, 0, 0, None) == -1     # N
    assert X(*okx, 4, 2, 0, 8, 64, 0, 0, None) == -1     # E
    assert X(*okx, 4, 2, 1025, 8, 64, 0, 0, None) == -1
    assert X(*okx, 4, 0, 3, 8, 64, 0, 0, None) == -1     # S
    assert X(*okx, 4, 33, 3, 8, 64, 0, 0, None) == -1
    assert X(*okx, 0, 2, 3, 8, 64, 0, 0, None) == -1     # T
    assert X(*okx, (1 << 22), 2, 3, 8, 64, 0, 0, None) == -1
    assert X(*okx, 4, 2, 3, 8, 64, 2, 0, None) == -2     # fp32 gy
    assert X(*okx, 4, 2, 3, 8, 64, 0, 2, None) == -1     # out_fp32 is 0 or 1
    for i in range(7):
        a = list(okx)
        a[i] = None
        assert X(*a, 4, 2, 3, 8, 64, 0, 1, None) == -1, i
    for i in (2, 5, 6):                                  # alignment of qweight, gx, workspace
        a = list(okx)
        a[i] = fake + 8
        assert X(*a, 4, 2, 3, 8, 64, 0, 0, None) == -1, i
    a = list(okx)
    a[1] = fake + 2                                      # idx is 4-byte data
    assert X(*a, 4, 2, 3, 8, 64, 0, 0, None) == -1


def test_grad_input_keyword_of_the_layers():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A8ExpertsLinearCuda, MXFP6A8ExpertsLinearCuda, MXFP6A8LinearCuda
    assert MXFP6A8LinearCuda(64, 8).grad_input == "torch" and MXFP6A8ExpertsLinearCuda(3, 64, 8).grad_input == "torch"
    assert MXFP6A8LinearCuda(64, 8, grad_input="kernel").grad_input == "kernel"
    assert MXFP6A8ExpertsLinearCuda(3, 64, 8, grad_input="kernel").grad_input == "kernel"
    for bad in ("nope", "", None, "Kernel"):
        with pytest.raises(ValueError):
            MXFP6A8LinearCuda(64, 8, grad_input=bad)
        with pytest.raises(ValueError):
            MXFP6A8ExpertsLinearCuda(3, 64, 8, grad_input=bad)
    # no new buffer or parameter: checkpoints are those of the layers without the keyword
    a, b = MXFP6A8LinearCuda(64, 8, bias=True, grad_input="kernel"), MXFP6A8LinearCuda(64, 8, bias=True)
    assert set(a.state_dict()) == set(b.state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    b.load_state_dict(a.state_dict())
    ea, eb = MXFP6A8ExpertsLinearCuda(3, 64, 8, grad_input="kernel"), MXFP6A8ExpertsLinearCuda(3, 64, 8)
    assert set(ea.state_dict()) == set(eb.state_dict()) and [n for n, _ in ea.named_buffers()] == [n for n, _ in eb.named_buffers()]
    # the W4A8 expert layer, which shares the backward, constructs as before
    layer = MXFP4A8ExpertsLinearCuda(3, 64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"} and layer.qweight.shape == (3, 8, 32)


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp6_a8_linear_cuda as w6, mxfp6_experts_a8_cuda as ex
    q, s = torch.zeros((8, 48), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        w6.blk_exp(s)
    with pytest.raises(RuntimeError):
        w6.grad_input(torch.zeros((3, 8), dtype=torch.half), q, s)
    qe, se = torch.zeros((2, 8, 48), dtype=torch.uint8), torch.zeros((2, 8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ex.blk_exp(se)
    with pytest.raises(RuntimeError):
        ex.grad_input(torch.zeros((3, 2, 8), dtype=torch.half), torch.zeros((3, 2), dtype=torch.int32), qe, se)


def test_grad_reference_is_the_plain_sum():
    """grad_reference against a loop over (m, k, n) on codes placed with mxfp6_ref.pack, and its NaN block-column."""
    ref = gref.ref
    g = torch.Generator().manual_seed(3)
    N, K, M = 5, 64, 3
    codes = torch.randint(0, 64, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(120, 131, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    q = ref.pack(codes)
    gy = torch.randn((M, N), generator=g).half()
    gx, a = gref.grad_reference(gy, q, s)
    vals = ref.e2m3(codes)
    for m in range(M):
        for k in (0, 1, 31, 32, 63):
            terms = [float(gy[m, n]) * float(vals[n, k]) * 2.0 ** (int(s[n, k // 32]) - 127) for n in range(N)]
            assert abs(float(gx[m, k]) - sum(terms)) <= 1e-12 * sum(abs(t) for t in terms)
            assert abs(float(a[m, k]) - sum(abs(t) for t in terms)) <= 1e-12 * sum(abs(t) for t in terms)
    s[2, 1] = 255
    gx2, _ = gref.grad_reference(gy, q, s)
    assert torch.isnan(gx2[:, 32:]).all() and torch.equal(gx2[:, :32], gx[:, :32])
    q2, s2 = gref.rand_mx(7, 96, g)
    assert q2.shape == (7, 72) and s2.shape == (7, 3) and int(s2.max()) - int(s2.min()) <= 11


def test_mxfp6_grad_kernels_do_not_spill():
    """Every kernel of mxfp6_grad.hip compiles without warnings and with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp6_grad.hip")
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
    assert sum("mx6_dgrad_kernel" in n for n in seen) == 2, list(seen)
    assert sum("mx6m_dgrad_kernel" in n for n in seen) == 4, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp6_grad kernel spills: {seen}"
