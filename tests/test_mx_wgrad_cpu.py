"""MX weight gradient, the parts that need no GPU: the three entries in the header, the ctypes table and the library, host-side argument
validation, the workspace size and the plan's range, the layers' grad_weight attribute, and the compiler's resource report for
csrc/mx_wgrad.hip."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bie_mx_wgrad_splits", "bie_mx_wgrad_workspace_bytes", "bie_mx_linear_grad_weight")


def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert "bie_mx_wgrad_splits" in _hip._HOST_ONLY and "bie_mx_linear_grad_weight" not in _hip._HOST_ONLY
    from bitorch_engine.extensions import mx_grad_weight_cuda as G
    with pytest.raises(RuntimeError):  # host tensors are refused
        G.grad_weight(torch.zeros((3, 8), dtype=torch.half), torch.zeros((3, 32), dtype=torch.half))


def test_argument_validation_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    G = L.bie_mx_linear_grad_weight
    ok = [fake] * 5  # gy, x, gw, gb, workspace
    assert G(*ok, 64, 8, 48, 0, 0, -1, None) == -1            # K % 32
    assert b"bie_mx_linear_grad_weight" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert G(*ok, 64, 8, (1 << 20) + 32, 0, 0, -1, None) == -1  # K <= 2^20
    assert G(*ok, 0, 8, 64, 0, 0, -1, None) == -1             # M
    assert G(*ok, 64, 0, 64, 0, 0, -1, None) == -1            # N
    assert G(*ok, 64, 8, 64, 2, 0, -1, None) == -2            # fp32 operands
    assert G(*ok, 64, 8, 64, 0, 2, -1, None) == -1            # out_fp32 is 0 or 1
    assert G(*ok, 64, 8, 64, 0, 0, 0, None) == -1 and b"splits=0" in L.bie_last_error()
    assert G(*ok, 64, 8, 64, 0, 0, -2, None) == -1
    assert G(*ok, 65, 8, 64, 0, 0, 4, None) == -1             # beyond ceil(65 / 32) = 3
    for i in range(3):                                        # NULL gy, x, gw
        a = list(ok)
        a[i] = None
        assert G(*a, 64, 8, 64, 0, 0, 1, None) == -1 and b"NULL" in L.bie_last_error(), i
    for i in (1, 2, 4):                                       # alignment of x, gw, workspace
        a = list(ok)
        a[i] = fake + 8
        assert G(*a, 64, 8, 64, 0, 0, 2, None) == -1, i
    a = list(ok)
    a[0] = fake + 1                                           # gy is 2-byte data
    assert G(*a, 64, 8, 64, 0, 0, 1, None) == -1
    a = list(ok)
    a[4] = None                                               # S > 1 needs the workspace
    assert G(*a, 64, 8, 64, 0, 0, 2, None) == -1 and b"workspace" in L.bie_last_error()


def test_workspace_size_and_the_plan():
    from bitorch_engine import _hip
    L = _hip.lib()
    W, P = L.bie_mx_wgrad_workspace_bytes, L.bie_mx_wgrad_splits
    assert W(65, 5, 32, 1) == 0 and W(65, 5, 48, 2) == 0 and W(65, 5, 32, 4) == 0 and W(65, 5, 32, 0) == 0
    for M, N, K, S in ((65, 5, 32, 2), (65, 5, 32, 3), (4096, 136, 160, 7), (33, 1, 32, 2)):
        assert W(M, N, K, S) == (S * (N * K + N) * 4 + 15) // 16 * 16, (M, N, K, S)
    for M, N, K in ((1, 5, 32), (65, 136, 160), (2048, 128, 128), (8192, 1024, 1024), (8192, 4096, 4096), (512, 11008, 4096), (1 << 20, 32, 32)):
        S = P(M, N, K)
        assert 1 <= S <= (M + 31) // 32, (M, N, K, S)  # at most one slice per slab of 32 rows
        assert W(M, N, K, -1) == W(M, N, K, S)
    assert P(2048, 128, 128) > 1 and P(8192, 4096, 4096) == 1  # one tile is split, a grid that already fills the device is not
    assert P(64, 8, 48) == 0 and P(0, 8, 64) == 0


@pytest.mark.parametrize("cls", ["MXFP4LinearCuda", "MXFP6LinearCuda", "MXFP8LinearCuda"])
def test_grad_weight_attribute_of_the_layers(cls):
    from bitorch_engine.layers.qlinear.nbit import cuda as layers
    a, b = getattr(layers, cls)(64, 8, bias=True), getattr(layers, cls)(64, 8, bias=True)
    assert a.grad_weight == "torch" and a.grad_input == "torch"
    a.grad_weight = "kernel"
    assert a.grad_weight == "kernel" and a.grad_input == "torch" and b.grad_weight == "torch"  # per object, independent of grad_input
    for bad in ("nope", "", None, "Kernel"):
        with pytest.raises(ValueError):
            a.grad_weight = bad
    assert a.grad_weight == "kernel"
    assert set(a.state_dict()) == set(b.state_dict()) and not any("grad_weight" in k for k in a.state_dict())
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    with pytest.raises(TypeError):
        getattr(layers, cls)(64, 8, grad_weight="kernel")  # not a constructor argument


def test_mx_wgrad_kernels_do_not_spill():
    """Every kernel of mx_wgrad.hip compiles without warnings and with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mx_wgrad.hip")
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
    assert sum("mx_wgrad_kernel" in n for n in seen) == 4 and sum("mx_wgrad_reduce_kernel" in n for n in seen) == 3, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mx_wgrad kernel spills: {seen}"
