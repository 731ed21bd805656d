"""MXFP8 input gradient, the parts that need no GPU: the two entries' declarations and host-side refusals, the layers' grad_input
attribute, host-tensor refusal of the new module, and the compiler's resource report for csrc/mxfp8_grad.hip."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bie_mx8_linear_grad_input", "bie_mx8_moe_grad_input")
FAKE = 1 << 20  # never dereferenced: every call below fails validation first


def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    from bitorch_engine.extensions import mxfp4_experts_cuda, mxfp4_linear_cuda, mxfp8_grad_cuda as m
    from bitorch_engine.utils.safe_import import import_extension
    declared = re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S))
    L = _hip.lib()
    for name, twin in zip(NEW, ("bie_mxfp6_linear_grad_input", "bie_mxfp6_moe_grad_input")):
        assert name in declared and hasattr(L, name) and name not in _hip._HOST_ONLY, name
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[twin] and not name.startswith(("bie_mxfp", "bie_ternary"))
    assert L.bie_version() == 300 and import_extension("mxfp8_grad_cuda") is m
    assert m.blk_exp is mxfp4_linear_cuda.blk_exp and m.experts_blk_exp is mxfp4_experts_cuda.blk_exp


@pytest.mark.parametrize("entry", NEW)
def test_refusals_come_before_any_launch(entry):
    from bitorch_engine import _hip
    L = _hip.lib()
    moe = entry.endswith("moe_grad_input")
    nptr, qpos = (7, 2) if moe else (5, 1)  # (gy, [idx,] qweight, scales, e_blk, gx[, workspace])

    def call(ptrs=None, M=4, K=64, dtype=0, out_fp32=0):
        ptrs = [FAKE] * nptr if ptrs is None else ptrs
        return getattr(L, entry)(*ptrs, M, *((2, 3, 8, K, dtype, out_fp32) if moe else (8, K, dtype)), None)

    cases = [dict(K=48), dict(M=0), dict(ptrs=[FAKE] * (nptr - 1) + [None]), dict(ptrs=[FAKE] * qpos + [FAKE + 8] + [FAKE] * (nptr - qpos - 1))]
    for kw in cases + ([dict(out_fp32=2)] if moe else []):
        assert call(**kw) == -1 and entry.encode() in L.bie_last_error(), kw
    assert call(dtype=2) == -2 and entry.encode() in L.bie_last_error()  # fp32


def test_grad_input_attribute_of_the_layers_and_host_tensors():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP8ExpertsLinearCuda, MXFP8LinearCuda
    for make in (lambda: MXFP8LinearCuda(64, 8, bias=True), lambda: MXFP8ExpertsLinearCuda(3, 64, 8, bias=True)):
        a, b = make(), make()
        assert a.grad_input == "torch"
        a.grad_input = "kernel"
        assert a.grad_input == "kernel" and b.grad_input == "torch"
        for bad in ("nope", "", None, "Kernel"):
            with pytest.raises(ValueError):
                a.grad_input = bad
        assert a.grad_input == "kernel"
        assert list(a.state_dict()) == list(b.state_dict()) and [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        b.load_state_dict(a.state_dict())
        assert b.grad_input == "torch"
    from bitorch_engine.extensions import mxfp8_grad_cuda as m  # host tensors are refused
    q, s = torch.zeros((8, 64), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        m.grad_input(torch.zeros((3, 8), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        m.experts_grad_input(torch.zeros((3, 2, 8), dtype=torch.half), torch.zeros((3, 2), dtype=torch.int32), q[None], s[None])


def test_mxfp8_grad_kernels_do_not_spill():
    """Every kernel of mxfp8_grad.hip compiles without warnings and with ScratchSize 0."""
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp8_grad.hip")
    flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -Wall -Wno-unused-function -Xclang -target-feature " \
            "-Xclang -packed-fp32-ops -Rpass-analysis=kernel-resource-usage"
    p = subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags.split() + ["-c", src, "-o", os.devnull], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert sum("mx8_dgrad_kernel" in n for n in names) == 2 and sum("mx8m_dgrad_kernel" in n for n in names) == 4, names
    assert len(scratch) == len(names) == 6 and not any(scratch), dict(zip(names, scratch))
