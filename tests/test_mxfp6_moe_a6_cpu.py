"""MXFP6 W6A6 mixture-of-experts layer, the parts that need no GPU: the entries are declared, bound and exported, host-side argument
validation of every bie_mxfp6_moe_a6_* entry, the form plan and its knob, the workspace formula against a restatement, the layers' export,
refusals and state dicts (cross-loading with the W6A8 / W6A16 expert layers and blocks), the restatement (mxfp6_moe_a6_ref.py) against the
W6A6 linear restatement, and the compiler's resource report for csrc/mxfp6_moe_a6.hip (no scratch, the static LDS of the 128 x 128 tile)."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mxfp6_moe_a6_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp6_moe_a6_ref.py"))
aref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(aref)

ENTRIES = ("bie_mxfp6_moe_a6_form", "bie_mxfp6_moe_a6_workspace_bytes", "bie_mxfp6_moe_a6_forward", "bie_mxfp6_moe_a6_gemm")
ONE_K = 16384  # the largest K of the one-launch decode form (include/bie_hip.h)


def test_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    L = _hip.lib()
    header = open(os.path.join(ROOT, "include", "bie_hip.h")).read()
    for name in ENTRIES:
        assert name in _hip.SIGNATURES and re.search(r"\b%s\(" % name, header) and callable(getattr(L, name))
        # argument for argument the W6A8 expert entry of the same name
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[name.replace("moe_a6", "moe_a8")]
    assert "bie_mxfp6_moe_a6_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300


def test_argument_validation_of_every_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first

    def fwd(x=fake, idx=fake, q=fake, s=fake, e=fake, b=None, y=fake, ws=fake, T=4, S=2, E=8, N=8, K=64, xpp=0, dt=0, form=-1):
        return L.bie_mxfp6_moe_a6_forward(x, idx, q, s, e, b, y, ws, T, S, E, N, K, xpp, dt, form, None)

    def gemm(xq=fake, xs=fake, rf=fake, idx=fake, q=fake, s=fake, e=fake, b=None, y=fake, ws=fake, T=4, S=2, E=8, N=8, K=64, xpp=0, dt=0, form=-1):
        return L.bie_mxfp6_moe_a6_gemm(xq, xs, rf, idx, q, s, e, b, y, ws, T, S, E, N, K, xpp, dt, form, None)

    for call, name in ((fwd, b"bie_mxfp6_moe_a6_forward"), (gemm, b"bie_mxfp6_moe_a6_gemm")):
        assert call(K=48) == -1
        assert name in L.bie_last_error() and b"K=48" in L.bie_last_error()
        assert call(K=0) == -1 and call(K=(1 << 20) + 32) == -1
        assert call(N=0) == -1
        assert call(E=0) == -1 and call(E=1025) == -1
        assert b"E=1025" in L.bie_last_error()
        assert call(S=0) == -1 and call(S=33) == -1
        assert call(T=0) == -1 and call(T=(1 << 22) // 2 + 1, S=2) == -1  # P beyond 2^22
        assert b"T * S" in L.bie_last_error()
        assert call(xpp=2) == -1
        assert call(dt=2) == -2  # fp32
        assert call(form=2) == -1 and call(form=-2) == -1
        assert call(T=513, S=2, form=0) == -2  # a forced decode form beyond its bound (P = 1026 > 1024)
        assert b"P=1026" in L.bie_last_error()
        assert call(E=1024, N=(1 << 21)) == -2  # E * N = 2^31
        assert call(idx=None) == -1 and call(q=None) == -1 and call(s=None) == -1 and call(y=None) == -1
        assert call(e=None, form=0) == -1 and call(e=None, form=1) == -1  # e_col is read by every form
        assert call(ws=None, form=1) == -1   # the prefill form needs the workspace
        assert call(q=fake + 8) == -1        # qweight alignment (16 bytes, though a block is only 8-byte aligned)
        assert call(idx=fake + 2) == -1      # idx alignment
        assert call(b=fake + 1) == -1        # bias alignment
        assert call(y=fake + 8) == -1        # y alignment
        assert call(ws=fake + 8, form=1) == -1  # workspace alignment
    assert fwd(x=None) == -1 and fwd(x=fake + 8) == -1
    assert fwd(ws=None, form=0, K=ONE_K + 32) == -1  # beyond the one-launch K the decode form quantises into the workspace
    assert gemm(xq=None) == -1 and gemm(xs=None) == -1 and gemm(rf=None) == -1 and gemm(xq=fake + 8) == -1


def test_form_plan_is_monotone_in_p():
    """At fixed E the plan never returns to the decode form once it has left it, and it never takes the decode form where that form does
    not exist (P > 1024)."""
    from bitorch_engine import _hip
    F = _hip.lib().bie_mxfp6_moe_a6_form
    for E in (1, 8, 32, 64, 128, 1024):
        for N, K in ((5760, 2880), (2880, 2880), (1, 32)):
            for dt in (0, 1):
                forms = [F(P, E, N, K, dt) for P in list(range(1, 1100)) + [2048, 4096, 16384, 1 << 22]]
                assert forms == sorted(forms) and forms[0] == 0 and forms[-1] == 1, (E, N, K, dt)
                assert all(f == 1 for f in forms[1024:])


def test_form_knob_forces_either_form():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mxfp6_moe_a6_form(P, 32, 64, 64, 0) for P in (1, 1024, 1025, 16384)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP6_MOE_A6_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1", "1", "1", "1"]
    assert out["0"] == ["0", "0", "1", "1"]  # the decode form exists for P <= 1024 only


def al16(v):
    return (v + 15) // 16 * 16


def regions(T, S, E, K, xpp, form):
    """The workspace of bie_mxfp6_moe_a6_forward restated: [(name, offset, bytes)] and the total."""
    R, P = (T * S if xpp else T), T * S
    out, off = [], 0
    for name, n in (("xq6", R * (3 * K // 4)), ("xs", R * (K // 32)), ("row_flag", R)):
        out.append((name, off, n))
        off += al16(n)
    if form == 1:
        max_tiles = min(P, P // 128 + E + 1)
        n = 4 * (4 + 3 * max_tiles + P)  # head, tile table, pair list: bie_mxfp4_moe_workspace_bytes
        out.append(("routing", off, n))
        off += al16(n)
    return out, off


def test_workspace_formula_and_alignment():
    from bitorch_engine import _hip
    L = _hip.lib()
    W = L.bie_mxfp6_moe_a6_workspace_bytes
    for T in (1, 3, 17, 128, 1000, 4096):
        for S in (1, 3, 4, 32):
            for E in (1, 32, 1024):
                for K in (32, 96, 2880, ONE_K + 32):
                    for xpp in (0, 1):
                        for form in (0, 1):
                            if form == 0 and T * S > 1024:
                                assert W(T, S, E, K, xpp, form) == 0
                                continue
                            reg, total = regions(T, S, E, K, xpp, form)
                            assert W(T, S, E, K, xpp, form) == total, (T, S, E, K, xpp, form)
                            assert W(T, S, E, K, xpp, form) <= L.bie_mxfp6_moe_a8_workspace_bytes(T, S, E, K, xpp, form)  # 3K/4-byte code rows
                            assert all(off % 16 == 0 for _, off, _ in reg) and total % 16 == 0
                            if form == 1:
                                assert reg[-1][2] <= L.bie_mxfp4_moe_workspace_bytes(T * S, E) == al16(reg[-1][2])
                        assert W(T, S, E, K, xpp, -1) == regions(T, S, E, K, xpp, 1)[1]  # -1: the layout that serves either form
    assert W(0, 4, 32, 64, 0, 1) == 0 and W(4, 0, 32, 64, 0, 1) == 0 and W(4, 33, 32, 64, 0, 1) == 0 and W(4, 4, 0, 64, 0, 1) == 0
    assert W(4, 4, 1025, 64, 0, 1) == 0 and W(4, 4, 32, 48, 0, 1) == 0 and W(4, 4, 32, (1 << 20) + 32, 0, 1) == 0 and W(4, 4, 32, 64, 2, 1) == 0
    assert W(4, 4, 32, 64, 0, 2) == 0 and W((1 << 22) + 1, 1, 32, 64, 0, 1) == 0


def test_layers_are_exported_refuse_bad_shapes_and_cross_load():
    from bitorch_engine.layers.qlinear.nbit.cuda import (MXFP4A8ExpertsLinearCuda, MXFP4MoECuda, MXFP6A6ExpertsLinearCuda,
                                                         MXFP6A6ExpertsLinearForward, MXFP6A6MoECuda, MXFP6A8ExpertsLinearCuda,
                                                         MXFP6A16MoECuda, MXFP6ExpertsLinearCuda, MXFP6MoECuda)
    from bitorch_engine.utils.safe_import import KNOWN
    from bitorch_engine.extensions import mxfp6_a6_linear_cuda, mxfp6_experts_a6_cuda as ext, mxfp6_experts_a8_cuda
    assert "mxfp6_experts_a6_cuda" in KNOWN and issubclass(MXFP6A6ExpertsLinearForward, torch.autograd.Function)
    for name in ("form", "forward", "gemm", "quantize", "dequant", "col_exp", "blk_exp", "grad_input", "quantize_act", "dequant_act"):
        assert callable(getattr(ext, name))
    for name in ("quantize", "dequant", "col_exp", "blk_exp", "grad_input"):  # the weights are the same bytes: the same objects
        assert getattr(ext, name) is getattr(mxfp6_experts_a8_cuda, name)
    assert ext.quantize_act is mxfp6_a6_linear_cuda.quantize_act and ext.dequant_act is mxfp6_a6_linear_cuda.dequant_act
    assert ext.forward is not mxfp6_experts_a8_cuda.forward and ext.gemm is not mxfp6_experts_a8_cuda.gemm
    E, K, N = 3, 64, 8
    assert issubclass(MXFP6A6ExpertsLinearCuda, MXFP6A8ExpertsLinearCuda)
    layer = MXFP6A6ExpertsLinearCuda(E, K, N, bias=True)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales", "bias"} and layer.grad_input == "torch"
    assert MXFP6A6ExpertsLinearCuda(E, K, N, grad_input="kernel").grad_input == "kernel"
    with pytest.raises(ValueError):
        MXFP6A6ExpertsLinearCuda(E, K, N, grad_input="hip")
    assert tuple(layer.weight.shape) == (E, N, K) and tuple(layer.qweight.shape) == (E, N, 3 * K // 4) and tuple(layer.scales.shape) == (E, N, K // 32)
    assert tuple(layer.bias.shape) == (E, N)
    for e, k, n in ((3, 48, 8), (3, 0, 8), (3, 64, 0), (0, 64, 8), (1025, 64, 8), (3, 16, 8)):
        with pytest.raises(ValueError):
            MXFP6A6ExpertsLinearCuda(e, k, n)
    with pytest.raises(ValueError):
        MXFP6A6ExpertsLinearCuda(E, K, N, dtype=torch.float32)
    for shape in ((E, N, K // 2), (E, N, K // 32, 16), (E, N, K), (E, N + 1, 3 * K // 4), (E * N, 3 * K // 4)):  # the first two: MXFP4
        with pytest.raises(ValueError, match="MXFP6"):
            layer.set_mx_weight(torch.zeros(shape, dtype=torch.uint8), torch.zeros((E, N, K // 32), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((E, N, 3 * K // 4), dtype=torch.uint8), torch.zeros((E, N, K // 32 + 1), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((E, N, 3 * K // 4), dtype=torch.int8), torch.zeros((E, N, K // 32), dtype=torch.uint8))
    # an MXFP4 expert state dict is refused by name, and nothing is loaded from it
    four = MXFP4A8ExpertsLinearCuda(E, K, N, bias=True)
    before = layer.weight.detach().clone()
    with pytest.raises(RuntimeError, match="MXFP4.*MXFP6A6ExpertsLinearCuda"):
        layer.load_state_dict(four.state_dict())
    assert torch.equal(layer.weight, before)
    # the W6A8 and W6A16 expert layers' state dicts load, and they load this layer's
    for cls in (MXFP6A8ExpertsLinearCuda, MXFP6ExpertsLinearCuda):
        torch.manual_seed(1)
        other = cls(E, K, N, bias=True)
        assert set(other.state_dict()) == set(layer.state_dict())
        layer.load_state_dict(other.state_dict())
        assert torch.equal(layer.weight, other.weight) and not torch.equal(layer.weight, before)
        torch.manual_seed(2)
        back = cls(E, K, N, bias=True)
        back.load_state_dict(layer.state_dict())
        assert torch.equal(back.weight, layer.weight) and torch.equal(back.bias, layer.bias)
    # the block
    moe = MXFP6A6MoECuda(64, 32, 4, 2)
    assert isinstance(moe, MXFP4MoECuda) and type(moe.gate_up) is MXFP6A6ExpertsLinearCuda and type(moe.down) is MXFP6A6ExpertsLinearCuda
    assert tuple(moe.gate_up.qweight.shape) == (4, 64, 48) and tuple(moe.down.qweight.shape) == (4, 64, 24) and moe.dtype == torch.bfloat16
    assert set(moe.state_dict()) == set(MXFP6MoECuda(64, 32, 4, 2).state_dict())
    with pytest.raises(RuntimeError, match="MXFP4"):
        moe.load_state_dict(MXFP4MoECuda(64, 32, 4, 2, activations="mxfp4").state_dict())
    for cls in (MXFP6MoECuda, MXFP6A16MoECuda, MXFP6A6MoECuda):
        other = cls(64, 32, 4, 2)
        other.load_state_dict(moe.state_dict())
        assert torch.equal(other.gate_up.weight, moe.gate_up.weight) and torch.equal(other.router.weight, moe.router.weight)
        mine = MXFP6A6MoECuda(64, 32, 4, 2)
        mine.load_state_dict(cls(64, 32, 4, 2).state_dict())
    for top_k in (0, 5, 33):
        with pytest.raises(ValueError, match="mxfp6 moe"):
            MXFP6A6MoECuda(64, 32, 4, top_k)
    with pytest.raises(TypeError):
        MXFP6A6MoECuda(64, 32, 4, 2, activations="mxfp8")  # the block has one activation format
    with pytest.raises(TypeError, match="MXFP6"):
        moe.load_gpt_oss_experts(None, None, None, None, None, None)
    assert callable(moe.load_mx_experts)
    with pytest.raises(ValueError):
        moe.set_expert_mask(torch.ones(5, dtype=torch.bool))
    # the siblings are as they were
    assert type(MXFP6MoECuda(64, 32, 4, 2).gate_up) is MXFP6A8ExpertsLinearCuda and type(MXFP6A16MoECuda(64, 32, 4, 2).gate_up) is MXFP6ExpertsLinearCuda
    with pytest.raises(ValueError, match=r"^mxfp4 moe: activations must be 'dtype', 'mxfp4' or 'mxfp8' \(got 'mxfp6'\)$"):
        MXFP4MoECuda(64, 32, 4, 2, activations="mxfp6")


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp6_experts_a6_cuda as ext
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A6ExpertsLinearCuda, MXFP6A6MoECuda
    q, s = torch.zeros((3, 8, 48), dtype=torch.uint8), torch.zeros((3, 8, 2), dtype=torch.uint8)
    idx = torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.forward(torch.zeros((2, 64), dtype=torch.half), idx, q, s)
    with pytest.raises(RuntimeError):
        ext.gemm(torch.zeros((2, 48), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8), idx, q, s)
    with pytest.raises(RuntimeError):
        ext.quantize_act(torch.zeros((2, 64), dtype=torch.half))
    with pytest.raises(RuntimeError):
        ext.quantize(torch.zeros((3, 8, 64)))
    with pytest.raises(RuntimeError):
        ext.dequant(q, s)
    with pytest.raises(RuntimeError):
        MXFP6A6ExpertsLinearCuda(3, 64, 8).eval()(torch.zeros((2, 64), dtype=torch.half), idx)
    with pytest.raises(RuntimeError):
        MXFP6A6MoECuda(64, 32, 4, 2).eval()(torch.zeros((2, 64), dtype=torch.bfloat16))


def test_restatement_agrees_with_the_w6a6_linear_restatement_on_one_expert():
    """E = 1, S = 1: the expert restatement is mxfp6_a6_ref.reference, value for value."""
    g = torch.Generator().manual_seed(0)
    M, N, K = 7, 5, 96
    q = torch.randint(0, 256, (1, N, 3 * K // 4), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(118, 131, (1, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    s[0, 2, 1] = 255
    x = torch.randn((M, K), generator=g).half()
    x[3, 40] = float("inf")
    bias = torch.randn((1, N), generator=g)
    idx = torch.zeros((M, 1), dtype=torch.int32)
    xq, xs, flag = aref.a6.quantize_act(x)
    assert tuple(xq.shape) == (M, 3 * K // 4) and tuple(xs.shape) == (M, K // 32)
    want, wabs = aref.a6.reference(xq, xs, flag, q[0], s[0], bias[0])
    W = aref.dequant(q, s)
    assert W.dtype == torch.float64 and tuple(W.shape) == (1, N, K)
    for y, a in (aref.experts(x, idx, W, bias), aref.experts(x[:, None, :], idx, W, bias), aref.experts_from_codes(xq, xs, flag, idx, W, bias)):
        torch.testing.assert_close(y[:, 0], want, rtol=0, atol=0, equal_nan=True)
        ok = ~torch.isnan(want)
        torch.testing.assert_close(a[:, 0][ok], wabs[ok], rtol=0, atol=0)
    assert torch.isnan(want[3]).all() and torch.isnan(want[:, 2]).all() and torch.isfinite(want[0, 0])
    idx[3, 0] = -1  # a flagged row whose slot is skipped is +0
    y, _ = aref.experts(x, idx, W, bias)
    assert (y[3] == 0).all()
    assert aref.tolerance is aref.a6.tolerance  # the W6A6 contract, no constant of this layer's own
    # the activation quantiser is the weight quantiser: a finite row of x has the bytes quantize_packed gives it as a weight row
    xf = torch.randn((1, N, K), generator=g).half()
    qp, sp = aref.quantize_packed(xf.float())
    cq, cs, cf = aref.quantize_rows(xf[0])
    assert torch.equal(cq, qp[0]) and torch.equal(cs, sp[0]) and not cf.any()
    # the block restatement quantises at both projection inputs: it differs from the unquantised block and from the MXFP8 one
    H, inter, E, k, T = 64, 32, 4, 2, 6
    Wgu, Wd = torch.randn((E, 2 * inter, H), generator=g).double() * 0.1, torch.randn((E, H, inter), generator=g).double() * 0.1
    rw, xb = torch.randn((E, H), generator=g), torch.randn((T, H), generator=g)
    y6, i6 = aref.block(xb, rw, None, k, Wgu, None, Wd, None)
    y8, i8 = aref.m8.block(xb, rw, None, k, Wgu, None, Wd, None)
    y0, i0 = aref.mref.block(xb, rw, None, k, Wgu, None, Wd, None)
    assert torch.equal(i6, i8) and torch.equal(i6, i0) and not torch.equal(y6, y8) and not torch.equal(y6, y0)
    assert (y6 - y0).norm() / y0.norm() < 0.2


def test_mxfp6_moe_a6_kernels_do_not_spill():
    """Every kernel of mxfp6_moe_a6.hip compiles with ScratchSize 0, and the 128 x 128 grouped instance's static LDS is the 55808 bytes the
    source asserts (two stages of mx6a6_gemm_tile and the pair list)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp6_moe_a6.hip")
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
    assert sum("mx6m6_decode_kernel" in n for n in scratch) == 4, list(scratch)  # fp16 / bf16, fused or not
    assert sum("mx6m6_gemm_kernel" in n for n in scratch) == 4, list(scratch)    # fp16 / bf16, 128 x 128 and 128 x 64
    assert all(v == 0 for v in scratch.values()), f"an mxfp6 a6 moe kernel spills: {scratch}"
    gemm_lds = sorted(v for n, v in lds.items() if "mx6m6_gemm_kernel" in n)
    assert gemm_lds == [41984, 41984, 55808, 55808], lds
    assert all(v <= 65536 for v in lds.values())
