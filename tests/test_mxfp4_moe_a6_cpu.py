"""MXFP4 W4A6 mixture-of-experts layer, the parts that need no GPU: the entries are declared, bound and exported, host-side argument
validation of every bie_mx4a6_moe_* entry, the form plan and its knob, the workspace formula against a restatement, the layers' export,
refusals and state dicts (the four MXFP4 expert layers load each other's; an MXFP6 one is refused), the restatement (mxfp4_moe_a6_ref.py)
against the W4A6 linear restatement, the CPU-side inputs of the GPU tests' constructions, and the compiler's resource report for
csrc/mxfp4_moe_a6.hip (no scratch, the static LDS of both tile widths)."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


aref = _load("mxfp4_moe_a6_ref")

ENTRIES = ("bie_mx4a6_moe_form", "bie_mx4a6_moe_workspace_bytes", "bie_mx4a6_moe_forward", "bie_mx4a6_moe_gemm")
ONE_K = 16384  # the largest K of the one-launch decode form (include/bie_hip.h)


def test_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    L = _hip.lib()
    header = open(os.path.join(ROOT, "include", "bie_hip.h")).read()
    for name in ENTRIES:
        assert name in _hip.SIGNATURES and re.search(r"\b%s\(" % name, header) and callable(getattr(L, name))
        # argument for argument the W6A6 expert entry of the same name
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[name.replace("bie_mx4a6_moe", "bie_mxfp6_moe_a6")]
    assert "bie_mx4a6_moe_form" in _hip._HOST_ONLY and "bie_mx4a6_moe_forward" not in _hip._HOST_ONLY and "bie_mx4a6_moe_gemm" not in _hip._HOST_ONLY


def test_argument_validation_of_every_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first

    def fwd(x=fake, idx=fake, q=fake, s=fake, e=fake, b=None, y=fake, ws=fake, T=4, S=2, E=8, N=8, K=64, xpp=0, dt=0, form=-1):
        return L.bie_mx4a6_moe_forward(x, idx, q, s, e, b, y, ws, T, S, E, N, K, xpp, dt, form, None)

    def gemm(xq=fake, xs=fake, rf=fake, idx=fake, q=fake, s=fake, e=fake, b=None, y=fake, ws=fake, T=4, S=2, E=8, N=8, K=64, xpp=0, dt=0, form=-1):
        return L.bie_mx4a6_moe_gemm(xq, xs, rf, idx, q, s, e, b, y, ws, T, S, E, N, K, xpp, dt, form, None)

    for call, name in ((fwd, b"bie_mx4a6_moe_forward"), (gemm, b"bie_mx4a6_moe_gemm")):
        assert call(K=48) == -1
        assert name in L.bie_last_error() and b"K=48" in L.bie_last_error()
        assert call(K=0) == -1 and call(K=(1 << 20) + 32) == -1
        assert call(N=0) == -1
        assert call(E=0) == -1 and call(E=1025) == -1
        assert name in L.bie_last_error() and b"E=1025" in L.bie_last_error()
        assert call(S=0) == -1 and call(S=33) == -1
        assert name in L.bie_last_error() and b"S=33" in L.bie_last_error()
        assert call(T=0) == -1 and call(T=(1 << 22) // 2 + 1, S=2) == -1  # P beyond 2^22
        assert b"T * S" in L.bie_last_error()
        assert call(xpp=2) == -1
        assert call(dt=2) == -2  # fp32
        assert call(form=2) == -1 and call(form=-2) == -1
        assert call(T=513, S=2, form=0) == -2  # a forced decode form beyond its bound (P = 1026 > 1024)
        assert name in L.bie_last_error() and b"P=1026" in L.bie_last_error()
        assert call(E=1024, N=(1 << 21)) == -2  # E * N = 2^31
        assert call(idx=None) == -1 and call(q=None) == -1 and call(s=None) == -1 and call(y=None) == -1
        assert call(e=None, form=0) == -1 and call(e=None, form=1) == -1  # e_col is read by every form
        assert name in L.bie_last_error() and b"NULL" in L.bie_last_error()
        assert call(ws=None, form=1) == -1   # the prefill form needs the workspace
        for kw in ({"q": fake + 8}, {"idx": fake + 2}, {"b": fake + 1}, {"y": fake + 8}, {"ws": fake + 8, "form": 1}):  # each at half its alignment
            assert call(**kw) == -1, kw
            assert name in L.bie_last_error() and b"aligned" in L.bie_last_error()
    assert fwd(x=None) == -1 and fwd(x=fake + 8) == -1
    assert fwd(ws=None, form=0, K=ONE_K + 32) == -1  # beyond the one-launch K the decode form quantises into the workspace
    assert fwd(ws=fake + 8, form=0, K=ONE_K + 32) == -1
    assert gemm(xq=None) == -1 and gemm(xs=None) == -1 and gemm(rf=None) == -1 and gemm(xq=fake + 8) == -1


def test_form_plan_is_monotone_in_p():
    """At fixed E the plan never returns to the decode form once it has left it, and it never takes the decode form where that form does
    not exist (P > 1024)."""
    from bitorch_engine import _hip
    F = _hip.lib().bie_mx4a6_moe_form
    for E in (1, 8, 32, 64, 100, 128, 1024):
        for N, K in ((5760, 2880), (2880, 2880), (1, 32)):
            for dt in (0, 1):
                forms = [F(P, E, N, K, dt) for P in range(1, 8194)]
                assert forms == sorted(forms) and forms[0] == 0 and forms[-1] == 1, (E, N, K, dt)
                assert all(f == 1 for f in forms[1024:])
                assert F(1 << 22, E, N, K, dt) == 1


def test_form_knob_forces_either_form():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mx4a6_moe_form(P, 32, 64, 64, 0) for P in (1, 1024, 1025, 16384)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP4_MOE_A6_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1", "1", "1", "1"]
    assert out["0"] == ["0", "0", "1", "1"]  # the decode form exists for P <= 1024 only


def al16(v):
    return (v + 15) // 16 * 16


def regions(T, S, E, K, xpp, form):
    """The workspace of bie_mx4a6_moe_forward restated: [(name, offset, bytes)] and the total."""
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
    W = L.bie_mx4a6_moe_workspace_bytes
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
                            assert W(T, S, E, K, xpp, form) == L.bie_mxfp6_moe_a6_workspace_bytes(T, S, E, K, xpp, form)  # the stated layout
                            assert all(off % 16 == 0 for _, off, _ in reg) and total % 16 == 0
                            if form == 1:
                                assert reg[-1][2] <= L.bie_mxfp4_moe_workspace_bytes(T * S, E) == al16(reg[-1][2])
                        assert W(T, S, E, K, xpp, -1) == regions(T, S, E, K, xpp, 1)[1]  # -1: the layout that serves either form
    assert W(0, 4, 32, 64, 0, 1) == 0 and W(4, 0, 32, 64, 0, 1) == 0 and W(4, 33, 32, 64, 0, 1) == 0 and W(4, 4, 0, 64, 0, 1) == 0
    assert W(4, 4, 1025, 64, 0, 1) == 0 and W(4, 4, 32, 48, 0, 1) == 0 and W(4, 4, 32, (1 << 20) + 32, 0, 1) == 0 and W(4, 4, 32, 64, 2, 1) == 0
    assert W(4, 4, 32, 64, 0, 2) == 0 and W((1 << 22) + 1, 1, 32, 64, 0, 1) == 0 and W(4, 4, 32, 0, 0, 1) == 0 and W(1 << 21, 4, 32, 64, 0, 1) == 0


def test_layers_are_exported_refuse_bad_shapes_and_cross_load():
    from bitorch_engine.layers.qlinear.nbit.cuda import (MXFP4A4ExpertsLinearCuda, MXFP4A6ExpertsLinearCuda, MXFP4A6ExpertsLinearForward,
                                                         MXFP4A6MoECuda, MXFP4A8ExpertsLinearCuda, MXFP4ExpertsLinearCuda, MXFP4MoECuda,
                                                         MXFP6A6ExpertsLinearCuda, MXFP6A6MoECuda)
    from bitorch_engine.utils.safe_import import KNOWN
    from bitorch_engine.extensions import mxfp4_experts_a6_cuda as ext, mxfp4_experts_a8_cuda, mxfp4_experts_cuda, mxfp6_a6_linear_cuda
    assert "mxfp4_experts_a6_cuda" in KNOWN and issubclass(MXFP4A6ExpertsLinearForward, torch.autograd.Function)
    for name in ("form", "forward", "gemm", "quantize", "dequant", "col_exp", "blk_exp", "grad_input", "quantize_act", "dequant_act"):
        assert callable(getattr(ext, name))
    for name in ("quantize", "dequant", "col_exp", "blk_exp", "grad_input"):  # the weights are the same bytes: the same objects
        assert getattr(ext, name) is getattr(mxfp4_experts_cuda, name)
    assert ext.quantize_act is mxfp6_a6_linear_cuda.quantize_act and ext.dequant_act is mxfp6_a6_linear_cuda.dequant_act
    assert ext.forward is not mxfp4_experts_a8_cuda.forward and ext.gemm is not mxfp4_experts_a8_cuda.gemm
    E, K, N = 3, 64, 8
    # the hierarchy: beside the A4 and A8 classes, not below them
    assert issubclass(MXFP4A6ExpertsLinearCuda, MXFP4ExpertsLinearCuda)
    assert not issubclass(MXFP4A6ExpertsLinearCuda, (MXFP4A4ExpertsLinearCuda, MXFP4A8ExpertsLinearCuda))
    assert MXFP4A6ExpertsLinearCuda.__bases__ == (MXFP4ExpertsLinearCuda,)
    for name in ("set_mx_weight", "prepare_params", "generate_quantized_weight"):  # inherited, not overridden
        assert getattr(MXFP4A6ExpertsLinearCuda, name) is getattr(MXFP4ExpertsLinearCuda, name)
    layer = MXFP4A6ExpertsLinearCuda(E, K, N, bias=True)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales", "bias"} and layer.grad_input == "torch"
    assert MXFP4A6ExpertsLinearCuda(E, K, N, grad_input="kernel").grad_input == "kernel"
    with pytest.raises(ValueError):
        MXFP4A6ExpertsLinearCuda(E, K, N, grad_input="hip")
    assert tuple(layer.weight.shape) == (E, N, K) and tuple(layer.qweight.shape) == (E, N, K // 2) and tuple(layer.scales.shape) == (E, N, K // 32)
    assert tuple(layer.bias.shape) == (E, N)
    for e, k, n in ((3, 48, 8), (3, 0, 8), (3, 64, 0), (0, 64, 8), (1025, 64, 8), (3, 16, 8)):
        with pytest.raises(ValueError):
            MXFP4A6ExpertsLinearCuda(e, k, n)
    with pytest.raises(ValueError):
        MXFP4A6ExpertsLinearCuda(E, K, N, dtype=torch.float32)
    for shape in ((E, N, 3 * K // 4), (E, N, K // 32, 24), (E, N, K), (E, N + 1, K // 2), (E * N, K // 2)):  # the first two: MXFP6
        with pytest.raises(ValueError):
            layer.set_mx_weight(torch.zeros(shape, dtype=torch.uint8), torch.zeros((E, N, K // 32), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((E, N, K // 2), dtype=torch.uint8), torch.zeros((E, N, K // 32 + 1), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((E, N, K // 2), dtype=torch.int8), torch.zeros((E, N, K // 32), dtype=torch.uint8))
    # an MXFP6 expert state dict is refused with a message that names both formats, and nothing is loaded from it
    six = MXFP6A6ExpertsLinearCuda(E, K, N, bias=True)
    before = layer.weight.detach().clone()
    with pytest.raises(RuntimeError, match="MXFP6.*MXFP4A6ExpertsLinearCuda"):
        layer.load_state_dict(six.state_dict())
    assert torch.equal(layer.weight, before)
    # the four MXFP4 expert classes load each other's state dicts
    four = (MXFP4ExpertsLinearCuda, MXFP4A4ExpertsLinearCuda, MXFP4A8ExpertsLinearCuda, MXFP4A6ExpertsLinearCuda)
    for i, src in enumerate(four):
        torch.manual_seed(10 + i)
        a = src(E, K, N, bias=True)
        for j, dst in enumerate(four):
            torch.manual_seed(20 + j)
            b = dst(E, K, N, bias=True)
            assert set(a.state_dict()) == set(b.state_dict()) and not torch.equal(a.weight, b.weight)
            b.load_state_dict(a.state_dict())
            assert torch.equal(b.weight, a.weight) and torch.equal(b.bias, a.bias) and torch.equal(b.qweight, a.qweight)
    # the block
    moe = MXFP4A6MoECuda(64, 32, 4, 2)
    assert isinstance(moe, MXFP4MoECuda) and type(moe.gate_up) is MXFP4A6ExpertsLinearCuda and type(moe.down) is MXFP4A6ExpertsLinearCuda
    assert moe.activations == "mxfp6"
    assert tuple(moe.gate_up.qweight.shape) == (4, 64, 32) and tuple(moe.down.qweight.shape) == (4, 64, 16) and moe.dtype == torch.bfloat16
    assert set(moe.state_dict()) == set(MXFP4MoECuda(64, 32, 4, 2).state_dict())
    with pytest.raises(RuntimeError, match="MXFP6"):
        moe.load_state_dict(MXFP6A6MoECuda(64, 32, 4, 2).state_dict())
    for kw in ({}, {"activations": "mxfp4"}, {"activations": "mxfp8"}):
        other = MXFP4MoECuda(64, 32, 4, 2, **kw)
        other.load_state_dict(moe.state_dict())
        assert torch.equal(other.gate_up.weight, moe.gate_up.weight) and torch.equal(other.router.weight, moe.router.weight)
        mine = MXFP4A6MoECuda(64, 32, 4, 2)
        src = MXFP4MoECuda(64, 32, 4, 2, **kw)
        mine.load_state_dict(src.state_dict())
        assert torch.equal(mine.down.weight, src.down.weight)
    for top_k in (0, 5, 33):
        with pytest.raises(ValueError, match="mxfp4 moe"):
            MXFP4A6MoECuda(64, 32, 4, top_k)
    with pytest.raises(TypeError):
        MXFP4A6MoECuda(64, 32, 4, 2, activations="mxfp8")  # the block has one activation format
    with pytest.raises(ValueError):
        moe.set_expert_mask(torch.ones(5, dtype=torch.bool))
    # the siblings are as they were: "mxfp6" is no value of MXFP4MoECuda's activations
    assert type(MXFP4MoECuda(64, 32, 4, 2, activations="mxfp8").gate_up) is MXFP4A8ExpertsLinearCuda
    assert type(MXFP4MoECuda(64, 32, 4, 2).gate_up) is MXFP4ExpertsLinearCuda
    with pytest.raises(ValueError, match=r"^mxfp4 moe: activations must be 'dtype', 'mxfp4' or 'mxfp8' \(got 'mxfp6'\)$"):
        MXFP4MoECuda(64, 32, 4, 2, activations="mxfp6")


def test_block_loads_gpt_oss_expert_blocks():
    """load_gpt_oss_experts is inherited: the checkpoint's [E, N, K/32, 16] blocks are taken as they are, the latent weights dropped."""
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A6MoECuda
    H, inter, E = 64, 32, 4
    g = torch.Generator().manual_seed(3)
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.uint8)  # noqa: E731
    gu_q, gu_s = u8(0, 256, E, 2 * inter, H // 32, 16), u8(120, 130, E, 2 * inter, H // 32)
    d_q, d_s = u8(0, 256, E, H, inter // 32, 16), u8(120, 130, E, H, inter // 32)
    gu_b, d_b = torch.randn((E, 2 * inter), generator=g), torch.randn((E, H), generator=g)
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4MoECuda
    assert MXFP4A6MoECuda.load_gpt_oss_experts is MXFP4MoECuda.load_gpt_oss_experts
    moe = MXFP4A6MoECuda(H, inter, E, 2)
    # the block lives on the host here, so the layout is accepted and the call then stops at e_col, a device computation (the GPU suite
    # loads the same layout on the card and runs it)
    with pytest.raises(RuntimeError, match="tensors must live on the GPU"):
        moe.load_gpt_oss_experts(gu_q, gu_s, gu_b, d_q, d_s, d_b)
    assert moe.gate_up.weight is None and torch.equal(moe.gate_up.qweight, gu_q.reshape(E, 2 * inter, H // 2)) and torch.equal(moe.gate_up.scales, gu_s)
    # MXFP6 blocks ([E, N, K/32, 24]) are no gpt-oss layout
    with pytest.raises(ValueError, match="set_mx_weight"):
        MXFP4A6MoECuda(H, inter, E, 2).load_gpt_oss_experts(u8(0, 256, E, 2 * inter, H // 32, 24), gu_s, gu_b, d_q, d_s, d_b)


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp4_experts_a6_cuda as ext
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A6ExpertsLinearCuda, MXFP4A6MoECuda
    q, s = torch.zeros((3, 8, 32), dtype=torch.uint8), torch.zeros((3, 8, 2), dtype=torch.uint8)
    idx = torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.forward(torch.zeros((2, 64), dtype=torch.half), idx, q, s)
    with pytest.raises(RuntimeError):
        ext.gemm(torch.zeros((2, 48), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8), idx, q, s)
    with pytest.raises(RuntimeError):
        ext.quantize_act(torch.zeros((2, 64), dtype=torch.half))
    with pytest.raises(RuntimeError):
        MXFP4A6ExpertsLinearCuda(3, 64, 8).eval()(torch.zeros((2, 64), dtype=torch.half), idx)
    with pytest.raises(RuntimeError):
        MXFP4A6MoECuda(64, 32, 4, 2).eval()(torch.zeros((2, 64), dtype=torch.bfloat16))


def test_restatement_agrees_with_the_w4a6_linear_restatement_on_one_expert():
    """E = 1, S = 1: the expert restatement is mxfp4_a6_ref.reference, value for value."""
    g = torch.Generator().manual_seed(0)
    M, N, K = 7, 5, 96
    q = torch.randint(0, 256, (1, N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(118, 131, (1, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    s[0, 2, 1] = 255
    x = torch.randn((M, K), generator=g).half()
    x[3, 40] = float("inf")
    bias = torch.randn((1, N), generator=g)
    idx = torch.zeros((M, 1), dtype=torch.int32)
    xq, xs, flag = aref.a6.quantize_act(x)
    assert tuple(xq.shape) == (M, 3 * K // 4) and tuple(xs.shape) == (M, K // 32)
    want, wabs = aref.a46.reference(xq, xs, flag, q[0], s[0], bias[0])
    W = aref.dequant(q, s)
    assert W.dtype == torch.float64 and tuple(W.shape) == (1, N, K)
    assert torch.equal(torch.nan_to_num(W[0], nan=-1.0), torch.nan_to_num(aref.mx.dequant(q[0], s[0]), nan=-1.0))
    for y, a in (aref.experts(x, idx, W, bias), aref.experts(x[:, None, :], idx, W, bias), aref.experts_from_codes(xq, xs, flag, idx, W, bias)):
        torch.testing.assert_close(y[:, 0], want, rtol=0, atol=0, equal_nan=True)
        ok = ~torch.isnan(want)
        torch.testing.assert_close(a[:, 0][ok], wabs[ok], rtol=0, atol=0)
    assert torch.isnan(want[3]).all() and torch.isnan(want[:, 2]).all() and torch.isfinite(want[0, 0])
    idx[3, 0] = -1  # a flagged row whose slot is skipped is +0
    y, _ = aref.experts(x, idx, W, bias)
    assert (y[3] == 0).all()
    assert aref.tolerance is aref.a46.tolerance and aref.a46.PROBE_ULPS == 0.75  # the W4A6 contract, no constant of this layer's own
    assert aref.quantize_rows is not aref.m8.quantize_rows and aref.mref is aref.m8.mref
    qp, sp = aref.quantize_packed(torch.randn((2, N, K), generator=g))
    assert tuple(qp.shape) == (2, N, K // 2) and tuple(sp.shape) == (2, N, K // 32)
    # the block restatement quantises at both projection inputs: it differs from the unquantised block and from the MXFP8 one
    H, inter, E, k, T = 64, 32, 4, 2, 6
    Wgu, Wd = torch.randn((E, 2 * inter, H), generator=g).double() * 0.1, torch.randn((E, H, inter), generator=g).double() * 0.1
    rw, xb = torch.randn((E, H), generator=g), torch.randn((T, H), generator=g)
    y6, i6 = aref.block(xb, rw, None, k, Wgu, None, Wd, None)
    y8, i8 = aref.m8.block(xb, rw, None, k, Wgu, None, Wd, None)
    y0, i0 = aref.mref.block(xb, rw, None, k, Wgu, None, Wd, None)
    assert torch.equal(i6, i8) and torch.equal(i6, i0) and not torch.equal(y6, y8) and not torch.equal(y6, y0)
    assert (y6 - y0).norm() / y0.norm() < 0.2


def test_cpu_side_inputs_of_the_gpu_constructions():
    """What the GPU tests assume of their inputs, checked where no card is needed: the routing of make_idx meets assert_coverage on every
    shape that admits it, exact_x is a fixed point of the activation quantiser under one scale code, the selector's x codes give a
    distinct exact value per k, and its weight rows are one-hot E2M1 code 1.0 with pi visiting every block."""
    G = _load("test_mxfp4_moe_a6_gpu")
    assert len(G.COVERAGE) == 5 and len(G.OTHER) == 2
    for E, S, K, N, T in G.COVERAGE:
        G.assert_coverage(G.make_idx(T, S, E, E * 1000 + S * 100 + K + N + T), E)
    with pytest.raises(AssertionError):
        G.assert_coverage(torch.zeros((4, 4), dtype=torch.int32), 3)
    for dt in (torch.float16, torch.bfloat16):
        x = G.exact_x(20, 256, dt)
        assert torch.equal(aref.fake_quant(x), x.double())
        assert len(set(aref.quantize_rows(x)[1].flatten().tolist())) == 1
        xq, xs = G.selector_x(12, 160)
        xh = aref.a6.dequant_act(xq, xs)
        assert all(len(set(row.tolist())) == 160 for row in xh) and torch.equal(xh.to(dt).double(), xh)
    codes, pi = G.selector_codes(3, 24, 160)
    assert len(set(pi.flatten().tolist())) == 3 * 24 and all(set((pi[e] // 32).tolist()) == set(range(5)) for e in range(3))
    assert int((codes != 0).sum()) == 3 * 24 and set(codes.flatten().tolist()) == {0, 2}
    W = aref.dequant(torch.stack([aref.pack(c) for c in codes]), torch.full((3, 24, 5), 127, dtype=torch.uint8))
    assert torch.equal(W.sum(-1), torch.ones((3, 24), dtype=torch.float64))
    assert torch.equal(W[torch.arange(3)[:, None], torch.arange(24)[None, :], pi], torch.ones((3, 24), dtype=torch.float64))


def test_mxfp4_moe_a6_kernels_do_not_spill():
    """Every kernel of mxfp4_moe_a6.hip compiles with ScratchSize 0, and the grouped instances' static LDS is the 49664 / 38912 bytes the
    source asserts (two stages of mx4a6_gemm_tile and the pair list)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp4_moe_a6.hip")
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
    assert sum("mx4m6_decode_kernel" in n for n in scratch) == 4, list(scratch)  # fp16 / bf16, fused or not
    assert sum("mx4m6_gemm_kernel" in n for n in scratch) == 4, list(scratch)    # fp16 / bf16, 128 x 128 and 128 x 64
    assert all(v == 0 for v in scratch.values()), f"an mxfp4 a6 moe kernel spills: {scratch}"
    gemm_lds = sorted(v for n, v in lds.items() if "mx4m6_gemm_kernel" in n)
    assert gemm_lds == [38912, 38912, 49664, 49664], lds
    assert all(v <= 65536 for v in lds.values())
    recorded = open(os.path.join(ROOT, "profiles", "mxfp4_moe_a6_resources.txt")).read()
    assert "49664" in recorded and "38912" in recorded and "ScratchSize 0: yes" in recorded
