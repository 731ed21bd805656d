"""MXFP4 mixture-of-experts layer, the parts that need no GPU: host-side argument validation of every bie_mxfp4_moe_* entry, the form plan
and its knob, the workspace size, the layers' export, state_dict keys and shape refusals, the restatement (mxfp4_moe_ref.py) against two
hand-worked routings, and the compiler's resource report for csrc/mxfp4_moe.hip (no scratch)."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mxfp4_moe_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_moe_ref.py"))
mref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mref)


def test_argument_validation_of_every_moe_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    F = L.bie_mxfp4_moe_forward

    def call(x=fake, idx=fake, q=fake, s=fake, e=fake, b=None, y=fake, ws=fake, T=4, S=2, E=8, N=8, K=64, xpp=0, dt=0, form=-1):
        return F(x, idx, q, s, e, b, y, ws, T, S, E, N, K, xpp, dt, form, None)

    assert call(K=48) == -1
    assert b"bie_mxfp4_moe_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert call(K=0) == -1 and call(K=(1 << 20) + 32) == -1
    assert call(N=0) == -1
    assert call(E=0) == -1 and call(E=1025) == -1
    assert b"E=1025" in L.bie_last_error()
    assert call(S=0) == -1 and call(S=33) == -1
    assert call(T=0) == -1 and call(T=(1 << 22) // 2 + 1, S=2) == -1  # P beyond 2^22
    assert call(xpp=2) == -1
    assert call(dt=2) == -2  # fp32 x
    assert call(form=2) == -1 and call(form=-2) == -1
    assert call(T=513, S=2, form=0) == -2  # a forced decode form beyond its bound (P = 1026 > 1024)
    assert b"P=1026" in L.bie_last_error()
    assert call(x=None) == -1 and call(idx=None) == -1 and call(q=None) == -1 and call(s=None) == -1 and call(y=None) == -1
    assert call(e=None, form=1) == -1   # the prefill form needs e_col ...
    assert call(ws=None, form=1) == -1  # ... and the workspace
    assert call(x=fake + 8) == -1       # x alignment
    assert call(q=fake + 4) == -1       # qweight alignment
    assert call(idx=fake + 2) == -1     # idx alignment
    assert call(b=fake + 1) == -1       # bias alignment
    assert call(ws=fake + 8, form=1) == -1  # workspace alignment


def test_validation_never_reaches_the_device_for_the_largest_refused_p():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20
    assert L.bie_mxfp4_moe_forward(fake, fake, fake, fake, fake, None, fake, fake, (1 << 22) + 1, 1, 8, 8, 64, 0, 0, 1, None) == -1
    assert b"T * S" in L.bie_last_error()


def test_form_plan():
    """The measured bound (profiles/mxfp4_moe_bench.jsonl): the decode form for P <= 64, and up to P = 256 while P <= 2 E."""
    from bitorch_engine import _hip
    L = _hip.lib()
    for E, N, K in ((32, 5760, 2880), (32, 2880, 2880), (1, 1, 32), (8, 33, 96)):
        for dt in (0, 1):
            assert all(L.bie_mxfp4_moe_form(P, E, N, K, dt) == 0 for P in (1, 2, 4, 16, 63, 64)), (E, N, K, dt)
            assert all(L.bie_mxfp4_moe_form(P, E, N, K, dt) == 1 for P in (65, 128, 256, 4096, 16384, 1 << 22)), (E, N, K, dt)
    for dt in (0, 1):
        assert [L.bie_mxfp4_moe_form(P, 128, 5760, 2880, dt) for P in (1, 64, 65, 128, 256, 257, 1024, 16384)] == [0, 0, 0, 0, 0, 1, 1, 1]
        assert [L.bie_mxfp4_moe_form(P, 64, 5760, 2880, dt) for P in (64, 128, 129, 256)] == [0, 0, 1, 1]
        assert [L.bie_mxfp4_moe_form(P, 1024, 5760, 2880, dt) for P in (256, 257, 1024)] == [0, 1, 1]


def test_form_knob_forces_either_form():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mxfp4_moe_form(P, 32, 64, 64, 0) for P in (1, 1024, 1025, 16384)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP4_MOE_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1", "1", "1", "1"]
    assert out["0"] == ["0", "0", "1", "1"]  # the decode form exists for P <= 1024 only


def test_workspace_bytes_is_monotone_and_zero_for_refused_shapes():
    from bitorch_engine import _hip
    W = _hip.lib().bie_mxfp4_moe_workspace_bytes
    for E in (1, 32, 1024):
        sizes = [W(P, E) for P in (1, 2, 127, 128, 129, 4096, 16384, 1 << 22)]
        assert all(s > 0 and s % 16 == 0 for s in sizes)
        assert sizes == sorted(sizes)
    for P in (1, 300, 16384):
        sizes = [W(P, E) for E in (1, 2, 32, 128, 1024)]
        assert sizes == sorted(sizes)
    assert W(16384, 32) >= 4 * 16384  # at least the pair list
    assert W(0, 32) == 0 and W(-1, 32) == 0 and W((1 << 22) + 1, 32) == 0 and W(64, 0) == 0 and W(64, 1025) == 0


def test_layers_are_exported_and_refuse_bad_shapes():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4ExpertsLinearCuda, MXFP4MoECuda
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp4_experts_cuda" in KNOWN
    layer = MXFP4ExpertsLinearCuda(3, 64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP4ExpertsLinearCuda(3, 64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.weight.shape == (3, 8, 64)
    assert layer.qweight.shape == (3, 8, 32) and layer.qweight.dtype == torch.uint8
    assert layer.scales.shape == (3, 8, 2) and layer.scales.dtype == torch.uint8
    for E, K, N in ((3, 48, 8), (3, 0, 8), (3, 64, 0), (0, 64, 8), (1025, 64, 8), (3, 16, 8)):
        with pytest.raises(ValueError):
            MXFP4ExpertsLinearCuda(E, K, N)
    with pytest.raises(ValueError):
        MXFP4ExpertsLinearCuda(3, 64, 8, dtype=torch.float32)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    with pytest.raises(ValueError):
        layer.set_mx_weight(u8(3, 8, 16), u8(3, 8, 2))
    with pytest.raises(ValueError):
        layer.set_mx_weight(u8(3, 8, 32), u8(3, 8, 3))
    with pytest.raises(ValueError):
        layer.set_mx_weight(u8(2, 8, 2, 16), u8(2, 8, 2))
    with pytest.raises(ValueError):
        layer.set_mx_weight(u8(24, 32), u8(24, 2))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((3, 8, 32), dtype=torch.int8), u8(3, 8, 2))
    moe = MXFP4MoECuda(64, 32, 4, 2)
    assert set(moe.state_dict()) == {"router.weight", "router.bias"} | {f"{p}.{k}" for p in ("gate_up", "down") for k in ("weight", "qweight", "scales", "bias")}
    assert moe.gate_up.qweight.shape == (4, 64, 32) and moe.down.qweight.shape == (4, 64, 16) and moe.router.weight.dtype == torch.bfloat16
    for k in (0, 5):
        with pytest.raises(ValueError):
            MXFP4MoECuda(64, 32, 4, k)
    with pytest.raises(ValueError):
        moe.set_expert_mask(torch.ones(3, dtype=torch.bool))


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp4_experts_cuda as mx
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4ExpertsLinearCuda
    q, s = torch.zeros((3, 8, 32), dtype=torch.uint8), torch.zeros((3, 8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        mx.forward(torch.zeros((2, 64), dtype=torch.half), torch.zeros((2, 1), dtype=torch.int32), q, s)
    with pytest.raises(RuntimeError):
        mx.quantize(torch.zeros((3, 8, 64)))
    with pytest.raises(RuntimeError):
        mx.col_exp(s)
    with pytest.raises(RuntimeError):
        MXFP4ExpertsLinearCuda(3, 64, 8).eval()(torch.zeros((2, 64), dtype=torch.half), torch.zeros((2, 1), dtype=torch.int32))


def hand_weights():
    """E = 2, N = 2, K = 32.  Expert 0: row 0 = [1, 2, 0, ...] * 2^0, row 1 = [-0.5, 0, 3, 0, ...] * 2^1; expert 1: row 0 = all 1 * 2^-1,
    row 1 = [6, 0, ...] * 2^0."""
    codes = torch.zeros((2, 2, 32), dtype=torch.uint8)
    codes[0, 0, 0], codes[0, 0, 1] = 2, 4          # 1, 2
    codes[0, 1, 0], codes[0, 1, 2] = 9, 5          # -0.5, 3
    codes[1, 0, :] = 2                             # 1
    codes[1, 1, 0] = 7                             # 6
    scales = torch.tensor([[[127], [128]], [[126], [127]]], dtype=torch.uint8)
    q = mref.ref.pack(codes.reshape(4, 32)).reshape(2, 2, 16)
    return q, scales


def test_stacked_dequant_is_the_linear_layers_rule_per_expert():
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 256, (3, 5, 48), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(0, 256, (3, 5, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    s[1, 2, 0] = 255
    W = mref.dequant(q, s)
    for e in range(3):
        want = mref.ref.dequant(q[e], s[e])
        torch.testing.assert_close(W[e], want, rtol=0, atol=0, equal_nan=True)
        assert torch.equal(torch.signbit(W[e]), torch.signbit(want))


def test_restatement_against_a_hand_worked_routing():
    q, s = hand_weights()
    W = mref.dequant(q, s)
    assert W[0, 0, :3].tolist() == [1.0, 2.0, 0.0] and W[0, 1, :3].tolist() == [-1.0, 0.0, 6.0]
    assert W[1, 0].tolist() == [0.5] * 32 and W[1, 1, :2].tolist() == [6.0, 0.0]
    x = torch.zeros((2, 32))
    x[0, :3] = torch.tensor([1.0, 2.0, 3.0])
    x[1, :] = 1.0
    bias = torch.tensor([[10.0, 20.0], [30.0, 40.0]])
    idx = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32)
    y, a = mref.experts(x, idx, W, bias)
    # token 0: expert 0 -> [1 + 4, -1 + 18] + [10, 20]; expert 1 -> [0.5 * 6, 6] + [30, 40]
    assert y[0].tolist() == [[15.0, 37.0], [33.0, 46.0]]
    # token 1 (all ones): expert 1 -> [16, 6] + [30, 40]; expert 0 -> [3, 5] + [10, 20]
    assert y[1].tolist() == [[46.0, 46.0], [13.0, 25.0]]
    assert a[0, 0].tolist() == [15.0, 39.0]  # |x| . |W| + |bias|


def test_restatement_with_a_skipped_slot_and_per_pair_rows():
    q, s = hand_weights()
    W = mref.dequant(q, s)
    x = torch.zeros((2, 2, 32))  # [T, S, K]: every pair has a row of its own
    x[0, 0, 0], x[0, 1, 0], x[1, 0, 0], x[1, 1, 0] = 1.0, 2.0, 3.0, 4.0
    idx = torch.tensor([[1, -1], [0, 2]], dtype=torch.int32)  # one slot skipped by convention, one beyond E
    y, _ = mref.experts(x, idx, W, None)
    assert y[0].tolist() == [[0.5, 6.0], [0.0, 0.0]]
    assert y[1].tolist() == [[3.0, -3.0], [0.0, 0.0]]
    y, _ = mref.experts(x, idx, W, torch.ones((2, 2)))
    assert y[0, 1].tolist() == [0.0, 0.0] and y[1, 1].tolist() == [0.0, 0.0]  # a skipped slot gets no bias either


def test_block_restatement_on_a_hand_worked_token():
    # E = 2, top-1, hidden = intermediate = 32; only expert 1's first gate / up pair and one down weight are non-zero
    E, H, inter = 2, 32, 32
    Wgu = torch.zeros((E, 2 * inter, H), dtype=torch.float64)
    Wd = torch.zeros((E, H, inter), dtype=torch.float64)
    Wgu[1, 0, 0], Wgu[1, 1, 0] = 2.0, 10.0  # expert 1: g = 2 x0, u = 10 x0 (clamped to 7)
    Wd[1, 3, 0] = 0.5
    router_w = torch.zeros((E, H))
    router_w[1, 0] = 1.0
    x = torch.zeros((1, H))
    x[0, 0] = 1.0
    y, idx = mref.block(x, router_w, None, 1, Wgu, None, Wd, None)
    assert idx.tolist() == [[1]]
    g = 2.0
    want = (7.0 + 1.0) * g / (1.0 + torch.exp(torch.tensor(-1.702 * g, dtype=torch.float64))) * 0.5
    assert abs(y[0, 3].item() - want.item()) < 1e-12 and y[0].abs().sum().item() == pytest.approx(abs(want.item()))
    y16, _ = mref.block(x, router_w, None, 1, Wgu, None, Wd, None, dt=torch.bfloat16)
    assert y16[0, 3].item() == y16[0, 3].to(torch.bfloat16).item() and abs(y16[0, 3].item() - want.item()) <= 2 * 2.0 ** -8 * abs(want.item())


def test_mxfp4_moe_kernels_do_not_spill():
    """Every kernel of mxfp4_moe.hip compiles with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp4_moe.hip")
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
    assert sum("mxm_decode_kernel" in n for n in seen) == 2, list(seen)
    assert sum("mxm_route_kernel" in n for n in seen) == 1, list(seen)
    assert sum("mxm_gemm_kernel" in n for n in seen) == 2, list(seen)
    assert len(seen) == 5, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp4 moe kernel spills: {seen}"
