"""MXFP6 W6A16 mixture-of-experts layer, the parts that need no GPU: the new entries in the header, the ctypes table and the library, the
re-exports, host-side argument validation of bie_mxfp6_moe_forward, the form plan and its knob, the layers' constructor, export and
checkpoint rules (the keys and shapes of MXFP6A8ExpertsLinearCuda / MXFP6MoECuda), the routing condition of the GPU suite's coverage
cases, the fuzz generator's draws and the compiler's resource report for csrc/mxfp6_moe.hip."""
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

NEW = ("bie_mxfp6_moe_form", "bie_mxfp6_moe_forward")
DECODE_PAIRS = 1024


def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert _hip.SIGNATURES["bie_mxfp6_moe_forward"] == _hip.SIGNATURES["bie_mxfp4_moe_forward"]
    assert "bie_mxfp6_moe_form" in _hip._HOST_ONLY and "bie_mxfp6_moe_forward" not in _hip._HOST_ONLY
    assert L.bie_version() == 300


def test_re_exports_are_the_same_objects():
    from bitorch_engine.extensions import mxfp4_experts_cuda as w4, mxfp6_experts_a8_cuda as w6a8, mxfp6_experts_cuda as w6
    from bitorch_engine.utils.safe_import import KNOWN, import_extension
    assert "mxfp6_experts_cuda" in KNOWN and import_extension("mxfp6_experts_cuda") is w6
    assert w6.quantize is w6a8.quantize and w6.dequant is w6a8.dequant and w6.grad_input is w6a8.grad_input
    assert w6.col_exp is w4.col_exp and w6.blk_exp is w4.blk_exp
    assert w6.forward is not w6a8.forward and w6.form is not w6a8.form and w6.forward is not w4.forward and callable(w6.forward) and callable(w6.form)


def test_argument_validation_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    F = L.bie_mxfp6_moe_forward

    def call(x=fake, idx=fake, q=fake, s=fake, e=fake, b=None, y=fake, ws=fake, T=4, S=2, E=8, N=8, K=64, xpp=0, dt=0, form=-1):
        return F(x, idx, q, s, e, b, y, ws, T, S, E, N, K, xpp, dt, form, None)

    assert call(K=48) == -1                                          # K % 32
    assert b"bie_mxfp6_moe_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert call(K=0) == -1 and call(K=(1 << 20) + 32) == -1          # K range
    assert call(N=0) == -1                                           # N
    assert call(N=(1 << 31) - 127, E=1) == -2                        # the column tiles are counted in int
    assert call(E=0) == -1 and call(E=1025) == -1                    # E
    assert b"E=1025" in L.bie_last_error()
    assert call(S=0) == -1 and call(S=33) == -1                      # S
    assert b"S=33" in L.bie_last_error()
    assert call(T=0) == -1 and call(T=(1 << 22) // 2 + 1, S=2) == -1  # T * S beyond 2^22
    assert b"T * S" in L.bie_last_error()
    assert call(T=(1 << 22) + 1, S=1, form=1) == -1
    assert call(E=1024, N=1 << 21) == -2                             # E * N beyond int
    assert call(xpp=2) == -1 and call(xpp=-1) == -1                  # x_per_pair
    assert b"x_per_pair" in L.bie_last_error()
    assert call(dt=2) == -2 and call(dt=-1) == -2                    # fp32 x
    assert call(form=2) == -1 and call(form=-2) == -1                # form
    assert call(T=1025, S=1, form=0) == -2                           # form 0 at P = 1025
    assert b"bie_mxfp6_moe_forward" in L.bie_last_error() and b"P=1025" in L.bie_last_error()
    assert call(T=513, S=2, form=0) == -2 and call(T=1024, S=1, form=0, x=None) == -1  # P = 1024 passes the form check
    for form, T in ((0, 4), (1, 4), (-1, 4), (-1, 4096)):
        for k in ("x", "idx", "q", "s", "y"):
            assert call(**{k: None}, form=form, T=T) == -1, (k, form, T)
            assert b"NULL tensor pointer" in L.bie_last_error()
    assert call(e=None, form=1) == -1 and b"e_col" in L.bie_last_error()   # the prefill form needs e_col ...
    assert call(ws=None, form=1) == -1                                     # ... and the workspace
    assert call(e=None, T=4096) == -1 and call(ws=None, T=4096) == -1      # also when the plan takes it
    assert call(x=fake + 8) == -1 and b"aligned" in L.bie_last_error()     # x alignment
    assert call(q=fake + 8) == -1       # qweight alignment
    assert call(idx=fake + 2) == -1     # idx alignment
    assert call(b=fake + 1) == -1       # bias alignment
    assert call(y=fake + 1) == -1       # y alignment
    assert call(ws=fake + 8, form=1) == -1 and b"aligned" in L.bie_last_error()  # workspace alignment


def test_form_is_a_total_host_function_monotone_in_p_and_never_picks_a_missing_decode_form():
    from bitorch_engine import _hip
    L = _hip.lib()
    for E in (1, 2, 8, 32, 128, 1024):
        for N, K in ((5760, 2880), (2880, 2880), (1, 32), (33, 96)):
            for dt in (0, 1):
                fs = [L.bie_mxfp6_moe_form(P, E, N, K, dt) for P in range(1, 2049)] + [L.bie_mxfp6_moe_form(P, E, N, K, dt) for P in (4096, 16384, 1 << 22)]
                assert set(fs) == {0, 1} and fs == sorted(fs), (E, N, K)  # decode below one bound, grouped above it
                assert fs[0] == 0 and all(f == 1 for f in fs[DECODE_PAIRS:])


def test_form_knob_forces_either_form_where_it_is_legal():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mxfp6_moe_form(P, E, 64, 64, d) for P in (1, 1024, 1025, 16384) for E in (1, 32, 1024) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    env.pop("BIE_MXFP6_MOE_FORM", None)
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP6_MOE_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 24
    assert out["0"] == ["0"] * 12 + ["1"] * 12  # the decode form exists for P <= 1024 only


def test_layers_are_exported_and_follow_the_w6a8_checkpoint_rules():
    from bitorch_engine.layers.qlinear.nbit.cuda import (MXFP4ExpertsLinearCuda, MXFP6A16MoECuda, MXFP6A8ExpertsLinearCuda, MXFP6ExpertsLinearCuda,
                                                         MXFP6ExpertsLinearForward, MXFP6MoECuda)  # noqa: F401
    layer = MXFP6ExpertsLinearCuda(3, 64, 8)
    for bias in (False, True):
        mine, theirs = MXFP6ExpertsLinearCuda(3, 64, 8, bias=bias).state_dict(), MXFP6A8ExpertsLinearCuda(3, 64, 8, bias=bias).state_dict()
        assert list(mine) == list(theirs)
        assert all(mine[k].shape == theirs[k].shape and mine[k].dtype == theirs[k].dtype for k in mine)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert layer.weight.shape == (3, 8, 64) and layer.qweight.shape == (3, 8, 48) and layer.scales.shape == (3, 8, 2) and layer.e_col.shape == (3, 8)
    assert layer.qweight.dtype == torch.uint8 and "e_col" not in layer.state_dict()
    for E, K, N in ((3, 48, 8), (3, 0, 8), (3, 64, 0), (0, 64, 8), (1025, 64, 8), (3, 16, 8), (3, (1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP6ExpertsLinearCuda(E, K, N)
    with pytest.raises(ValueError):
        MXFP6ExpertsLinearCuda(3, 64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        MXFP6ExpertsLinearCuda(3, 64, 8, grad_input="hip")
    assert MXFP6ExpertsLinearCuda(3, 64, 8, grad_input="kernel").grad_input == "kernel"
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    for blocks, scales in ((u8(3, 8, 32), u8(3, 8, 2)), (u8(3, 8, 2, 16), u8(3, 8, 2)), (u8(3, 8, 48), u8(3, 8, 3)), (u8(2, 8, 2, 24), u8(2, 8, 2)),
                           (u8(24, 48), u8(24, 2)), (torch.zeros((3, 8, 48), dtype=torch.int8), u8(3, 8, 2))):
        with pytest.raises(ValueError):
            layer.set_mx_weight(blocks, scales)
    # the two MXFP6 expert layers load each other's state dict, with and without the latent weight
    a8 = MXFP6A8ExpertsLinearCuda(3, 64, 8)
    a8.load_state_dict(layer.state_dict())
    assert torch.equal(a8.weight, layer.weight)
    other = MXFP6ExpertsLinearCuda(3, 64, 8)
    other.load_state_dict(a8.state_dict())
    assert torch.equal(other.weight, layer.weight)
    other.load_state_dict({k: v for k, v in a8.state_dict().items() if k != "weight"})
    assert other.weight is None and set(other.state_dict()) == {"qweight", "scales"}
    a8.load_state_dict(other.state_dict())
    assert a8.weight is None
    # an MXFP4 state dict is refused with a message that says why, and nothing is loaded
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    with pytest.raises(RuntimeError, match="MXFP4 weight"):
        layer.load_state_dict(MXFP4ExpertsLinearCuda(3, 64, 8).state_dict())
    assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())
    # the block: MXFP6MoECuda's keys and shapes, its own expert class, the same refusals
    moe, w6a8 = MXFP6A16MoECuda(64, 32, 4, 2), MXFP6MoECuda(64, 32, 4, 2)
    assert list(moe.state_dict()) == list(w6a8.state_dict())
    assert all(v.shape == w6a8.state_dict()[k].shape and v.dtype == w6a8.state_dict()[k].dtype for k, v in moe.state_dict().items())
    assert type(moe.gate_up) is MXFP6ExpertsLinearCuda and type(moe.down) is MXFP6ExpertsLinearCuda and moe.activations == "dtype"
    assert moe.gate_up.qweight.shape == (4, 64, 48) and moe.down.qweight.shape == (4, 64, 24) and moe.router.weight.dtype == torch.bfloat16
    w6a8.load_state_dict(moe.state_dict())
    moe.load_state_dict(w6a8.state_dict())
    for k in (0, 5):
        with pytest.raises(ValueError):
            MXFP6A16MoECuda(64, 32, 4, k)
    with pytest.raises(TypeError, match="MXFP4"):
        moe.load_gpt_oss_experts(None, None, None, None, None, None)
    with pytest.raises(TypeError):
        MXFP6A16MoECuda(64, 32, 4, 2, activations="mxfp8")
    with pytest.raises(TypeError):
        MXFP6MoECuda(64, 32, 4, 2, activations="dtype")  # unchanged: it still takes no activations argument


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp6_experts_cuda as w6
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP6A16MoECuda, MXFP6ExpertsLinearCuda
    q, s = torch.zeros((3, 8, 48), dtype=torch.uint8), torch.zeros((3, 8, 2), dtype=torch.uint8)
    x, idx = torch.zeros((2, 64), dtype=torch.half), torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        w6.forward(x, idx, q, s)
    with pytest.raises(RuntimeError):
        w6.forward(x[:0], idx[:0], q, s)  # refused before the empty call's early return
    with pytest.raises(RuntimeError):
        MXFP6ExpertsLinearCuda(3, 64, 8).eval()(x, idx)
    with pytest.raises(RuntimeError):
        MXFP6A16MoECuda(64, 32, 4, 2, dtype=torch.half).eval()(x)


def test_routing_condition_holds_for_every_coverage_case():
    """A condition on the inputs of test_mxfp6_moe_gpu.py, checked here so that the seeds are chosen on the CPU: every coverage case's
    idx has an expert without pairs, a count that is not a multiple of 128 and a segment of more than one tile."""
    import test_mxfp6_moe_gpu as G
    assert len(G.COVERAGE) >= 10 and all(E >= 2 and T * S >= 130 for E, S, K, N, T in G.COVERAGE)
    assert all(not (E >= 2 and T * S >= 130) for E, S, K, N, T in G.OTHER)
    for E, S, K, N, T in G.COVERAGE:
        idx = G.coverage_idx(E, S, K, N, T)
        assert idx.shape == (T, S) and idx.dtype == torch.int32
        zero, partial, multi = G.coverage(idx, E)
        assert zero and partial and multi, (E, S, K, N, T)
        G.assert_coverage(idx, E)
    for seed, (T, S, E) in ((93, (70, 2, 3)), (57, (50, 3, 4))):  # the bit-identity and the non-finite tests' routings
        G.assert_coverage(G.make_idx(T, S, E, seed), E)


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the entry's host checks and every form is drawn."""
    import fuzz_mxfp6_moe as F
    import test_mxfp6_moe_fuzz_gpu as S
    from bitorch_engine import _hip
    L = _hip.lib()
    rng = np.random.default_rng(S.SEED)
    seen = {f: 0 for f in F.FORMS}
    modes, skips = set(), set()
    fake = 1 << 20
    for _ in range(S.CASES):
        c = F.draw(rng)
        E, T, Sl, N, K = c["E"], c["T"], c["S"], c["N"], F.k_of(c)
        assert 1 <= E <= 40 and 1 <= Sl <= 8 and T >= 1 and N >= 1 and K % 32 == 0 and 32 <= K <= (1 << 20) and c["dt"] in F.DTS
        assert E * N * K <= F.MAX_W and T * Sl * N <= F.MAX_Y  # the float64 reference stays small
        modes.add(c["mode"])
        skips.add(c["skip"])
        for f in F.forms_of(c):
            seen[f] += 1
            form = 0 if f.startswith("decode") else 1
            rc = L.bie_mxfp6_moe_forward(None, fake, fake, fake, fake, None, fake, fake, T, Sl, E, N, K, c["xpp"], 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
    assert all(n > 0 for n in seen.values()), seen
    assert modes == {"normal", "exact", "nonfinite"} and skips == {0.0, 0.3, 1.0}, (modes, skips)


def test_mxfp6_moe_kernels_do_not_spill():
    """Every kernel of mxfp6_moe.hip compiles without warnings and with ScratchSize 0, and the grouped tile's static LDS (two stages and
    the pair list) is at most 64 KiB."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp6_moe.hip")
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
    assert sum("mx6m_decode_kernel" in n for n in scratch) >= 2, list(scratch)
    assert sum("mx6m_gemm_kernel" in n for n in scratch) == 2, list(scratch)
    assert all(v == 0 for v in scratch.values()), f"an mxfp6 moe kernel spills: {scratch}"
    assert all(v <= 65536 for v in lds.values()), lds
    assert all(v >= 53248 + 512 for n, v in lds.items() if "mx6m_gemm_kernel" in n), lds  # two stages and prow[128]
