"""MXFP4 W4A8 linear layer, the parts that need no GPU: the new entries in the header, the ctypes table and the library, host-side
argument validation of every new entry, the form plan / workspace size over M = 1 .. 8192 under every forced form, the layer's
constructor and export, properties of the torch restatement of the MXFP8 activation quantiser (idempotent on x^, never a NaN code,
saturation, ties to even, both zeros, subnormal blocks, its error against the W4A4 quantiser's), the fuzz generator's draws (all
accepted by the host predicates, every form drawn) and the compiler's resource report for csrc/mxfp4_a8.hip."""
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
import mxfp4_a4_ref as ref4  # noqa: E402
import mxfp4_a8_ref as ref  # noqa: E402

NEW = ("bie_mxfp8_quantize_act", "bie_mxfp4_a8_form", "bie_mxfp4_a8_workspace_bytes", "bie_mxfp4_a8_linear_forward", "bie_mxfp4_a8_gemm")
BENCH_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))  # (K, N)
DTS = [torch.float16, torch.bfloat16]


def test_new_entries_are_declared_bound_and_exported():
    from bitorch_engine import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bie_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bie_[a-z0-9_]+)\s*\(", text))
    L = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.SIGNATURES and hasattr(L, name), name
    assert "bie_mxfp4_a8_form" in _hip._HOST_ONLY
    assert L.bie_version() == 300
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as a8, mxfp4_linear_cuda as w4
    assert a8.quantize is w4.quantize and a8.dequant is w4.dequant and a8.col_exp is w4.col_exp  # the weight side is re-used, not copied
    assert all(callable(getattr(a8, n)) for n in ("quantize_act", "dequant_act", "form", "forward", "gemm"))


def test_argument_validation_of_every_new_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    Q = L.bie_mxfp8_quantize_act
    assert Q(fake, fake, fake, fake, 4, 48, 0, None) == -1
    assert b"bie_mxfp8_quantize_act" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert Q(fake, fake, fake, fake, 0, 64, 0, None) == -1
    assert Q(fake, fake, fake, fake, 4, 64, 2, None) == -2   # fp32 x
    assert Q(None, fake, fake, fake, 4, 64, 0, None) == -1
    assert Q(fake, fake, fake, None, 4, 64, 0, None) == -1   # the row flag is not optional
    assert Q(fake + 8, fake, fake, fake, 4, 64, 0, None) == -1
    assert Q(fake, fake + 4, fake, fake, 4, 64, 0, None) == -1
    assert Q(fake, fake, fake, fake, 4, (1 << 20) + 32, 0, None) == -1
    F = L.bie_mxfp4_a8_linear_forward
    ok = [fake, fake, fake, fake, None, fake, fake]
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert F(*ok, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(*ok, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(*ok, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(*ok, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(*ok, 65, 8, 64, 0, 0, None) == -2      # the decode form takes M <= 64
    assert b"bie_mxfp4_a8_linear_forward" in L.bie_last_error() and b"M=65" in L.bie_last_error()
    for i in (0, 1, 2, 3, 5, 6):                     # x, qweight, scales, e_col, y, workspace
        a = list(ok)
        a[i] = None
        assert F(*a, 1, 8, 64, 0, -1, None) == -1, i
    for i in (0, 1, 5, 6):                           # alignment of x, qweight, y, workspace
        a = list(ok)
        a[i] = fake + 8
        assert F(*a, 1, 8, 64, 0, -1, None) == -1, i
    a = list(ok)
    a[4] = fake + 1                                  # bias alignment
    assert F(*a, 1, 8, 64, 0, -1, None) == -1
    G = L.bie_mxfp4_a8_gemm
    okg = [fake, fake, fake, fake, fake, fake, None, fake, None]
    assert G(*okg, 1, 8, 48, 1, -1, None) == -1
    assert G(*okg, 0, 8, 64, 1, -1, None) == -1
    assert G(*okg, 1, 8, 64, 2, -1, None) == -2
    assert G(*okg, 1, 8, 64, 1, -2, None) == -1
    assert G(*okg, 65, 8, 64, 1, 0, None) == -2
    for i in (0, 1, 2, 3, 4, 5, 7):                  # xq, xs, row_flag, qweight, scales, e_col, y
        a = list(okg)
        a[i] = None
        assert G(*a, 1, 8, 64, 1, -1, None) == -1, i
    for i in (0, 3, 7):
        a = list(okg)
        a[i] = fake + 8
        assert G(*a, 1, 8, 64, 1, -1, None) == -1, i


def test_form_and_workspace_are_total():
    from bitorch_engine import _hip
    L = _hip.lib()
    shapes = [(K, N) for K, N in BENCH_SHAPES] + [(32, 1), (96, 7), (1 << 20, 3)]
    for K, N in shapes:
        for dt in (0, 1):
            fs = [L.bie_mxfp4_a8_form(M, N, K, dt) for M in range(1, 8193)]
            assert set(fs) == {0, 1} and fs == sorted(fs), (K, N)   # decode below one bound, prefill above it: monotone
            assert all(f == 1 for f in fs[64:])                      # never the decode form where it is refused
        for M in (1, 2, 16, 17, 64, 65, 1000, 8192):
            for form in (-1, 0, 1):
                b = L.bie_mxfp4_a8_workspace_bytes(M, N, K, form)
                need = M * K + M * (K // 32) + M
                assert need <= b <= need + 32 and b % 16 == 0
    assert L.bie_mxfp4_a8_workspace_bytes(0, 8, 64, -1) == 0
    assert L.bie_mxfp4_a8_workspace_bytes(4, 8, 48, -1) == 0


def test_form_knob_forces_either_form_where_it_is_legal():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(*[L.bie_mxfp4_a8_form(M, N, K, d) for M in (1, 64, 65, 4096) for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (32, 1)) for d in (0, 1)])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP4_A8_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1"] * 32
    assert out["0"] == ["0"] * 16 + ["1"] * 16  # the decode form exists for M <= 64 only


def test_layer_is_exported_shares_the_weight_state_and_refuses_bad_shapes():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4A4LinearCuda, MXFP4A8LinearCuda, MXFP4A8LinearForward, MXFP4LinearCuda  # noqa: F401
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp4_a8_linear_cuda" in KNOWN
    assert issubclass(MXFP4A8LinearCuda, MXFP4LinearCuda)
    for name in ("prepare_params", "set_mx_weight", "generate_quantized_weight", "_load_from_state_dict"):
        assert getattr(MXFP4A8LinearCuda, name) is getattr(MXFP4LinearCuda, name), name   # shared, not copied
    assert MXFP4A8LinearCuda.forward is not MXFP4LinearCuda.forward and MXFP4A8LinearCuda.forward is not MXFP4A4LinearCuda.forward
    layer = MXFP4A8LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP4A8LinearCuda(64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.qweight.shape == (8, 32) and layer.scales.shape == (8, 2)
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP4A8LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP4A8LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((8, 16), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    for cls in (MXFP4LinearCuda, MXFP4A4LinearCuda):
        other = cls(64, 8)
        other.load_state_dict(layer.state_dict())   # the same keys and shapes every way
        layer.load_state_dict(other.state_dict())


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as a8
    q, s = torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        a8.forward(torch.zeros((1, 64), dtype=torch.half), q, s)
    with pytest.raises(RuntimeError):
        a8.quantize_act(torch.zeros((8, 64), dtype=torch.half))
    with pytest.raises(RuntimeError):
        a8.gemm(torch.zeros((1, 64), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), q, s)


def test_dequant_act_of_the_extension_is_the_restatement():
    from bitorch_engine.extensions import mxfp4_a8_linear_cuda as a8
    g = torch.Generator().manual_seed(9)
    x = torch.randn((5, 96), generator=g).half()
    xq, xs, _ = ref.quantize_act(x)
    assert torch.equal(a8.dequant_act(xq, xs, torch.float32).double(), ref.dequant_act(xq, xs))


@pytest.mark.parametrize("dt", DTS)
def test_restatement_is_idempotent_and_never_gives_a_nan_code(dt):
    g = torch.Generator().manual_seed(2)
    for M, K in ((8, 4096), (64, 1024), (3, 32)):
        x = (torch.randn((M, K), generator=g) * torch.exp2(torch.randint(-12, 12, (M, 1), generator=g).float())).to(dt)
        xq, xs, flag = ref.quantize_act(x)
        assert not flag.any() and xq.shape == (M, K) and xs.shape == (M, K // 32)
        assert ((xq & 0x7F) != 0x7F).all()
        xh = ref.dequant_act(xq, xs)
        assert torch.equal(xh.to(dt).double(), xh)  # x^ is a value of the dtype
        q2, s2, _ = ref.quantize_act(xh.to(dt))
        assert torch.equal(q2, xq) and torch.equal(s2, xs)
    # the non-finite row rule
    x = torch.randn((4, 64), generator=g).to(dt)
    x[1, 3], x[3, 63] = float("inf"), float("nan")
    xq, xs, flag = ref.quantize_act(x)
    assert flag.tolist() == [0, 1, 0, 1] and ((xq & 0x7F) != 0x7F).all()
    y, _ = ref.reference(xq, xs, flag, torch.zeros((2, 32), dtype=torch.uint8), torch.full((2, 2), 127, dtype=torch.uint8))
    assert torch.isnan(y[1]).all() and torch.isnan(y[3]).all() and torch.isfinite(y[0]).all() and torch.isfinite(y[2]).all()


def _block(vals, amax):
    """One block of 32: vals, then the block maximum, zeros behind."""
    x = torch.zeros((1, 32))
    x[0, :len(vals)] = torch.tensor(vals)
    x[0, 31] = amax
    return x


def test_restatement_saturation_ties_and_zeros():
    # amax 256 * 2^t -> e = t, scale code t + 127: the scaled magnitudes are the values themselves at t = 0
    for t in (0, -7, 5):
        s = 2.0 ** t
        # saturation: the block maximum itself lies in (448, 512): 449, 464 (the midpoint to the absent 480), 480, 511.9 all give 0x7E
        for big in (449.0, 464.0, 480.0, 511.9):
            xq, xs, _ = ref.quantize_act(_block([-big * s], big * s))
            assert xs.item() == t + 127 and xq[0, 31].item() == 0x7E and xq[0, 0].item() == 0xFE, (t, big)
        # ties on E4M3 midpoints go to the even mantissa, in several binades (spacing 32 at 256 .. 448, 1 at 8 .. 16, 2^-9 subnormals)
        vals = [272.0, 304.0, 432.0, 8.5, 9.5, 1.0625, 1.1875, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -10 * 1.01, 0.0, -0.0, -272.0, -9.5]
        want = [0x78, 0x7A, 0x7E, 0x50, 0x52, 0x38, 0x3A, 0x00, 0x02, 0x01, 0x00, 0x80, 0xF8, 0xD2]
        xq, xs, _ = ref.quantize_act(_block([v * s for v in vals], 256.0 * s))
        assert xs.item() == t + 127 and xq[0, 31].item() == 0x78
        assert xq[0, :len(vals)].tolist() == want, (t, xq[0, :len(vals)].tolist())
    # both zeros: an all-zero block and a block of negative zeros give scale code 0 and 32 zero bytes
    for z in (0.0, -0.0):
        xq, xs, flag = ref.quantize_act(torch.full((1, 32), z))
        assert xs.item() == 0 and not xq.any() and not flag.any()


@pytest.mark.parametrize("dt", DTS)
def test_restatement_on_subnormal_blocks(dt):
    sub = torch.arange(32, dtype=torch.int16).repeat(2)
    x = ((sub + 1).view(dt) if dt == torch.float16 else (sub * 3 + 1).view(dt)).reshape(1, 64)
    xq, xs, flag = ref.quantize_act(x)
    assert not flag.any() and ((xq & 0x7F) != 0x7F).all()
    err = (ref.dequant_act(xq, xs) - x.double()).abs()
    if dt == torch.float16:  # amax 32 * 2^-24 = 2^-19: e = -27; the scaled values 8 j (j = 1 .. 32) are E4M3 normals: 3 mantissa bits
        assert xs.tolist() == [[100, 100]]
        assert (err <= x.double().abs() * 2.0 ** -4).all() and torch.equal(ref.dequant_act(xq, xs)[0, :16], x.double()[0, :16])
    else:  # bf16 subnormals lie below 2^-126: e clamps at -127 and the scaled values are j * 2^-133 * 2^127 = j / 64, 94 / 64 and below
        assert xs.tolist() == [[0, 0]]
        assert (err <= x.double().abs() * 2.0 ** -4 + 2.0 ** -127 * 2.0 ** -10).all()  # 3 mantissa bits, or half a subnormal step of 2^-9


@pytest.mark.parametrize("dt", DTS)
def test_e4m3_activations_have_less_than_half_the_error_of_e2m1(dt):
    for seed in (0, 1, 2):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((64, 4096), generator=g).to(dt)
        xd = x.double()
        e8 = (ref.dequant_act(*ref.quantize_act(x)[:2]) - xd).norm() / xd.norm()
        e4 = (ref4.dequant_act(*ref4.quantize_act(x)[:2]) - xd).norm() / xd.norm()
        print(f"seed {seed} {dt}: relative error e4m3 {e8.item():.4f}, e2m1 {e4.item():.4f}, ratio {(e8 / e4).item():.3f}")
        assert e8 < 0.5 * e4


def test_fuzz_generator_draws_only_accepted_cases_and_every_form():
    """A host-only count of the draws of the GPU slice: every draw passes the layer's host checks (so the slice skips none on its own)
    and every form is drawn; the prefill tile predicate restated in the sweep is the launcher's (ceil(M/128) * ceil(N/128) >= 512)."""
    import fuzz_mxfp4_a8 as F
    import test_mxfp4_a8_fuzz_gpu as S
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
        fs = F.forms_of(c)
        for f in fs:
            seen[f] += 1
            form = 0 if f.startswith("decode") else 1
            # everything but the pointers is checked first: a shape the layer refuses would fail here with -1 / -2 before the NULL test
            rc = L.bie_mxfp4_a8_linear_forward(None, fake, fake, fake, None, fake, fake, M, N, K, 0, form, None)
            assert rc == -1 and b"NULL tensor pointer" in L.bie_last_error(), (c, L.bie_last_error())
        planned = L.bie_mxfp4_a8_form(M, N, K, 0)
        assert (planned == 0) == (M <= 64 and planned == 0) and any((f.startswith("decode")) == (planned == 0) for f in fs)
    assert all(n > 0 for n in seen.values()), seen


def test_mxfp4_a8_kernels_do_not_spill():
    """Every kernel of mxfp4_a8.hip compiles without warnings and with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp4_a8.hip")
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
    assert sum("mxa8_quantize_kernel" in n for n in seen) == 2, list(seen)
    assert sum("mxa8_decode_kernel" in n for n in seen) == 6, list(seen)
    assert sum("mxa8_gemm_kernel" in n for n in seen) == 4, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp4_a8 kernel spills: {seen}"
