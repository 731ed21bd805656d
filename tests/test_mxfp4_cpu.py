"""MXFP4 linear layer, the parts that need no GPU: the torch restatement of the quantiser and the format (mxfp4_ref.py) against hand-worked
blocks (every tie, saturation, an all-zero block, a subnormal amax, the sign of zero), the nibble order, host-side argument validation of
every bie_mxfp4_* entry, the form plan and its knob, the layer's shape refusals and state_dict keys, and the compiler's resource report
for csrc/mxfp4.hip (no scratch)."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mxfp4_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxfp4_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def block(vals, fill=0.0):
    """One 32-value block (the rest filled) as a [1, 32] fp32 tensor."""
    return torch.tensor([list(vals) + [fill] * (32 - len(vals))], dtype=torch.float32)


def test_ties_round_to_the_even_code():
    # amax 4 -> e = floor(log2 4) - 2 = 0: the codes are the values themselves
    w = block([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.5, 1.5, 3.0, 6.0, 0.2499, 0.2501, 4.99, 5.01])
    codes, scales = ref.quantize(w)
    assert scales.tolist() == [[127]]
    #                            4  .25 .75 1.25 1.75 2.5 3.5 5  .5 1.5 3  6  <.25 >.25 <5 >5
    assert codes[0, :16].tolist() == [6, 0, 2, 2, 4, 4, 6, 6, 1, 3, 5, 7, 0, 1, 6, 7]
    # the same at another scale, negated: the sign bit follows, the magnitude rule is unchanged
    codes, scales = ref.quantize(-w * 2.0 ** -20)
    assert scales.tolist() == [[107]]
    assert codes[0, :16].tolist() == [c | 8 for c in [6, 0, 2, 2, 4, 4, 6, 6, 1, 3, 5, 7, 0, 1, 6, 7]]


def test_saturation_in_six_to_eight_times_the_scale():
    for e in (-100, -3, 0, 5, 100):
        w = block([7.99 * 2.0 ** e, 6.0 * 2.0 ** e, 5.5 * 2.0 ** e, -7.0 * 2.0 ** e])
        codes, scales = ref.quantize(w)
        assert scales.item() == e + 127
        assert codes[0, :4].tolist() == [7, 7, 7, 15]
        W = ref.dequant(ref.pack(codes), scales)
        assert W[0, :4].tolist() == [6.0 * 2.0 ** e, 6.0 * 2.0 ** e, 6.0 * 2.0 ** e, -6.0 * 2.0 ** e]
    # the largest finite fp32 value: e = 127 - 2, no overflow
    codes, scales = ref.quantize(block([3.4028235e38]))
    assert scales.item() == 252 and codes[0, 0].item() == 7


def test_all_zero_block_and_sign_of_zero():
    codes, scales = ref.quantize(block([0.0, -0.0, 0.0], fill=-0.0))
    assert scales.item() == 0 and (codes == 0).all()
    # in a non-zero block -0.0 and values rounding to zero keep their sign bit
    codes, scales = ref.quantize(block([4.0, -0.0, 0.0, -0.1, 0.1, -0.25]))
    assert codes[0, :6].tolist() == [6, 8, 0, 8, 0, 8]
    W = ref.dequant(ref.pack(codes), scales)
    assert torch.signbit(W[0, 1]) and not torch.signbit(W[0, 2]) and W[0, 3] == 0


def test_subnormal_amax():
    tiny = 2.0 ** -127  # an fp32 subnormal; floor(log2) from the leading mantissa bit
    w = block([1.5 * tiny, tiny, 0.5 * tiny, 0.25 * tiny, -tiny])
    assert ref.floor_log2_f32(torch.tensor([1.5 * tiny, tiny, 2.0 ** -149, 2.0 ** -126])).tolist() == [-127, -127, -149, -126]
    codes, scales = ref.quantize(w)
    assert scales.item() == 0  # e = -129 clamped to -127
    assert codes[0, :5].tolist() == [3, 2, 1, 0, 10]
    W = ref.dequant(ref.pack(codes), scales).float()
    assert W[0, :5].tolist() == [1.5 * tiny, tiny, 0.5 * tiny, 0.0, -tiny]
    # the smallest normal amax: e = -128 clamped, the values are 2 * 2^-127
    codes, scales = ref.quantize(block([2.0 ** -126]))
    assert scales.item() == 0 and codes[0, 0].item() == 4
    # a subnormal amax far below: everything rounds to zero, the scale stays 0
    codes, scales = ref.quantize(block([2.0 ** -149, -(2.0 ** -140)]))
    assert scales.item() == 0 and codes[0, :2].tolist() == [0, 8]


def test_half_precision_inputs_are_quantised_in_fp32():
    w = block([4.0, 0.75, 1.75, 3.5, -5.0, 2.5])
    for dt in (torch.float16, torch.bfloat16):
        codes, scales = ref.quantize(w.to(dt))
        assert scales.item() == 127 and codes[0, :6].tolist() == [6, 2, 4, 6, 14, 4]
    codes, scales = ref.quantize(block([65504.0]).half())  # fp16 max: 65504 = 1.999 * 2^15, e = 13, 65504 / 8192 = 7.996 -> 6
    assert scales.item() == 140 and codes[0, 0].item() == 7


def test_nibble_order_and_e8m0():
    codes = torch.arange(32, dtype=torch.uint8)[None, :] % 16
    q = ref.pack(codes)
    assert q[0, :3].tolist() == [0x10, 0x32, 0x54]  # element 2j low nibble, 2j + 1 high
    assert torch.equal(ref.unpack(q), codes)
    W = ref.dequant(q, torch.tensor([[127]], dtype=torch.uint8))
    assert W[0, :16].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    s = ref.e8m0(torch.tensor([0, 1, 127, 254, 255], dtype=torch.uint8))
    assert s[:4].tolist() == [2.0 ** -127, 2.0 ** -126, 1.0, 2.0 ** 127] and torch.isnan(s[4])
    assert torch.isnan(ref.dequant(torch.zeros((1, 16), dtype=torch.uint8), torch.tensor([[255]], dtype=torch.uint8))).all()


def test_quantise_dequant_round_trip_is_a_fixed_point():
    g = torch.Generator().manual_seed(0)
    w = torch.randn((16, 256), generator=g) * torch.exp2(torch.randint(-30, 30, (16, 8), generator=g).float()).repeat_interleave(32, dim=1)
    codes, scales = ref.quantize(w)
    W = ref.dequant(ref.pack(codes), scales).float()
    c2, s2 = ref.quantize(W)
    # the scale of a block may drop where amax rounded down to 4 * 2^e, but the values are kept
    assert torch.equal(ref.dequant(ref.pack(c2), s2).float(), W)
    assert ((W - w).abs() <= w.abs().reshape(16, 8, 32).amax(-1).repeat_interleave(32, dim=1) / 4 + 0).all()


def test_argument_validation_of_every_mxfp4_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    assert L.bie_mxfp4_quantize(fake, fake, fake, 8, 48, 2, None) == -1
    assert b"bie_mxfp4_quantize" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert L.bie_mxfp4_quantize(fake, fake, fake, 8, 0, 2, None) == -1
    assert L.bie_mxfp4_quantize(fake, fake, fake, 0, 64, 2, None) == -1
    assert L.bie_mxfp4_quantize(fake, fake, fake, 8, 64, 3, None) == -2
    assert L.bie_mxfp4_quantize(None, fake, fake, 8, 64, 2, None) == -1
    assert L.bie_mxfp4_quantize(fake, fake + 8, fake, 8, 64, 2, None) == -1
    assert L.bie_mxfp4_dequant(fake, fake, fake, 8, 96 + 16, 0, None) == -1
    assert L.bie_mxfp4_dequant(fake, None, fake, 8, 96, 0, None) == -1
    assert L.bie_mxfp4_dequant(fake + 4, fake, fake, 8, 96, 0, None) == -1
    assert L.bie_mxfp4_dequant(fake, fake, fake, 8, 96, 7, None) == -2
    assert L.bie_mxfp4_col_exp(fake, None, 8, 96, None) == -1
    assert L.bie_mxfp4_col_exp(fake, fake, 8, (1 << 20) + 32, None) == -1
    F = L.bie_mxfp4_linear_forward
    assert F(fake, fake, fake, fake, None, fake, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert F(fake, fake, fake, fake, None, fake, 0, 8, 64, 0, -1, None) == -1      # M
    assert F(fake, fake, fake, fake, None, fake, 1, 0, 64, 0, -1, None) == -1      # N
    assert F(fake, fake, fake, fake, None, fake, 1, 8, 64, 2, -1, None) == -2      # fp32 x
    assert F(fake, fake, fake, fake, None, fake, 1, 8, 64, 0, 2, None) == -1       # form
    assert F(fake, fake, fake, fake, None, fake, 17, 8, 64, 0, 0, None) == -2      # the decode form takes M <= 16
    assert F(fake, fake, fake, None, None, fake, 64, 8, 64, 0, 1, None) == -1      # the prefill form needs e_col
    assert F(None, fake, fake, fake, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert F(fake, fake, None, fake, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert F(fake + 8, fake, fake, fake, None, fake, 1, 8, 64, 0, 0, None) == -1   # x alignment
    assert F(fake, fake + 4, fake, fake, None, fake, 1, 8, 64, 0, 0, None) == -1   # qweight alignment
    assert F(fake, fake, fake, fake, fake + 1, fake, 1, 8, 64, 0, 0, None) == -1   # bias alignment


def test_form_plan():
    from bitorch_engine import _hip
    L = _hip.lib()
    for N in (1, 33, 4096, 11008):
        for K in (32, 4096, 11008):
            for dt in (0, 1):
                assert [L.bie_mxfp4_form(M, N, K, dt) for M in (1, 2, 3, 4, 8, 9, 16)] == [0] * 7, (N, K, dt)
                assert [L.bie_mxfp4_form(M, N, K, dt) for M in (17, 64, 4096)] == [1] * 3, (N, K, dt)


def test_form_knob_forces_either_form():
    code = ("from bitorch_engine import _hip; L = _hip.lib(); "
            "print(L.bie_mxfp4_form(1, 64, 64, 0), L.bie_mxfp4_form(4096, 64, 64, 0), L.bie_mxfp4_form(16, 64, 64, 1), L.bie_mxfp4_form(17, 64, 64, 1))")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bitorch-engine_amd"), os.environ.get("PYTHONPATH", "")]))
    out = {}
    for v in ("0", "1"):
        env["BIE_MXFP4_FORM"] = v
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out[v] = p.stdout.split()
    assert out["1"] == ["1", "1", "1", "1"]
    assert out["0"] == ["0", "1", "0", "1"]  # the decode form exists for M <= 16 only


def test_layer_is_exported_and_refuses_bad_shapes():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda
    from bitorch_engine.utils.safe_import import KNOWN
    assert "mxfp4_linear_cuda" in KNOWN
    layer = MXFP4LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scales"}
    assert set(MXFP4LinearCuda(64, 8, bias=True).state_dict()) == {"weight", "qweight", "scales", "bias"}
    assert layer.qweight.shape == (8, 32) and layer.qweight.dtype == torch.uint8
    assert layer.scales.shape == (8, 2) and layer.scales.dtype == torch.uint8
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP4LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP4LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((8, 16), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        layer.set_mx_weight(torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 3), dtype=torch.uint8))


def test_host_tensors_are_refused():
    from bitorch_engine.extensions import mxfp4_linear_cuda as mx
    with pytest.raises(RuntimeError):
        mx.forward(torch.zeros((1, 64), dtype=torch.half), torch.zeros((8, 32), dtype=torch.uint8), torch.zeros((8, 2), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        mx.quantize(torch.zeros((8, 64)))


def test_mxfp4_kernels_do_not_spill():
    """Every kernel of mxfp4.hip compiles with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "mxfp4.hip")
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
    assert sum("mx_quantize_kernel" in n for n in seen) == 3, list(seen)
    assert sum("mx_dequant_kernel" in n for n in seen) == 3, list(seen)
    assert sum("mx_col_exp_kernel" in n for n in seen) == 1, list(seen)
    assert sum("mx_decode_kernel" in n for n in seen) == 10, list(seen)
    assert sum("mx_gemm_kernel" in n for n in seen) == 2, list(seen)
    assert all(v == 0 for v in seen.values()), f"an mxfp4 kernel spills: {seen}"
