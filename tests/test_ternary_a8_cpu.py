"""Ternary W1.58A8 linear layer, the parts that need no GPU: the absmean ternarisation against a numpy restatement, the activation
quantiser's restatement on hand-made vectors (ties, an all-zero row, fp16 and bf16 extremes), host-side argument validation of every
bie_ternary_a8_* entry, the decode-form predicate, and the compiler's resource report for csrc/ternary_a8.hip (no scratch)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_absmean(w):
    w = w.astype(np.float32)
    beta = np.float32(max(np.abs(w).astype(np.float64).mean(), 1e-5))
    t = np.clip(np.rint(w / beta), -1, 1).astype(np.int8)
    return t, beta


def quant(x):
    """The INTEGRATION.md restatement (torch, fp32, correctly rounded division): (q int8, r fp32)."""
    xf = x.float()
    a = xf.abs().amax(dim=1).clamp(min=1e-5)
    s = torch.full_like(a, 127.0) / a
    return torch.round(xf * s[:, None]).clamp(-128, 127).to(torch.int8), a / 127.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_ternarize_absmean_matches_numpy(dtype):
    from bitorch_engine.layers.qlinear.ternary import ternarize_absmean
    g = torch.Generator().manual_seed(4)
    w = (torch.randn((67, 256), generator=g) * 0.05).to(dtype)
    t, alpha = ternarize_absmean(w)
    rt, beta = np_absmean(w.float().numpy())
    assert t.dtype == torch.int8 and alpha.shape == (67,)
    np.testing.assert_allclose(alpha.numpy(), np.full(67, beta), rtol=1e-6)
    wf = w.float().numpy()
    near = np.abs(np.abs(wf / beta) - 0.5) < 1e-4  # a mean summed in another order may flip a value at the rounding boundary
    assert np.array_equal(t.numpy()[~near], rt[~near])
    assert set(np.unique(t.numpy())) <= {-1, 0, 1}
    z, za = ternarize_absmean(torch.zeros((3, 32), dtype=dtype))
    assert (z == 0).all() and torch.allclose(za, torch.full((3,), 1e-5))


def test_ternarize_absmean_rounds_half_to_even():
    from bitorch_engine.layers.qlinear.ternary import ternarize_absmean
    w = torch.tensor([[0.5, -0.5, 1.5, -1.5, 0.49, 1.0, 0.0, 1.0]])
    beta = w.abs().mean()
    t, alpha = ternarize_absmean(w)
    assert alpha.item() == beta.item()
    want = torch.round(w / beta).clamp(-1, 1).to(torch.int8)
    assert torch.equal(t, want)
    w2 = torch.tensor([[1.0, -1.0, 0.5, -0.5]]) * 4 / 3  # beta = 1: w / beta = +-4/3, +-2/3
    assert torch.equal(ternarize_absmean(w2 / (w2.abs().mean() / 1.0))[0], torch.tensor([[1, -1, 1, -1]], dtype=torch.int8))


def test_quantiser_restatement_on_hand_made_vectors():
    # ties at .5: with a = 127, s = 1 and x * s = x exactly
    x = torch.tensor([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5] + [0.0] * 24])
    q, r = quant(x)
    assert q[0, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 126]
    assert r.item() == np.float32(1.0)
    # all-zero row: a = 1e-5, q = 0 (so y = 0 whatever the weights)
    q, r = quant(torch.zeros((1, 32)))
    assert (q == 0).all() and r.item() == np.float32(np.float32(1e-5) / np.float32(127.0))
    # fp16 65504 and the smallest subnormal: no overflow, the largest magnitude maps to +-127
    x = torch.zeros((1, 32), dtype=torch.float16)
    x[0, 0], x[0, 1], x[0, 2] = 65504.0, -65504.0, torch.finfo(torch.float16).tiny
    q, r = quant(x)
    assert q[0, :3].tolist() == [127, -127, 0] and r.item() == np.float32(np.float32(65504.0) / np.float32(127.0))
    # bf16 extremes: the largest finite value, and a row whose absmax (2e-6) is below the 1e-5 floor
    x = torch.tensor([[3.3895e38, -3.3895e38, 1.0] + [0.0] * 29, [1e-6] * 31 + [-2e-6]], dtype=torch.bfloat16)
    q, r = quant(x)
    assert q[0, :3].tolist() == [127, -127, 0]
    s = np.float32(127.0) / np.float32(1e-5)
    xs = x[1].float().numpy()
    assert q[1].tolist() == np.clip(np.rint(xs * s), -128, 127).astype(np.int8).tolist()
    assert q[1, 0].item() == 13 and q[1, 31].item() == -25
    assert r[1].item() == np.float32(np.float32(1e-5) / np.float32(127.0))


def test_quantiser_restatement_clamps_to_int8():
    x = torch.tensor([[-1.0] + [0.25] * 31])
    q, _ = quant(x)
    assert q[0, 0].item() == -127 and (q[0, 1:] == 32).all()  # 0.25 * 127 = 31.75 -> 32


def test_argument_validation_of_every_a8_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    # bie_ternary_a8_quantize: K, dtype, NULL, ldq, alignment
    assert L.bie_ternary_a8_quantize(fake, fake, fake, 2, 48, 48, 0, None) == -1
    assert b"bie_ternary_a8_quantize" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert L.bie_ternary_a8_quantize(fake, fake, fake, 2, 65568, 65568, 0, None) == -1       # K > 65536
    assert L.bie_ternary_a8_quantize(fake, fake, fake, 0, 64, 64, 0, None) == -1             # M
    assert L.bie_ternary_a8_quantize(fake, fake, fake, 2, 64, 64, 3, None) == -2             # dtype
    assert L.bie_ternary_a8_quantize(None, fake, fake, 2, 64, 64, 0, None) == -1
    assert L.bie_ternary_a8_quantize(fake, fake, None, 2, 64, 64, 0, None) == -1
    assert L.bie_ternary_a8_quantize(fake, fake, fake, 2, 64, 32, 0, None) == -1             # ldq < K
    assert L.bie_ternary_a8_quantize(fake, fake, fake, 2, 64, 72, 0, None) == -1             # ldq % 16
    assert L.bie_ternary_a8_quantize(fake + 8, fake, fake, 2, 64, 64, 0, None) == -1         # x alignment
    assert L.bie_ternary_a8_quantize(fake, fake + 4, fake, 2, 64, 64, 0, None) == -1         # q alignment
    # bie_ternary_a8_linear_fused: shape, dtype, raw with alpha, range, NULL, alignment
    assert L.bie_ternary_a8_linear_fused(fake, fake, None, fake, 1, 8, 48, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake, fake, None, fake, 1, 0, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake, fake, None, fake, 1, 8, 64, 5, 0, None) == -2
    assert L.bie_ternary_a8_linear_fused(fake, fake, fake, fake, 1, 8, 64, 0, 1, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake, fake, None, fake, 4096, 8, 64, 0, 0, None) == -2
    assert L.bie_ternary_a8_linear_fused(None, fake, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake, None, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake, fake, None, None, 1, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake + 2, fake, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_fused(fake, fake + 1, None, fake, 1, 8, 64, 0, 0, None) == -1
    # bie_ternary_a8_linear_gemm
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 64, fake, None, fake, 64, 8, 48, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 64, fake, None, fake, 0, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 64, fake, None, fake, 64, 8, 64, 4, 0, None) == -2
    assert L.bie_ternary_a8_linear_gemm(None, fake, 64, fake, None, fake, 64, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_gemm(fake, None, 64, fake, None, fake, 64, 8, 64, 0, 0, None) == -1   # r needed unless raw
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 64, fake, fake, fake, 64, 8, 64, 0, 1, None) == -1   # raw takes no alpha
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 96, fake, None, fake, 64, 8, 96, 0, 0, None) == -1   # ldq < K rounded up to 64
    assert L.bie_ternary_a8_linear_gemm(fake + 8, fake, 64, fake, None, fake, 64, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 64, fake + 2, None, fake, 64, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 64, fake, None, fake + 4, 64, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_a8_linear_gemm(fake, fake, 65600, fake, None, fake, 64, 8, 65568, 0, 0, None) == -1


def test_fused_predicate_on_a_grid():
    from bitorch_engine import _hip
    L = _hip.lib()
    for N in (1, 33, 4096, 11008):
        for K in (32, 96, 4096, 4128, 11008):
            assert L.bie_ternary_a8_fused_ok(0, N, K) == 0
            for M in (1, 2, 3, 4):
                assert L.bie_ternary_a8_fused_ok(M, N, K) == 1, (M, N, K)
            for M in (9, 16, 17, 33, 64, 4096):
                assert L.bie_ternary_a8_fused_ok(M, N, K) == 0, (M, N, K)
        for M in (5, 8):  # the 8-row instance holds 8 * K bytes of q in LDS
            assert L.bie_ternary_a8_fused_ok(M, N, 4096) == 1
            assert L.bie_ternary_a8_fused_ok(M, N, 11008) == 0
    assert L.bie_ternary_a8_fused_ok(1, 8, 48) == 0
    assert L.bie_ternary_a8_fused_ok(1, 0, 64) == 0
    assert L.bie_ternary_a8_fused_ok(1, 8, 64512) == 1
    assert L.bie_ternary_a8_fused_ok(1, 8, 65536) == 0
    assert L.bie_ternary_a8_fused_ok(2, 8, 32256) == 1
    assert L.bie_ternary_a8_fused_ok(2, 8, 32512) == 0


def test_layer_is_exported_and_refuses_bad_shapes():
    from bitorch_engine.layers.qlinear.ternary.cuda import TernaryA8LinearCuda
    from bitorch_engine.utils.safe_import import KNOWN
    assert "ternary_a8_linear_cuda" in KNOWN
    layer = TernaryA8LinearCuda(64, 8)
    assert set(layer.state_dict()) == {"weight", "qweight", "scale_w"}
    assert layer.qweight.shape == (2, 8, 8) and layer.qweight.dtype == torch.uint8
    for K, N in ((48, 8), (0, 8), (64, 0), (65568, 8)):
        with pytest.raises(ValueError):
            TernaryA8LinearCuda(K, N)


def test_ternary_a8_kernels_do_not_spill():
    """Every kernel of ternary_a8.hip compiles with ScratchSize 0, and no epilogue folds its last multiply into the fp16 conversion."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "bitorch-engine_amd", "csrc", "ternary_a8.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only"]
    p = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    assert sum("ta8_quantize_kernel" in n for n in seen) == 3, list(seen)
    assert sum("ta8_fused_kernel" in n for n in seen) == 12, list(seen)
    assert sum("ta8_gemm_kernel" in n for n in seen) == 7, list(seen)
    assert all(v == 0 for v in seen.values()), f"a ternary a8 kernel spills: {seen}"
