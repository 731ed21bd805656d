"""Ternary linear layer, the parts that need no GPU: the TWN ternarisation against a numpy restatement, the qweight plane layout on
hand-made vectors, host-side argument validation of every bie_ternary_* entry, the decode-form predicate, and the compiler's resource
report for csrc/ternary.hip (no scratch)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_ternarize(w, tf):
    w = w.astype(np.float32)
    a = np.abs(w)
    delta = (tf * a.mean(axis=1)).astype(np.float32)
    t = np.where(w > delta[:, None], 1, np.where(w < -delta[:, None], -1, 0)).astype(np.int8)
    nz = t != 0
    cnt = nz.sum(axis=1)
    alpha = np.where(cnt > 0, (a * nz).sum(axis=1) / np.maximum(cnt, 1), 0.0).astype(np.float32)
    return t, alpha, delta


def np_pack(t):
    """trits [N, K] -> uint8 [2, N, K/8]: plane 0 non-zero, plane 1 +1, LSB first."""
    m = np.packbits(t != 0, axis=1, bitorder="little")
    p = np.packbits(t > 0, axis=1, bitorder="little")
    return np.stack([m, p])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("tf", [0.7, 0.5, 1.0])
def test_ternarize_matches_numpy(dtype, tf):
    from bitorch_engine.layers.qlinear.ternary import ternarize
    g = torch.Generator().manual_seed(3)
    w = (torch.randn((67, 256), generator=g) * 0.05).to(dtype)
    w[5] = 0  # a row without non-zeros: alpha 0
    w[6, :] = 0.01
    w[6, 7] = -0.3
    t, alpha, delta = ternarize(w, tf)
    rt, ralpha, rdelta = np_ternarize(w.float().numpy(), tf)
    np.testing.assert_allclose(delta.numpy(), rdelta, rtol=1e-5, atol=1e-9)
    wf = w.float().numpy()
    near = np.abs(np.abs(wf) - rdelta[:, None]) <= 1e-4 * rdelta[:, None]
    assert t.dtype == torch.int8
    assert np.array_equal(t.numpy()[~near], rt[~near])
    if not near.any():
        np.testing.assert_allclose(alpha.numpy(), ralpha, rtol=1e-5, atol=1e-9)
    assert alpha[5].item() == 0.0 and (t[5] == 0).all()
    assert t[6, 7].item() == -1


def test_numpy_packer_plane_layout_on_keyed_vectors():
    t = np.zeros((2, 32), np.int8)
    t[0, 0] = 1     # plane 0 bit 0, plane 1 bit 0
    t[0, 9] = -1    # plane 0 byte 1 bit 1 only
    t[0, 31] = 1    # byte 3 bit 7 in both planes
    t[1, 8:16] = -1
    t[1, 3] = 1
    q = np_pack(t)
    assert q.shape == (2, 2, 4) and q.dtype == np.uint8
    assert list(q[0, 0]) == [0x01, 0x02, 0x00, 0x80]
    assert list(q[1, 0]) == [0x01, 0x00, 0x00, 0x80]
    assert list(q[0, 1]) == [0x08, 0xFF, 0x00, 0x00]
    assert list(q[1, 1]) == [0x08, 0x00, 0x00, 0x00]
    assert ((q[1] & ~q[0]) == 0).all()  # plane 1 is a subset of plane 0


def test_argument_validation_of_every_ternary_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    # bie_ternary_pack / unpack / fp4_image: K % 32, N >= 1, NULL pointers
    assert L.bie_ternary_pack(fake, fake, 4, 48, None) == -1
    assert b"bie_ternary_pack" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert L.bie_ternary_pack(fake, fake, 0, 64, None) == -1
    assert L.bie_ternary_pack(None, fake, 4, 64, None) == -1
    assert L.bie_ternary_unpack(fake, fake, 4, 40, None) == -1
    assert L.bie_ternary_unpack(fake, None, 4, 64, None) == -1
    assert L.bie_ternary_fp4_image(fake, fake, 4, 16, None) == -1
    assert L.bie_ternary_fp4_image(None, fake, 4, 64, None) == -1
    assert L.bie_ternary_fp4_image(fake, fake + 4, 4, 64, None) == -1  # image not 16-byte aligned
    # bie_ternary_linear_fused: shape, dtype, y_f32 with scales, range, NULL, alignment
    assert L.bie_ternary_linear_fused(fake, None, fake, None, None, fake, 1, 8, 48, 0, 0, None) == -1
    assert L.bie_ternary_linear_fused(fake, None, fake, None, None, fake, 1, 8, 64, 5, 0, None) == -2
    assert L.bie_ternary_linear_fused(fake, None, fake, fake, None, fake, 1, 8, 64, 0, 1, None) == -1
    assert L.bie_ternary_linear_fused(fake, None, fake, None, None, fake, 4096, 8, 64, 0, 0, None) == -2
    assert L.bie_ternary_linear_fused(None, None, fake, None, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_linear_fused(fake + 2, None, fake, None, None, fake, 1, 8, 64, 0, 0, None) == -1
    assert L.bie_ternary_linear_fused(fake, None, fake + 1, None, None, fake, 1, 8, 64, 0, 0, None) == -1
    # bie_ternary_linear_layer_fp4
    assert L.bie_ternary_linear_layer_fp4(fake, fake, None, None, fake, 64, 8, 48, 0, None) == -1
    assert L.bie_ternary_linear_layer_fp4(fake, fake, None, None, fake, 0, 8, 64, 0, None) == -1
    assert L.bie_ternary_linear_layer_fp4(None, fake, None, None, fake, 64, 8, 64, 0, None) == -1
    assert L.bie_ternary_linear_layer_fp4(fake, fake, None, None, fake, 64, 8, 64, 3, None) == -2
    assert L.bie_ternary_linear_layer_fp4(fake + 8, fake, None, None, fake, 64, 8, 64, 0, None) == -1
    assert L.bie_ternary_linear_layer_fp4(fake, fake, None, None, fake, 64, 8, 1 << 24, 0, None) == -1


def test_fused_predicate_on_a_grid():
    from bitorch_engine import _hip
    L = _hip.lib()
    for K in (32, 4096, 11008, 16384):
        for N in (1, 33, 4096, 11008):
            for M in (0, 1, 2, 3, 4):
                assert L.bie_ternary_linear_fused_ok(M, N, K) == (1 if M >= 1 else 0), (M, N, K)
            for M in (5, 8, 16, 17, 64, 4096):
                assert L.bie_ternary_linear_fused_ok(M, N, K) == 0, (M, N, K)
    assert L.bie_ternary_linear_fused_ok(1, 8, 48) == 0          # K % 32
    assert L.bie_ternary_linear_fused_ok(1, 0, 64) == 0          # N
    assert L.bie_ternary_linear_fused_ok(4, 8, 131040) == 1      # 4 rows of x bits fill 64 KiB of LDS
    assert L.bie_ternary_linear_fused_ok(4, 8, 131072) == 0


def test_ternary_kernels_do_not_spill():
    """Every kernel of ternary.hip, and every instance of the FP4 GEMM that serves the ternary layer epilogue (the per-column-scale
    instances in binary_fp4.hip), compiles with ScratchSize 0."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    seen = {}
    for src, want in (("ternary.hip", lambda n: True), ("binary_fp4.hip", lambda n: "xnor_fp4_gemm_kernel" in n and n.endswith("Lb1EEEvPKhS2_PviiiiiifPKvS5_i"))):
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
                            "--cuda-device-only", "-c", os.path.join(ROOT, "bitorch-engine_amd", "csrc", src), "-o", os.devnull],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        name = None
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name and want(name):
                seen[name] = int(m.group(1))
    assert sum("ternary_fused_kernel" in n for n in seen) == 3, list(seen)
    assert sum("xnor_fp4_gemm_kernel" in n for n in seen) == 9, list(seen)
    assert all(v == 0 for v in seen.values()), f"a ternary kernel spills: {seen}"
