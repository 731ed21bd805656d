"""Ternary conv2d, the parts that need no GPU: the qweight plane layout for [OC, C, k, k] trits in OIHW order (numpy restatement), host-side
argument validation of every new C entry, the form chosen by bie_ternary_conv2d_form on a grid, and the compiler's resource report for
csrc/binary_conv_fused.hip (no scratch in any instance; ternary instances of both one-launch kernels exist)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_pack_conv(t):
    """trits [OC, C, k, k] -> uint8 [2, OC, C*k*k/8]: the linear's planes over the OIHW flatten order."""
    r = t.reshape(t.shape[0], -1)
    return np.stack([np.packbits(r != 0, axis=1, bitorder="little"), np.packbits(r > 0, axis=1, bitorder="little")])


def test_numpy_packer_plane_layout_for_oihw_trits():
    OC, C, k = 2, 32, 3
    t = np.zeros((OC, C, k, k), np.int8)
    t[0, 0, 0, 0] = 1      # k-index 0
    t[0, 0, 1, 2] = -1     # c*9 + kh*3 + kw = 5
    t[0, 1, 0, 0] = 1      # 9: byte 1 bit 1
    t[0, 31, 2, 2] = -1    # 31*9 + 8 = 287: byte 35 bit 7
    t[1, 3, 2, 1] = 1      # 27 + 7 = 34: byte 4 bit 2
    q = np_pack_conv(t)
    assert q.shape == (2, OC, C * k * k // 8) and q.dtype == np.uint8
    m, p = q[0], q[1]
    assert m[0, 0] == 0b00100001 and p[0, 0] == 0b00000001
    assert m[0, 1] == 0b00000010 and p[0, 1] == 0b00000010
    assert m[0, 35] == 0x80 and p[0, 35] == 0
    assert m[1, 4] == 0b100 and p[1, 4] == 0b100
    assert int(m.astype(np.int64).sum()) == 0b00100001 + 2 + 0x80 + 4
    assert ((p & ~m) == 0).all()
    # the flatten order is torch's reshape of OIHW: element (oc, c, kh, kw) -> bit c*k*k + kh*k + kw of row oc
    g = np.random.default_rng(0)
    t = g.integers(-1, 2, (5, 64, 3, 3)).astype(np.int8)
    q = np_pack_conv(t)
    bits = np.unpackbits(q, axis=2, bitorder="little")
    for (oc, c, kh, kw) in ((0, 0, 0, 0), (4, 63, 2, 2), (2, 17, 1, 0), (3, 40, 0, 2)):
        kidx = c * 9 + kh * 3 + kw
        assert bits[0, oc, kidx] == (t[oc, c, kh, kw] != 0) and bits[1, oc, kidx] == (t[oc, c, kh, kw] > 0)


def test_argument_validation_of_every_ternary_conv_entry_happens_on_the_host():
    from bitorch_engine import _hip
    L = _hip.lib()
    fake = 1 << 20  # never dereferenced: every call below fails validation first
    fused, mfma = L.bie_ternary_conv2d_forward_fused, L.bie_ternary_conv2d_forward_mfma
    geo = (2, 512, 7, 7, 512, 3, 1, 1, 1)  # a geometry both forms run
    # (x, wlanes_mask, wlanes_pos, scale_a, alpha, y, *geometry, dtype, y_f32, stream)
    assert fused(None, fake, fake, None, None, fake, *geo, 0, 0, None) == -1
    assert fused(fake, None, fake, None, None, fake, *geo, 0, 0, None) == -1
    assert fused(fake, fake, None, None, None, fake, *geo, 0, 0, None) == -1
    assert fused(fake, fake, fake, None, None, None, *geo, 0, 0, None) == -1
    assert fused(fake, fake, fake, None, None, fake, 0, 512, 7, 7, 512, 3, 1, 1, 1, 0, 0, None) == -1       # B = 0
    assert fused(fake, fake, fake, None, None, fake, 2, 512, 7, 7, 512, 3, 0, 1, 1, 0, 0, None) == -1       # stride 0
    assert fused(fake, fake, fake, None, None, fake, 2, 512, 7, 7, 512, 3, 1, -1, 1, 0, 0, None) == -1      # pad < 0
    assert fused(fake, fake, fake, None, None, fake, 2, 512, 2, 2, 512, 5, 1, 0, 1, 0, 0, None) == -1       # empty output
    assert fused(fake, fake, fake, None, None, fake, 2, 48, 7, 7, 64, 3, 1, 1, 1, 0, 0, None) == -1         # C % 32
    assert fused(fake, fake, fake, None, None, fake, *geo, 3, 0, None) == -2                                 # dtype
    assert b"dtype" in L.bie_last_error()
    assert fused(fake, fake, fake, fake, None, fake, *geo, 0, 1, None) == -1                                 # y_f32 with a scale
    assert fused(fake, fake + 4, fake, None, None, fake, *geo, 0, 0, None) == -1                             # misaligned lane image
    assert fused(fake, fake, fake + 8, None, None, fake, *geo, 0, 0, None) == -1
    assert b"16-byte" in L.bie_last_error()
    assert fused(fake, fake, fake, None, None, fake, 1, 1 << 19, 1, 1, 8, 7, 1, 3, 1, 0, 0, None) == -2    # C*k*k >= 2^24
    assert b"2^24" in L.bie_last_error()
    assert fused(fake, fake, fake, None, None, fake, 1, 512, 7, 7, 512, 5, 1, 2, 1, 0, 0, None) == -2       # k = 5: outside the form
    assert b"outside the one-launch VALU form" in L.bie_last_error()
    assert fused(fake, fake, fake, None, None, fake, 1, 64, 56, 56, 64, 3, 1, 1, 1, 0, 0, None) == -2      # C = 64: not this form
    # (x, wimage, scale_a, alpha, y, *geometry, dtype, y_f32, stream)
    assert mfma(None, fake, None, None, fake, *geo, 0, 0, None) == -1
    assert mfma(fake, None, None, None, fake, *geo, 0, 0, None) == -1
    assert mfma(fake, fake, None, None, None, *geo, 0, 0, None) == -1
    assert mfma(fake, fake, None, None, fake, 2, 512, 7, 7, 512, 3, 1, 1, 0, 0, 0, None) == -1              # dilation 0
    assert mfma(fake, fake, None, None, fake, 2, 96, 7, 7, 64, 3, 1, 1, 1, 0, 0, None) == -2                # C = 96: not this form
    assert mfma(fake, fake, None, None, fake, *geo, -1, 0, None) == -2
    assert mfma(fake, fake, None, fake, fake, *geo, 0, 1, None) == -1
    assert mfma(fake, fake + 2, None, None, fake, *geo, 0, 0, None) == -1
    assert mfma(fake, fake, None, None, fake, 1, 1 << 19, 1, 1, 8, 7, 1, 3, 1, 0, 0, None) == -2
    assert mfma(fake, fake, None, None, fake, 1, 128, 8, 300, 8, 3, 1, 1, 1, 0, 0, None) == -2            # OW > 128
    assert b"outside the one-launch matrix-pipe form" in L.bie_last_error()
    assert mfma(fake, fake, None, None, fake, 1, 1024, 7, 7, 64, 3, 1, 1, 1, 0, 0, None) == -2             # C = 1024
    assert mfma(fake, fake, None, None, fake, 1 << 14, 512, 512, 1, 8, 1, 1, 0, 1, 0, 0, None) == -2       # beyond 2^31 elements


RESNET = [(64, 56, 64, 3, 1, 1), (128, 28, 128, 3, 1, 1), (256, 14, 256, 3, 1, 1), (512, 7, 512, 3, 1, 1),
          (64, 56, 128, 3, 2, 1), (128, 28, 256, 3, 2, 1), (256, 14, 512, 3, 2, 1),
          (64, 56, 128, 1, 2, 0), (128, 28, 256, 1, 2, 0), (256, 14, 512, 1, 2, 0)]


def test_form_on_a_grid():
    from bitorch_engine import _hip
    form = _hip.lib().bie_ternary_conv2d_form
    for (C, H, OC, k, s, p) in RESNET:
        for B in (1, 2, 8, 32, 128):
            f = form(B, C, H, H, OC, k, s, p, 1)
            assert f in (1, 2), (B, C, H, OC, k, s, p)
            if C == 64:
                assert f == 2  # no four K quarters of whole channel words: the matrix pipe only
    assert form(128, 512, 7, 7, 512, 3, 1, 1, 1) == 2   # 6272 output pixels
    assert form(1, 512, 7, 7, 512, 3, 1, 1, 1) == 1     # 49
    assert form(2, 512, 5, 60, 72, 3, 1, 1, 1) == 1     # beyond the matrix-pipe form's LDS image: the VALU form at any size
    for args in ((1, 512, 7, 7, 512, 5, 1, 2, 1),       # k = 5
                 (1, 512, 7, 7, 512, 3, 1, 2, 2),       # dilation 2
                 (1, 32, 8, 8, 64, 3, 1, 1, 1),         # C = 32
                 (1, 96, 8, 8, 64, 3, 1, 1, 1),         # C = 96
                 (1, 1024, 7, 7, 64, 3, 1, 1, 1),       # C = 1024
                 (1, 128, 8, 300, 8, 3, 1, 1, 1),       # OW > 128
                 (1, 64, 4, 140, 16, 3, 1, 1, 1),
                 (1, 48, 8, 8, 64, 3, 1, 1, 1),         # C % 32: no form at all (the layer refuses it)
                 (0, 512, 7, 7, 512, 3, 1, 1, 1)):
        assert form(*args) == 0, args


def test_conv_kernels_do_not_spill_and_ternary_instances_exist():
    """Every kernel of binary_conv_fused.hip compiles with ScratchSize 0, and both one-launch kernels have ternary (TERN) instances."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", os.path.join(ROOT, "bitorch-engine_amd", "csrc", "binary_conv_fused.hip"), "-o", os.devnull],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    # the template flag is the last template argument: Lb1E = ternary, Lb0E = binary
    tern_fused = [n for n in seen if "xnor_conv_fused_kernel" in n and "Lb1EE" in n]
    tern_mfma = [n for n in seen if "xnor_conv_mfma_kernel" in n and "Lb1EE" in n]
    bin_fused = [n for n in seen if "xnor_conv_fused_kernel" in n and "Lb0EE" in n]
    bin_mfma = [n for n in seen if "xnor_conv_mfma_kernel" in n and "Lb0EE" in n]
    assert len(tern_fused) >= 1 and len(tern_mfma) >= 1, list(seen)
    assert len(bin_fused) == 24 and len(bin_mfma) == 16, (len(bin_fused), len(bin_mfma))
    assert all(v == 0 for v in seen.values()), f"a conv kernel spills: {seen}"


def test_host_tensors_are_refused_before_any_launch():
    """Every Python entry of the ternary conv checks that x, qweight and the weight images live on the GPU before it builds an image or
    calls a C entry: host tensors raise RuntimeError here, where there is no GPU at all."""
    import torch
    from bitorch_engine.extensions import ternary_conv2d_cuda as tc
    x = torch.zeros((1, 128, 7, 7))
    q = torch.zeros((2, 16, 128 * 9 // 8), dtype=torch.uint8)
    calls = [lambda: tc.forward(x, q, 3, 1, 1, 1), lambda: tc.layer_forward(x, q, None, None, 3, 1, 1, 1),
             lambda: tc.conv_fused(x, q, 3, 1, 1, 1), lambda: tc.conv_mfma(x, q, 3, 1, 1, 1), lambda: tc.conv_general(x, q, 3, 1, 1, 1),
             lambda: tc.weight_taps(q, 128, 3), lambda: tc.weight_lanes(q, 128, 3), lambda: tc.weight_fp4_image(q, 128, 3),
             lambda: tc.w_unpack(q, 128, 3)]
    for call in calls:
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
