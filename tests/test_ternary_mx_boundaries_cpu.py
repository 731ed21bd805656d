"""Host-side guard of the ternary / MXFP4 boundary tests (no GPU, no launch): the shapes of tests/test_ternary_mx_boundaries_gpu.py
straddle the library's form predicates (bie_ternary_linear_fused_ok, bie_ternary_a8_fused_ok, bie_mxfp4_form, bie_ternary_conv2d_form),
so a retuned bound fails here instead of leaving the GPU test on one side of it; and the draws of the GPU slices in
tests/test_gpu_fuzz.py reach every form of every op of tests/sweeps/fuzz_ternary_mx.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def _lib():
    from bitorch_engine import _hip
    return _hip.lib()


def test_ternary_linear_shapes_straddle_the_decode_bounds():
    import fuzz_ternary_mx as F
    import test_ternary_mx_boundaries_gpu as B
    L = _lib()
    for M, N, K, forms in B.TERN_CASES:
        assert set(F.forms_of("tern", dict(M=M, N=N, K=K))) == forms, (M, N, K)
    for M in (1, 4):  # the last K inside the LDS bound and the first past it are both in the list
        assert L.bie_ternary_linear_fused_ok(M, 40, F.TERN_K_MAX) == 1 and L.bie_ternary_linear_fused_ok(M, 40, F.TERN_K_MAX + 32) == 0
        assert {(M, F.TERN_K_MAX), (M, 131072)} <= {(m, k) for m, _, k, _ in B.TERN_CASES}
    # N = 16384 keeps one 16-column sweep per workgroup, 16385 takes two: cols = ceil(ceil(N / 1024) / 16) * 16
    cols = lambda n: -(-(-(-n // 1024)) // 16) * 16
    assert cols(16384) == 16 and cols(16385) == 32 and {16384, 16385} <= {n for _, n, _, _ in B.TERN_CASES}


def test_ternary_a8_shapes_straddle_the_decode_and_tile_bounds():
    import fuzz_ternary_mx as F
    import test_ternary_mx_boundaries_gpu as B
    L = _lib()
    for M, N, K, forms in B.TA8_CASES:
        assert set(F.forms_of("ta8", dict(M=M, N=N, K=K))) == forms, (M, N, K)
    for R, K in F.TA8_K_MAX.items():
        assert R * K == 64512
        for M in range(R // 2 + 1, R + 1):
            assert L.bie_ternary_a8_fused_ok(M, 33, K) == 1 and L.bie_ternary_a8_fused_ok(M, 33, K + 32) == 0, (M, K)
        assert {(R, K), (R, K + 32)} <= {(m, k) for m, _, k, _ in B.TA8_CASES}
    tiles = lambda m, n: -(-m // 256) * -(-n // 256)
    assert tiles(2048, 5888) == 184 and tiles(2048, 6144) == 192 and tiles(3000, 4100) >= 192 and 3000 % 256 and 4100 % 256


def test_mxfp4_shapes_straddle_the_form_bound():
    import test_ternary_mx_boundaries_gpu as B
    L = _lib()
    for dt in (0, 1):
        for M in range(1, 18):
            assert L.bie_mxfp4_form(M, 5, 160, dt) == (0 if M <= 16 else 1), (M, dt)
    assert {1, 3, 4, 5, 7, 8, 9} <= set(B.MX_NS) and any(n % 8 == 1 and n > 4096 for n in B.MX_NS)


def test_ternary_conv_shapes_take_the_documented_forms_on_either_side():
    import test_ternary_mx_boundaries_gpu as B
    L = _lib()
    for c in B.TCONV_CASES:
        assert L.bie_ternary_conv2d_form(*c[:8], 1) == c[8], c
    forms = {c[:8]: c[8] for c in B.TCONV_CASES}
    assert forms[(1, 128, 2, 64, 64, 3, 1, 1)] == 1 and forms[(1, 128, 2, 65, 64, 3, 1, 1)] == 2      # OW 64 | 65
    assert forms[(1, 64, 2, 128, 64, 3, 1, 1)] == 2 and forms[(1, 64, 2, 129, 64, 3, 1, 1)] == 0      # OW 128 | 129
    assert forms[(1, 128, 112, 7, 64, 3, 1, 1)] == 1 and forms[(1, 128, 157, 5, 64, 3, 1, 1)] == 2    # 784 | 785 pixels
    assert forms[(1, 512, 7, 7, 64, 3, 1, 1)] == 1 and forms[(1, 544, 7, 7, 64, 3, 1, 1)] == 0        # C 512 | 544


@pytest.mark.parametrize("op", ["tern", "tconv", "ta8", "mx"])
def test_the_gpu_slice_seeds_draw_every_form(op):
    import fuzz_ternary_mx as F
    import test_gpu_fuzz
    cases, seed = test_gpu_fuzz.TERNARY_MX_SLICES[op]
    rng = np.random.default_rng(seed)
    seen = {f: 0 for f in F.FORMS[op]}
    for _ in range(cases):
        for f in F.forms_of(op, F.draw(op, rng)):
            seen[f] += 1
    assert all(n > 0 for n in seen.values()), seen
