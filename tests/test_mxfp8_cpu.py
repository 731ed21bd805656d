"""MXFP8 weight-only linear layer (W8A16), the parts that need no GPU: the layer's constructor and checkpoint refusals, the plan with the
knob unset, and bie_mx8_linear_forward's refusals before any launch."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FAKE = 1 << 20  # never dereferenced: every call below ends in the host-side checks


def decode_bound():
    """fuzz_mxfp6.decode_bound's loop on bie_mx8_linear_forward: form 0 is refused beyond it, before the NULL x is found."""
    from bitorch_engine import _hip
    L = _hip.lib()
    b = 0
    while L.bie_mx8_linear_forward(None, FAKE, FAKE, FAKE, None, FAKE, b + 1, 8, 64, 0, 0, None) == -1:
        b += 1
        assert b < 4096
    return b


def test_constructor_refusals_and_state_dict_messages():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4LinearCuda, MXFP6LinearCuda, MXFP8A8LinearCuda, MXFP8LinearCuda, MXFP8LinearForward  # noqa: F401
    for K, N in ((48, 8), (0, 8), (64, 0), (16, 8), ((1 << 20) + 32, 1)):
        with pytest.raises(ValueError):
            MXFP8LinearCuda(K, N)
    with pytest.raises(ValueError):
        MXFP8LinearCuda(64, 8, dtype=torch.float32)
    with pytest.raises(TypeError):  # no MXFP8 gradient kernel: the class takes no grad_input
        MXFP8LinearCuda(64, 8, grad_input="kernel")
    layer = MXFP8LinearCuda(64, 8, bias=True)
    mine, theirs = layer.state_dict(), MXFP8A8LinearCuda(64, 8, bias=True).state_dict()
    assert list(mine) == list(theirs) and all(mine[k].shape == theirs[k].shape and mine[k].dtype == theirs[k].dtype for k in mine)
    before = {k: v.clone() for k, v in mine.items()}
    for other, what in ((MXFP4LinearCuda, "MXFP4 weight"), (MXFP6LinearCuda, "MXFP6 weight")):
        with pytest.raises(RuntimeError, match=what):
            layer.load_state_dict(other(64, 8, bias=True).state_dict())
    assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())
    z = torch.zeros((8, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="do not match an MXFP8 weight"):
        layer.set_mx_weight(torch.zeros((8, 48), dtype=torch.uint8), z)
    q = torch.zeros((8, 64), dtype=torch.uint8)
    q[3, 5] = 0xFF
    with pytest.raises(ValueError, match=r"blocks\[3, 5\] = 0xFF is an E4M3 NaN code"):
        layer.set_mx_weight(q, z)


def test_form_with_the_knob_unset():
    from bitorch_engine import _hip
    from bitorch_engine.extensions import mxfp8_a8_linear_cuda as w8a8, mxfp4_linear_cuda as w4, mxfp8_linear_cuda as w8
    assert "BIE_MXFP8_FORM" not in os.environ and "bie_mx8_form" in _hip._HOST_ONLY
    assert w8.quantize is w8a8.quantize and w8.dequant is w8a8.dequant and w8.col_exp is w4.col_exp
    L = _hip.lib()
    b = decode_bound()
    assert b >= 1
    for K, N in ((4096, 4096), (2880, 5760), (32, 1), (1 << 20, 3)):
        for dt in (0, 1):
            fs = [L.bie_mx8_form(M, N, K, dt) for M in list(range(1, 1025)) + [1 << 20]]
            assert set(fs) == {0, 1} and fs == sorted(fs) and all(f == 1 for f in fs[b:]), (K, N)  # never the decode form where it is refused


def test_forward_refuses_on_the_host_before_any_launch():
    from bitorch_engine import _hip
    L = _hip.lib()
    b = decode_bound()
    F = L.bie_mx8_linear_forward
    ok = [FAKE, FAKE, FAKE, FAKE, None, FAKE]  # x, qweight, scales, e_col, bias, y
    assert F(*ok, 1, 8, 48, 0, -1, None) == -1      # K % 32
    assert b"bie_mx8_linear_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()
    assert F(*ok, 1, 8, 0, 0, -1, None) == -1       # the K bounds
    assert F(*ok, 1, 8, (1 << 20) + 32, 0, -1, None) == -1
    assert F(*ok, b + 1, 8, 64, 0, 0, None) == -2   # form 0 beyond decode_rows
    assert f"M={b + 1}".encode() in L.bie_last_error()
    for i in (0, 1, 2, 5):                           # a NULL x, qweight, scales, y
        a = list(ok)
        a[i] = None
        assert F(*a, 1, 8, 64, 0, -1, None) == -1 and b"NULL tensor pointer" in L.bie_last_error(), i
    a = list(ok)
    a[3] = None                                      # e_col: the prefill form needs it
    assert F(*a, 1, 8, 64, 0, 1, None) == -1 and b"e_col" in L.bie_last_error()
    for i in (0, 1):                                 # x and qweight 16-byte aligned
        a = list(ok)
        a[i] = FAKE + 8
        assert F(*a, 1, 8, 64, 0, -1, None) == -1 and b"aligned" in L.bie_last_error(), i
