"""MXFP8 weight-only expert layers (W8A16), the parts that need no GPU: bie_mx8_moe_forward's refusals before any launch, the plan with
the knob unset, and the layers' constructor and checkpoint refusals."""
import os

import pytest
import torch

FAKE = 1 << 20  # never dereferenced: every call below ends in the host-side checks
DECODE_PAIRS = 1024


def test_forward_refuses_on_the_host_before_any_launch():
    from bitorch_engine import _hip
    L = _hip.lib()
    assert _hip.SIGNATURES["bie_mx8_moe_forward"] == _hip.SIGNATURES["bie_mxfp6_moe_forward"] and L.bie_version() == 300

    def call(x=FAKE, idx=FAKE, q=FAKE, s=FAKE, e=FAKE, y=FAKE, ws=FAKE, T=4, S=2, E=8, K=64, form=-1):
        return L.bie_mx8_moe_forward(x, idx, q, s, e, None, y, ws, T, S, E, 8, K, 0, 0, form, None)

    assert call(K=48) == -1 and b"bie_mx8_moe_forward" in L.bie_last_error() and b"K=48" in L.bie_last_error()  # K % 32
    assert call(K=0) == -1 and call(K=(1 << 20) + 32) == -1 and call(E=0) == -1 and call(E=1025) == -1 and b"E=1025" in L.bie_last_error()
    assert call(T=DECODE_PAIRS + 1, S=1, form=0) == -2                     # form 0 beyond the decode bound
    assert b"bie_mx8_moe_forward" in L.bie_last_error() and f"P={DECODE_PAIRS + 1}".encode() in L.bie_last_error()
    assert call(T=DECODE_PAIRS, S=1, form=0, x=None) == -1                 # P = 1024 passes the form check
    for form, T in ((0, 4), (1, 4), (-1, 4), (-1, 4096)):
        for k in ("x", "idx", "q", "s", "y"):                              # each NULL tensor
            assert call(**{k: None}, form=form, T=T) == -1 and b"NULL tensor pointer" in L.bie_last_error(), (k, form, T)
    assert call(ws=None, form=1) == -1 and call(e=None, form=1) == -1 and b"e_col" in L.bie_last_error()  # form 1 needs the workspace and e_col
    for k in ("x", "q"):                                                   # misaligned x, qweight
        assert call(**{k: FAKE + 8}) == -1 and b"aligned" in L.bie_last_error(), k


def test_form_with_the_knob_unset_is_monotone_and_never_a_refused_decode():
    from bitorch_engine import _hip
    from bitorch_engine.extensions import mxfp4_experts_cuda as w4, mxfp8_experts_cuda as w8
    from bitorch_engine.utils.safe_import import import_extension
    assert "BIE_MXFP8_MOE_FORM" not in os.environ and "bie_mx8_moe_form" in _hip._HOST_ONLY and "bie_mx8_moe_forward" not in _hip._HOST_ONLY
    assert import_extension("mxfp8_experts_cuda") is w8 and w8.col_exp is w4.col_exp and not hasattr(w8, "grad_input") and not hasattr(w8, "blk_exp")
    L = _hip.lib()
    for E in (1, 2, 32, 128, 1024):
        for N, K in ((5760, 2880), (1, 32)):
            for dt in (0, 1):
                fs = [L.bie_mx8_moe_form(P, E, N, K, dt) for P in list(range(1, 2049)) + [1 << 22]]
                assert set(fs) == {0, 1} and fs == sorted(fs) and fs[0] == 0 and all(f == 1 for f in fs[DECODE_PAIRS:]), (E, N, K)


def test_constructor_and_state_dict_refusals():
    from bitorch_engine.layers.qlinear.nbit.cuda import MXFP4ExpertsLinearCuda, MXFP6ExpertsLinearCuda, MXFP8A16MoECuda, MXFP8ExpertsLinearCuda
    for E, K, N in ((3, 48, 8), (3, 0, 8), (3, 64, 0), (0, 64, 8), (1025, 64, 8), (3, (1 << 20) + 32, 1)):
        with pytest.raises(ValueError, match="mxfp8 experts need"):
            MXFP8ExpertsLinearCuda(E, K, N)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        MXFP8ExpertsLinearCuda(3, 64, 8, dtype=torch.float32)
    with pytest.raises(TypeError):  # no MXFP8 gradient kernel: the class takes no grad_input
        MXFP8ExpertsLinearCuda(3, 64, 8, grad_input="kernel")
    layer = MXFP8ExpertsLinearCuda(3, 64, 8, bias=True)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {"weight": (3, 8, 64), "bias": (3, 8), "qweight": (3, 8, 64), "scales": (3, 8, 2)}
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    for other, what in ((MXFP4ExpertsLinearCuda, "MXFP4 weight"), (MXFP6ExpertsLinearCuda, "MXFP6 weight")):
        with pytest.raises(RuntimeError, match=what):
            layer.load_state_dict(other(3, 64, 8, bias=True).state_dict())
    assert all(torch.equal(before[k], v) for k, v in layer.state_dict().items())
    q, z = torch.zeros((3, 8, 64), dtype=torch.uint8), torch.zeros((3, 8, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="do not match an MXFP8 weight"):
        layer.set_mx_weight(q[..., :48], z)
    q[2, 3, 5] = 0x7F
    with pytest.raises(ValueError, match=r"blocks\[2, 3, 5\] = 0x7F is an E4M3 NaN code"):
        layer.set_mx_weight(q, z)
    moe = MXFP8A16MoECuda(64, 32, 4, 2)
    assert type(moe.gate_up) is MXFP8ExpertsLinearCuda and moe.gate_up.qweight.shape == (4, 64, 64) and moe.down.qweight.shape == (4, 64, 32)
    with pytest.raises(ValueError, match="mxfp8 moe needs"):
        MXFP8A16MoECuda(64, 32, 4, 5)
    with pytest.raises(TypeError, match="MXFP8"):
        moe.load_gpt_oss_experts(None, None, None, None, None, None)
