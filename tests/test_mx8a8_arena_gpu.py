"""bie_mx8a8_linear_forward and bie_mx8a8_gemm called through _hip.lib() with raw addresses inside the arena of tests/abi_arena.py (its
public parts, imported): each operand at exactly the alignment the header states (x, qweight, xq, y and workspace 16 bytes, bias 2,
scales / e_col / xs / row_flag odd addresses), poisoned guards around the inputs, a workspace of exactly bie_mx8a8_workspace_bytes
pre-filled with 0xFF and with 0x00.  A case passes when the call returns 0, no byte outside its outputs changed, the outputs have the
bits of the same call on allocator-aligned copies, and that result meets mxfp8_a8_ref.tolerance against the float64 restatement.  The
refusal test moves every pointer capi.hip validates to half its alignment: BIE_ERR_INVALID_ARG, nothing launched, nothing changed.

The table of abi_arena.py lists the bie_ternary_* / bie_mxfp* entries; these two carry another prefix and get the same treatment here.
tests/test_mxfp8_a8_cpu.py checks the layout of every case below without a GPU."""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import abi_arena as A  # noqa: E402
from abi_arena import Case, In, Out, TorchBackend, Ws, check, refusals  # noqa: E402

ENTRIES = ("bie_mx8a8_linear_forward", "bie_mx8a8_gemm")
MS, KNS, DECODE_ROWS = (1, 17, 64, 65, 130), ((32, 1), (160, 17), (1024, 130)), 64


def ref():
    return A._load("mxfp8_a8_ref")


def grid(entry):
    """(entry, M, N, K, dt, bias, form): both forms where M <= 64, the prefill form beyond; the last case has a bias and the prefill form."""
    return [(entry, M, N, K, dt, bias, form) for dt in A.DTS for bias in (False, True) for K, N in KNS for M in MS
            for form in ((0, 1) if M <= DECODE_ROWS else (1,))]


def mx8a8_case(entry, M, N, K, dt, bias, form):
    gemm = entry.endswith("_gemm")
    g = A.gen(M, N, K, A.DT_CODE[dt], bias, form, gemm, 88)
    q, s = ref().rand_w(N, K, g)
    x = (torch.randn((M, K), generator=g) * 0.5).to(dt)
    b = torch.randn(N, generator=g).to(dt) if bias else None
    xq, xs, flag = ref().quantize_act(x)
    if gemm:
        ops = [In("xq", xq, 16, K), In("xs", xs, 1, K // 32), In("row_flag", flag, 1, 1)]
    else:
        ops = [In("x", x, 16, K * A.es(dt))]
    ops += [In("qweight", q, 16, K), In("scales", s, 1, K // 32), In("e_col", s.amax(dim=1), 1, 1)]
    if bias:
        ops.append(In("bias", b, 2, A.es(dt)))
    ops.append(Out("y", M * N * A.es(dt), 16, N * A.es(dt)))
    ws = None
    if not gemm:
        ws = ("bie_mx8a8_workspace_bytes", (M, N, K, form))
        ops.append(Ws(getattr(A.lib(), ws[0])(*ws[1])))
    tail = (M, N, K, A.DT_CODE[dt], form)
    if gemm:
        argv = lambda a: (a("xq"), a("xs"), a("row_flag"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), None) + tail  # noqa: E731
    else:
        argv = lambda a: (a("x"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), a("workspace")) + tail  # noqa: E731

    def the_gate(outs):
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        yref, a = ref().reference(xq, xs, flag, q, s, b, dev)
        y = A.bt(outs["y"], dt, (M, N))
        tol = ref().tolerance(yref, a, K, dt)
        err = (y.to(dev).double() - yref).abs()
        assert torch.isfinite(y).all(), f"{entry}: non-finite output (an element never written reads as NaN)"
        assert (err <= tol).all(), f"{entry}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"

    return Case(entry, f"M{M} N{N} K{K} {'bf16' if dt == torch.bfloat16 else 'f16'} bias{int(bias)} form{form}", ops, argv, the_gate, ws)


CHUNK = 48  # cases per test: each stays within a few seconds


@pytest.mark.parametrize("entry,first", [(e, i) for e in ENTRIES for i in range(0, len(grid(e)), CHUNK)])
def test_entry_in_the_arena(entry, first):
    be = TorchBackend()
    t0 = time.time()
    g = grid(entry)
    for args in g[first:first + CHUNK]:
        check(mx8a8_case(*args), be)
    print(f"{entry}: cases {first} .. {min(first + CHUNK, len(g)) - 1} of {len(g)} in {time.time() - t0:.2f} s")


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_pointers_are_refused_before_any_launch(entry):
    """The first and the last case of the entry's grid (the last one has a bias and the prefill form): every validated pointer at half
    its alignment.  x / xq, qweight, y (and the workspace of the forward entry) without a bias, the bias as well with one."""
    be = TorchBackend()
    g = grid(entry)
    n = sum(refusals(mx8a8_case(*args), be) for args in (g[0], g[-1]))
    print(f"{entry}: {n} misaligned pointers refused")
    assert n == (9 if entry.endswith("forward") else 7)
