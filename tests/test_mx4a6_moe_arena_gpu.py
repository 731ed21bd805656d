"""bie_mx4a6_moe_forward and bie_mx4a6_moe_gemm called through _hip.lib() with raw addresses inside the arena of tests/abi_arena.py (its
public parts, imported): each operand at exactly the alignment the header states (x, qweight, xq6, y and workspace 16 bytes, idx 4,
bias 2, scales / e_col / xs / row_flag odd addresses), poisoned guards around the inputs (idx between valid expert numbers), a workspace
of exactly bie_mx4a6_moe_workspace_bytes (the routing region alone for the gemm entry) pre-filled with 0xFF and with 0x00, both forms.
A case passes when the call returns 0, no byte outside its outputs changed, the outputs have the bits of the same call on
allocator-aligned copies, and that result meets mxfp4_a6_ref.tolerance against the float64 restatement with +0 rows in the skipped
slots.  The refusal test moves every pointer capi.hip validates to half its alignment: BIE_ERR_INVALID_ARG, nothing launched, nothing
changed.

The table of abi_arena.py lists the bie_ternary_* / bie_mxfp* entries; these two carry another prefix and get the same treatment here,
on the grid of abi_arena.experts_grid."""
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

ENTRIES = ("bie_mx4a6_moe_forward", "bie_mx4a6_moe_gemm")
ONE_K = 16384  # the header's bound of the one-launch decode form, which reads no workspace


def ref():
    return A._load("mxfp4_moe_a6_ref")


def grid(entry):
    """(entry, T, S, E, N, K, dt, bias, xpp, form): abi_arena.experts_grid's cases; the last one has a bias and the prefill form."""
    return [(entry, T, 2, 3, N, K, dt, bias, xpp, form) for dt in A.DTS for T in (1, 5, 70) for xpp in (0, 1) for form in (0, 1)
            for bias, (N, K) in ((False, (17, 32)), (True, (130, 160)))]


def moe_case(entry, T, S, E, N, K, dt, bias, xpp, form):
    gemm = entry.endswith("_gemm")
    P, R = T * S, T * S if xpp else T
    g = A.gen(T, S, E, N, K, A.DT_CODE[dt], bias, xpp, form, gemm, 46)
    q, s = A.rand_w("fp4", E * N, K, g)
    q, s = q.reshape(E, N, -1), s.reshape(E, N, -1)
    x = (torch.randn((R, K), generator=g) * 0.5).to(dt)
    b = torch.randn((E, N), generator=g).to(dt) if bias else None
    idx = A.routing(T, S, E, g)
    xq, xs, flag = ref().quantize_rows(x)
    if gemm:
        ops = [In("xq6", xq, 16, K // 32 * 24), In("xs", xs, 1, K // 32), In("row_flag", flag, 1, 1)]
    else:
        ops = [In("x", x, 16, K * A.es(dt))]
    ops += [In("idx", idx, 4, 4 * S, poison=("idx", E - 1)), In("qweight", q, 16, K // 2), In("scales", s, 1, K // 32),
            In("e_col", s.amax(dim=2), 1, 1)]
    if bias:
        ops.append(In("bias", b, 2, A.es(dt)))
    ops.append(Out("y", P * N * A.es(dt), 16, N * A.es(dt)))
    L = A.lib()
    if gemm:  # the routing region alone, and only for the prefill form
        ws = ("bie_mxfp4_moe_workspace_bytes", (P, E)) if form == 1 else None
    else:
        ws = ("bie_mx4a6_moe_workspace_bytes", (T, S, E, K, xpp, form))
    if ws:
        ops.append(Ws(getattr(L, ws[0])(*ws[1])))
        # the header: the one-launch decode form does not read the workspace, and only a workspace that is read is validated
        ops[-1].validated = not (not gemm and form == 0 and K <= ONE_K)
    tail = (T, S, E, N, K, xpp, A.DT_CODE[dt], form)
    if gemm:
        argv = lambda a: (a("xq6"), a("xs"), a("row_flag"), a("idx"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), a("workspace")) + tail  # noqa: E731
    else:
        argv = lambda a: (a("x"), a("idx"), a("qweight"), a("scales"), a("e_col"), a("bias"), a("y"), a("workspace")) + tail  # noqa: E731

    def the_gate(outs):
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        yref, a = ref().experts_from_codes(xq, xs, flag, idx, ref().dequant(q, s).to(dev), b)
        yref, a = yref.reshape(P, N), a.reshape(P, N)
        y = A.bt(outs["y"], dt, (P, N))
        skipped = idx.reshape(-1) < 0
        assert (y[skipped].view(torch.int16) == 0).all(), f"{entry}: a skipped slot's row is not +0"
        tol = ref().tolerance(yref, a, K, dt)
        err = (y.to(dev).double() - yref).abs()
        assert torch.isfinite(y).all(), f"{entry}: non-finite output (an element never written reads as NaN)"
        assert (err <= tol).all(), f"{entry}: max err {err.max().item()} (tol there {tol.flatten()[err.argmax()].item()})"

    tag = f"T{T} S{S} E{E} N{N} K{K} dt{A.DT_CODE[dt]} bias{int(bias)} xpp{xpp} form{form}"
    return Case(entry, tag, ops, argv, the_gate, ws)


CHUNK = 24  # cases per test: each stays within a few seconds


@pytest.mark.parametrize("entry,first", [(e, i) for e in ENTRIES for i in range(0, len(grid(e)), CHUNK)])
def test_entry_in_the_arena(entry, first):
    be = TorchBackend()
    t0 = time.time()
    g = grid(entry)
    forms = set()
    for args in g[first:first + CHUNK]:
        check(moe_case(*args), be)
        forms.add(args[-1])
    assert forms == {0, 1}
    print(f"{entry}: cases {first} .. {min(first + CHUNK, len(g)) - 1} of {len(g)} in {time.time() - t0:.2f} s")


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_pointers_are_refused_before_any_launch(entry):
    """The first and the last case of the entry's grid.  The first (no bias, the decode form): x / xq6, idx, qweight and y; the forward's
    workspace is not read by the one-launch form and so not validated, and the gemm takes none.  The last (a bias, the prefill form):
    those four, the bias and the workspace."""
    be = TorchBackend()
    g = grid(entry)
    n = sum(refusals(moe_case(*args), be) for args in (g[0], g[-1]))
    print(f"{entry}: {n} misaligned pointers refused")
    assert n == 4 + 6
