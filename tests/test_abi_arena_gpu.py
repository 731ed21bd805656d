"""Every launching ternary / MX entry of include/bie_hip.h called through _hip.lib() with raw addresses inside the arena of
tests/abi_arena.py: each operand at exactly the alignment the header states (x, qweight, xq, gx and workspaces 16 bytes, y and bias of the
weight-only and expert entries 2, ternary qweight 4, scales / e_col / row_flag / xs odd addresses), poisoned guards around the inputs, a
workspace of exactly bie_*_workspace_bytes pre-filled with 0xFF and with 0x00.  A case passes when the call returns 0, no byte outside its
outputs changed, the outputs have the bits of the same call on allocator-aligned copies, and that result meets the operator's own gate
against its float64 restatement.  The refusal tests move every pointer capi.hip validates to half its alignment: BIE_ERR_INVALID_ARG,
nothing launched, nothing changed.  tests/test_abi_contract_cpu.py checks the table and the layouts without a GPU."""
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import abi_arena as A  # noqa: E402

CHUNK = 64  # cases per test: each stays within a few seconds


def chunks():
    out = []
    for entry, (_, grid) in sorted(A.entries().items()):
        out += [(entry, i) for i in range(0, len(grid), CHUNK)]
    return out


@pytest.mark.parametrize("entry,first", chunks())
def test_entry_in_the_arena(entry, first):
    build, grid = A.entries()[entry]
    be = A.TorchBackend()
    t0 = time.time()
    for args in grid[first:first + CHUNK]:
        A.check(build(*args), be)
    print(f"{entry}: cases {first} .. {min(first + CHUNK, len(grid)) - 1} of {len(grid)} in {time.time() - t0:.2f} s")


@pytest.mark.parametrize("entry", sorted(A.entries()))
def test_misaligned_pointers_are_refused_before_any_launch(entry):
    """The first and the last case of the entry's grid (the last one has a bias and, where the entry has one, the prefill form's
    workspace): every validated pointer at half its alignment."""
    build, grid = A.entries()[entry]
    be = A.TorchBackend()
    n = sum(A.refusals(build(*args), be) for args in (grid[0], grid[-1]))
    print(f"{entry}: {n} misaligned pointers refused")
    validated = any(o.validated and o.align >= 2 for o in build(*grid[-1]).ops)
    assert (n > 0) == validated
