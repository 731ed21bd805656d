"""A 150-case slice of the randomised MXFP4 W4A6 mixture-of-experts sweep (tests/sweeps/fuzz_mxfp4_moe_a6.py): no failures, nothing
refused, both forms, both tile widths of the grouped form and the one-launch decode form's K bound (K = 16384 itself and its neighbours)
reached.  A 600-case run is recorded in profiles/fuzz_mxfp4_moe_a6.txt."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES, SEED = 150, 1


def test_mxfp4_moe_a6_fuzz_slice():
    import fuzz_mxfp4_moe_a6 as F
    r = F.run(CASES, SEED)
    print({k: v for k, v in r.items() if k != "bad"})
    assert not r["bad"], r["bad"][:5]
    assert r["ok"] == CASES, r["refused"]
    assert all(n > 0 for n in r["forms"].values()), r["forms"]
    assert all(n > 0 for n in r["tile_widths"].values()), r["tile_widths"]
    assert r["k_edge_cases"] > 0 and r["k_bound_cases"] > 0
    assert r["k_edge_cases"] > r["k_bound_cases"]  # a neighbour of the bound as well
