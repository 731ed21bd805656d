"""A 30-case slice of the randomised MXFP6 W6A16 mixture-of-experts sweep (tests/sweeps/fuzz_mxfp6_moe.py): no failures, nothing
refused, every form reached (test_mxfp6_moe_cpu.py checks on the host that this seed's draws cover every form)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES, SEED = 30, 3


def test_mxfp6_moe_fuzz_slice():
    import fuzz_mxfp6_moe as F
    r = F.run(CASES, SEED)
    print({k: v for k, v in r.items() if k != "bad"})
    assert r["fatal"] is None, r["fatal"]
    assert not r["bad"], r["bad"][:5]
    assert r["ok"] == CASES, r["refused"]
    assert all(n > 0 for n in r["forms"].values()), r["forms"]
