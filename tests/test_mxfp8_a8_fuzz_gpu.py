"""A 40-case slice of the randomised MXFP8 W8A8 sweep (tests/sweeps/fuzz_mxfp8_a8.py): no failures, every form reached, none
skipped.  tests/test_mxfp8_a8_cpu.py shows on the host that the generator's draws are all accepted and cover every form."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES, SEED = 40, 1


def test_mxfp8_a8_fuzz_slice():
    import fuzz_mxfp8_a8 as F
    r = F.run(CASES, SEED)
    print({k: v for k, v in r.items() if k != "bad"})
    assert not r["bad"], r["bad"][:5]
    assert r["ok"] == CASES, r["refused"]
    assert all(n > 0 for n in r["forms"].values()), r["forms"]
