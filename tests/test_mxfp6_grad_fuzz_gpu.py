"""A 40-case slice of the randomised MXFP6 input-gradient sweep (tests/sweeps/fuzz_mxfp6_grad.py) with a fixed seed and bounded shapes:
no failures, the dense and the grouped form both reached.  The long run (300 cases) is profiles/fuzz_mxfp6_grad.txt."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "sweeps"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES, SEED = 40, 1


def test_mxfp6_grad_fuzz_slice():
    import fuzz_mxfp6_grad as F
    r = F.run(CASES, SEED, small=True)
    print({k: v for k, v in r.items() if k != "bad"})
    assert not r["bad"], r["bad"][:5]
    assert r["ok"] == CASES
    assert all(n > 0 for n in r["kinds"].values()), r["kinds"]
