"""Every tensor the entry points of the pointwise GEMM family write, bit for bit, against tests/golden/pw_bits.json: the sha256 of
the bytes csrc/pwconv.hip, csrc/pwgrad.hip and csrc/tapsum.hip produced before their two kernel generations were put on one
shared ring, epilogue and dispatch (recorded by tools/gen_pw_bits_golden.py at the last commit that spelled each out).

tests/test_pw_arms_gpu.py holds the same rows to float64 references within a rounding bound: a shared helper that changed an
association, a rounding or the order of a split sum would stay inside it.  This one holds the arithmetic itself still, on
every row of the pin (all 63 pwconv instantiations, both pwgrad main kernels, the pair form, the reduce kernels, tapsum), each
under its own hook variables.  The inputs are not stored: the generator's `compute()` draws them again from the pin's seeded
generators.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT
from oracle import pw_inputs as P

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("gen_pw_bits_golden", os.path.join(ROOT, "tools", "gen_pw_bits_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pointwise_kernels_reproduce_the_recorded_bits(device):
    with open(os.path.join(GOLDEN, "pw_bits.json")) as f:
        want = json.load(f)
    gen = _generator()
    got = gen.compute(device)
    assert sorted(got) == sorted(want)
    rows = {k.rsplit("/", 2 if k.startswith("pair/") else 1)[0] for k in want}
    assert len(rows) == gen.ROWS == 162
    differing = sorted(k for k in want if got[k] != want[k])
    assert not differing, (len(differing), differing[:20])
    # the fixture holds every output: both of each EPI 1 / 5 row, the partials of each EPI 4 row
    epis = [c.epi for c in P.TILE_CASES + P.EDGE_CASES]
    assert sum(k.endswith("/y2") for k in want) == sum(e in (1, 5) for e in epis) > 0
    assert sum(k.endswith("/sums") for k in want) == epis.count(4) > 0
