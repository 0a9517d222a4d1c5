"""The rows kernel's three piecewise task laws on every branch, on the device: b1, bc, blb and bub of wbcqp_problem_data against the
high-precision statement of tests/task_laws.py -- the exact logarithm for log3 (Taylor branch, both ends of the middle one, the near-pi
branch with its sign selectors in every octant), computeAccLimits on all 27 reachable combinations of its eleven decisions, the 5PL
repulsor from deep penetration to five margins away -- per entry:

    |dev - ref| <= TOL_ROWS max(1, |ref|) + 4 S.

tests/test_task_laws_host.py checks on the CPU that the inputs reach all of that and holds the C oracle to the same bar.
The worst error per regime is printed before anything is asserted (pytest -s).  Measured on an MI355X (profiles/task_laws/INDEX.md), as
|dev - ref| / max(1, |ref|): Taylor branch 4.1e-12 (the law's own truncation), low end of the middle branch 3.1e-14 -- 2.5e-10 on the random tree,
24 entries over the bar, while the kernel still took theta from acos() alone there --, near pi 2.6e-12, 5PL 1.9e-11, bounds 1.6e-11."""
import numpy as np
import pytest

from inria_wbc_amd import capi
from tests import task_laws as tl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(oracle_mod):
    h = capi.Handle(0, capi.F64)
    yield h
    h.close()


@pytest.mark.parametrize("name", ["talos", "franka", "tree"])
def test_task_laws_on_every_branch(handle, name):
    C = tl.case(name)
    handle.set_structure(3, C["st"])
    handle.set_model(3, C["m"], C["tm"])
    dev = handle.problem_data_host(3, C["q"], C["v"], C["ref"])
    tl.report(name + ", device", tl.worst_per_regime(C, dev))
    for k, r in C["rows"].items():
        assert np.isfinite(dev[k]).all(), k
        bad = np.argwhere(np.abs(dev[k] - r) > tl.bar(r, C["S"][k]))
        assert bad.size == 0, (k, [(tuple(b), tl.REGIMES[C["regime"][k][tuple(b)]], dev[k][tuple(b)], r[tuple(b)]) for b in bad[:6]])
