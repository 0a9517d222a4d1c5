"""The cases of the inverse dynamics' derivatives, their committed truth (tests/golden/id_derivatives/, written by tests/id_derivatives_exact.py)
and the bar: everything the tests need that needs no mpmath.  Models, states and wrench frames are those of tests/rbd_exact_cases.py."""
from __future__ import annotations

import functools
import os
from typing import Dict

import numpy as np

from tests.rbd_exact_cases import CASES as RBD_CASES, EPS, SMALL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "id_derivatives")
CASES = tuple(SMALL) + ("talos",)
# the five small cases with all their states; Talos with its first
N_STATES = {name: (1 if name == "talos" else RBD_CASES[name][1]) for name in CASES}
MATRICES = ("dtau_dq", "dtau_dv")

# K_STATEMENT: the worst error(...) below of the numpy statement inria_wbc_amd/id_derivatives.py against the fixtures, over every case, state and
# matrix.  Measured on the CPU with `pytest -s tests/test_id_derivatives_host.py -k statement_against_truth` (the line "K_STATEMENT measured",
# three digits: 2.60e-15, on the single revolute body; Talos 2.28e-15), written here rounded UP in the third digit.  The device's bar is DEVICE_MARGIN times this: statement and kernel evaluate
# the same formulas in float64 and differ in origin and summation order; four is the margin the project gives elsewhere.  Neither figure comes
# from the kernel's output.
K_STATEMENT = 2.60e-15
DEVICE_MARGIN = 4.0


def path(name):
    return os.path.join(GOLDEN, name + ".npz")


@functools.lru_cache(maxsize=None)
def load(name) -> Dict[str, np.ndarray]:
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


def error(x, truth, fallback=None) -> float:
    """max |x - truth| / max |truth| of one state's matrix.  A matrix that is zero for rigid bodies (dtau_dv of a single revolute body on a fixed
    base) has no scale of its own -- its truth is 0, or 1e-17 of the state's other matrix because the tables' rotations are orthogonal to 1e-16
    only, and a float64 evaluation of it (the numpy statement, where the device is held to that) is a few roundings of terms of the other
    matrix's size: where max |truth| is under 64 eps times `fallback`, the largest entry of the state's other matrix, it is held against `fallback`."""
    x, truth = np.asarray(x, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert x.shape == truth.shape, (x.shape, truth.shape)
    big = np.abs(truth).max()
    if fallback is not None and big <= 64 * EPS * fallback:
        big = fallback
    assert big > 0.0
    return float(np.abs(x - truth).max() / big)


def worst_error(got: Dict[str, np.ndarray], want: Dict[str, np.ndarray]) -> float:
    """The worst error(...) over the states [n, nv, nv] and matrices that `got` holds; `want` holds both matrices."""
    worst = 0.0
    for k in got:
        other = MATRICES[1 - MATRICES.index(k)]
        for i in range(want[k].shape[0]):
            worst = max(worst, error(got[k][i], want[k][i], float(np.abs(want[other][i]).max())))
    return worst
