"""The cases of the exact statement of the rigid-body terms (tests/rbd_exact.py), its committed fixtures and the entrywise bar: everything the
tests need that needs no mpmath.  tests/test_gpu_rbd_exact.py uses this module alone -- fixtures only, nothing is computed there;
tests/rbd_exact.py (the statement itself) and tests/test_rbd_exact_host.py build on it.  The module's docstring there says what a scale is."""
from __future__ import annotations

import functools
import os
from typing import Dict, List

import numpy as np

from inria_wbc_amd import model as mdl

EPS = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rbd_exact")
TOTALS = ("M", "nle", "tau_a", "tau_aw", "Agv")  # the quantities that also carry a scale_total
QUANTITIES = ("placement", "com", "J_world", "J_local", "J_lwa", "Jcom", "Ag", "M", "velocity", "vcom", "Agv", "drift_local", "drift_lwa", "acom",
              "dAgv", "nle", "tau_a", "tau_aw")
ORIGINS = ("world", "base")
NO_ORIGIN = ("placement", "com", "nle", "tau_a", "tau_aw")  # computed directly, or held to scale_total: no scale_world / scale_base
CONVENTIONS = ("world", "local", "lwa")  # wbcqp_reference_frame, as the Jacobians' names spell them
HESSIANS = tuple("H_" + c for c in CONVENTIONS)   # [states, frames, 6, nv, nv]: d J[f, r, j] / d q_k
RATES = tuple("dJ_" + c for c in CONVENTIONS)     # [states, frames, 6, nv]: d/dt of J along the curve that leaves q with the velocity v
SECOND_ORDER = HESSIANS + RATES                   # fixtures of their own (<case>.hessians.npz), with scale and scale_world

# K_ORACLE[quantity]: the worst ratio |x - value| / (eps scale) of the C oracle (rbd.rbd_terms, rbd.rnea) and of the numpy statements (observe,
# jacobians, dynamics, forward_dynamics.mass_matrix) over all seven cases.  Measured 2026-10-20 with
# `pytest -s tests/test_rbd_exact_host.py -k oracle_ratio` (the line "K_ORACLE measured", three digits), written here rounded UP in the third digit
# so that no run exceeds it; the same figures came out on three different CPUs.  Every one is under 256.
K_ORACLE = {
    "placement": 1.19, "com": 1.83, "J_world": 95.9, "J_local": 4.74, "J_lwa": 95.9, "Jcom": 100.0, "Ag": 101.0, "M": 8.95, "velocity": 0.913,
    "vcom": 1.25, "Agv": 2.84, "drift_local": 0.575, "drift_lwa": 1.90, "acom": 0.696, "dAgv": 0.803, "nle": 1.80, "tau_a": 1.54, "tau_aw": 0.543,
}
# The six second-order quantities: the worst ratio of inria_wbc_amd/hessians.py alone -- NO C oracle exists for them -- over all seven cases, H
# against `scale`, dJ against `scale_world` (tests/test_gpu_rbd_exact.py says why).  Measured 2026-10-21 with the same command (37.6, 0.251, 10.5,
# 0.996, 0.811, 0.996 on the line "K_ORACLE measured"), written rounded UP in the third digit.  Every one is under 256.
K_ORACLE.update({"H_world": 37.7, "H_local": 0.252, "H_lwa": 10.6, "dJ_world": 0.997, "dJ_local": 0.812, "dJ_lwa": 0.997})
assert set(K_ORACLE) == set(QUANTITIES) | set(SECOND_ORDER)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
def _tree(seed, nb, fb, parent=None, jtype=None, nframe=8):
    m = mdl.random_tree(seed, nb, fb, nframe=nframe)
    if parent is not None:
        m.parent = np.array(parent, dtype=np.int32)
    if jtype is not None:
        m.jtype = np.array(jtype, dtype=np.int32)
    m.frame_body[0], m.frame_body[1] = 0, nb - 1  # the root, and the last body: a leaf
    m.frame_body[3] = m.frame_body[2]             # two frames on one body
    m.validate()
    return m


def _light_leaf():
    """A floating tree of 12: body 7 is a leaf at depth 5 between the subtrees {5, 6} and {8, 9}, both 8 kg a body; it has 1e-3 of the typical
    mass (4 kg) and 1e-5 of the typical rotational inertia (1.3e-2 kg m^2), its CoM a centimetre off its joint."""
    m = _tree(71, 12, True, parent=[-1, 0, 1, 2, 3, 4, 5, 4, 4, 8, 0, 10])
    for b in (5, 6, 8, 9):
        m.inertia[b] *= 8.0 / m.inertia[b, 0]
        m.inertia[b, 1:4] *= m.inertia[b, 0] / 8.0  # (the line above scaled the CoM too: put it back)
    r = m.inertia[7].copy()
    m.inertia[7, 0] = 4e-3
    m.inertia[7, 1:4] = 0.1 * r[1:4]
    m.inertia[7, 4:10] = r[4:10] * (1.3e-7 / max(r[4], r[7], r[9]))
    assert m.depth()[7] == 5 and m.subtree_last()[7] == 7
    return m


def _tree_59():
    m = mdl.random_tree(63, 59, True, nframe=12)  # the model of tests/test_forward_dynamics_host.py's tree_59_floating_nv_limit
    m.frame_body[0], m.frame_body[1] = 0, 58
    m.frame_body[3] = m.frame_body[2]
    m.validate()
    return m


def _talos_wrench_frames(m):
    return [m.frame("base_link"), m.frame("v_base_link_left"), m.frame("gripper_left_fingertip_1_joint")]


# name -> (model, states, what it exercises)
CASES = {
    "one_revolute_fixed": (lambda: _tree(72, 1, False, jtype=[mdl.J_RZ]), 3, "the minimum"),
    "prismatic_revolute_fixed": (lambda: _tree(73, 2, False, parent=[-1, 0], jtype=[mdl.J_PX, mdl.J_RY]), 3, "both joint families"),
    "chain_8_fixed": (lambda: _tree(74, 8, False, parent=list(range(-1, 7))), 3, "three rounds of ancestor doubling"),
    "star_9_floating": (lambda: _tree(75, 9, True, parent=[-1] + [0] * 8), 3, "every subtree but the root's is a single lane"),
    "light_leaf_12_floating": (_light_leaf, 3, "both running totals are large where they are differenced"),
    "talos": (mdl.talos_like, 2, "the shipped robot"),
    "tree_59_floating": (_tree_59, 1, "the lane limit"),
}
SMALL = tuple(list(CASES)[:5])
FULL_ONLY = ("talos", "tree_59_floating")


@functools.lru_cache(maxsize=None)
def model(name):
    return CASES[name][0]()


def wrench_frames(name) -> List[int]:
    m = model(name)
    return _talos_wrench_frames(m) if name == "talos" else [2, 3, 1]  # two frames on one body, one on a leaf


def hessian_frames(name) -> List[int]:
    """The frames of the second-order quantities: every frame of the small cases (the root, a leaf and two frames on one body among them); Talos:
    the wrench frames and one on the other arm; the 59-body tree: the root, the last body and two on one body."""
    m = model(name)
    if name == "talos":
        return _talos_wrench_frames(m) + [m.frame("gripper_right_joint")]
    return [0, 1, 2, 3] if name == "tree_59_floating" else list(range(m.nframe))


@functools.lru_cache(maxsize=None)
def states(name) -> Dict[str, np.ndarray]:
    """q within 0.5 of q0, v and a of order 1, a random unit quaternion as float64 rounds it, the base 1 to 3 m from the origin; wrenches of
    order 10 at wrench_frames(name)."""
    m = model(name)
    n = CASES[name][1]
    rng = np.random.default_rng(9_000 + list(CASES).index(name))
    q = np.tile(m.q0, (n, 1))
    q[:, m.nq - m.na:] += rng.uniform(-0.5, 0.5, (n, m.na))
    if m.floating_base:
        d = rng.standard_normal((n, 3))
        q[:, 0:3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (n, 1))
        u = rng.standard_normal((n, 4))
        q[:, 3:7] = u / np.linalg.norm(u, axis=1, keepdims=True)
    return dict(q=q, v=rng.standard_normal((n, m.nv)), a=rng.standard_normal((n, m.nv)), wrench=10.0 * rng.standard_normal((n, 3, 6)))


def path(name):
    return os.path.join(GOLDEN, name + ".npz")


def hessians_path(name):
    return os.path.join(GOLDEN, name + ".hessians.npz")


@functools.lru_cache(maxsize=None)
def load(name) -> Dict[str, np.ndarray]:
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def load_hessians(name) -> Dict[str, np.ndarray]:
    with np.load(hessians_path(name)) as z:
        return {k: z[k] for k in z.files}


# ---- the bar -----------------------------------------------------------------------------------------------------------------------------------
def ratios(x, value, scale):
    """|x - value| / (eps scale) per entry; a structural zero (scale 0) gives 0 where x is an exact zero and inf where it is not."""
    x, value, scale = np.asarray(x, dtype=np.float64), np.asarray(value), np.asarray(scale)
    assert x.shape == value.shape, (x.shape, value.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(x - value) / (EPS * scale)
    return np.where(scale == 0.0, np.where(x == 0.0, 0.0, np.inf), r)


def worst_ratio(x, value, scale) -> float:
    r = ratios(x, value, scale)
    return float(r.max()) if r.size else 0.0
