"""CPU tests of the differential kinematics of a fleet (wbcqp_set_jacobian_frames, wbcqp_jacobians): the numpy statement
inria_wbc_amd/jacobians.py against the rigid-body oracle, and the library's surface (symbols declared, exported, bound, refusing a NULL handle).
No GPU.

The reference quantity everywhere: the oracle's rbd_terms(...)["Jl"], ["Jw"], ["Jcom"], ["Ag"], ["dAgv"] and ["af"] (oracle/rbd_oracle.c, which
tests/test_oracle_rbd.py holds to finite differences and momentum sums).  The oracle has no LOCAL_WORLD_ALIGNED Jacobian: the reference there is
blockdiag(R, R) Jl and R af with R from the oracle's oMf.

Bar: TOL_ROWS (1e-10, the project's bar for two formulations in double), relative to max(1, the array's largest entry)."""
import ctypes
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import model as mdl
from tests.test_forward_dynamics_host import CASES, case_states
from tests.test_inverse_dynamics_host import ERR_INVALID, TOL_ROWS, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STATES = 3
SHAPES = ("one_body_fixed", "tree_64_fixed_lane_limit", "tree_59_floating_nv_limit", "chain_62", "star_17_floating", "talos")
NEW = {"wbcqp_set_jacobian_frames", "wbcqp_jacobians", "wbcqp_jacobians_host"}


def selections(m):
    """none, one frame, all 64 slots with repeats, a frame on body 0 together with one on the last body, two frames on one body (the cases of
    tests/model_queries.tree_case put frames 0 and 1 on body 0 and on the last body, frames 2 and 3 on one body)."""
    full = np.random.default_rng(11).integers(0, m.nframe, 64)
    full[40] = full[7]
    return {"none": [], "one": [m.nframe // 2], "sixty_four_with_repeats": full.tolist(), "first_and_last_body": [0, 1], "two_on_one_body": [2, 3]}


def oracle_terms(m, q, v):
    """The oracle's terms of every state, stacked: {name: [n, ...]}."""
    from oracle import rbd
    om = rbd.OracleModel(m)
    terms = [rbd.rbd_terms(om, q[i], v[i]) for i in range(q.shape[0])]
    return {k: np.stack([t[k] for t in terms]) for k in ("Jl", "Jw", "Jcom", "Ag", "dAgv", "af", "oMf", "vf", "vcom")}


def reference(terms, frames, rf):
    """(J [n, n_frames, 6, nv], drift [n, n_frames, 6] or None) of the frames `frames` in the convention rf, from the oracle's terms."""
    from inria_wbc_amd import jacobians as jac
    frames = np.asarray(frames, dtype=np.int64)
    if rf == jac.WORLD:
        return terms["Jw"][:, frames], None
    Jl, af = terms["Jl"][:, frames], terms["af"][:, frames]
    if rf == jac.LOCAL:
        return Jl, af
    R = terms["oMf"][:, frames, :9].reshape(Jl.shape[0], frames.size, 3, 3)
    J = np.concatenate([np.einsum("nfij,nfjk->nfik", R, Jl[:, :, :3]), np.einsum("nfij,nfjk->nfik", R, Jl[:, :, 3:])], axis=2)
    drift = np.concatenate([np.einsum("nfij,nfj->nfi", R, af[:, :, :3]), np.einsum("nfij,nfj->nfi", R, af[:, :, 3:])], axis=2)
    return J, drift


@pytest.mark.parametrize("name", SHAPES)
def test_numpy_statement_against_the_oracle(name):
    from inria_wbc_amd import jacobians as jac
    m, st, tm = CASES[name]()
    q, v, _ = case_states(m, tm, N_STATES, 71_000)
    terms = oracle_terms(m, q, v)
    frames = list(range(m.nframe))  # every frame of the model once: any selection is a gather of these
    worst = {}
    for rf in (jac.WORLD, jac.LOCAL, jac.LOCAL_WORLD_ALIGNED):
        got = jac.jacobians(m, q, v, frames, rf)
        wantJ, want_drift = reference(terms, frames, rf)
        want = {"J": wantJ, "Jcom": terms["Jcom"], "Ag": terms["Ag"], "dAgv": terms["dAgv"]}
        if want_drift is not None:
            want["drift"] = want_drift
        assert set(got) == set(want)
        for k in want:
            assert got[k].shape == want[k].shape, k
            worst[k] = max(worst.get(k, 0.0), rel_err(got[k], want[k]))
    print("jacobians.py against the oracle, %-26s %s" % (name, "  ".join("%s %.1e" % kv for kv in worst.items())))
    assert max(worst.values()) <= TOL_ROWS, worst
    # what the matrices are for: J_local v is the frame's velocity, Jcom v the CoM's
    local = jac.jacobians(m, q, None, frames, jac.LOCAL, which=["J", "Jcom"])
    assert rel_err(np.einsum("nfij,nj->nfi", local["J"], v), terms["vf"]) <= TOL_ROWS
    assert rel_err(np.einsum("nij,nj->ni", local["Jcom"], v), terms["vcom"]) <= TOL_ROWS


def test_selections_are_gathers_and_unsupported_columns_are_zero():
    from inria_wbc_amd import jacobians as jac
    m, st, tm = CASES["star_17_floating"]()
    q, v, _ = case_states(m, tm, 2, 72_000)
    every = jac.jacobians(m, q, v, list(range(m.nframe)), jac.LOCAL_WORLD_ALIGNED)
    body, sup = jac.dof_bodies(m), jac.supports(m)
    for sel, frames in selections(m).items():
        got = jac.jacobians(m, q, v, frames, jac.LOCAL_WORLD_ALIGNED)
        assert got["J"].shape == (2, len(frames), 6, m.nv) and got["drift"].shape == (2, len(frames), 6), sel
        assert np.array_equal(got["J"], every["J"][:, frames]) and np.array_equal(got["drift"], every["drift"][:, frames]), sel
        assert np.array_equal(got["Ag"], every["Ag"]) and np.array_equal(got["Jcom"], every["Jcom"]), sel
        for k, f in enumerate(frames):
            off = ~sup[body, m.frame_body[f]]
            assert off.any() and (got["J"][:, k][:, :, off] == 0.0).all(), (sel, f)  # (a star: whatever the body, some leaf's dof does not move it)
    # a star: a leaf's frame moves with the base's six dofs and its own joint alone
    leaf = jac.jacobians(m, q, None, [1], jac.WORLD, which=["J"])["J"][:, 0]
    assert (np.abs(leaf).max(axis=(0, 1)) > 0).sum() == 7


def test_what_is_refused():
    from inria_wbc_amd import jacobians as jac
    m = mdl.franka_like()
    q = m.q0[None]
    with pytest.raises(ValueError):
        jac.jacobians(m, q, None, [0], jac.LOCAL, which=["drift"])       # drift without v
    with pytest.raises(ValueError):
        jac.jacobians(m, q, None, [], jac.LOCAL, which=["dAgv"])         # dAgv without v
    with pytest.raises(ValueError):
        jac.jacobians(m, q, np.zeros((1, m.nv)), [0], jac.WORLD, which=["drift"])  # drift in WORLD
    with pytest.raises(ValueError):
        jac.jacobians(m, q, None, [0], 3)                                # an unknown reference frame
    assert set(jac.jacobians(m, q, np.zeros((1, m.nv)), [0], jac.WORLD)) == {"J", "Jcom", "Ag", "dAgv"}
    assert (jac.WORLD, jac.LOCAL, jac.LOCAL_WORLD_ALIGNED) == (0, 1, 2)  # pinocchio's values


def test_symbols_declared_exported_bound_and_null_handle(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(capi.EXPORTS)
    assert re.search(r"#define\s+WBCQP_MAX_JACOBIAN_FRAMES\s+64\b", hdr) and re.search(r"#define\s+WBCQP_VERSION\s+151\b", hdr)
    assert re.search(r"WBCQP_RF_WORLD = 0, WBCQP_RF_LOCAL = 1, WBCQP_RF_LOCAL_WORLD_ALIGNED = 2 \} wbcqp_reference_frame;", hdr)
    assert (capi.RF_WORLD, capi.RF_LOCAL, capi.RF_LOCAL_WORLD_ALIGNED) == (0, 1, 2)
    assert capi.JACOBIAN_OUTPUTS == ("J", "Jcom", "Ag", "drift", "dAgv") and [k for k, _ in capi.CJacobianOutputs._fields_] == list(capi.JACOBIAN_OUTPUTS)
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in NEW:
        assert hasattr(raw, sym), sym
        assert getattr(lib, sym).argtypes, sym
    assert raw.wbcqp_version() == 151
    for name in ("set_jacobian_frames", "jacobians", "jacobians_host"):
        assert callable(getattr(capi.Handle, name))
    # a NULL handle is refused before anything else is looked at
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    out = capi.CJacobianOutputs(None, p, None, None, None)
    frames = (ctypes.c_int32 * 2)(0, 0)
    assert lib.wbcqp_set_jacobian_frames(None, 0, 2, frames) == ERR_INVALID
    assert lib.wbcqp_jacobians(None, 0, 1, p, None, capi.RF_LOCAL, ctypes.byref(out), None) == ERR_INVALID
    assert lib.wbcqp_jacobians_host(None, 0, 1, p, None, capi.RF_LOCAL, ctypes.byref(out)) == ERR_INVALID


def test_algorithmic_bytes():
    from inria_wbc_amd import jacobians as jac
    m = mdl.talos_like()
    assert jac.algorithmic_bytes(m, 8) == (m.nq + m.nv + 8 * 6 * m.nv + 3 * m.nv + 6 * m.nv + 8 * 6 + 6) * 8
    assert jac.algorithmic_bytes(m, 2, ("J",)) == (m.nq + 2 * 6 * m.nv) * 8                 # v is not read
    assert jac.algorithmic_bytes(m, 0, ("Jcom", "Ag"), itemsize=4) == (m.nq + 9 * m.nv) * 4
    assert jac.algorithmic_bytes(m, 2, ("dAgv",)) == (m.nq + m.nv + 6) * 8
    with pytest.raises(ValueError):
        jac.algorithmic_bytes(m, 2, ("other",))
