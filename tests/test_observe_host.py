"""CPU tests of the observables (wbcqp_observe): the numpy statement inria_wbc_amd/observe.py against the rigid-body oracle and against
finite differences of its own positions, and the library's surface (symbols declared, exported, bound).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import model as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ROWS = 1e-10  # tests/test_gpu_terms.py: two formulations, relative to max(1, the array's largest entry)
FD_EPS, FD_TOL = 1e-6, 1e-7  # tests/test_oracle_rbd.py::test_jacobians_and_drifts_by_finite_differences: step and bar of its first derivatives
N_STATES = 8

MODELS = {"talos": lambda: mdl.talos_like(), "icub": lambda: mdl.icub_like(), "franka": lambda: mdl.franka_like(),
          "tree_fb": lambda: mdl.random_tree(3, 24, True), "tree_fixed": lambda: mdl.random_tree(4, 17, False)}


def _states(m, seed):
    """N_STATES states around q0, as tests/test_oracle_rbd.py draws them."""
    qs, vs = [], []
    for k in range(N_STATES):
        rng = np.random.default_rng(seed + k)
        q = m.q0.copy()
        q[(7 if m.floating_base else 0):] += 0.3 * rng.standard_normal(m.na)
        if m.floating_base:
            q[0:3] += rng.standard_normal(3)
            q[3:7] += 0.3 * rng.standard_normal(4)
            q[3:7] /= np.linalg.norm(q[3:7])
        qs.append(q)
        vs.append(0.5 * rng.standard_normal(m.nv))
    return np.stack(qs), np.stack(vs)


@pytest.fixture(scope="module", params=list(MODELS))
def case(request):
    """(model, q, v, all frames, observe.py's outputs): computed once per model, read by the tests below."""
    from inria_wbc_amd import observe
    m = MODELS[request.param]()
    q, v = _states(m, 40_000)
    frames = np.arange(m.nframe)
    return m, q, v, frames, observe.observe(m, q, v, frames)


def test_conventions_of_the_oracle(case):
    """What include/wbcqp.h states for placement and velocity is what the oracle's oMf and vf hold: rotation row-major then translation;
    (linear, angular) in the frame's own axes -- R_f v_lin is the derivative of the frame's position."""
    from oracle import rbd, oracle as orc
    m, q, v, frames, _ = case
    t = rbd.rbd_terms(m, q[0], v[0])
    Rf, pf = m.frame_placements(q[0])
    assert np.abs(t["oMf"][:, :9].reshape(-1, 3, 3) - Rf).max() < 1e-13 and np.abs(t["oMf"][:, 9:] - pf).max() < 1e-13
    adv = lambda e: orc.integrate(m.floating_base, e, q[0][None], v[0][None], np.zeros((1, m.nv)))["q_next"][0]
    dp = (m.frame_placements(adv(FD_EPS))[1] - m.frame_placements(adv(-FD_EPS))[1]) / (2 * FD_EPS)
    assert np.abs(dp - np.einsum("fij,fj->fi", Rf, t["vf"][:, :3])).max() < FD_TOL


def test_numpy_statement_against_the_oracle(case):
    from oracle import rbd
    m, q, v, frames, got = case
    om = rbd.OracleModel(m)
    ora = {k: [] for k in ("com", "vcom", "oMf", "vf")}
    for i in range(N_STATES):
        t = rbd.rbd_terms(om, q[i], v[i])
        for k in ora:
            ora[k].append(t[k].copy())
    worst = {}
    for mine, theirs in (("com", "com"), ("vcom", "vcom"), ("placement", "oMf"), ("velocity", "vf")):
        want = np.stack(ora[theirs])
        worst[mine] = np.abs(got[mine] - want).max() / max(1.0, np.abs(want).max())
    print("observe.py against the oracle, %s: %s" % (m.name, {k: "%.1e" % e for k, e in worst.items()}))
    assert max(worst.values()) <= TOL_ROWS, worst


def test_velocities_against_finite_differences_of_the_positions(case):
    """vcom and the linear part of velocity (turned into the world's axes) are the derivatives of com and of the frames' positions along
    integrate(q, v h): a central difference of observe.py's own positions."""
    from inria_wbc_amd import observe
    from oracle import oracle as orc
    m, q, v, frames, got = case
    adv = lambda e: orc.integrate(m.floating_base, e, q, v, np.zeros((N_STATES, m.nv)))["q_next"]
    plus, minus = observe.observe(m, adv(FD_EPS), None, frames), observe.observe(m, adv(-FD_EPS), None, frames)
    dcom = (plus["com"] - minus["com"]) / (2 * FD_EPS)
    dpos = (plus["placement"][..., 9:] - minus["placement"][..., 9:]) / (2 * FD_EPS)
    R = got["placement"][..., :9].reshape(N_STATES, -1, 3, 3)
    assert np.abs(dcom - got["vcom"]).max() < FD_TOL
    assert np.abs(dpos - np.einsum("bfij,bfj->bfi", R, got["velocity"][..., :3])).max() < FD_TOL


def test_frame_ids_and_repeats():
    from inria_wbc_amd import observe
    m = mdl.talos_like()
    ids = observe.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "leg_left_6_joint"])
    assert ids.dtype == np.int32 and ids.tolist() == [m.frame("leg_left_6_joint"), m.frame("gripper_right_joint"), m.frame("leg_left_6_joint")]
    with pytest.raises(KeyError):
        observe.frame_ids(m, ["no_such_frame"])
    out = observe.observe(m, m.q0, None, ids)
    assert out["placement"].shape == (1, 3, 12) and "vcom" not in out and np.array_equal(out["placement"][0, 0], out["placement"][0, 2])
    Rf, pf = m.frame_placements(m.q0)
    assert np.array_equal(out["placement"][0, 1, 9:], pf[ids[1]]) and np.abs(out["com"][0] - m.com(m.q0)).max() < 1e-15
    assert observe.observe(m, m.q0).get("placement").shape == (1, 0, 12)


def test_symbols_declared_exported_bound(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    new = {"wbcqp_set_observed_frames", "wbcqp_observe", "wbcqp_observe_host"}
    assert new <= declared and new <= set(capi.EXPORTS)
    assert re.search(r"#define\s+WBCQP_MAX_OBSERVED\s+64\b", hdr) and "wbcqp_observables" in hdr
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in new:
        assert hasattr(raw, sym), sym
        assert getattr(lib, sym).argtypes, sym
    assert ctypes.sizeof(capi.CObservables) == 32
    assert [k for k, _ in capi.CObservables._fields_] == ["com", "vcom", "placement", "velocity"]
    assert raw.wbcqp_version() == 151
    for name in ("set_observed_frames", "observe", "observe_host"):
        assert callable(getattr(capi.Handle, name))
