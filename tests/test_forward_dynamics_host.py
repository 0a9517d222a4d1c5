"""CPU tests of forward dynamics (wbcqp_mass_matrix, wbcqp_forward_dynamics, wbcqp_spd_commands): the numpy statement
inria_wbc_amd/forward_dynamics.py against the rigid-body oracle and against a literal transcription of the reference's compute_spd, and the
library's surface (symbols declared, exported, bound, refusing a NULL handle).  No GPU.

The reference quantity everywhere: the oracle's rbd_terms(...)["M"], ["nle"], ["Jl"] and rbd.rnea.

Bars.  TOL_ROWS (1e-10, tests/test_inverse_dynamics_host.py's bar for two formulations in double), relative to max(1, the array's largest entry).
The accelerations themselves are NOT held to it: cond M is 2e7 on Talos, so two correct solvers differ by up to cond * eps ~ 4e-9 in a.  What a
solver owes is a small residual in force space -- the round trip rnea(q, v, a_out) + damping * a_out - sum J'w = tau_in -- and that is what is
checked.  With the oracle's M and a plain Cholesky the worst round-trip figures measured over 8 states per case were 1.3e-12 (62-body chain),
5.7e-14 (Talos, nv 50), 4.9e-14 (64 bodies fixed), 4.0e-14 (59 bodies floating), every pivot positive (the smallest 4.9e-6, on Talos): the
reference alone stays 75 x under the bar.  The SPD commands are well conditioned (cond(M + Kd dt) 9.5e2 on Talos, 1.4e4 on the 24-body tree)
and are compared directly."""
import ctypes
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import model as mdl
from tests import model_queries as mq
from tests.test_inverse_dynamics_host import ERR_INVALID, MODELS, TOL_ROWS, rel_err, states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROUND = 8  # states per case of the round trip
DT = 0.001


def _tree(seed, nb, fb, shape=None):
    return mq.tree_case("fdyn_", seed, nb, fb, shape, two_on_one_body=True)


def _franka():
    m = mdl.franka_like()
    return (m,) + mq.minimal(m, "fdyn_")


# the cases of tests/test_gpu_inverse_dynamics.py, Talos and a fixed-base arm (every dof has SPD gains)
CASES = {"one_body_fixed": _tree(61, 1, False), "tree_64_fixed_lane_limit": _tree(62, 64, False), "tree_59_floating_nv_limit": _tree(63, 59, True),
         "chain_62": _tree(64, 62, False, "chain"), "star_17_floating": _tree(65, 17, True, "star"), "tree_24_floating": _tree(66, 24, True),
         "talos": mq.talos_case, "franka": _franka}
ROUND_TRIP = ("chain_62", "talos", "tree_64_fixed_lane_limit", "tree_59_floating_nv_limit")


def case_states(m, tm, n, seed):
    """(q, v, tau) of n states with the noise tests/test_gpu_inverse_dynamics.py uses for trees; tau: all nv rows, a robot's joint torques in size."""
    s = mdl.sample_states(m, tm, n, seed, q_noise=0.3, v_noise=0.5)
    return s["q"], s["v"], 20.0 * np.random.default_rng(seed + 1).standard_normal((n, m.nv))


def oracle_round_trip(rbd, om, m, q, v, a, frames=(), wrench=None, damping=None, Jl=None):
    """rnea(q, v, a) + damping * a - sum_k J_k' w_k, one state at a time: what tau_in must come back as.  v None: zero.  Jl: the states' local
    frame Jacobians [n, nframe, 6, nv] where the caller has them already (they depend on q alone)."""
    out = np.zeros((q.shape[0], m.nv))
    for i in range(q.shape[0]):
        vi = np.zeros(m.nv) if v is None else v[i]
        out[i] = rbd.rnea(om, q[i], vi, a[i])
        if damping is not None:
            out[i] += damping * a[i]
        if len(frames):
            Ji = rbd.rbd_terms(om, q[i], vi)["Jl"] if Jl is None else Jl[i]
            for k, f in enumerate(frames):
                out[i] -= Ji[f].T @ wrench[i, k]
    return out


def transcribed_spd(rbd, om, m, q, dq, targetpos, dt, frames=(), wrench=None):
    """cmd.hpp:10-38 line by line for one robot, floating_base = true; q, dq and targetpos over all nv dofs as robot->positions(joints) gives them
    (the base's entries meet zero gains).  mass_matrix, coriolis_gravity_forces and constraint_forces are the oracle's M, nle and sum J'w."""
    from inria_wbc_amd import forward_dynamics as fd
    stiffness, damping = fd.spd_gains(dt)
    ndofs = m.nv
    Kp = np.identity(ndofs)
    Kd = np.identity(ndofs)
    for i in range(ndofs):
        Kp[i, i] = stiffness
        Kd[i, i] = damping
    if m.floating_base:
        for i in range(6):
            Kp[i, i] = 0
            Kd[i, i] = 0
    terms = rbd.rbd_terms(om, q, dq)
    fc = np.zeros(ndofs)
    for k, f in enumerate(frames):
        fc += terms["Jl"][f].T @ wrench[k]
    pos = np.zeros(ndofs)
    pos[ndofs - m.na:] = q[m.nq - m.na:]
    invM = np.linalg.inv(terms["M"] + Kd * dt)
    p = -Kp @ (pos + dq * dt - targetpos)
    d = -Kd @ dq
    qddot = invM @ (-terms["nle"] + p + d + fc)
    commands = p + d - Kd @ qddot * dt
    return commands


@pytest.mark.parametrize("name", list(MODELS))
def test_mass_matrix_statement_against_the_oracle(name):
    from inria_wbc_amd import forward_dynamics as fd
    from oracle import rbd
    m = MODELS[name]()
    om = rbd.OracleModel(m)
    q, v, _ = states(m, 52_000)
    got = fd.mass_matrix(m, q)
    want = np.stack([rbd.rbd_terms(om, q[i], v[i])["M"] for i in range(q.shape[0])])
    e = rel_err(got, want)
    print("forward_dynamics.mass_matrix against the oracle, %s: %.1e (|M| up to %.3g)" % (m.name, e, np.abs(want).max()))
    assert got.shape == (q.shape[0], m.nv, m.nv) and e <= TOL_ROWS
    assert np.array_equal(got, got.transpose(0, 2, 1))


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_force_space_round_trip(name):
    from inria_wbc_amd import forward_dynamics as fd
    from oracle import rbd
    m, st, tm = CASES[name]()
    om = rbd.OracleModel(m)
    q, v, tau = case_states(m, tm, N_ROUND, 53_000)
    frames = [2, 3]
    w = 50.0 * np.random.default_rng(53_500).standard_normal((N_ROUND, 2, 6))
    worst = 0.0
    for damping in (None, np.linspace(0.0, 0.2, m.nv)):
        a, info = fd.forward_dynamics(m, q, v, tau, frames, w, damping)
        assert (info == 0).all()
        back = oracle_round_trip(rbd, om, m, q, v, a, frames, w, damping)
        worst = max(worst, rel_err(back, tau))
    print("force-space round trip of the statement, %s: %.1e (|tau| up to %.3g, |a| up to %.3g)" % (name, worst, np.abs(tau).max(), np.abs(a).max()))
    assert worst <= TOL_ROWS


def test_a_pivot_that_is_not_positive_is_reported():
    from inria_wbc_amd import forward_dynamics as fd
    A = np.diag([2.0, 3.0, -1.0, 4.0])
    x, info = fd.cholesky_solve(A, np.ones(4))
    assert info == 3 and np.isnan(x).all()
    A[2, 2] = np.nan
    assert fd.cholesky_solve(A, np.ones(4))[1] == 3
    x, info = fd.cholesky_solve(np.array([[4.0, 2.0], [2.0, 3.0]]), np.array([2.0, 1.0]))
    assert info == 0 and np.allclose(x, np.linalg.solve([[4.0, 2.0], [2.0, 3.0]], [2.0, 1.0]), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", ["talos", "tree_24_floating", "franka"])
def test_spd_commands_against_the_transcribed_reference(name):
    from inria_wbc_amd import forward_dynamics as fd
    from oracle import rbd
    m, st, tm = CASES[name]()
    om = rbd.OracleModel(m)
    n = 6
    q, v, _ = case_states(m, tm, n, 54_000)
    target = q[:, m.nq - m.na:] + 0.05 * np.random.default_rng(54_500).standard_normal((n, m.na))
    frames = [2, 3]
    w = 50.0 * np.random.default_rng(54_600).standard_normal((n, 2, 6))
    got = fd.spd_commands(m, q, v, target, DT, frames=frames, wrench=w)
    full = np.zeros((n, m.nv))
    full[:, m.nv - m.na:] = target
    want = np.stack([transcribed_spd(rbd, om, m, q[i], v[i], full[i], DT, frames, w[i]) for i in range(n)])
    e = float(np.abs(got["commands"] - want).max() / np.abs(want).max())
    print("forward_dynamics.spd_commands against cmd.hpp transcribed, %s: %.1e (|commands| up to %.3g)" % (name, e, np.abs(want).max()))
    assert (got["info"] == 0).all() and e <= TOL_ROWS
    if m.floating_base:
        assert np.abs(got["commands"][:, :6]).max() == 0.0  # no gains on the base: no command there
    kp, kd = fd.spd_gains(DT)
    assert kp.dtype == np.float32 and kd.dtype == np.float32 and float(kp) == 10000.0 and float(kd) == 100.0
    assert fd.spd_gains(0.003)[0] == np.float32(10000 / 3.0)
    # a q array serves as the target: no position error, the commands are the damping's and the bias's alone
    wide = fd.spd_commands(m, q, v, q[:, m.nq - m.na:], DT)
    assert np.array_equal(wide["commands"], fd.spd_commands(m, q, v, np.concatenate([q[:, m.nq - m.na:], np.full((n, 5), np.nan)], axis=1), DT)["commands"])


def test_symbols_declared_exported_bound_and_null_handle(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    new = {"wbcqp_mass_matrix", "wbcqp_mass_matrix_host", "wbcqp_forward_dynamics", "wbcqp_forward_dynamics_host", "wbcqp_spd_commands",
           "wbcqp_spd_commands_host"}
    assert new <= declared and new <= set(capi.EXPORTS)
    assert re.search(r"#define\s+WBCQP_VERSION\s+151\b", hdr)
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in new:
        assert hasattr(raw, sym), sym
        assert getattr(lib, sym).argtypes, sym
    assert raw.wbcqp_version() == 151
    for name in ("mass_matrix", "mass_matrix_host", "forward_dynamics", "forward_dynamics_host", "spd_commands", "spd_commands_host"):
        assert callable(getattr(capi.Handle, name))
    # a NULL handle is refused before anything else is looked at
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    law = capi.CSpd(0.001, 10000.0, 100.0)
    assert lib.wbcqp_mass_matrix(None, 0, 1, p, p, None) == ERR_INVALID
    assert lib.wbcqp_mass_matrix_host(None, 0, 1, p, p) == ERR_INVALID
    assert lib.wbcqp_forward_dynamics(None, 0, 1, p, p, p, 8, None, None, p, None, None) == ERR_INVALID
    assert lib.wbcqp_forward_dynamics_host(None, 0, 1, p, p, p, 8, None, None, p, None) == ERR_INVALID
    assert lib.wbcqp_spd_commands(None, 0, 1, ctypes.byref(law), p, p, p, 8, None, p, None, None, None) == ERR_INVALID
    assert lib.wbcqp_spd_commands_host(None, 0, 1, ctypes.byref(law), p, p, p, 8, None, p, None, None) == ERR_INVALID


def test_algorithmic_bytes():
    from inria_wbc_amd import forward_dynamics as fd
    m = mdl.talos_like()
    assert fd.algorithmic_bytes(m, "mass_matrix") == (m.nq + m.nv * m.nv) * 8
    assert fd.algorithmic_bytes(m, "forward_dynamics", n_frames=2) == (m.nq + 3 * m.nv + 12) * 8 + 4
    assert fd.algorithmic_bytes(m, "spd_commands", itemsize=4) == (m.nq + 3 * m.nv + m.na) * 4 + 4
    with pytest.raises(ValueError):
        fd.algorithmic_bytes(m, "other")
