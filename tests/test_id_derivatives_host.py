"""CPU tests of the inverse dynamics' derivatives (wbcqp_inverse_dynamics_derivatives): the numpy statement inria_wbc_amd/id_derivatives.py
against the committed 80-digit truth (tests/id_derivatives_exact.py, tests/golden/id_derivatives/), against central differences of the C oracle's
rnea (independent code), the identities that tie it to inria_wbc_amd/dynamics.py, its zero pattern, and the library's surface.  No GPU.

Bars.  Against the truth: K_STATEMENT (tests/id_derivatives_cases.py says how it was measured).  Against the oracle's central differences: twice
what those differences themselves leave against the truth on the same case, computed here -- at h = 1e-5 they carry h^2 |tau'''| / 6 of
truncation and eps |tau| / h of rounding, about 1e-10, and the statement cannot be told from the truth at that level.  The two identities compare
two float64 formulations: TOL_ROWS (1e-10) of tests/test_inverse_dynamics_host.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import id_derivatives_cases as IC
from tests import rbd_exact_cases as RC
from tests.test_inverse_dynamics_host import ERR_INVALID, TOL_ROWS, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wbcqp_inverse_dynamics_derivatives", "wbcqp_inverse_dynamics_derivatives_host"}
STEP = 1e-5


def inputs(name):
    C = IC.load(name)
    return RC.model(name), C["in.q"], C["in.v"], C["in.a"], C["in.wrench"], [int(f) for f in C["in.wrench_frames"]]


def statement(name, **kw):
    from inria_wbc_amd import id_derivatives as idd
    m, q, v, a, w, wf = inputs(name)
    return idd.derivatives(m, q, v, a, wf, w, **kw)


def test_fixtures_are_the_cases():
    """The fixtures hold the inputs of tests/rbd_exact_cases.py, and the truth's own tau is the committed exact tau_aw of tests/golden/rbd_exact/:
    the lean d'Alembert statement the derivatives difference IS that module's."""
    for name in IC.CASES:
        C, n = IC.load(name), IC.N_STATES[name]
        s, exact = RC.states(name), RC.load(name)
        for k in ("q", "v", "a", "wrench"):
            assert np.array_equal(C["in." + k], s[k][:n]), (name, k)
        assert list(C["in.wrench_frames"]) == RC.wrench_frames(name)
        nv = RC.model(name).nv
        assert C["dtau_dq"].shape == C["dtau_dv"].shape == (n, nv, nv)
        assert np.array_equal(C["tau"], exact["tau_aw"][:n]), name  # (both are the 80-digit value rounded to float64 once)


def test_statement_against_truth():
    """inria_wbc_amd/id_derivatives.py against the truth, every case: the worst error is K_STATEMENT."""
    worst = {}
    for name in IC.CASES:
        C = IC.load(name)
        worst[name] = IC.worst_error(statement(name), C)
        print("id_derivatives.py against the truth, %-26s %.3e" % (name, worst[name]))
    print("K_STATEMENT measured %.3e (written: %.3e)" % (max(worst.values()), IC.K_STATEMENT))
    assert max(worst.values()) <= IC.K_STATEMENT, worst


@pytest.mark.parametrize("name", IC.CASES)
def test_statement_against_central_differences_of_the_oracle(name):
    """dtau/dq against (tau(q (+) h e_j) - tau(q (+) -h e_j)) / 2h of the C oracle's rnea minus its LOCAL Jacobians' transposes times the
    wrenches, (+) the oracle's own integration: at twice what the differences leave against the truth."""
    from oracle import oracle as orc
    from oracle import rbd
    m, q, v, a, w, wf = inputs(name)
    om = rbd.OracleModel(m)
    n, nv = q.shape[0], m.nv

    def tau(qq):
        out = np.zeros((n, nv))
        for i in range(n):
            Jl = rbd.rbd_terms(om, qq[i], v[i])["Jl"]
            out[i] = rbd.rnea(om, qq[i], v[i], a[i]) - sum(Jl[f].T @ w[i, k] for k, f in enumerate(wf))
        return out

    fd, zero = np.zeros((n, nv, nv)), np.zeros((n, nv))
    for j in range(nv):
        e = np.zeros((n, nv))
        e[:, j] = 1.0
        plus = orc.integrate(m.floating_base, STEP, q, e, zero)["q_next"]
        minus = orc.integrate(m.floating_base, -STEP, q, e, zero)["q_next"]
        fd[:, :, j] = (tau(plus) - tau(minus)) / (2 * STEP)
    C = IC.load(name)
    got = statement(name, which=["dtau_dq"])["dtau_dq"]
    for i in range(n):
        left = IC.error(fd[i], C["dtau_dq"][i])  # what the differences themselves leave
        gap = IC.error(got[i], fd[i])
        print("central differences of the oracle, %-26s state %d: differences against the truth %.2e, statement against differences %.2e" %
              (name, i, left, gap))
        assert 0.0 < left < 1e-6 and gap <= 2.0 * left, (name, i, left, gap)


@pytest.mark.parametrize("name", IC.CASES)
def test_velocity_identity(name):
    """tau is quadratic in v, so dtau_dv d = (tau(v + d) - tau(v - d)) / 2 exactly, for any d."""
    from inria_wbc_amd import dynamics
    m, q, v, a, w, wf = inputs(name)
    d = np.random.default_rng(31_000).standard_normal(v.shape)
    want = (dynamics.inverse_dynamics(m, q, v + d, a, wf, w) - dynamics.inverse_dynamics(m, q, v - d, a, wf, w)) / 2
    got = np.einsum("bij,bj->bi", statement(name, which=["dtau_dv"])["dtau_dv"], d)
    if m.nv > 1:  # (one revolute body on a fixed base: both sides are zero)
        assert np.abs(want).max() > 1e-3
    assert np.abs(got - want).max() <= TOL_ROWS * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("name", IC.CASES)
def test_dtau_dq_is_affine_in_a(name):
    """dtau_dq(a) - dtau_dq(a = 0) = d(M a)/dq is linear in a."""
    from inria_wbc_amd import id_derivatives as idd
    m, q, v, a, w, wf = inputs(name)
    rng = np.random.default_rng(32_000)
    a2, s, t = rng.standard_normal(a.shape), 0.7, -1.9
    f = lambda acc: idd.derivatives(m, q, v, acc, wf, w, which=["dtau_dq"])["dtau_dq"]  # noqa: E731
    base = f(None)
    assert np.array_equal(base, f(np.zeros_like(a)))
    lin = lambda acc: f(acc) - base  # noqa: E731
    assert rel_err(lin(s * a + t * a2), s * lin(a) + t * lin(a2)) <= TOL_ROWS
    if m.nv > 1:  # (one revolute body: M is a constant)
        assert np.abs(lin(a)).max() > 1e-3
    # a is read through its first nv columns
    wide = np.concatenate([a, np.full((a.shape[0], 13), np.nan)], axis=1)
    assert np.array_equal(f(wide), f(a))


@pytest.mark.parametrize("name", IC.CASES)
def test_zero_pattern(name):
    """Both matrices, the statement's and the truth's, are +0.0 outside structure_mask, which is the zero pattern of M, and in columns 0..2 of
    dtau_dq on a floating base."""
    from inria_wbc_amd import forward_dynamics as fdn
    from inria_wbc_amd import id_derivatives as idd
    m, q, v, a, w, wf = inputs(name)
    mask = idd.structure_mask(m)
    M = fdn.mass_matrix(m, q)
    assert (M[:, ~mask] == 0.0).all()
    if name != "talos":  # (the shipped robot's axis-aligned geometry leaves exact zeros inside the pattern as well)
        assert np.array_equal((M != 0.0).any(axis=0), mask)
    got, C = statement(name), IC.load(name)
    for k in IC.MATRICES:
        for x in (got[k], C[k]):
            off = x[:, ~mask]
            assert (off == 0.0).all() and not np.signbit(off).any(), (name, k)
    if m.floating_base:
        for x in (got["dtau_dq"], C["dtau_dq"]):
            assert (x[:, :, :3] == 0.0).all() and not np.signbit(x[:, :, :3]).any()
        assert (~mask).any()  # (the zero check had entries to look at)
    if name in ("star_9_floating", "light_leaf_12_floating"):  # (random geometry: next to nothing else is zero)
        inside = np.broadcast_to(mask, got["dtau_dq"].shape).copy()
        inside[:, :, :3] = False
        for k in IC.MATRICES:
            assert (got[k][inside] != 0.0).mean() > 0.95 and (C[k][inside] != 0.0).mean() > 0.95, (name, k)


def test_velocity_terms_vanish_without_v():
    """v None is v = 0, and the gravity stiffness dg/dq is dtau_dq at v = a = 0 without wrenches."""
    from inria_wbc_amd import id_derivatives as idd
    m, q, v, a, w, wf = inputs("light_leaf_12_floating")
    assert np.array_equal(idd.derivatives(m, q, None, a, wf, w)["dtau_dq"], idd.derivatives(m, q, np.zeros_like(v), a, wf, w, which=["dtau_dq"])["dtau_dq"])
    assert set(idd.derivatives(m, q)) == {"dtau_dq"} and set(idd.derivatives(m, q, v)) == {"dtau_dq", "dtau_dv"}
    with pytest.raises(ValueError):
        idd.derivatives(m, q, None, a, which=["dtau_dv"])  # dtau_dv without v
    with pytest.raises(ValueError):
        idd.derivatives(m, q, v, a, which=[])              # nothing asked for
    with pytest.raises(ValueError):
        idd.derivatives(m, q, v, a, which=["M"])           # not an output of this call


def test_symbols_declared_exported_bound_and_null_handle(built_lib, tmp_path):
    from inria_wbc_amd import capi
    from tests.test_capi_binding import layout_mismatches
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(capi.EXPORTS) and NEW <= set(capi.SIGNATURES)
    assert re.search(r"#define\s+WBCQP_VERSION\s+151\b", hdr)
    assert re.search(r"typedef struct \{\s*void \*dtau_dq, \*dtau_dv;\s*\} wbcqp_id_derivative_outputs;", hdr)
    assert capi.ID_DERIVATIVE_OUTPUTS == ("dtau_dq", "dtau_dv")
    assert [k for k, _ in capi.CIdDerivativeOutputs._fields_] == list(capi.ID_DERIVATIVE_OUTPUTS)
    assert layout_mismatches({"CIdDerivativeOutputs": capi.CIdDerivativeOutputs}, tmp_path) == []  # size and offsets against the header's struct
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in NEW:
        assert hasattr(raw, sym), sym
        assert getattr(lib, sym).argtypes, sym
    assert raw.wbcqp_version() == 151
    for name in ("inverse_dynamics_derivatives", "inverse_dynamics_derivatives_host"):
        assert callable(getattr(capi.Handle, name))
    # a NULL handle is refused before anything else is looked at
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    out = capi.CIdDerivativeOutputs(p, None)
    assert lib.wbcqp_inverse_dynamics_derivatives(None, 0, 1, p, None, None, 0, None, ctypes.byref(out), None) == ERR_INVALID
    assert lib.wbcqp_inverse_dynamics_derivatives_host(None, 0, 1, p, None, None, 0, None, ctypes.byref(out)) == ERR_INVALID


def test_algorithmic_bytes():
    from inria_wbc_amd import id_derivatives as idd
    from inria_wbc_amd import model as mdl
    m = mdl.talos_like()
    nq, nv = m.nq, m.nv
    assert idd.algorithmic_bytes(m, 2) == (nq + 2 * nv + 12 + 2 * nv * nv) * 8
    assert idd.algorithmic_bytes(m, 0, ("dtau_dq",), itemsize=4) == (nq + 2 * nv + nv * nv) * 4
    with pytest.raises(ValueError):
        idd.algorithmic_bytes(m, 2, ("M",))
