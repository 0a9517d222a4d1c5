"""CPU tests of the exact statement of the rigid-body terms (tests/rbd_exact.py): the committed fixtures are what the statement gives, the statement
meets the identities of rigid bodies to the accuracy of its own differences, and the C oracle (oracle/rbd_oracle.c: rbd_terms, rnea) and the numpy
statements (inria_wbc_amd/observe.py, jacobians.py, dynamics.py, forward_dynamics.py) agree with it ENTRY BY ENTRY: ratio = |x - value| / (eps scale),
structural zeros exact.  No GPU.

K_ORACLE[quantity] (tests/rbd_exact_cases.py) is the worst ratio of any of those CPU implementations over all seven cases, as measured: the K of the device's bar
4 K_ORACLE eps scale in tests/test_gpu_rbd_exact.py.  Sanity condition: under 256 for every quantity (fifty bodies times a chain of about ten
operations is the most a sound double-precision recursion loses).

The last test is the proof that the entrywise bar sees what the norm-wise one (1e-10 max(1, largest entry)) does not: three small errors
in the inertia table of Talos's six lightest links, handed to the oracle, move M by 3e-10 to 2e-8 norm-wise -- over that bar by a factor of 3 to
300 -- and miss the entrywise one by more than a factor of 1e6 in the row of M of every one of those links."""
import copy
import os

import numpy as np
import pytest

from tests import rbd_exact as X
from tests.rbd_exact_cases import K_ORACLE

FULL = os.environ.get("WBCQP_RBD_EXACT_FULL") == "1"
TOL_ROWS = 1e-10  # the norm-wise bar the entrywise ones sit next to

_seen = {}  # quantity -> worst ratio of this run, per case


def implementations(name):
    """impl -> quantity -> [states, ...]: what the oracle and the numpy statements give for the fixture's inputs."""
    from inria_wbc_amd import dynamics, forward_dynamics, jacobians, observe
    from oracle import rbd
    C, m = X.load(name), X.model(name)
    q, v, a, w, wf = (C["in." + k] for k in ("q", "v", "a", "wrench", "wrench_frames"))
    n, frames = q.shape[0], list(range(m.nframe))
    om = rbd.OracleModel(m)
    T = [rbd.rbd_terms(om, q[i], v[i]) for i in range(n)]
    st = lambda k: np.stack([t[k] for t in T])  # noqa: E731
    tau_a = np.stack([rbd.rnea(om, q[i], v[i], a[i]) for i in range(n)])
    oracle = dict(M=st("M"), nle=st("nle"), com=st("com"), vcom=st("vcom"), acom=st("acom"), Jcom=st("Jcom"), Ag=st("Ag"), dAgv=st("dAgv"),
                  placement=st("oMf"), velocity=st("vf"), drift_local=st("af"), J_local=st("Jl"), J_world=st("Jw"), tau_a=tau_a,
                  tau_aw=tau_a - np.einsum("nkij,nki->nj", st("Jl")[:, wf], w), Agv=np.einsum("nij,nj->ni", st("Ag"), v))
    seen = observe.observe(m, q, v, frames, acom=True)
    J = {rf: jacobians.jacobians(m, q, v, frames, rf) for rf in (jacobians.WORLD, jacobians.LOCAL, jacobians.LOCAL_WORLD_ALIGNED)}
    L = J[jacobians.LOCAL]
    numpy_ = dict(M=forward_dynamics.mass_matrix(m, q), nle=dynamics.inverse_dynamics(m, q, v), tau_a=dynamics.inverse_dynamics(m, q, v, a),
                  tau_aw=dynamics.inverse_dynamics(m, q, v, a, wf, w), com=seen["com"], vcom=seen["vcom"], acom=seen["acom"],
                  placement=seen["placement"], velocity=seen["velocity"], J_world=J[jacobians.WORLD]["J"], J_local=L["J"],
                  J_lwa=J[jacobians.LOCAL_WORLD_ALIGNED]["J"], drift_local=L["drift"], drift_lwa=J[jacobians.LOCAL_WORLD_ALIGNED]["drift"],
                  Jcom=L["Jcom"], Ag=L["Ag"], dAgv=L["dAgv"], Agv=np.einsum("nij,nj->ni", L["Ag"], v))
    return {"oracle": oracle, "numpy": numpy_}


@pytest.mark.parametrize("name", list(X.CASES))
def test_fixture_is_what_the_statement_gives(name):
    if name in X.FULL_ONLY and not FULL:
        pytest.skip("recomputing %s takes a few seconds more than the small cases together: set WBCQP_RBD_EXACT_FULL=1" % name)
    got, want = X.computed(name), X.load(name)
    assert set(got) - set(X.CHECKS) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (name, k)
    # the statement's own identities, for every state it was just computed for (with the env var: all seven cases)
    assert got["check.M_asymmetry"].max() <= 1e-40, got["check.M_asymmetry"]      # both triangles are summed on their own
    assert got["check.Agv_identity"].max() <= 1e-25, got["check.Agv_identity"]  # (Ag of the first derivatives) v = the bodies' momenta on the curve


def test_fixtures_hold_values_and_scales_only():
    for name in X.CASES:
        C = X.load(name)
        names = set(X.QUANTITIES)
        origins = {k + ".scale_" + o for k in names - set(X.NO_ORIGIN) for o in X.ORIGINS}
        allowed = names | {k + ".scale" for k in names} | {k + ".scale_total" for k in X.TOTALS} | origins | {
            "in." + k for k in ("q", "v", "a", "wrench", "wrench_frames")}
        assert set(C) == allowed, set(C) ^ allowed
        assert C["in.q"].shape[0] == X.CASES[name][1]
        for k in names:
            assert C[k].shape == C[k + ".scale"].shape and np.isfinite(C[k]).all() and (C[k + ".scale"] >= 0).all()
            assert (C[k][C[k + ".scale"] == 0.0] == 0.0).all()
        for k in names - set(X.NO_ORIGIN):  # levers split at a common origin sum no less; the two origins are one for a fixed base
            assert (C[k + ".scale_world"] >= C[k + ".scale_base"]).all() and (C[k + ".scale_base"] >= C[k + ".scale"]).all(), k
            assert X.model(name).floating_base or np.array_equal(C[k + ".scale_world"], C[k + ".scale_base"]), k
        for k in X.TOTALS:  # a running total of the whole robot sums no less than the subtree alone ... where there is anything to sum
            assert C[k + ".scale_total"].shape == C[k].shape and (C[k + ".scale_total"] > 0).all()
        assert os.path.getsize(X.path(name)) < (1 << 20)


@pytest.mark.parametrize("name", ["one_revolute_fixed", "light_leaf_12_floating"])
def test_halving_the_step_moves_nothing(name):
    worst = X.check_steps(name)  # (asserts 1e-25 itself)
    print("halving the step, %-26s largest move over scale %.1e" % (name, worst))


@pytest.mark.parametrize("name", X.SMALL)
def test_the_statement_holds_itself_to_physics(name):
    """The energy identity (M's symmetry and the momentum identity: with the fixtures' recomputation, above)."""
    n = X.CASES[name][1]
    exact = [X.energy_identity(name, i) for i in range(n)]
    as_given = [X.energy_identity(name, i, exact_rotations=False) for i in range(n)]
    print("v' nle(g = 0) = v' M_dot v / 2, %-26s exact rotations %.1e, the tables' own %.1e" % (name, max(exact), max(as_given)))
    assert max(exact) <= 1e-25, exact
    assert max(as_given) <= 1e-20, as_given  # (the tables' rotations are orthogonal to 1e-16: the defect enters squared, and no further down)


@pytest.mark.parametrize("name", list(X.CASES))
def test_oracle_ratio(name):
    C = X.load(name)
    worst = {}
    for impl, got in implementations(name).items():
        for k, x in got.items():
            r = X.ratios(x, C[k], C[k + ".scale"])
            assert np.isfinite(r).all(), (name, impl, k, "a structural zero is not an exact zero", np.argwhere(~np.isfinite(r))[:4].tolist())
            worst[(impl, k)] = float(r.max())
    for impl in ("oracle", "numpy"):
        print("ratio to the statement, %-26s %-6s %s" % (name, impl, "  ".join("%s %.3g" % (k, worst[(impl, k)]) for k in X.QUANTITIES if (impl, k) in worst)))
    per = {k: max(w for (_, kk), w in worst.items() if kk == k) for k in X.QUANTITIES}
    _seen[name] = per
    if len(_seen) == len(X.CASES):
        print("K_ORACLE measured: %s" % {k: float("%.3g" % max(p[k] for p in _seen.values())) for k in X.QUANTITIES})
    for k, w in per.items():
        assert w <= K_ORACLE[k], (name, k, w, K_ORACLE[k])


def test_k_oracle_is_sane():
    assert all(0.0 < K < 256.0 for K in K_ORACLE.values()), K_ORACLE


def test_structural_zeros_are_counted():
    """The zeros the tree's structure puts into M and the Jacobians are there to be checked (Talos: the limbs do not move one another)."""
    C = X.load("talos")
    nz = int((C["M.scale"][0] == 0.0).sum())
    print("structural zeros of Talos's M: %d of %d" % (nz, C["M"][0].size))
    assert nz == 1428 and (C["J_local.scale"] == 0.0).any()
    # 12 of them are no unrelated branches but zero levers (a leaf whose CoM lies on its own joint's origin, against the base's translations):
    # exact zeros for a body-local recursion, the origin's levers times eps for one about a common origin
    assert int((C["M.scale_base"][0] == 0.0).sum()) == 1416


MUTATIONS = {
    "rotational inertia x 1.001": lambda Y, b: Y.__setitem__((b, slice(4, 10)), Y[b, 4:10] * 1.001),
    "products of inertia dropped": lambda Y, b: Y.__setitem__((b, [5, 6, 8]), 0.0),
    "CoM x 1.0001": lambda Y, b: Y.__setitem__((b, slice(1, 4)), Y[b, 1:4] * 1.0001),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_small_error_in_the_lightest_links_is_seen(what):
    from oracle import rbd
    C, m = X.load("talos"), X.model("talos")
    light = np.argsort(m.inertia[:, 0])[:6]
    dofs = [m.idx_v(int(b)) for b in light]
    wrong = copy.deepcopy(m)
    for b in light:
        MUTATIONS[what](wrong.inertia, int(b))
    assert not np.array_equal(wrong.inertia, m.inertia)
    om = rbd.OracleModel(wrong)
    q, v = C["in.q"], C["in.v"]
    M = np.stack([rbd.rbd_terms(om, q[i], v[i])["M"] for i in range(q.shape[0])])
    normwise = float(np.abs(M - C["M"]).max() / max(1.0, np.abs(C["M"]).max()))
    r = X.ratios(M, C["M"], C["M.scale"])
    on_the_links = float(min(r[:, j, :].max() for j in dofs)) / K_ORACLE["M"]
    allowed = TOL_ROWS * max(1.0, np.abs(C["M"]).max()) / np.abs(C["M"][0][dofs, dofs]).min()
    print("%-28s norm-wise %.1e (bar %.0e), entrywise over the bar on every one of the six links' rows of M by at least %.1e; the norm-wise "
          "bar allows %.1e relative there" % (what, normwise, TOL_ROWS, on_the_links, allowed))
    assert on_the_links >= 1e6  # (the norm-wise bar sees these three with a factor of 3 to 300 to spare, and nothing ten times subtler)
