"""CPU tests of the exact statement of the rigid-body terms (tests/rbd_exact.py): the committed fixtures are what the statement gives, the statement
meets the identities of rigid bodies to the accuracy of its own differences, and the C oracle (oracle/rbd_oracle.c: rbd_terms, rnea) and the numpy
statements (inria_wbc_amd/observe.py, jacobians.py, dynamics.py, forward_dynamics.py) agree with it ENTRY BY ENTRY: ratio = |x - value| / (eps scale),
structural zeros exact.  No GPU.

K_ORACLE[quantity] (tests/rbd_exact_cases.py) is the worst ratio of any of those CPU implementations over all seven cases, as measured: the K of the device's bar
4 K_ORACLE eps scale in tests/test_gpu_rbd_exact.py.  Sanity condition: under 256 for every quantity (fifty bodies times a chain of about ten
operations is the most a sound double-precision recursion loses).

The second-order kinematics (H = dJ/dq and dJ/dt in the three conventions, fixtures <case>.hessians.npz) are held in the same way: the fixtures
are what the statement gives, either step of the nested difference halved moves nothing, the statement meets its own identities
(rbd_exact.second_order_identities), its structural zeros -- decided from its values -- are those of inria_wbc_amd/hessians.py's structure_masks,
and hessians.py agrees with it entry by entry: that ratio is their K_ORACLE, for no C oracle exists for them.

The last test is the proof that the entrywise bar sees what the norm-wise one (1e-10 max(1, largest entry)) does not: three small errors
in the inertia table of Talos's six lightest links, handed to the oracle, move M by 3e-10 to 2e-8 norm-wise -- over that bar by a factor of 3 to
300 -- and miss the entrywise one by more than a factor of 1e6 in the row of M of every one of those links."""
import copy
import os

import numpy as np
import pytest

from tests import rbd_exact as X
from tests.rbd_exact_cases import K_ORACLE

CONVENTION_OF = {"world": 0, "local": 1, "lwa": 2}  # wbcqp_reference_frame (jacobians.WORLD, LOCAL, LOCAL_WORLD_ALIGNED)

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


def second_order_implementation(name):
    """quantity -> [states, frames, ...]: what inria_wbc_amd/hessians.py gives for the fixture's inputs.  No C oracle exists for these six."""
    from inria_wbc_amd import hessians
    C, S, m = X.load(name), X.load_hessians(name), X.model(name)
    got = {}
    for c, rf in CONVENTION_OF.items():
        r = hessians.hessians(m, C["in.q"], C["in.v"], [int(f) for f in S["in.hessian_frames"]], rf)
        got["H_" + c], got["dJ_" + c] = r["H"], r["dJ"]
    return got


def masks(name):
    """H_<c> -> [frames, 6, nv, nv] bool: hessians.structure_masks, row by row."""
    from inria_wbc_amd import hessians
    frames = [int(f) for f in X.load_hessians(name)["in.hessian_frames"]]
    out = {}
    for c, rf in CONVENTION_OF.items():
        lin, ang = hessians.structure_masks(X.model(name), frames, rf)
        out["H_" + c] = np.concatenate([np.repeat(lin[:, None], 3, axis=1), np.repeat(ang[:, None], 3, axis=1)], axis=1)
    return out


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


@pytest.mark.parametrize("name", list(X.CASES))
def test_second_order_fixture_is_what_the_statement_gives(name):
    if name in X.FULL_ONLY and not FULL:
        pytest.skip("recomputing %s takes a minute: set WBCQP_RBD_EXACT_FULL=1" % name)
    got, want = X.computed_hessians(name), X.load_hessians(name)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (name, k)


def _largest_fixture_before():
    root = os.path.dirname(X.GOLDEN)
    sizes = [os.path.getsize(os.path.join(d, f)) for d, _, files in os.walk(root) for f in files if not f.endswith(".hessians.npz")]
    return max(sizes)


def test_second_order_fixtures_hold_values_and_scales_only():
    limit = _largest_fixture_before()
    for name in X.CASES:
        C, S, m = X.load(name), X.load_hessians(name), X.model(name)
        frames = [int(f) for f in S["in.hessian_frames"]]
        assert frames == X.hessian_frames(name)
        assert set(S) == {k + e for k in X.SECOND_ORDER for e in ("", ".scale", ".scale_world")} | {"in.hessian_frames"}
        n, nv = C["in.q"].shape[0], m.nv
        for k in X.SECOND_ORDER:
            assert S[k].shape == S[k + ".scale"].shape == S[k + ".scale_world"].shape == (n, len(frames), 6) + (nv,) * (2 if k in X.HESSIANS else 1)
            assert np.isfinite(S[k]).all() and (S[k + ".scale"] >= 0).all() and (S[k + ".scale_world"] >= 0).all()
            assert (S[k][S[k + ".scale"] == 0.0] == 0.0).all() and (np.abs(S[k]) <= S[k + ".scale"] * (1 + 1e-12)).all(), k
        for k in X.HESSIANS:  # levers split at the world's origin sum no less
            assert (S[k + ".scale_world"] >= S[k + ".scale"]).all(), k
        assert os.path.getsize(X.hessians_path(name)) <= limit, (name, os.path.getsize(X.hessians_path(name)), limit)
    # the small cases: every frame of the model; the root, a leaf and two frames on one body are among them
    for name in X.SMALL:
        m = X.model(name)
        assert X.hessian_frames(name) == list(range(m.nframe)) and m.frame_body[0] == 0 and m.frame_body[2] == m.frame_body[3]


def _magnitudes(name, c):
    """[states, frames, 6, nv, nv]: the motion cross product of two columns of the committed J_<c>.scale with every term added, in numpy: what the
    statement's H_<c>.scale is wherever it is not 0.  LOCAL_WORLD_ALIGNED: the one linear term the entry has (tests/rbd_exact.py, _second_order)."""
    from inria_wbc_amd import hessians
    frames = X.load_hessians(name)["in.hessian_frames"]
    J = X.load(name)["J_%s.scale" % c][:, frames]
    l, w = J[:, :, :3], J[:, :, 3:]
    lj, wj, lk, wk = l[..., :, None], w[..., :, None], l[..., None, :], w[..., None, :]

    def cmag(a, b):
        return np.stack([a[:, :, 1] * b[:, :, 2] + a[:, :, 2] * b[:, :, 1], a[:, :, 2] * b[:, :, 0] + a[:, :, 0] * b[:, :, 2],
                         a[:, :, 0] * b[:, :, 1] + a[:, :, 1] * b[:, :, 0]], axis=2)

    if c == "lwa":
        lin = np.where(hessians.precedes(X.model(name))[None, None, None], cmag(wk, lj), cmag(wj, lk))
    else:
        lin = cmag(wk, lj) + cmag(lk, wj)
    return np.concatenate([lin, cmag(wk, wj)], axis=2)


@pytest.mark.parametrize("name", list(X.CASES))
def test_the_zero_set_is_the_structure(name):
    """The statement decides its structural zeros from its own values (rbd_exact.dependence); hessians.structure_masks says the same: the scale is
    0 wherever the mask is False, and where the mask is True only where a factor's own scale is 0 (a prismatic dof's angular part, a zero lever)."""
    S, M = X.load_hessians(name), masks(name)
    for c in CONVENTION_OF:
        k = "H_" + c
        scale, mask = S[k + ".scale"], np.broadcast_to(M[k][None], S[k].shape)
        assert (scale[~mask] == 0.0).all() and (S[k + ".scale_world"][~mask] == 0.0).all(), (name, k)
        assert np.allclose(scale[mask], _magnitudes(name, c)[mask], rtol=1e-12, atol=0.0), (name, k)
        assert (S[k + ".scale_world"][mask] >= scale[mask]).all()
        # dJ: the sum over k of H's scale with |v_k|
        want = np.einsum("nfrjk,nk->nfrj", scale, np.abs(X.load(name)["in.v"]))
        assert np.allclose(S["dJ_%s.scale" % c], want, rtol=1e-12, atol=0.0), (name, c)
    print("structural zeros of H, %-26s %s" % (name, "  ".join("%s %d of %d (on the mask: %d)" % (
        k, int((S[k + ".scale"] == 0).sum()), S[k].size, int((S[k + ".scale"][np.broadcast_to(M[k][None], S[k].shape)] == 0).sum())) for k in X.HESSIANS)))


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


@pytest.mark.parametrize("name", ["one_revolute_fixed", "star_9_floating"])
def test_halving_either_step_moves_nothing_second_order(name):
    worst = X.check_steps_hessians(name)  # (asserts 1e-25 itself)
    print("halving either step, second order, %-26s largest move over scale %.1e" % (name, worst))


@pytest.mark.parametrize("name", X.SMALL)
def test_the_second_order_statement_holds_itself_to_its_identities(name):
    worst = {}
    for i in range(X.CASES[name][1]):
        for k, w in X.second_order_identities(name, i).items():
            worst[k] = max(worst.get(k, 0.0), w)
    print("second-order identities, %-26s %s" % (name, "  ".join("%s: %.1e" % kv for kv in worst.items())))
    assert {"H v = dJ, world", "H v = dJ, local", "H v = dJ, lwa", "dJ_lwa v = drift_lwa", "dJ_local v + (w x l, 0) = drift_local"} <= set(worst)
    assert X.model(name).nv == 1 or "H_world[j][k] - H_world[k][j] = J_k x_m J_j" in worst
    assert not X.model(name).floating_base or "H_world[j][k] - H_world[k][j] = 2 J_k x_m J_j" in worst
    assert max(worst.values()) <= 1e-25, worst


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
    # the six second-order quantities: hessians.py alone (no C oracle exists for them).  H against `scale`; dJ against `scale_world` -- the
    # statement forms it from partial sums of v_k J_k that hold dof j's own term, which cancels to rounding only -- with the ratio against `scale` beside it
    S, line = X.load_hessians(name), []
    for k, x in second_order_implementation(name).items():
        r = X.ratios(x, S[k], S[k + (".scale" if k in X.HESSIANS else ".scale_world")])
        assert np.isfinite(r).all(), (name, "hessians.py", k, "a structural zero is not an exact zero", np.argwhere(~np.isfinite(r))[:4].tolist())
        per[k] = float(r.max())
        line.append("%s %.3g" % (k, per[k]))
        if k in X.RATES:
            rl = X.ratios(x, S[k], S[k + ".scale"])
            line[-1] += " (against the local scale %.3g, not an exact zero where it is 0: %d)" % (float(rl[np.isfinite(rl)].max()) if np.isfinite(rl).any() else 0.0,
                                                                                             int((~np.isfinite(rl)).sum()))
    print("ratio to the statement, %-26s %-6s %s" % (name, "hessians.py", "  ".join(line)))
    _seen[name] = per
    if len(_seen) == len(X.CASES):
        print("K_ORACLE measured: %s" % {k: float("%.3g" % max(p[k] for p in _seen.values())) for k in X.QUANTITIES + X.SECOND_ORDER})
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


def test_a_small_error_in_the_small_entries_of_H_is_seen():
    """What the norm-wise bar of tests/test_gpu_hessians.py cannot see: Talos's H from hessians.py with every entry under 1e-3 of the array's largest
    off by 1e-7 of itself -- wrong in the seventh digit -- is within 1e-10 of the largest entry, and over the entrywise bar by a factor of 1e2 (LOCAL, whose magnitude sums grow with the depth of the chain) and more."""
    S = X.load_hessians("talos")
    got = second_order_implementation("talos")
    for k in X.HESSIANS:
        small = np.abs(S[k]) <= 1e-3 * np.abs(S[k]).max()
        assert (small & (S[k + ".scale"] > 0)).sum() > 20  # (there are such entries: a short lever, a frame near its joint's origin)
        wrong = np.where(small, got[k] * (1 + 1e-7), got[k])
        normwise = float(np.abs(wrong - S[k]).max() / max(1.0, np.abs(S[k]).max()))
        over = X.worst_ratio(wrong, S[k], S[k + ".scale"]) / (4 * K_ORACLE[k])
        print("%-8s entries under 1e-3 of the largest off by 1e-7: norm-wise %.1e (bar %.0e), entrywise over the bar by %.1e" % (k, normwise, TOL_ROWS, over))
        assert normwise <= TOL_ROWS and over >= 1e2, (k, normwise, over)


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
