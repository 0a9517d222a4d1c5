"""The rows' three piecewise task laws -- log3 in the SE(3) / contact law, computeAccLimits, the 5PL self-collision repulsor -- on every
branch, on the CPU: the inputs of tests/task_laws.py reach what they claim to reach, and the C oracle (oracle/rbd_oracle.c) meets the
high-precision statement there within the bar the device is held to (tests/test_gpu_task_laws.py):

    |x - ref| <= TOL_ROWS max(1, |ref|) + 4 S    per entry of b1, bc, blb, bub.

Measured figures: profiles/task_laws/INDEX.md."""
import collections

import numpy as np
import pytest

from tests import task_laws as tl

NAMES = ("talos", "franka", "tree")
NA = len(tl.ANGLES)


@pytest.fixture(scope="module")
def rbd(oracle_mod):
    from oracle import rbd as r
    return r


@pytest.fixture(scope="module", params=NAMES)
def case(request, rbd):
    return request.param, tl.case(request.param)


def _seen(C, lanes, still):
    return {C["combos"][(i, l[0], l[1])] for i in range(C["q"].shape[0]) if bool(C["still"][i]) == still for l in lanes}


def test_exact_log3_is_the_logarithm():
    """The statement's own logarithm against scipy's, on exp(theta a) formed at 50 digits, every angle and octant."""
    import mpmath as mp
    from scipy.spatial.transform import Rotation
    mp.mp.dps = tl.DPS
    for th in tl.ANGLES:
        for a in tl.OCTANTS:
            R = tl.exp3(th, a)
            w = np.array([float(x) for x in tl.exact_log3(R)])
            assert np.abs(w - th * a / np.linalg.norm(a)).max() <= 4e-16 * max(th, 1e-300) + 1e-30, (th, a, w)
            got = Rotation.from_matrix(np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])).as_rotvec()
            assert np.abs(got - w).max() <= 1e-12, (th, a)  # (scipy sees the matrix rounded to double: 1e-16 / (pi - theta) near pi)


def test_every_reference_is_finite_and_no_case_is_excluded(case):
    name, C = case
    B = C["q"].shape[0]
    L = dict(C["st"].field_lengths())
    for k, a in C["rows"].items():
        assert a.shape == (B, L[k]) and np.isfinite(a).all() and np.isfinite(C["S"][k]).all(), k
    assert set(C["rows"]) == {k for k in ("b1", "bc", "blb", "bub") if L[k]}
    assert C["still"].sum() == B // 2 and not C["v"][C["still"]].any()
    for i in np.where(C["still"])[0]:  # Kp log3 is the whole angular right-hand side there
        for l in C["lanes"]:
            assert not C["ref"][i, l[3] + 12:l[3] + 24].any()


def test_references_reach_every_angle_on_every_kind_of_lane(case):
    name, C = case
    every = set(range(tl.NCOMBO))
    angles = lambda seen: {c % NA for c in seen}
    near_pi = {o * NA + a for o in range(8) for a in tl.NEAR_PI}
    # the references hold the angle they claim: the exact logarithm of R_frame(q)' R_ref has that length (R_ref is rounded to double)
    import mpmath as mp
    Rf = [C["m"].frame_placements(C["q"][i])[0] for i in range(C["q"].shape[0])]
    for (i, kind, k), c in C["combos"].items():
        l = next(l for l in C["lanes"] if l[0] == kind and l[1] == k)
        Rr = C["ref"][i, l[3] + 3:l[3] + 12].reshape(3, 3).T
        E = Rf[i][l[2]].T @ Rr
        ang = float(mp.sqrt(sum(x * x for x in tl.exact_log3({(a, b): mp.mpf(float(E[a, b])) for a in range(3) for b in range(3)}))))
        assert abs(ang - tl.ANGLES[c % NA]) <= 1e-14, (i, kind, k, ang)
    if name == "talos":
        assert len(C["cont"]) == 2 and len(C["full"]) == 4 and len(C["part"]) == 3
        assert _seen(C, C["cont"], False) | _seen(C, C["cont"], True) == every           # a contact (bc)
        assert angles(_seen(C, C["cont"], False)) == angles(_seen(C, C["cont"], True)) == set(range(NA))
        assert _seen(C, C["full"], False) == _seen(C, C["full"], True) == every           # an SE(3) task with all six rows (b1)
        assert angles(_seen(C, C["part"], False)) == angles(_seen(C, C["part"], True)) == set(range(NA))  # a masked one
    else:
        six = [l for l in C["lanes"] if l[4] == 63]
        assert six
        assert angles(_seen(C, six, False)) == angles(_seen(C, six, True)) == set(range(NA))
        assert near_pi <= _seen(C, six, False) | _seen(C, six, True)  # the three sign selectors, both ways each
    if name == "tree":
        assert C["cont"] and C["part"]
        assert angles(_seen(C, C["part"], False)) == angles(_seen(C, C["part"], True)) == set(range(NA))


@pytest.mark.parametrize("name", ["talos", "tree"])  # (the Franka stack has no bounds task)
def test_joint_states_reach_every_combination_of_the_bounds_law(name, rbd):
    C = tl.case(name)
    m, tm = C["m"], C["tm"]
    assert tm.n_bound == m.na and not tl.case("franka")["tm"].n_bound
    seen = collections.Counter(d for row in C["decisions"] for d in row)
    missing = [d for d in tl.REACHABLE if d not in seen]
    assert not missing, missing
    print("%s: %d combinations of the eleven decisions, each at least %d times" % (name, len(seen), min(seen.values())))
    for d in sorted(seen, key=str):
        print("   %s  x %d" % ("".join("-" if x is None else str(int(x)) for x in d), seen[d]))
    # every inequality decided with a relative margin no rounding can cross
    margins = [g for row in C["margins"] for G in row for i, g in enumerate(G) if g is not None and i not in tl.EXACT]
    assert min(margins) > 1e-9, min(margins)
    print("smallest margin of an inequality: %.2e" % min(margins))
    qa, va = C["q"][:, m.nq - m.na:], C["v"][:, m.nv - m.na:]
    D = np.array([[tuple(-1 if x is None else int(x) for x in d) for d in row] for row in C["decisions"]])
    assert ((va == 0) & ~np.signbit(va)).any() and ((va == 0) & np.signbit(va)).any()              # dq = +0.0 and -0.0
    assert (qa == m.q_lb).any() and (qa == m.q_ub).any()                                           # on a limit exactly ...
    lo, hi = D[..., 2] == 0, D[..., 5] == 0
    assert lo.any() and hi.any() and (np.abs(C["rows"]["blb"][lo]) >= 1e6).any() and (D[..., 9][lo | hi] == 1).all()  # ... sentinel, then reconciled
    assert ((qa < m.q_lb) & (va < 0)).any() and ((qa > m.q_ub) & (va > 0)).any()                   # outside, moving outward
    assert (np.abs(va) > m.dq_max).any()                                                           # faster than dq_max
    assert ((D[..., 9] == 1) & (D[..., 10] == 1)).any() and ((D[..., 9] == 1) & (D[..., 10] == 0)).any()  # both reconciliations
    assert not ((D[..., 7] == 0) & (D[..., 8] == 0)).any()  # (both discriminants negative: impossible with q_min < q_max, see REACHABLE)


def test_self_collision_pairs_sit_at_every_distance():
    C = tl.case("tree")
    pop = np.array([[int((C["bands"][:, p] == b).sum()) for b in range(6)] for p in range(C["bands"].shape[1])])
    print("pairs per distance (rows: pairs; columns: %s):\n%s" % (", ".join(tl.BANDS), pop))
    assert (pop.sum(axis=0) >= 3).all(), pop          # every distance, on several pairs
    assert (pop[0] >= 1).all(), pop                   # and all six on the block that has ONE pair: its row is that pair's term alone
    assert len(C["tm"].blocks[[b.kind for b in C["tm"].blocks].index(tl.mdl.T_SELFCOLLISION)].avoided) == 1
    for i, p, b in C["aimed"]:                        # what was aimed at was hit
        assert C["bands"][i, p] == b


def test_sensitivity_stays_below_the_bar(case):
    """4 S < TOL_ROWS max(1, |ref|) everywhere but at the three angles next to pi: were it not so, the inputs would be ill-conditioned."""
    name, C = case
    exempt = {tl.REGIMES.index(g) for g in ("middle, top end", "near pi")}
    worst = collections.defaultdict(float)
    for k, r in C["rows"].items():
        ratio = 4.0 * C["S"][k] / (tl.TOL_ROWS * np.maximum(1.0, np.abs(r)))
        for g in np.unique(C["regime"][k]):
            sel = C["regime"][k] == g
            worst[tl.REGIMES[g]] = max(worst[tl.REGIMES[g]], float((C["S"][k] / np.maximum(1.0, np.abs(r)))[sel].max()))
            if g not in exempt:
                assert ratio[sel].max() < 1.0, (k, tl.REGIMES[g], ratio[sel].max())
    for g in tl.REGIMES:
        if g in worst:
            print("%-8s S / max(1, |ref|)  %-18s %.2e" % (name, g, worst[g]))


def test_oracle_meets_the_statement(case, rbd):
    name, C = case
    ora = rbd.task_rows(C["m"], C["tm"], C["st"], C["q"], C["v"], C["ref"], n_threads=4)
    tl.report(name + ", C oracle", tl.worst_per_regime(C, ora))
    for k, r in C["rows"].items():
        bad = np.argwhere(np.abs(ora[k] - r) > tl.bar(r, C["S"][k]))
        assert bad.size == 0, (k, bad[:5], [(ora[k][tuple(b)], r[tuple(b)]) for b in bad[:5]])


def test_log3_formulas_through_the_bar_at_the_low_end():
    """Float64 models of log3's middle branch through the same bar at theta = 1.3e-4, in the still rows (scale 1), under each stack's largest
    Kp: theta(acos) / |w| (the kernel's before the series), theta / sin(theta) / 2 (the oracle's), the series in sin^2(theta) (the kernel's now)
    and, as a deliberately wrong one, the Taylor branch's 1/2 (what a misplaced threshold would give).  acos carries the rounding of the trace
    divided by sin(theta) into its quotient: four orders of magnitude above the other two, 0.7 of the bar under Talos' Kp = 30 on these references
    and 3.3 times the bar under the tree's Kp = 40, so that model MISSES the bar; the wrong threshold must miss the bar at theta = 1e-3."""
    import mpmath as mp
    worst = {}
    for name in NAMES:
        C = tl.case(name)
        m = C["m"]
        kp = max(l[5] for l in C["lanes"])
        for th in (1.3e-4, 1e-3):
            a13 = tl.ANGLES.index(th)
            w_ = dict(acos_over_w=0.0, oracle=0.0, series=0.0, half=0.0)
            n = 0
            for i in np.where(C["still"])[0]:
                Rf, _ = m.frame_placements(C["q"][i])
                for l in C["lanes"]:
                    if C["combos"][(i, l[0], l[1])] % NA != a13:
                        continue
                    E = Rf[l[2]].T @ C["ref"][i, l[3] + 3:l[3] + 12].reshape(3, 3).T
                    exact = np.array([float(x) for x in tl.exact_log3({(a, b): mp.mpf(float(E[a, b])) for a in range(3) for b in range(3)})])
                    w = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
                    theta = np.arccos((np.trace(E) - 1.0) / 2.0)
                    s2 = 0.25 * (w @ w)
                    forms = dict(acos_over_w=theta / np.sqrt(w @ w), oracle=theta / np.sin(theta) / 2.0, half=0.5,
                                 series=0.5 * (1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0 + s2 * (15.0 / 336.0 + s2 * 105.0 / 3456.0)))))
                    for k, t in forms.items():
                        w_[k] = max(w_[k], kp * float(np.abs(t * w - exact).max()))
                    n += 1
            print("%-6s Kp = %5.2f, %2d references at theta = %.1e: Kp |log3 - exact| = %s; bar %.1e" % (name, kp, n, th, {k: "%.2e" % e for k, e in w_.items()}, tl.TOL_ROWS))
            assert n >= 1
            worst[(name, th)] = w_
    for (name, th), w_ in worst.items():
        assert w_["oracle"] <= 1e-4 * tl.TOL_ROWS and w_["series"] <= 1e-4 * tl.TOL_ROWS, (name, th, w_)
        assert w_["acos_over_w"] > 1e3 * max(w_["oracle"], w_["series"]), (name, th, w_)
    assert worst[("tree", 1.3e-4)]["acos_over_w"] > tl.TOL_ROWS
    assert all(w_["half"] > tl.TOL_ROWS for (name, th), w_ in worst.items() if th == 1e-3)  # the bar bites on a wrong branch
