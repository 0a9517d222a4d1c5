"""CPU tests of the exact statement of the state integration (tests/se3_exact.py): the committed fixtures are what the statement gives, the
statement meets its own identities to 1e-40 and scipy's rotations at scipy's precision, the cases keep the margins their bars rely on, the C oracle
(oracle/wbc_oracle.c: wbco_integrate) agrees with the statement ENTRY BY ENTRY within K_ORACLE -- ratio = |x - value| / (eps scale) -- and the
statement SEES MUTANTS: eleven copies of the oracle with one textual substitution each, compiled as oracle.build() compiles the original, each of
which must miss the oracle's own bar on at least one case.  No GPU.

K_ORACLE[family][quantity] (tests/se3_exact_cases.py) is the oracle's worst ratio as measured here (`-s -k oracle_ratio` prints it): the K of the
device's bar 4 K_ORACLE eps scale in tests/test_gpu_se3_exact.py.  The oracle takes no status: it is held on the integrated instances, and the kept
state is a statement of copies and of one rotation vector that tests/test_gpu_se3_exact.py holds the kernel to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import se3_exact_cases as X
from tests.se3_exact_cases import K_ORACLE, KSTEPS

ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
_seen = {}


# ---- the oracle (or a mutant of it) on a group ---------------------------------------------------------------------------------------------------
def _integrate(cdll, fb, dt, q, dq, dv):
    f = cdll.wbco_integrate
    f.restype = None
    B, nv = dq.shape
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    q, dq, dv = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, dq, dv))
    qn, vn, qs = np.zeros_like(q), np.zeros_like(dq), np.zeros_like(dq)
    for i in range(B):
        f(C.c_int(int(fb)), C.c_int(nv), C.c_double(dt), dp(q[i]), dp(dq[i]), dp(dv[i]), dp(qn[i]), dp(vn[i]), dp(qs[i]))
    return dict(q_next=qn, v_next=vn, q_solver=qs)


def _integrated(G):
    return (G["status"] == 0) if "status" in G else np.ones(G["q"].shape[0], dtype=bool)


def figures(cdll):
    """family -> quantity -> the worst ratio of `cdll`'s wbco_integrate against the fixtures, over the family's float64 groups."""
    out = {}
    for family in X.FAMILIES:
        w = {k: 0.0 for k in K_ORACLE[family] if k != "norm"}  # (the K ticks' norm is measured after the ticks: ksteps_end)
        for g, G in X.load(family).items():
            if not int(G["f64"]):
                continue
            ok = _integrated(G)
            fb, nv, dt = int(G["fb"]), int(G["nv"]), float(G["dt"])
            got = _integrate(cdll, fb, dt, G["q"][ok], G["dq"][ok], G["x"][ok, :nv])
            sub = {k: (a[ok] if isinstance(a, np.ndarray) and a.ndim == 2 else a) for k, a in G.items()}
            for k, r in X.worst(sub, got).items():
                w[k] = max(w[k], r)
            if family == "drifted":
                w["norm_abs"] = max(w["norm_abs"], float(X.norm_defect(got["q_next"][:, 3:7]).max()))
            if family == "ksteps":
                out["ksteps_end"] = _k_ticks(cdll, G)
        out[family] = w
    return out


def _k_ticks(cdll, G):
    q, dq, dt = G["q"], G["dq"], float(G["dt"])
    for _ in range(int(G["K"])):
        o = _integrate(cdll, 1, dt, q, dq, np.zeros_like(dq))
        q, dq = o["q_next"], o["v_next"]
    assert np.array_equal(dq, G["dq"])
    w = X.worst(G, {"q_next": q}, prefix="end.")
    return {"position": w["position"], "quaternion": w["quaternion"], "norm": float(X.norm_defect(q[:, 3:7]).max() / X.EPS)}


def misses(figs):
    """The (family, quantity) at which figures() is over the oracle's own bar."""
    over = [(f, k) for f in X.FAMILIES for k, v in figs[f].items() if not v <= K_ORACLE[f][k]]
    e = figs["ksteps_end"]
    over += [("ksteps_end", k) for k in ("position", "quaternion") if not e[k] <= KSTEPS * K_ORACLE["ksteps"][k]]
    return over + ([("ksteps_end", "norm")] if not e["norm"] <= K_ORACLE["ksteps"]["norm"] else [])


# ---- the fixtures and the statement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", X.FAMILIES)
def test_fixture_is_what_the_statement_gives(family, oracle_mod):
    pytest.importorskip("mpmath")
    from tests import se3_exact as S
    got, want = S.computed(family), X.flat(X.load(family))
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        a = np.asarray(got[k])
        if family == "drifted" and k.split(".", 1)[1] in ("q_next", "v_next", "q_solver"):
            # the oracle's own outputs: another libm may move a last bit of sin or cos, never more
            assert np.abs(a - want[k]).max() <= 4 * X.EPS * max(1.0, np.abs(want[k]).max()), (family, k)
            continue
        assert a.dtype == want[k].dtype and a.shape == want[k].shape and a.tobytes() == want[k].tobytes(), (family, k)


def test_the_statement_holds_its_own_identities():
    pytest.importorskip("mpmath")
    from tests import se3_exact as S
    d = S.identities()
    print("the statement against itself: | |q| - 1 | %.1e, exp6(a) exp6(b) - exp6(a + b) for parallel twists %.1e" % (d["norm"], d["parallel"]))
    assert d["norm"] <= 1e-40 and d["parallel"] <= 1e-40, d


def test_the_statement_agrees_with_scipy():
    from scipy.spatial.transform import Rotation as Rot
    for family in ("generic", "sign", "rot2quat"):
        G = X.load(family)["all"]
        dt, q, v = float(G["dt"]), G["q"], G["v_next"]
        R0 = Rot.from_quat(q[:, 3:7])
        w, u = dt * v[:, 3:6], dt * v[:, :3]
        q1 = (R0 * Rot.from_rotvec(w)).as_quat()
        q1 *= np.sign((q1 * q[:, 3:7]).sum(1))[:, None]
        assert np.abs(q1 - G["q_next"][:, 3:7]).max() < 1e-14, family
        p1 = []
        for i in range(q.shape[0]):
            t = np.linalg.norm(w[i])
            K = np.array([[0, -w[i, 2], w[i, 1]], [w[i, 2], 0, -w[i, 0]], [-w[i, 1], w[i, 0], 0]])
            V = np.eye(3) if t < 1e-12 else np.eye(3) + (1 - np.cos(t)) / t**2 * K + (t - np.sin(t)) / t**3 * K @ K
            p1.append(q[i, :3] + R0[i].apply(V @ u[i]))
        assert np.abs(np.array(p1) - G["q_next"][:, :3]).max() < 1e-14, family
        judged = np.isfinite(G["scale.q_solver"][:, 3])
        rv = Rot.from_quat(G["q_next"][:, 3:7]).as_rotvec()
        assert np.abs(rv - G["q_solver"][:, 3:6])[judged].max() < 1e-14, family


def test_fixtures_hold_what_the_cases_say():
    n = 0
    for family in X.FAMILIES:
        assert os.path.getsize(X.path(family)) < (1 << 20)
        L, I = X.load(family), X.inputs(family)
        assert list(L) == list(I)
        for g, G in L.items():
            n += G["q"].shape[0]
            for k, a in I[g].items():  # the inputs are the cases'
                assert np.asarray(G[k]).tobytes() == np.asarray(a).tobytes(), (family, g, k)
            assert ("status" in G) == ("status" in I[g])
            for tag in X.handles(G):
                if tag == "f32":
                    for k in ("q", "dq"):
                        assert np.array_equal(G[k].astype(np.float32).astype(np.float64), G[k]), (family, g, k)
                    fin = np.isfinite(G["x"])
                    assert np.array_equal(G["x"][fin].astype(np.float32).astype(np.float64), G["x"][fin])
            for k in ("q_next", "v_next", "q_solver"):
                assert np.isfinite(G[k]).all(), (family, g, k)  # no NaN of x reaches a statement
            assert (G["scale.q_next"] >= 0).all() and np.isfinite(G["scale.q_next"]).all() and (G["scale.q_solver"] >= 0).all()
    print("se3_exact: %d instances in %d families" % (n, len(X.FAMILIES)))
    # the sizes the issue names, each of them met
    S = X.load("sizes")
    met = {(int(G["fb"]), int(G["nv"]), G["q"].shape[0], int(G["ldx"]) - int(G["nv"]), int(G["qs"])) for G in S.values()}
    for fb in (1, 0):
        for nv in X.SIZES_NV[bool(fb)]:
            assert {(b, pad, qs) for (f, v, b, pad, qs) in met if f == fb and v == nv} == {(b, pad, int(qs)) for b, pad, qs in X.sizes_of(nv)}
            assert {qs for (f, v, _, _, qs) in met if f == fb and v == nv} == {0, 1} and {pad for (f, v, _, pad, _) in met if f == fb and v == nv} == {0, 13}
    assert {m[2] for m in met if m[1] > 7} == {1, 3, 4, 5}
    # every code of the enumeration but OPTIMAL keeps a state, floating and fixed
    for g in ("floating", "fixed"):
        assert set(X.load("kept")[g]["status"].tolist()) == {0, *X.HQP_NOT_OPTIMAL}
    assert "status" not in X.load("kept")["null_status"]


def test_cases_keep_their_margins():
    """|q1 . q0| >= 0.1 wherever an instance is integrated (nearer zero the sign is a rounding decision), |w| >= 0.05 of every judged rotation
    vector's quaternion and none unjudged in the families that are about q_solver, and no oblique t within 2^-42 of the switch (a t on a
    coordinate axis is an exact double, and the comparison with 1e-4 is exact)."""
    for family in X.FAMILIES:
        for g, G in X.load(family).items():
            if not int(G["fb"]):
                continue
            ok = _integrated(G)
            q0 = G["q"][:, 3:7] / np.linalg.norm(G["q"][:, 3:7], axis=1, keepdims=True)
            q1 = G["q_next"][:, 3:7]
            assert ((q1 * q0).sum(1)[ok] >= X.DOT_MARGIN).all(), (family, g)
            stored = np.where(ok[:, None], q1, q0)
            judged = np.isfinite(G["scale.q_solver"][:, 3])
            assert (np.abs(stored[judged, 3]) >= X.W_MARGIN * 0.999).all(), (family, g)
            if family in ("switch", "tiny", "qsolver", "kept"):  # (a step of 1 rad or more from a random start may land anywhere)
                assert judged.all(), (family, g)
            w = float(G["dt"]) * G["v_next"][:, 3:6]
            on_axis = (w != 0).sum(1) <= 1
            t = np.linalg.norm(w, axis=1)
            assert (on_axis | (np.abs(t / X.SWITCH - 1.0) >= 2.0 ** -42))[ok].all(), (family, g)
    # the switch family visits 1e-4 itself, both neighbours and both sides at every distance, on the axis exactly
    G = X.load("switch")["translation_f64"]
    t = np.abs(float(G["dt"]) * G["dq"][:, 3:6]).max(axis=1)[:len(X.switch_ts())]
    assert sorted(t.tolist()) == sorted(X.switch_ts()) and (t > X.SWITCH).sum() == 5 and (t == X.SWITCH).sum() == 1
    # q_solver: results of both signs of w, the identity's exact +0
    G = X.load("qsolver")["all"]
    assert (G["q_next"][:, 6] < 0).sum() >= 6 and (G["q_next"][:, 6] > 0).sum() >= 6
    assert (G["scale.q_solver"][:2, 3:6] == 0).all() and not np.signbit(G["q_solver"][:2, 3:6]).any()
    # sign continuity: steps that must flip (the step's own w is cos(t / 2) < 0) and steps that must not
    G = X.load("sign")["all"]
    half = 0.5 * np.linalg.norm(float(G["dt"]) * G["dq"][:, 3:6], axis=1)
    assert (np.cos(half) < -0.4).sum() == 4 and (G["q"][:, 6] < 0).sum() >= 6


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_figures(oracle_mod):
    from oracle import oracle
    return figures(oracle.lib())


@pytest.mark.parametrize("family", X.FAMILIES)
def test_oracle_ratio(family, oracle_figures):
    w = oracle_figures[family]
    print("ratio to the statement, %-9s %s" % (family, "  ".join("%s %.3g" % kv for kv in w.items())))
    _seen[family] = w
    if family == "ksteps":
        e = oracle_figures["ksteps_end"]
        print("after K = %d ticks against the subgroup statement: position %.3g eps scale, quaternion %.3g eps, | |q| - 1 | %.3g eps" % (
            KSTEPS, e["position"], e["quaternion"], e["norm"]))
        _seen[family] = dict(w, norm=e["norm"])
    if len(_seen) == len(X.FAMILIES):
        print("K_ORACLE measured: %s" % {f: {k: float("%.3g" % v) for k, v in _seen[f].items()} for f in X.FAMILIES})
    for k, v in w.items():
        assert v <= K_ORACLE[family][k], (family, k, v, K_ORACLE[family][k])
    assert not [m for m in misses(oracle_figures) if m[0] in (family, family + "_end")]


def test_the_f32_contract_meets_its_bar_on_the_host(oracle_mod):
    """An F32 handle computes in double and rounds once: the oracle on the float32 inputs, rounded to float32, stands in for it here.  v_next,
    the joints and a kept state bit for bit; the base within eps32 scale (a correctly rounded double result is within eps32 |x| / 2, and
    scale >= |x|).  The worst ratio is printed: the share of the bar that rounding and a float32 quaternion's norm (|q|^2 - 1 of 1e-9) take."""
    from oracle import oracle
    worst = {k: 0.0 for k in X.QUANTITIES}
    for family in X.FAMILIES:
        for g, G in X.load(family).items():
            if not int(G["f32"]):
                continue
            ok = _integrated(G)
            got = _integrate(oracle.lib(), int(G["fb"]), float(G["dt"]), G["q"][ok], G["dq"][ok], G["x"][ok, :int(G["nv"])])
            got = {k: a.astype(np.float32) for k, a in got.items()}
            sub = {k: (a[ok] if isinstance(a, np.ndarray) and a.ndim == 2 else a) for k, a in G.items()}
            for k, r in X.worst(sub, got, tag="f32").items():
                worst[k] = max(worst[k], r)
    print("the F32 contract on the host, worst |x - value| / (eps32 scale): %s" % "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_k_oracle_is_sane():
    """Every K under 16 with the scale as stated: no regime hides under a wide K."""
    for f, K in K_ORACLE.items():
        assert all(0.0 < v < 16.0 for k, v in K.items() if k != "norm_abs"), (f, K)
    # what a first-order normalisation leaves of |q0|^2 - 1 = 2e-6: (3/8) (2e-6)^2 = 1.5e-12, and what the rotation matrix of a non-unit
    # quaternion adds to it stays within a few times that
    assert 1.5e-12 <= K_ORACLE["drifted"]["norm_abs"] < 1e-11


# ---- the statement sees mutants --------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "alpha_wxv: t2 / 24 -> t2 / 12": ("t2 / 24.0", "t2 / 12.0"),
    "alpha_v: t2 / 6 -> t2 / 5": ("t2 / 6.0", "t2 / 5.0"),
    "ct = 1": ("ct = 1.0 - t2 / 2.0", "ct = 1.0"),
    "alpha_w: 1 / 6 -> 1 / 5": ("1.0 / 6.0 -", "1.0 / 5.0 -"),
    "the switch at 1e-3": ("if (t > 1e-4)", "if (t > 1e-3)"),
    "the switch at 1e-6": ("if (t > 1e-4)", "if (t > 1e-6)"),
    "no sign continuity": ("if (dotp < 0.0)", "if (0)"),
    "no normalisation": ("(3.0 - N2) / 2.0", "1.0"),
    "the axis case `one` never taken": ("if (R[4] > R[0]) i = 1;", "if (0) i = 1;"),
    "atan2 of w, not |w|": ("fabs(u[3])", "u[3]"),
    "the axis keeps its sign": ("if (u[3] < 0.0) n = -n;", ""),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """name -> the shared library of the mutant, all compiled at once with the Makefile's compiler and flags."""
    d = tmp_path_factory.mktemp("mutants")
    src = open(os.path.join(ORACLE_DIR, "wbc_oracle.c")).read()
    mk = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    flags = [ln for ln in mk.splitlines() if ln.startswith("CFLAGS ?=")][0].split("?=", 1)[1].split()
    jobs = {}
    for i, (name, (old, new)) in enumerate(MUTANTS.items()):
        assert src.count(old) == 1, (name, old, src.count(old))
        c = os.path.join(str(d), "mutant_%02d.c" % i)
        with open(c, "w") as f:
            f.write(src.replace(old, new))
        so = os.path.join(str(d), "mutant_%02d.so" % i)
        cmd = [os.environ.get("CC", "gcc")] + flags + ["-w", "-I", ORACLE_DIR, "-shared", "-o", so, c, os.path.join(ORACLE_DIR, "rbd_oracle.c"), "-lm", "-lpthread"]
        jobs[name] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), so)
    libs = {}
    for name, (p, so) in jobs.items():
        out = p.communicate()[0]
        assert p.returncode == 0, (name, out)
        libs[name] = so
    return libs


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_statement_sees_the_mutant(name, mutant_libs):
    figs = figures(C.CDLL(mutant_libs[name]))
    over = misses(figs)
    worst = max(((figs[f][k] / (K_ORACLE[f][k] if f in K_ORACLE else KSTEPS * K_ORACLE["ksteps"][k] if k != "norm" else K_ORACLE["ksteps"]["norm"]), f, k)
                 for f, k in over), default=(0.0, "", ""))
    print("mutant %-34s over its bar in %2d (family, quantity) pairs; worst %.2e times the bar: %s %s" % (name, len(over), worst[0], worst[1], worst[2]))
    assert over, name
