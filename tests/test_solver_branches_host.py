"""The selected branch QPs (tests/solver_branches.py, tests/golden/solver_branches/selection.json) on the CPU:
  * every selected QP still has the class, the status, the iteration count and the census the selection recorded;
  * the selection holds the events it was made for (REQUIRED, MIN_DROPS_PER_POSITION);
  * the oracle itself against a 50-digit KKT solve on its own final active set (a few QPs per structure: one solve is a dense LU of
    n + iq <= 150 unknowns in mpmath);
  * the numpy model of the compact loop (tools/gi_rinv_proto.py, round5=True) against the oracle on the stacks that run the compact
    loop, at tests/test_gi_rinv_proto.py's tolerance where the oracle itself keeps x and its count (solver_branches.comparable), taking the dual-only, vertex and rejection branches where the oracle's log does.
"""
import mpmath as mp
import numpy as np
import pytest

from inria_wbc_amd import structure
from tests import solver_branches as sb
from tools import gi_rinv_proto as proto

EXACT_PER_STRUCTURE = 3
TOL_EXACT = 1e-9     # oracle against the exact solution on its final active set: dv, wrench, tau, relative to max(1, |.|inf)
EXACT_FIGURES = []   # (structure, entry, dict) per exact solve; each is printed as it is made (pytest -s), profiles/solver_branches/INDEX.md holds them
COMPACT = ("talos", "talos_single_support", "icub", "tiago")  # the stacks whose default kernel runs the compact loop


@pytest.fixture(scope="module")
def sel():
    return sb.load_selection()


_RUNS = {}


def runs(name, oracle, sel):
    """(st, entries, inputs [B, len], tick_batch outputs, logs, censuses) of a structure's selected QPs, computed once."""
    if name not in _RUNS:
        st = structure.STRUCTURES[name]()
        entries = sb.entries_of(name, sel)
        inp = sb.stack_inputs(st, entries)
        ref = oracle.tick_batch(st, inp)
        logs = [oracle.tick_log(st, inp, i, ref) for i in range(len(entries))]
        _RUNS[name] = (st, entries, inp, ref, logs, [sb.census(st, lg, oracle) for lg in logs])
    return _RUNS[name]


@pytest.mark.parametrize("name", sb.STRUCTS)
def test_every_selected_qp_keeps_its_class_and_census(oracle_mod, sel, name):
    st, entries, inp, ref, logs, cs = runs(name, oracle_mod, sel)
    assert 0 < len(entries) <= sb.MAX_PER_STRUCTURE
    for i, (e, c) in enumerate(zip(entries, cs)):
        assert e["class"] in ("A", "B")
        assert (c["status"], c["iters"]) == (e["status"], e["iters"]) and c["status"] == ref["status"][i], (name, e, c["status"], c["iters"])
        assert c["iters"] <= 500 < st.max_iter
        assert sb.brief(c) == e["events"], (name, e, sb.brief(c))
        one = {k: v[i:i + 1] for k, v in inp.items()}
        cls, fig = sb.classify(st, one, e["seed"], oracle_mod, base=logs[i])
        if sb.entry_key(e) in sb.RECLASSIFIED:  # a class-A QP by the perturbations, filed under B for a near tie they missed: the tie is there
            tie = sb.parting_pick(st, one, oracle_mod)
            assert (cls, e["class"]) == ("A", "B") and tie["rel"] < sb.NEAR_TIE and tie["oracle_row"] == tie["other"], (name, e, cls, tie)
            assert fig["max_move"] <= sb.TOL_CLASS_B, (name, e, fig)  # class B's own condition: classify() returns A before it compares the move
            cls = "B"
        assert cls == e["class"], (name, e, cls, fig)
        assert e["x_stable"] == (fig["max_move_x"] <= sb.TOL_CLASS_B)
        assert (fig["iters_seen"][0], fig["iters_seen"][-1]) == (e["iters_lo"], e["iters_hi"]) and (cls != "A" or e["iters_lo"] == e["iters_hi"] == e["iters"])


def test_f32_entries_keep_their_class_on_rounded_inputs(oracle_mod, sel):
    st = structure.STRUCTURES["icub"]()
    assert sel["f32"]
    for e in sel["f32"]:
        inp = sb.entry_inputs(st, e, f32=True)
        log = oracle_mod.tick_log(st, inp, 0)
        c = sb.census(st, log, oracle_mod)
        assert (c["status"], c["iters"], sb.brief(c)) == (e["status"], e["iters"], e["events"])
        assert sb.classify(st, inp, e["seed"], oracle_mod, base=log)[0] == e["class"]


@pytest.mark.parametrize("name", sb.STRUCTS)
def test_the_selection_holds_the_required_events(oracle_mod, sel, name):
    st, entries, inp, ref, logs, cs = runs(name, oracle_mod, sel)
    assert sel["unmet"] == []
    for feat, least, cls in sb.REQUIRED[name]:
        got = sum(1 for e, c in zip(entries, cs) if feat in sb.features(c) and (cls is None or e["class"] == cls))
        assert got >= least, (name, feat, got, least)
    tot = sb.census_sum(cs)
    for k in ("drop_first", "drop_interior", "drop_last"):
        assert tot[k] >= sb.MIN_DROPS_PER_POSITION, (name, k, tot[k])
    # what the branches are made of, beyond their counts: a dual-only step happens where z vanishes, that is at a vertex or where the
    # candidate's normal lies in the span of the active ones; an INFEASIBLE end comes with a non-empty active set on these inputs
    assert tot["dual_drop"] > 0 and tot["unbounded_nonempty"] >= 4
    if name == "three_contact":
        assert tot["repick_after_dependent"] + tot["exit_none"] >= tot["dependent"] > 0  # a rejection goes back to step 2: another pick, or nothing left


# ---- the oracle against an exact solve on its own final active set ----------------------------------------------------------

def exact_on_active_set(st, oracle, inp, i, A):
    """50-digit solution of  H x + g = N u,  N' x + c0 = 0  over the rows of A (eiquadprog's tags) of QP i's dense form as the solver sees it.
    Returns (x, u, tau) as mpmath columns / lists; tau = h_a + M_a dv - J_a' f from the inputs."""
    H, g, CE, ce0, CI, ci0 = oracle.assemble(st, inp, i)
    n, q = st.n, len(A)
    rows = [CE[-a - 1] if a < 0 else CI[a] for a in A]
    c0 = [ce0[-a - 1] if a < 0 else ci0[a] for a in A]
    with mp.workdps(50):
        K = mp.zeros(n + q, n + q)
        rhs = mp.zeros(n + q, 1)
        for r in range(n):
            for c in range(n):
                K[r, c] = mp.mpf(float(H[r, c]))
            rhs[r] = -mp.mpf(float(g[r]))
        for k in range(q):
            for c in range(n):
                v = mp.mpf(float(rows[k][c]))
                K[c, n + k] = -v
                K[n + k, c] = v
            rhs[n + k] = -mp.mpf(float(c0[k]))
        sol = mp.lu_solve(K, rhs)
        x = [sol[r] for r in range(n)]
        u = [sol[n + k] for k in range(q)]
        nv, na, nu, nc = st.nv, st.na, st.nu, st.nc
        M = np.zeros((nv, nv)); M[np.tril_indices(nv)] = inp["M"][i]; M = M + np.tril(M, -1).T
        Ac = inp["Ac"][i].reshape(nc, 6, nv) if nc else np.zeros((0, 6, nv))
        T = np.asarray(st.force_gen()).reshape(nc, 6, 12) if nc else np.zeros((0, 6, 12))
        tau = []
        for a in range(na):
            t = mp.mpf(float(inp["h"][i][nu + a]))
            for j in range(nv):
                t += mp.mpf(float(M[nu + a, j])) * x[j]
            for c in range(nc):
                for m_ in range(12):
                    jc = mp.fsum(mp.mpf(float(T[c, r, m_])) * mp.mpf(float(Ac[c, r, nu + a])) for r in range(6))
                    t -= jc * x[nv + 12 * c + m_]
            tau.append(t)
        slack = [mp.fsum([mp.mpf(float(CI[r, c])) * x[c] for c in range(n)] + [mp.mpf(float(ci0[r]))]) for r in range(st.nin2)]
        return x, u, tau, slack


def _exact_choice(entries, cs):
    """At most EXACT_PER_STRUCTURE OPTIMAL QPs: those with a dual-only step, a vertex or a rejection first, short runs first."""
    idx = [i for i, c in enumerate(cs) if c["status"] == sb.OPTIMAL]
    idx.sort(key=lambda i: (not (cs[i]["dual_drop"] or cs[i]["vertex"] or cs[i]["dependent"]), cs[i]["iters"], i))
    return idx[:EXACT_PER_STRUCTURE]


@pytest.mark.parametrize("name", sb.STRUCTS)
def test_oracle_against_a_50_digit_kkt_solve_on_its_final_active_set(oracle_mod, sel, name):
    """Measured on the fifteen QPs solved here (profiles/solver_branches/INDEX.md holds the table): the oracle's dv, contact wrench and tau are
    within 4.0e-11 of the exact solution on its final active set (the bar: 1e-9), the smallest inequality multiplier is +1.8e-7, and the
    exact solution still violates a row outside the set by up to 2.8e-2 on Talos and 1.9e-2 on Talos on one foot -- the stopping rule's
    leftover; on iCub, three_contact and Tiago it violates none."""
    st, entries, inp, ref, logs, cs = runs(name, oracle_mod, sel)
    nv = st.nv
    for i in _exact_choice(entries, cs):
        A = logs[i]["A"]
        x, u, tau, slack = exact_on_active_set(st, oracle_mod, inp, i, A)
        with mp.workdps(50):
            u_in = [u[k] for k, a in enumerate(A) if a >= 0]
            assert all(v >= 0 for v in u_in), (name, entries[i], float(min(u_in)))
            xo = ref["x"][i]
            e_dv = float(max(abs(x[j] - mp.mpf(float(xo[j]))) for j in range(nv))) / max(1.0, float(np.abs(xo).max()))
            fig = dict(e_dv=e_dv, iq=len(A), iters=int(ref["iters"][i]), min_multiplier=float(min(u_in)) if u_in else 0.0,
                       min_slack_exact=float(min(slack)), min_slack_oracle=float((oracle_mod.assemble(st, inp, i)[4] @ xo + oracle_mod.assemble(st, inp, i)[5]).min()))
            if st.nc:
                T = np.asarray(st.force_gen()).reshape(st.nc, 6, 12)
                wo = np.einsum("cij,cj->ci", T, xo[nv:].reshape(st.nc, 12))
                ew = 0.0
                for c in range(st.nc):
                    for r in range(6):
                        w = mp.fsum(mp.mpf(float(T[c, r, m_])) * x[nv + 12 * c + m_] for m_ in range(12))
                        ew = max(ew, float(abs(w - mp.mpf(float(wo[c, r])))))
                fig["e_wrench"] = ew / max(1.0, float(np.abs(wo).max()))
            if st.na:
                fig["e_tau"] = float(max(abs(tau[a] - mp.mpf(float(ref["tau"][i][a]))) for a in range(st.na))) / max(1.0, float(np.abs(ref["tau"][i]).max()))
        EXACT_FIGURES.append((name, entries[i], fig))
        print("exact KKT", name, {k: entries[i][k] for k in ("family", "noise", "p", "seed", "class")}, fig)
        assert max(fig["e_dv"], fig.get("e_wrench", 0.0), fig.get("e_tau", 0.0)) <= TOL_EXACT, (name, entries[i], fig)


# ---- the numpy model of the compact loop -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", COMPACT)
def test_compact_loop_model_takes_the_branches_the_oracle_takes(oracle_mod, sel, name):
    st, entries, inp, ref, logs, cs = runs(name, oracle_mod, sel)
    seen = dict(dual_steps=0, vertices=0, rejected=0)
    asked = dict(dual_steps=0, vertices=0, rejected=0)
    listed, met = [], 0
    for i, (e, c) in enumerate(zip(entries, cs)):
        H, g, CE, ce0, CI, ci0 = oracle_mod.assemble(st, inp, i)
        tr = {}
        out = proto.solve(H, g, CE, ce0, CI, ci0, max_iter=st.max_iter, trace=tr, round5=True)
        assert out["status"] == ref["status"][i], (name, e, out["status"])
        opt = c["status"] == sb.OPTIMAL
        ex, ev, ew = sb.deviations(st, out["x"], ref["x"][i]) if opt else (0.0, 0.0, 0.0)
        if sb.comparable(e):  # tests/test_gi_rinv_proto.py's tolerance, as it is
            assert abs(out["iters"] - ref["iters"][i]) <= 2, (name, e, out["iters"], ref["iters"][i])
            assert ex <= 1e-8, (name, e, ex)
        else:
            listed.append((e["family"], e["noise"], e["p"], e["seed"], e["class"], out["iters"] - int(ref["iters"][i]), "x %.1e" % ex))
        assert max(ev, ew) <= 1e-8, (name, e, ev, ew)
        took = dict(dual_steps=tr.get("dual_steps", 0), vertices=tr.get("vertices", 0), rejected=tr.get("rejected", 0))
        want = dict(dual_steps=c["dual_drop"], vertices=c["vertex"], rejected=c["dependent"])
        if e["class"] == "A" and out["iters"] == ref["iters"][i]:  # the same path: the same branches, as often
            assert took == want and tr.get("partial_steps", 0) == c["dual_drop"] + c["partial_drop"], (name, e, took, want)
        if c["dependent"]:
            # Where the oracle's log has a rejection the row lies in the span of the active ones, and the new diagonal of R is rounding noise: the
            # oracle refuses when that noise is <= eps R_norm.  Measured on the selected QPs: the model's noise at the same row is 3e-12 ... 1e-10
            # against eps R_norm = 1.8e-12 (its d comes through the pending reflector: more cancellation than the oracle's single dot product), so
            # it ADDS the row and ends INFEASIBLE like the oracle.  Which side of eps R_norm noise falls on is no property of the inputs; what is,
            # and what is held here: the model meets the same numerically dependent row -- |new diagonal| <= sqrt(eps) R_norm, the usual numerical-
            # rank threshold halfway (in magnitude) between dependent and independent -- on at least one QP per stack (a class-B path need not come by that row with those rows active).
            rej = set(r for code, r, _, _ in logs[i]["events"].tolist() if code == oracle_mod.EV_DEPENDENT)
            tries = [abs(al) / rn for ip, _, al, rn in tr.get("adds", []) if ip in rej]
            found = bool(tries) and min(tries) <= np.sqrt(proto.EPS)
            met += int(found)
            print("\nmodel", name, e["family"], e["seed"], "oracle rejects rows", sorted(rej), "model: smallest |diag| / R_norm on them",
                  "%.1e" % min(tries) if tries else "-", "refused", took["rejected"])
        for k in seen:
            seen[k] += took[k]
            asked[k] += want[k]
    print("model", name, "not comparable on raw x and iteration count:", len(listed), "of", len(entries), listed)
    for k in ("dual_steps", "vertices"):
        assert (seen[k] > 0) == (asked[k] > 0), (name, k, seen, asked)
    # dual-only steps on every compact stack; rejections in the oracle's log on the three floating-base ones, met by the model as said above (Tiago's
    # rows are +-e_j: a row dependent on the active ones has z = 0 exactly and takes the dual-only step instead -- no rejection in 13 cells x 200 seeds)
    assert asked["dual_steps"] > 0 and seen["dual_steps"] > 0
    if name != "tiago":
        assert asked["rejected"] > 0 and met > 0, (name, seen, asked, met)
