"""Inputs that take the active-set loop through the branches the default parity inputs never reach, chosen by the reference alone.

Shared by tests/test_solver_branches_host.py (the oracle against a 50-digit KKT solve and the numpy model of the compact loop, on the
CPU) and tests/test_gpu_solver_branches.py (every solver loop of the library against the oracle).  `python -m tests.solver_branches`
runs the search and writes tests/golden/solver_branches/selection.json and profiles/solver_branches/search.json; the tests regenerate
the selected QPs from that list by seed and never search.

What is here:
  * census(): what a log of oracle.tick_log says about a run -- the branches of wbco_eiquadprog_fast taken, where in the inequality
    block each drop happened, the kind of every picked / dropped row, the kind of the pick after every accepted add;
  * three input families, all synth.generate with other parameters: tight limits (p_bnd = p_act = p), and tight limits with ONE
    contradictory acceleration bound or torque limit (lower above upper);
  * classify(): the oracle under eight seeded one-ulp perturbations of every non-zero input element.
        class A: status, iteration count and event log unchanged;  (selection.json records the counts seen as iters_lo .. iters_hi)
        class B: status unchanged and, where that status is OPTIMAL, dv, contact wrench and tau within TOL_CLASS_B of the unperturbed
                 run's (relative to max(1, |.|inf), assert_parity's measure): a hundredth of the 1e-8 parity bar.  An INFEASIBLE run
                 returns no solution, so there class B asks for the status alone;
        anything else is not used.
    x_stable: the WHOLE of x, raw contact-point forces included, moves at most TOL_CLASS_B too (comparable() says what that decides).
    Why select at all: eiquadprog stops when |psi| <= nIneq eps tr(H) tr(J) 100, which on these stacks (cond(H) ~ 1e12) leaves slacks
    of up to -2.8e-2 behind (the exact solution on the oracle's final set, tests/test_solver_branches_host.py); on most all-tight Talos QPs one ulp of the inputs changes the path and the end state with it.
  * select(): at most MAX_PER_STRUCTURE QPs per structure that meet REQUIRED (the issue's section 5).
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from inria_wbc_amd import structure, synth

HERE = os.path.dirname(os.path.abspath(__file__))
SELECTION_PATH = os.path.join(HERE, "golden", "solver_branches", "selection.json")
SEARCH_PATH = os.path.join(os.path.dirname(HERE), "profiles", "solver_branches", "search.json")

STRUCTS = ("talos", "talos_single_support", "icub", "three_contact", "tiago")  # (Franka: nin2 = 0, the loop is never entered)
FLOATING = ("talos", "talos_single_support", "icub", "three_contact")
SEED0 = 555000
GRID_NOISE, GRID_P = (2.0, 5.0, 20.0), (0.3, 0.6, 1.0)
GRID_SEEDS, EXTRA_SEEDS = 48, 200   # classified seeds per grid cell; seeds per cell looked at for the rare events (section 5, last item)
N_PERTURB = 8
TOL_CLASS_B = 1e-10
MAX_PER_STRUCTURE = 24
FAMILIES = ("tight", "contra_bound", "contra_torque")
KINDS = ("bound", "torque", "facet", "normal")

OPTIMAL, INFEASIBLE = 0, 1  # tick_batch's statuses (tsid's)
EIQ_TO_TSID = {0: 0, 1: 1, 2: 1, 3: 3, 4: 4}  # eiquadprog's status -> tsid's: UNBOUNDED (of the dual) is INFEASIBLE


# ---- inputs -------------------------------------------------------------------------------------------------------------

def make_inputs(st, family: str, noise: float, p: float, seed: int) -> Dict[str, np.ndarray]:
    """One QP ([1, len] arrays).  `tight`: synth.generate(task_noise=noise, p_bnd=p, p_act=p).  `contra_bound` / `contra_torque`: the
    same with the lower side of one acceleration bound / torque limit (which one: drawn from the seed) put 1 above its upper side."""
    inp = synth.generate(st, 1, seed, task_noise=noise, p_bnd=p, p_act=p)
    rng = np.random.default_rng(seed + 0xC0)
    if family == "contra_bound":
        j = int(rng.integers(st.n_bound))
        inp["blb"][0, j] = inp["bub"][0, j] + 1.0
    elif family == "contra_torque":
        assert st.act_bounds
        j = int(rng.integers(st.na))
        inp["tlb"][0, j] = inp["tub"][0, j] + 1.0
    else:
        assert family == "tight", family
    return inp


def entry_inputs(st, e: dict, f32: bool = False) -> Dict[str, np.ndarray]:
    inp = make_inputs(st, e["family"], e["noise"], e["p"], e["seed"])
    if f32:
        inp = {k: v.astype(np.float32).astype(np.float64) for k, v in inp.items()}
    return inp


def stack_inputs(st, entries: List[dict], f32: bool = False) -> Dict[str, np.ndarray]:
    """[len(entries), len] arrays: the batch the GPU tests launch."""
    ones = [entry_inputs(st, e, f32) for e in entries]
    return {k: np.concatenate([o[k] for o in ones], axis=0) for k in synth.FIELDS}


def perturbed(inp: Dict[str, np.ndarray], k: int, seed: int) -> Dict[str, np.ndarray]:
    """Perturbation k of a QP: every non-zero element of every array moved one ulp up or down (a fair coin per element, seeded by
    (seed, k)).  Zeros stay: they are structural (masked Jacobian columns), and one ulp of zero is no relative perturbation."""
    rng = np.random.default_rng([seed, 77, k])
    out = {}
    for name in synth.FIELDS:
        a = np.asarray(inp[name], np.float64)
        up = rng.random(a.shape) < 0.5
        b = np.nextafter(a, np.where(up, np.inf, -np.inf))
        out[name] = np.where(a == 0.0, a, b)
    return out


# ---- census -------------------------------------------------------------------------------------------------------------

def row_kinds(st) -> np.ndarray:
    """[nin2] index into KINDS of every one-sided CI row (a block's lower sides, then its upper sides)."""
    out = []
    for kind, _ in st.ineq_blocks:
        if kind == structure.INEQ_BOUNDS:
            side = [0] * st.n_bound
        elif kind == structure.INEQ_ACTUATION:
            side = [1] * st.na
        else:
            side = [2] * 16 + [3]
        out += side + side
    assert len(out) == st.nin2
    return np.asarray(out, np.int64)


def census(st, log: dict, oracle) -> dict:
    """Counts from one event log (oracle.tick_log's dict)."""
    ev = log["events"]
    kinds = row_kinds(st)
    n, neq = st.n, st.neq
    E = oracle
    c = dict(picks=0, full_add=0, dependent=0, partial_drop=0, dual_drop=0, exit_psi=0, exit_none=0, unbounded=0, max_iter=0,
             vertex=0, dual_drop_at_vertex=0, unbounded_nonempty=0, dual_drop_before_unbounded=0, repick_after_dependent=0,
             drop_first=0, drop_interior=0, drop_last=0,
             pick_kind={k: 0 for k in KINDS}, drop_kind={k: 0 for k in KINDS}, dual_drop_kind={k: 0 for k in KINDS},
             pick_after_add={}, iters=int(log["iters"]), status=EIQ_TO_TSID[int(log["status"])])
    last_add = None
    after_dependent = False
    for code, row, pos, iq in ev.tolist():
        if code == E.EV_PICK:
            c["picks"] += 1
            c["pick_kind"][KINDS[kinds[row]]] += 1
            if last_add is not None:
                key = "%s>%s" % (KINDS[kinds[last_add]], KINDS[kinds[row]])
                c["pick_after_add"][key] = c["pick_after_add"].get(key, 0) + 1
                last_add = None
            if after_dependent:
                c["repick_after_dependent"] += 1
                after_dependent = False
        elif code == E.EV_FULL_ADD:
            c["full_add"] += 1
            last_add = row
            if iq + 1 == n:
                c["vertex"] += 1
        elif code == E.EV_DEPENDENT:
            c["dependent"] += 1
            after_dependent = True
        elif code in (E.EV_PARTIAL_DROP, E.EV_DUAL_DROP):
            dual = code == E.EV_DUAL_DROP
            c["dual_drop" if dual else "partial_drop"] += 1
            c["drop_kind"][KINDS[kinds[row]]] += 1
            if dual:
                c["dual_drop_kind"][KINDS[kinds[row]]] += 1
                if iq == n:
                    c["dual_drop_at_vertex"] += 1
            m = iq - neq  # rows in the inequality block before the drop
            assert 0 <= pos < m
            if pos == 0:
                c["drop_first"] += 1
            if pos == m - 1:
                c["drop_last"] += 1
            if 0 < pos < m - 1:
                c["drop_interior"] += 1
        elif code == E.EV_EXIT_PSI:
            c["exit_psi"] += 1
        elif code == E.EV_EXIT_NONE:
            c["exit_none"] += 1
        elif code == E.EV_UNBOUNDED:
            c["unbounded"] += 1
            if iq > neq:
                c["unbounded_nonempty"] += 1
            if c["dual_drop"]:
                c["dual_drop_before_unbounded"] += 1
        elif code == E.EV_MAX_ITER:
            c["max_iter"] += 1
    return c


SUM_KEYS = ("picks", "full_add", "dependent", "partial_drop", "dual_drop", "exit_psi", "exit_none", "unbounded", "max_iter", "vertex",
            "dual_drop_at_vertex", "unbounded_nonempty", "dual_drop_before_unbounded", "repick_after_dependent", "drop_first",
            "drop_interior", "drop_last")
DICT_KEYS = ("pick_kind", "drop_kind", "dual_drop_kind", "pick_after_add")


def census_sum(cs: List[dict]) -> dict:
    tot = {k: int(sum(c[k] for c in cs)) for k in SUM_KEYS}
    for dk in DICT_KEYS:
        d = {}
        for c in cs:
            for k, v in c[dk].items():
                d[k] = d.get(k, 0) + int(v)
        tot[dk] = d
    tot["qps"] = len(cs)
    tot["max_iters"] = max([c["iters"] for c in cs], default=0)
    return tot


def brief(c: dict) -> dict:
    """The part of a census that selection.json records per QP (numbers only)."""
    return {k: int(c[k]) for k in ("full_add", "dependent", "partial_drop", "dual_drop", "vertex", "drop_first", "drop_interior", "drop_last")}


def features(c: dict) -> List[str]:
    """The required events a QP offers (what REQUIRED and select() count)."""
    f = []
    if c["status"] == OPTIMAL:
        if c["dual_drop"]:
            f.append("optimal_dual_drop")
        if c["vertex"]:
            f.append("optimal_vertex")
        if c["dependent"]:
            f.append("optimal_dependent")
        if c["exit_none"]:
            f.append("exit_none")
    if c["status"] == INFEASIBLE:
        if c["dual_drop_before_unbounded"]:
            f.append("infeasible_dual_drop")
        if c["unbounded_nonempty"]:
            f.append("unbounded_nonempty")
    if c["dependent"]:
        f.append("dependent")
    return f


# ---- classification -----------------------------------------------------------------------------------------------------

def _moves(st, a: dict, b: dict, i: int, j: int) -> float:
    """max relative move of dv, contact wrench, tau between run i of a and run j of b (assert_parity's measure)."""
    nv = st.nv
    xa, xb = a["x"][i], b["x"][j]
    m = float(np.abs(xa[:nv] - xb[:nv]).max() / max(1.0, np.abs(xa).max()))
    if st.nc:
        T = np.asarray(st.force_gen()).reshape(st.nc, 6, 12)
        wa = np.einsum("cij,cj->ci", T, xa[nv:].reshape(st.nc, 12))
        wb = np.einsum("cij,cj->ci", T, xb[nv:].reshape(st.nc, 12))
        m = max(m, float(np.abs(wa - wb).max() / max(1.0, np.abs(wa).max())))
    if st.na:
        m = max(m, float(np.abs(a["tau"][i] - b["tau"][j]).max() / max(1.0, np.abs(a["tau"][i]).max())))
    return m


def classify(st, inp: Dict[str, np.ndarray], seed: int, oracle, base: Optional[dict] = None, hint=None) -> Tuple[str, dict]:
    """('A' | 'B' | 'unused', figures) of one QP.  `base`: oracle.tick_log of the unperturbed QP if the caller has it.
    hint: the QP's warm-start hint (8 words), held fixed under the perturbations (tests/warm_hints.py); None: the cold oracle."""
    pert = [perturbed(inp, k, seed) for k in range(N_PERTURB)]
    both = {k: np.concatenate([inp[k]] + [q[k] for q in pert], axis=0) for k in synth.FIELDS}
    ref = oracle.tick_batch(st, both, hint=None if hint is None else np.tile(np.asarray(hint, np.uint32).reshape(1, 8), (N_PERTURB + 1, 1)))
    status, iters = ref["status"], ref["iters"]
    fig = dict(status=int(status[0]), iters=int(iters[0]), iters_seen=sorted(set(int(v) for v in iters)))
    if not (status == status[0]).all() or status[0] not in (OPTIMAL, INFEASIBLE):
        return "unused", fig
    move = max(_moves(st, ref, ref, 0, k) for k in range(1, N_PERTURB + 1)) if status[0] == OPTIMAL else 0.0
    fig["max_move"] = move
    # the whole of x, raw contact-point forces included: six directions of f per contact are held by the 1e-8 regulariser alone (tests/util.py)
    fig["max_move_x"] = float(np.abs(ref["x"][1:] - ref["x"][0]).max() / max(1.0, np.abs(ref["x"][0]).max())) if status[0] == OPTIMAL else 0.0
    same_path = bool((iters == iters[0]).all())
    if same_path:
        base = base or oracle.tick_log(st, both, 0, ref, hint=hint)
        for k in range(1, N_PERTURB + 1):
            if not np.array_equal(oracle.tick_log(st, both, k, ref, hint=hint)["events"], base["events"]):
                same_path = False
                break
    if same_path:
        return "A", fig  # (the same path ends on the same active set: what moves then is one linear solve's rounding; max_move records it)
    if move <= TOL_CLASS_B:
        return "B", fig
    return "unused", fig


# ---- near ties the perturbations missed ------------------------------------------------------------------------------------

NEAR_TIE = 1e-9
# class-A QPs on which a loop's iteration count differed from the oracle's, and where the paths part at a pick whose two candidates' s
# differ by less than NEAR_TIE relative: the last bits of s decide, eight perturbations happened not to flip them.  select() files such
# a QP under class B; tests/test_solver_branches_host.py checks that the near tie is there.  (structure, family, noise, p, seed): what was seen
RECLASSIFIED = {
    ("icub", "tight", 5.0, 0.6, 555056): "full layout (FLAG_FULL_LDS): 45 iterations against the oracle's 47, every other loop 47; pick 14 takes "
                                         "friction facet 92 where the oracle takes facet 90 of the same contact point: s = -17.60661900618978 "
                                         "against -17.606619006188936, 4.8e-14 relative",
}


def entry_key(e: dict) -> tuple:
    return (e["structure"], e["family"], e["noise"], e["p"], e["seed"])


def parting_pick(st, inp: Dict[str, np.ndarray], oracle, i: int = 0) -> Optional[dict]:
    """Where another arithmetic can leave the oracle's path on QP i: the numpy model of the compact loop (tools/gi_rinv_proto.py) beside
    the oracle's log.  Returns the first pick at which the two take different rows, or, if they never part, the pick with the smallest relative
    margin over its runner-up: dict(pick, row, s, other, s_other, oracle_row, rel).  The s values are the MODEL's, from its iterate just before
    that pick -- the oracle's log carries rows, not s; up to that pick the two have taken the same rows, so the iterates agree to rounding
    (1e-13 here), which is why a margin is only called a near tie well above that (NEAR_TIE).  The model stands in for the device loop whose count
    differed: it parts from the oracle at the same place whenever its count is the device's."""
    from tools import gi_rinv_proto as proto
    H, g, CE, ce0, CI, ci0 = oracle.assemble(st, inp, i)
    log = oracle.eiquadprog_log(H, g, CE, ce0, CI, ci0, max_iter=st.max_iter)
    tr = {}
    proto.solve(H, g, CE, ce0, CI, ci0, max_iter=st.max_iter, trace=tr, round5=True)
    mine = tr.get("picks", [])
    theirs = [r for c, r, _, _ in log["events"].tolist() if c == oracle.EV_PICK]
    rel = lambda p: abs(p[1] - p[3]) / abs(p[1])
    for k, (p, row) in enumerate(zip(mine, theirs)):
        if p[0] != row:
            return dict(pick=k, parted=True, row=p[0], s=p[1], other=p[2], s_other=p[3], oracle_row=row, rel=rel(p))
    if not mine:
        return None
    k = min(range(len(mine)), key=lambda j: rel(mine[j]))
    p = mine[k]
    return dict(pick=k, parted=False, row=p[0], s=p[1], other=p[2], s_other=p[3], oracle_row=theirs[k] if k < len(theirs) else -1, rel=rel(p))


# ---- search and selection -----------------------------------------------------------------------------------------------

# per structure: (feature, minimum among the used QPs, class the minimum asks for or None)
REQUIRED = {name: [("optimal_dual_drop", 3, None), ("infeasible_dual_drop", 4, None)] for name in FLOATING}
REQUIRED["three_contact"] = REQUIRED["three_contact"] + [("dependent", 4, None)]
REQUIRED["tiago"] = [("optimal_vertex", 4, "A"), ("infeasible_dual_drop", 4, None)]
MIN_DROPS_PER_POSITION = 10
# searched for within EXTRA_SEEDS per cell, used where found, reported as not found otherwise
# (a dual-only step on a class-A QP is wanted everywhere: only there is the path itself compared)
# (a rejection is wanted on every stack, whatever its end: on Talos, Talos on one foot and iCub it is how the compact loop's refusal and restore are reached)
WANTED = {"icub": ["optimal_vertex"], "*": ["optimal_dependent", "optimal_dual_drop_A", "dependent"]}


def cells(st) -> List[Tuple[str, float, float]]:
    out = [("tight", nz, p) for nz in GRID_NOISE for p in GRID_P]
    # contradictory limits on top of tight ones: the two tight columns of the grid at the middle noise
    for fam in ("contra_bound", "contra_torque"):
        if fam == "contra_torque" and not st.act_bounds:
            continue
        out += [(fam, 5.0, p) for p in (0.6, 1.0)]
    return out


def search(name: str, oracle, verbose: bool = True) -> dict:
    """Every cell of the grid for one structure: GRID_SEEDS seeds classified, EXTRA_SEEDS looked at (unperturbed log only) and
    classified where they offer a WANTED event or a pick-after-add pair not seen yet.  Returns dict(cells=[...], candidates=[...])."""
    st = structure.STRUCTURES[name]()
    wanted = set(WANTED.get(name, []) + WANTED["*"])
    seen_pairs = set()
    out_cells, cands = [], []
    for fam, nz, p in cells(st):
        shares = dict(A=0, B=0, unused=0)
        cs = []
        n_extra = EXTRA_SEEDS
        for k in range(n_extra):
            seed = SEED0 + k
            inp = make_inputs(st, fam, nz, p, seed)
            log = oracle.tick_log(st, inp, 0)
            c = census(st, log, oracle)
            feats = features(c)
            new_pairs = set(c["pick_after_add"]) - seen_pairs
            in_grid = k < GRID_SEEDS
            if in_grid:
                cs.append(c)
            if not in_grid and not (wanted & set(feats)) and not new_pairs and "optimal_dual_drop" not in feats:
                continue
            cls, fig = classify(st, inp, seed, oracle, base=log)
            if in_grid:
                shares[cls] += 1
            if cls == "A" and "optimal_dual_drop" in feats:
                feats = feats + ["optimal_dual_drop_A"]
            if cls != "unused":
                seen_pairs |= set(c["pick_after_add"])
                cands.append(dict(structure=name, family=fam, noise=nz, p=p, seed=seed, **{"class": cls}, features=feats,
                                  iters=c["iters"], status=c["status"], max_move=fig.get("max_move", 0.0), events=brief(c),
                                  iters_lo=fig["iters_seen"][0], iters_hi=fig["iters_seen"][-1], x_stable=bool(fig["max_move_x"] <= TOL_CLASS_B),
                                  pairs=sorted(c["pick_after_add"]), drops=[c["drop_first"], c["drop_interior"], c["drop_last"]]))
        tot = census_sum(cs)
        out_cells.append(dict(family=fam, noise=nz, p=p, drawn=len(cs), shares=shares, census=tot, looked_at=n_extra))
        if verbose:
            print(name, fam, nz, p, shares, {k: tot[k] for k in ("dual_drop", "vertex", "dependent", "unbounded", "exit_none")}, flush=True)
    return dict(structure=name, cells=out_cells, candidates=cands)


def select(name: str, cands: List[dict]) -> Tuple[List[dict], List[str]]:
    """At most MAX_PER_STRUCTURE of a structure's candidates: first what REQUIRED asks for (class A before B, short runs first), then
    the WANTED events, then QPs that add a pick-after-add pair or drops at a position still short of MIN_DROPS_PER_POSITION, then the
    rest in search order.  Returns (entries, what could not be met)."""
    chosen, keys = [], set()
    order = sorted(range(len(cands)), key=lambda i: (cands[i]["class"] != "A", cands[i]["iters"], i))

    def take(i):
        e = cands[i]
        k = (e["family"], e["noise"], e["p"], e["seed"])
        if k in keys or len(chosen) >= MAX_PER_STRUCTURE or e["iters"] > 500:
            return False
        keys.add(k)
        chosen.append(e)
        return True

    unmet = []
    for feat, least, cls in REQUIRED[name]:
        got = sum(1 for e in chosen if feat in e["features"] and (cls is None or e["class"] == cls))
        for i in order:
            if got >= least + 2:  # two to spare
                break
            e = cands[i]
            if feat in e["features"] and (cls is None or e["class"] == cls) and take(i):
                got += 1
        if got < least:
            unmet.append("%s: %s %d of %d" % (name, feat, got, least))
    for feat in WANTED.get(name, []) + WANTED["*"]:
        got = 0
        for i in order:
            if got >= 3:
                break
            if feat in cands[i]["features"] and take(i):
                got += 1
    drops = np.sum([e["drops"] for e in chosen], axis=0) if chosen else np.zeros(3, int)
    while (drops < MIN_DROPS_PER_POSITION).any() and len(chosen) < MAX_PER_STRUCTURE:
        short = drops < MIN_DROPS_PER_POSITION
        gain = [(int(np.asarray(cands[i]["drops"])[short].sum()), -n) for n, i in enumerate(order)]
        best = max(range(len(order)), key=lambda n: gain[n]) if order else None
        if best is None or gain[best][0] == 0 or not take(order[best]):
            break
        drops = drops + np.asarray(cands[order[best]]["drops"])
        order = [i for i in order if i != order[best]]
    if (drops < MIN_DROPS_PER_POSITION).any():
        unmet.append("%s: drops first/interior/last %s, %d each asked" % (name, drops.tolist(), MIN_DROPS_PER_POSITION))
    pairs = set(p for e in chosen for p in e["pairs"])
    for i in order:
        if set(cands[i]["pairs"]) - pairs and take(i):
            pairs |= set(cands[i]["pairs"])
    # then one QP per (family, noise, p) cell not represented yet, class A first: the plain partial / full steps on tight inputs
    for i in order:
        e = cands[i]
        if not any((c["family"], c["noise"], c["p"]) == (e["family"], e["noise"], e["p"]) for c in chosen):
            take(i)
    entries = [dict(structure=name, family=e["family"], noise=e["noise"], p=e["p"], seed=e["seed"], status=e["status"], iters=e["iters"],
                    iters_lo=e["iters_lo"], iters_hi=e["iters_hi"], x_stable=e["x_stable"], events=e["events"],
                    **{"class": "B" if entry_key(e) in RECLASSIFIED else e["class"]}) for e in chosen]
    return entries, unmet


def comparable(e: dict) -> bool:
    """The bars written for the default inputs on the WHOLE of x and on the iteration count (tests/test_gpu_dense.py, tests/test_gi_rinv_proto.py:
    |x - x_ref|inf <= 1e-8 max(1, |x_ref|inf), the count within two of the oracle's) apply to a QP on which the reference itself keeps both under the
    perturbations: x_stable and one iteration count.  The rest is listed by the tests as not comparable on raw x and count -- the oracle's own raw
    point forces move by up to 5e-7 of |x| there, its own count by up to ten -- and is held to its status and, where OPTIMAL, to dv and the contact
    wrenches at 1e-8, the quantities class B is defined on."""
    return bool(e["x_stable"]) and e["iters_lo"] == e["iters_hi"]


def deviations(st, x, x_ref) -> Tuple[float, float, float]:
    """(whole x, dv, contact wrench): max deviation relative to max(1, |x_ref|inf) (the wrench: to max(1, |wrench|inf)), assert_parity's measures."""
    sc = max(1.0, float(np.abs(x_ref).max()))
    ex = float(np.abs(x - x_ref).max()) / sc
    ev = float(np.abs(x[:st.nv] - x_ref[:st.nv]).max()) / sc
    ew = 0.0
    if st.nc:
        T = np.asarray(st.force_gen()).reshape(st.nc, 6, 12)
        wa = np.einsum("cij,cj->ci", T, np.asarray(x)[st.nv:].reshape(st.nc, 12))
        wb = np.einsum("cij,cj->ci", T, np.asarray(x_ref)[st.nv:].reshape(st.nc, 12))
        ew = float(np.abs(wa - wb).max() / max(1.0, np.abs(wb).max()))
    return ex, ev, ew


def load_selection() -> dict:
    with open(SELECTION_PATH) as f:
        return json.load(f)


def entries_of(name: str, sel: Optional[dict] = None) -> List[dict]:
    sel = sel or load_selection()
    return [e for e in sel["qps"] if e["structure"] == name]


def f32_entries(sel: Optional[dict] = None) -> List[dict]:
    return (sel or load_selection())["f32"]


def select_f32(oracle, entries: List[dict]) -> List[dict]:
    """The iCub entries once more with every input rounded to float: oracle and classification redone on the rounded inputs."""
    st = structure.STRUCTURES["icub"]()
    out = []
    for e in entries:
        inp = entry_inputs(st, e, f32=True)
        log = oracle.tick_log(st, inp, 0)
        c = census(st, log, oracle)
        cls, fig = classify(st, inp, e["seed"], oracle, base=log)
        if cls != "unused" and c["iters"] <= 500:
            out.append(dict(e, status=c["status"], iters=c["iters"], iters_lo=fig["iters_seen"][0], iters_hi=fig["iters_seen"][-1], events=brief(c),
                            x_stable=bool(fig["max_move_x"] <= TOL_CLASS_B), **{"class": cls}))
    return out


def default_census(oracle, per_cell: int = 96) -> List[dict]:
    """The census of what the parity tests drew before: synth.generate's default tightness, task_noise 0.5 / 3 / 5, every structure."""
    out = []
    for name, mk in structure.STRUCTURES.items():
        st = mk()
        for nz in (0.5, 3.0, 5.0):
            inp = synth.generate(st, per_cell, synth.SEED_BASE.get(name, synth.SEED_BASE["icub"]), task_noise=nz)
            ref = oracle.tick_batch(st, inp, nthreads=4)
            cs = [census(st, oracle.tick_log(st, inp, i, ref), oracle) for i in range(per_cell)] if st.nin2 else []
            out.append(dict(structure=name, noise=nz, census=census_sum(cs), entered_loop=bool(st.nin2)))
    return out


def selected_census(name: str, qps: List[dict], oracle) -> dict:
    st = structure.STRUCTURES[name]()
    return census_sum([census(st, oracle.tick_log(st, entry_inputs(st, e), 0), oracle) for e in qps if e["structure"] == name])


def main():
    from concurrent.futures import ProcessPoolExecutor
    from oracle import oracle
    oracle.build()
    with ProcessPoolExecutor(max_workers=len(STRUCTS)) as pool:
        found = list(pool.map(_search_job, STRUCTS))
    qps, unmet = [], []
    for res in found:
        e, u = select(res["structure"], res["candidates"])
        qps += e
        unmet += u
    f32 = select_f32(oracle, [e for e in qps if e["structure"] == "icub"])[:8]
    os.makedirs(os.path.dirname(SELECTION_PATH), exist_ok=True)
    with open(SELECTION_PATH, "w") as f:
        json.dump(dict(seed0=SEED0, n_perturb=N_PERTURB, tol_class_b=TOL_CLASS_B, qps=qps, f32=f32, unmet=unmet), f, indent=0, sort_keys=True)
        f.write("\n")
    os.makedirs(os.path.dirname(SEARCH_PATH), exist_ok=True)
    with open(SEARCH_PATH, "w") as f:
        json.dump(dict(default_inputs=default_census(oracle),
                       search=[dict(structure=r["structure"], cells=r["cells"], candidates=len(r["candidates"])) for r in found],
                       selected={n: selected_census(n, qps, oracle) for n in STRUCTS}), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("selected", {n: len([e for e in qps if e["structure"] == n]) for n in STRUCTS}, "f32", len(f32), "unmet", unmet)


def _search_job(name):
    from oracle import oracle
    return search(name, oracle)


if __name__ == "__main__":
    main()
