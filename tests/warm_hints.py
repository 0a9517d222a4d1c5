"""Inputs and hints on which WBCQP_FLAG_WARM_START's pick rule matters, chosen by the hinted oracle alone.

Shared by tests/test_warm_hints_host.py (the hinted oracle against its own cold run, a 50-digit KKT solve, the rule itself and the numpy
model, on the CPU) and tests/test_gpu_warm_hints.py (every kernel that takes the hint against the hinted oracle).  `python -m
tests.warm_hints` runs the search and writes tests/golden/warm_hints/selection.json and profiles/warm_hints/search.json; the tests
regenerate the selected QPs by seed and never search.

The QPs are tests/solver_branches.py's (make_inputs: synth.generate with p_bnd = p_act = p, and the family with one contradictory
acceleration bound); what is new is the hint each one is solved under:
  own         the active_mask of the cold oracle's solution of the same QP (for a contra_bound QP: of the tight QP it was made from, the
              previous tick before the contradiction appeared);
  neighbour   the same of seed + 1: a stale hint, another QP's active set;
  random      256 bits drawn from the seed, with every bit at and beyond nin2 set on top;
  complement  the complement of `own` (all 256 bits: those at and beyond nin2 are set);
  ones, zeros all bits / none: by the rule both are the cold run.
An entry's class is solver_branches.classify's, from the HINTED oracle under the eight one-ulp perturbations with the hint held fixed:
  A: status, iteration count and event log unchanged;  B: status unchanged and, where OPTIMAL, dv / wrench / tau within TOL_CLASS_B.
An INFEASIBLE run returns no solution, so both classes ask for the status alone there (class A for the iteration count as well); the
required count of infeasible entries takes either.

One more condition on class A, which the perturbations cannot see (sign_ties): the rule has a hard threshold -- a hinted row stands iff its s < 0,
however little -- and a friction facet of a contact point that carries no force has s = 0 EXACTLY at a vertex its three sister facets describe
(tests/util.py:assert_parity says the same of the masks): what the oracle computes there is rounding noise, 4e-14 on |x| = 439, whose sign no
one-ulp perturbation of the inputs flips (401 of 401 runs keep it) and any other order of the same sums may.  Flipped, the row is picked at once
where no other hinted row stands: a step of length zero, an add and a drop, one more iteration, the same solution.  So at every pick the
oracle's OWN iterate is looked at (the run cut short by max_iter), and an entry is class A only if no pick was decided by the sign of such a
zero: |s_i| <= SIGN_TIE (|CI_i|_1 max(1, |x|inf) + |ci0_i|) -- relative to the whole of x, assert_parity's measure, because the forces of such a
point are themselves noise of the solve for all of x.  Otherwise it is filed under B (sign_ties is counted for class-A candidates only).
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from inria_wbc_amd import structure, synth
from tests import solver_branches as sb

HERE = os.path.dirname(os.path.abspath(__file__))
SELECTION_PATH = os.path.join(HERE, "golden", "warm_hints", "selection.json")
SEARCH_PATH = os.path.join(os.path.dirname(HERE), "profiles", "warm_hints", "search.json")

STRUCTS = ("talos", "talos_single_support", "icub", "tiago")
FLOATING = ("talos", "talos_single_support", "icub")
HINT_KINDS = ("own", "neighbour", "random", "complement", "ones", "zeros")
HOSTILE = ("own", "neighbour", "random", "complement")  # the kinds whose run may leave the cold run's path
SEED0 = sb.SEED0
CELL_HOSTILE, CELL_HEAVY, CELL_INFEASIBLE = ("tight", 2.0, 0.3), ("tight", 5.0, 0.6), ("contra_bound", 5.0, 0.6)
GRID_SEEDS, EXTRA_SEEDS = 12, 48  # seeds per cell; seeds per cell looked at when a required count is not met within the grid
HEAVY_ITERS = 20
MAX_PER_STRUCTURE = sb.MAX_PER_STRUCTURE
MAX_F32 = 12
SIGN_TIE = sb.NEAR_TIE  # |s_i| <= SIGN_TIE (|CI_i|_1 max(1, |x|inf) + |ci0_i|): s is zero to rounding (two correct loops' iterates agree to 1e-13 here; the parity bar is 1e-8)
CHAIN = dict(structure="talos", batch=16, t0=40, ticks=3)  # tests/test_gpu_warm.py's squat stream: tick t0 cold, then `ticks` hinted ticks

# per structure: (feature, minimum).  Conditions, not measurements.
REQUIRED = {name: [("hostile_" + k, 3) for k in HOSTILE] for name in STRUCTS}
for _n in FLOATING:
    REQUIRED[_n] = REQUIRED[_n] + [("heavy_own", 4), ("infeasible_hostile", 3)]
for _n in ("talos", "talos_single_support"):  # the structures with actuation bounds
    REQUIRED[_n] = REQUIRED[_n] + [("actuation_pick", 2)]


# ---- hints --------------------------------------------------------------------------------------------------------------

def hint_bits(hint, nin2: int) -> np.ndarray:
    """bool [nin2]: the rows a hint names (bits at and beyond min(nin2, 256) mean nothing)."""
    w = np.ascontiguousarray(np.asarray(hint, np.uint32).reshape(8))
    bits = np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)
    out = np.zeros(nin2, bool)
    out[:min(nin2, 256)] = bits[:min(nin2, 256)]
    return out


def cleared_beyond(hint, nin2: int) -> np.ndarray:
    """The hint with every bit at and beyond nin2 cleared."""
    w = np.ascontiguousarray(np.asarray(hint, np.uint32).reshape(-1, 8)).copy()
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")
    bits[:, nin2:] = 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(np.asarray(hint).shape)


def beyond_mask(nin2: int) -> np.ndarray:
    """8 words with exactly the bits at and beyond nin2 set."""
    bits = np.zeros(256, np.uint8)
    bits[nin2:] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def cold_mask(st, noise: float, p: float, seed: int, oracle) -> np.ndarray:
    """active_mask of the cold oracle's run of the TIGHT QP (noise, p, seed)."""
    return oracle.tick_batch(st, sb.make_inputs(st, "tight", noise, p, seed))["active_mask"][0].copy()


def make_hint(st, kind: str, noise: float, p: float, seed: int, oracle) -> np.ndarray:
    if kind == "own":
        return cold_mask(st, noise, p, seed, oracle)
    if kind == "neighbour":
        return cold_mask(st, noise, p, seed + 1, oracle)
    if kind == "random":
        rng = np.random.default_rng([seed, 0xA17])
        return rng.integers(0, 2 ** 32, size=8, dtype=np.uint64).astype(np.uint32) | beyond_mask(st.nin2)
    if kind == "complement":
        return ~cold_mask(st, noise, p, seed, oracle)
    if kind == "ones":
        return np.full(8, 0xffffffff, np.uint32)
    assert kind == "zeros", kind
    return np.zeros(8, np.uint32)


# ---- what a hinted log says ------------------------------------------------------------------------------------------------

def replay(log: dict, oracle) -> List[Tuple[int, int, set, set]]:
    """Per PICK event of a log: (outer iteration from 1, row, rows active just before the pick, rows excluded at it), from the log's own events."""
    A, A_l1, excl, after_dep, out, it = [], [], set(), False, [], 0
    for code, row, pos, iq in log["events"].tolist():
        if code == oracle.EV_PICK:
            if not after_dep:  # a new outer iteration: the exclusions are lifted, the set is the one a rejection goes back to
                A_l1, excl, it = list(A), set(), it + 1
            after_dep = False
            out.append((it, row, set(A), set(excl)))
        elif code == oracle.EV_FULL_ADD:
            A.append(row)
        elif code in (oracle.EV_PARTIAL_DROP, oracle.EV_DUAL_DROP):
            A.remove(row)
        elif code == oracle.EV_DEPENDENT:
            excl.add(row)
            A, after_dep = list(A_l1), True
    return out


def oracle_iterate(st, inp: Dict[str, np.ndarray], hint, it: int, oracle) -> np.ndarray:
    """The oracle's x at the start of outer iteration `it` (from 1) of QP 0: the same run stopped by max_iter = it."""
    import copy
    cut = copy.copy(st)
    cut.max_iter = it
    return oracle.tick_batch(cut, inp, hint=None if hint is None else np.asarray(hint, np.uint32).reshape(1, 8))["x"][0]


def sign_ties(st, inp: Dict[str, np.ndarray], hint, log: dict, oracle) -> int:
    """Picks of a hinted log that the sign of a rounding-noise s decided (the module's docstring): no hinted row stood and a hinted, inactive,
    non-excluded row had 0 <= s <= SIGN_TIE scale, or every hinted row that stood had |s| <= SIGN_TIE scale."""
    if hint is None:
        return 0
    hb = hint_bits(hint, st.nin2)
    if not hb.any():
        return 0
    _, _, _, _, CI, ci0 = oracle.assemble(st, inp, 0)
    n, x, at = 0, None, -1
    for it, row, active, excl in replay(log, oracle):
        if it != at:
            x, at = oracle_iterate(st, inp, hint, it, oracle), it
        s = CI @ x + ci0
        scale = np.abs(CI).sum(axis=1) * max(1.0, float(np.abs(x).max())) + np.abs(ci0)
        free = hb.copy()
        free[list(active | excl)] = False
        noise = free & (np.abs(s) <= SIGN_TIE * scale)
        stood = free & (s < 0.0)
        n += int(noise.any() and not (stood & ~noise).any())
    return n


def classify(st, inp: Dict[str, np.ndarray], seed: int, oracle, hint, base: Optional[dict] = None) -> Tuple[str, dict]:
    """sb.classify with the hint held fixed, and class A only where no pick was decided by the sign of a zero (fig['sign_ties'])."""
    base = base or oracle.tick_log(st, inp, 0, hint=hint)
    cls, fig = sb.classify(st, inp, seed, oracle, base=base, hint=hint)
    fig["sign_ties"] = sign_ties(st, inp, hint, base, oracle) if cls == "A" else 0
    if cls == "A" and fig["sign_ties"]:
        cls = "B" if fig["max_move"] <= sb.TOL_CLASS_B else "unused"
    return cls, fig

def hinted_census(st, log: dict, cold: dict, hint, oracle) -> dict:
    """sb.census of a hinted log plus: does it differ from the cold log; picks of hinted rows, those on actuation rows; rejections of hinted rows."""
    c = sb.census(st, log, oracle)
    hb = hint_bits(hint, st.nin2)
    kinds = sb.row_kinds(st)
    torque = sb.KINDS.index("torque")
    ev = log["events"].tolist()
    c["differs"] = not np.array_equal(log["events"], cold["events"])
    c["hinted_picks"] = sum(1 for code, row, _, _ in ev if code == oracle.EV_PICK and hb[row])
    c["actuation_hinted_picks"] = sum(1 for code, row, _, _ in ev if code == oracle.EV_PICK and hb[row] and kinds[row] == torque)
    c["dependent_hinted"] = sum(1 for code, row, _, _ in ev if code == oracle.EV_DEPENDENT and hb[row])
    c["cold_iters"] = int(cold["iters"])
    return c


def features(e: dict) -> List[str]:
    """The required conditions an entry (or a candidate) meets."""
    f = []
    cell = (e["family"], e["noise"], e["p"])
    if e["status"] == sb.OPTIMAL and e["class"] == "A" and e["differs"] and e["kind"] in HOSTILE and e["family"] == "tight":
        f.append("hostile_" + e["kind"])
    if e["kind"] == "own" and cell == CELL_HEAVY and e["cold_iters"] >= HEAVY_ITERS and e["status"] == sb.OPTIMAL:
        f.append("heavy_own")
    if e["actuation_hinted_picks"] and e["differs"] and e["status"] == sb.OPTIMAL:
        f.append("actuation_pick")
    if e["family"] == "contra_bound" and e["status"] == sb.INFEASIBLE and e["kind"] in HOSTILE and e["kind"] != "own":
        f.append("infeasible_hostile")
    if e["dependent_hinted"]:
        f.append("dependent_hinted")
    if e["kind"] in ("ones", "zeros"):
        f.append(e["kind"])
    if e["sign_ties"]:
        f.append("sign_tied")
    return f


def entry_of(st, name: str, family: str, noise: float, p: float, seed: int, kind: str, hint, oracle, f32: bool = False,
             cold: Optional[dict] = None) -> Optional[dict]:
    """The entry of one (QP, hint): hinted log, census and class.  None where the class is 'unused' or the run is long."""
    inp = sb.make_inputs(st, family, noise, p, seed)
    if f32:
        inp = {k: v.astype(np.float32).astype(np.float64) for k, v in inp.items()}
    cold = cold or oracle.tick_log(st, inp, 0)
    log = oracle.tick_log(st, inp, 0, hint=hint)
    c = hinted_census(st, log, cold, hint, oracle)
    cls, fig = classify(st, inp, seed, oracle, hint, base=log)
    if cls == "unused" or c["iters"] > 500:
        return None
    return dict(structure=name, family=family, noise=noise, p=p, seed=seed, kind=kind, hint=[int(w) for w in np.asarray(hint, np.uint32)],
                status=c["status"], iters=c["iters"], iters_lo=fig["iters_seen"][0], iters_hi=fig["iters_seen"][-1], **{"class": cls},
                x_stable=bool(fig["max_move_x"] <= sb.TOL_CLASS_B), events=sb.brief(c), differs=bool(c["differs"]), cold_iters=c["cold_iters"],
                sign_ties=fig["sign_ties"],
                hinted_picks=c["hinted_picks"], actuation_hinted_picks=c["actuation_hinted_picks"], dependent_hinted=c["dependent_hinted"])


# ---- search and selection --------------------------------------------------------------------------------------------------

def cells(name: str) -> List[Tuple[str, float, float]]:
    out = [CELL_HOSTILE, CELL_HEAVY]
    if name in FLOATING:
        out.append(CELL_INFEASIBLE)
    return out


def search(name: str, oracle, n_seeds: int = GRID_SEEDS, verbose: bool = True) -> dict:
    """Every (cell, seed, hint kind) of one structure.  Returns dict(structure, seeds, census=[per cell and kind], candidates=[entries])."""
    st = structure.STRUCTURES[name]()
    cands, out = [], []
    for fam, nz, p in cells(name):
        per_kind = {k: dict(A=0, B=0, unused=0, sign_tied=0, differs=0, differs_A=0, optimal=0, infeasible=0, other_status=0, dependent_hinted=0, actuation_pick=0,
                            heavy=0, iters=0, cold_iters=0) for k in HINT_KINDS}
        for k in range(n_seeds):
            seed = SEED0 + k
            cold = oracle.tick_log(st, sb.make_inputs(st, fam, nz, p, seed), 0)
            for kind in HINT_KINDS:
                hint = make_hint(st, kind, nz, p, seed, oracle)
                e = entry_of(st, name, fam, nz, p, seed, kind, hint, oracle, cold=cold)
                t = per_kind[kind]
                if e is None:
                    t["unused"] += 1
                    continue
                t[e["class"]] += 1
                t["differs"] += int(e["differs"])
                t["sign_tied"] += int(e["sign_ties"] > 0)
                t["differs_A"] += int(e["differs"] and e["class"] == "A")
                t["optimal" if e["status"] == sb.OPTIMAL else "infeasible" if e["status"] == sb.INFEASIBLE else "other_status"] += 1
                t["dependent_hinted"] += int(e["dependent_hinted"] > 0)
                t["actuation_pick"] += int("actuation_pick" in features(e))
                t["heavy"] += int(e["cold_iters"] >= HEAVY_ITERS)
                t["iters"] += e["iters"]
                t["cold_iters"] += e["cold_iters"]
                cands.append(e)
        out.append(dict(family=fam, noise=nz, p=p, seeds=n_seeds, kinds=per_kind))
        if verbose:
            print(name, fam, nz, p, {k: (v["A"], v["B"], v["differs_A"], v["dependent_hinted"]) for k, v in per_kind.items()}, flush=True)
    return dict(structure=name, seeds=n_seeds, census=out, candidates=cands)


def select(name: str, cands: List[dict]) -> Tuple[List[dict], List[str]]:
    """At most MAX_PER_STRUCTURE candidates that meet REQUIRED[name] with one to spare where there is room, then a rejected hinted row
    and a run decided by the sign of a zero where the search found one, then one all-ones and one all-zeros hint.  Class A and short runs first.  Returns (entries, what is unmet)."""
    chosen, keys = [], set()
    order = sorted(range(len(cands)), key=lambda i: (cands[i]["class"] != "A", not cands[i]["differs"], cands[i]["iters"], i))

    def take(i):
        e = cands[i]
        k = (e["family"], e["noise"], e["p"], e["seed"], e["kind"])
        if k in keys or len(chosen) >= MAX_PER_STRUCTURE:
            return False
        keys.add(k)
        chosen.append(e)
        return True

    def fill(feat, least):
        got = sum(1 for e in chosen if feat in features(e))
        for i in order:
            if got >= least:
                break
            if feat in features(cands[i]) and take(i):
                got += 1
        return got

    unmet = []
    for feat, least in sorted(REQUIRED[name], key=lambda r: r[0] != "heavy_own"):  # heavy first: an own entry there serves hostile_own too
        got = fill(feat, least)
        if got < least:
            unmet.append("%s: %s %d of %d" % (name, feat, got, least))
    fill("dependent_hinted", 2)
    fill("sign_tied", 1)  # (class B by the sign of a zero: the answer is still held to the parity bars)
    fill("ones", 1)
    fill("zeros", 1)
    for feat, least in REQUIRED[name]:  # one to spare where there is room
        if len(chosen) < MAX_PER_STRUCTURE - 2:
            fill(feat, least + 1)
    return chosen, unmet


def select_f32(oracle, entries: List[dict]) -> List[dict]:
    """The iCub entries once more with every input rounded to float: oracle, census and class redone on the rounded inputs, the hint kept."""
    st = structure.STRUCTURES["icub"]()
    out = []
    for e in entries:
        r = entry_of(st, "icub", e["family"], e["noise"], e["p"], e["seed"], e["kind"], np.asarray(e["hint"], np.uint32), oracle, f32=True)
        if r is not None and len(out) < MAX_F32:
            out.append(r)
    return out


# ---- the chain --------------------------------------------------------------------------------------------------------------

def chain_inputs(st, B: int, t: int) -> Dict[str, np.ndarray]:
    """Tick t of tests/test_gpu_warm.py's squat stream: synth's default Talos QPs with the CoM task's right-hand side following the squat."""
    inputs = synth.generate(st, B, synth.SEED_BASE["talos"])
    com_rows = np.where(st.dense_row_task == st.task_names.index("com"))[0]
    idx = (np.arange(B) + t) % 4000
    rhs = np.stack([synth.squat_com_rhs(st, int(i), st.kp.get("com", 30.0)) for i in idx])
    d = {k: v.copy() for k, v in inputs.items()}
    d["b1"][:, com_rows] += rhs[:, :com_rows.size]
    return d


def chain(oracle, classified: bool = False) -> List[dict]:
    """The oracle's chain: tick t0 cold, then CHAIN['ticks'] ticks each hinted with the HINTED oracle's mask of the tick before.
    Returns per tick dict(t, inputs, hint, ref) (the cold tick first, hint None); classified: plus `classes`, one per QP, hint held fixed."""
    st = structure.STRUCTURES[CHAIN["structure"]]()
    B, t0 = CHAIN["batch"], CHAIN["t0"]
    out, hint = [], None
    for t in range(t0, t0 + CHAIN["ticks"] + 1):
        inp = chain_inputs(st, B, t)
        ref = oracle.tick_batch(st, inp, hint=hint)
        rec = dict(t=t, inputs=inp, hint=hint, ref=ref)
        if classified:
            rec["classes"] = [classify(st, {k: v[i:i + 1] for k, v in inp.items()}, 7000 + t * B + i, oracle,
                                       None if hint is None else hint[i])[0] for i in range(B)]
        out.append(rec)
        hint = ref["active_mask"].copy()
    return out


def chain_record(oracle) -> dict:
    ticks = chain(oracle, classified=True)
    return dict(CHAIN, status=[[int(v) for v in r["ref"]["status"]] for r in ticks], iters=[[int(v) for v in r["ref"]["iters"]] for r in ticks],
                classes=[r["classes"] for r in ticks])


# ---- access -----------------------------------------------------------------------------------------------------------------

def load_selection() -> dict:
    with open(SELECTION_PATH) as f:
        return json.load(f)


def entries_of(name: str, sel: Optional[dict] = None) -> List[dict]:
    return [e for e in (sel or load_selection())["qps"] if e["structure"] == name]


def hints_of(entries: List[dict]) -> np.ndarray:
    return np.asarray([e["hint"] for e in entries], np.uint32).reshape(len(entries), 8)


def main():
    from concurrent.futures import ProcessPoolExecutor
    from oracle import oracle
    oracle.build()
    with ProcessPoolExecutor(max_workers=len(STRUCTS)) as pool:
        found = list(pool.map(_search_job, [(n, GRID_SEEDS) for n in STRUCTS]))
        picked = [select(r["structure"], r["candidates"]) for r in found]
        again = [r["structure"] for r, (_, u) in zip(found, picked) if u]
        if again:  # a count not met inside the grid: more seeds, as solver_branches' EXTRA_SEEDS
            print("not met within %d seeds:" % GRID_SEEDS, [u for _, u in picked if u], "-> %d seeds" % EXTRA_SEEDS, flush=True)
            wide = dict(zip(again, pool.map(_search_job, [(n, EXTRA_SEEDS) for n in again])))
            found = [wide.get(r["structure"], r) for r in found]
            picked = [select(r["structure"], r["candidates"]) for r in found]
    qps = [e for entries, _ in picked for e in entries]
    unmet = [u for _, us in picked for u in us]
    f32 = select_f32(oracle, [e for e in qps if e["structure"] == "icub"])
    os.makedirs(os.path.dirname(SELECTION_PATH), exist_ok=True)
    with open(SELECTION_PATH, "w") as f:
        json.dump(dict(seed0=SEED0, n_perturb=sb.N_PERTURB, tol_class_b=sb.TOL_CLASS_B, qps=qps, f32=f32, chain=chain_record(oracle), unmet=unmet),
                  f, indent=0, sort_keys=True)
        f.write("\n")
    os.makedirs(os.path.dirname(SEARCH_PATH), exist_ok=True)
    with open(SEARCH_PATH, "w") as f:
        json.dump(dict(search=[dict(structure=r["structure"], seeds=r["seeds"], cells=r["census"], candidates=len(r["candidates"])) for r in found],
                       selected={n: {feat: sum(1 for e in qps if e["structure"] == n and feat in features(e))
                                     for feat in [r[0] for r in REQUIRED[n]] + ["dependent_hinted", "sign_tied", "ones", "zeros"]} for n in STRUCTS},
                       unmet=unmet), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("selected", {n: len([e for e in qps if e["structure"] == n]) for n in STRUCTS}, "f32", len(f32), "unmet", unmet)


def _search_job(arg):
    from oracle import oracle
    return search(arg[0], oracle, n_seeds=arg[1])


if __name__ == "__main__":
    main()
