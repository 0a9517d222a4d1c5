"""Every solve kernel at the edges of the sizes its host code admits: the case tables, the stack builders and the reference-side checks.

Shared by tests/test_size_edges_host.py (what concerns the reference and the host's layout arithmetic alone, on the CPU) and
tests/test_gpu_size_edges.py (the kernels against the oracle).  `python -m tests.size_edges` prints what the tables record -- the layout the
library reports per stack, the oracle's census per batch, the dense seam's seeds -- so that a changed recipe can be re-recorded; the tests
recompute all of it and compare.

  A  SMALL_CASES    one wavefront per QP (csrc/wbcqp_small.hpp, small_ok): fixed base, n = nv from 1 to 16; each batch also runs the compact and the
                    full four-wave kernels (FLAG_WORKGROUP_PER_QP, | FLAG_FULL_LDS), which the host admits at these sizes too
  B  COMPACT_CASES  the limits of derive_compact's envelope and the first stack past each
  C  DENSE_SIZES    the dense seam (wbcqp_solve_dense): tiny n, neq = n, more than 256 rows, the largest n that fits
  D  REFUSALS       stacks wbcqp_set_structure refuses, with the documented code
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np

from inria_wbc_amd import structure as S
from inria_wbc_amd import synth
from tests import solver_branches as sb

INVALID, UNSUPPORTED = 1, 3  # WBCQP_ERR_INVALID, WBCQP_ERR_UNSUPPORTED (include/wbcqp.h)


# ---- stacks ---------------------------------------------------------------------------------------------------------------------

def stack(name, nv, na, n_contacts, act, fmax=1500.0):
    """A humanoid-like stack of any size through structure._mk: 27 dense rows, posture, bounds, actuation bounds if `act`, n_contacts 6-D contacts
    (normal force within [5, fmax])."""
    pts = S.contact6d_points(lxn=0.06, lyn=0.045, lxp=0.14, lyp=0.045, lz=0.065)
    contacts = [S.Contact("contact_%d" % c, pts, (0.0, 0.0, 1.0), 0.3, 5.0, fmax) for c in range(n_contacts)]
    dense = [("lh", 6, 1.0), ("rh", 6, 1.0), ("lf", 6, 100.0), ("com", 3, 1000.0), ("momentum", 2, 100.0), ("__posture__", "posture", 0.5), ("torso", 3, 1.0),
             ("__contacts__",)]
    level0 = [(S.INEQ_BOUNDS, 0)] + ([(S.INEQ_ACTUATION, 0)] if act else []) + [(S.INEQ_FORCE, c) for c in range(n_contacts)]
    return S._mk(name, nv, na, contacts, dense, None, [("self_collision-a", 500.0)], True, act, level0, {"com": 30.0, "posture": 10.0})


SMALL_WEIGHTS = (1500.0, 500.0, 1000.0, 250.0)  # Tiago's magnitudes (etc/tiago/tasks.yaml), cycled over a stack's dense tasks
POSTURE_WEIGHT = 0.1


def small_stack(name, nv, dense, posture, bounds=True):
    """A fixed-base arm: dense tasks of `dense` rows each, a posture task over every joint if `posture`, acceleration bounds if `bounds`."""
    tasks = [("task_%d" % i, rows, SMALL_WEIGHTS[i % len(SMALL_WEIGHTS)]) for i, rows in enumerate(dense)]
    if posture:
        tasks.append(("__posture__", "posture", POSTURE_WEIGHT))
    st = S._mk(name, nv, nv, [], tasks, None, [], bounds, False, [(S.INEQ_BOUNDS, 0)] if bounds else [])
    if not posture:
        assert st.n_sel == 0
    return st


# ---- A: one wavefront per QP ------------------------------------------------------------------------------------------------------

SMALL_BATCH = 64
SMALL_RECIPE = dict(task_noise=30.0, p_bnd=0.3)  # tests/test_gpu_small.py::test_odd_sizes_on_the_four_wave_compact_kernel's
SMALL_SEED = 13_000_000


@dataclasses.dataclass(frozen=True)
class SmallCase:
    id: str
    nv: int
    dense: Tuple[int, ...]
    posture: bool
    bounds: bool = True
    recipe: Optional[dict] = None  # None: SMALL_RECIPE
    needs: Tuple[str, ...] = ()    # what the oracle must do on the batch (host test): "vertex", "drop", "drop_positions", "adds_only"
    lds_bytes: int = 0             # wbcqp_layout_of's answer: the four-wave (compact) workgroup's LDS; the one-wave kernel's block is fixed
    waves_per_cu: int = 0
    skipped: Tuple[int, ...] = ()  # seeds (offsets from the case's first) the batch leaves out: batch_of's rule

    batch = SMALL_BATCH

    def stack(self):
        return small_stack("edge_" + self.id, self.nv, self.dense, self.posture, self.bounds)

    def seed0(self):
        return SMALL_SEED + 1000 * SMALL_CASES.index(self)

    def recipe_(self):
        return self.recipe or SMALL_RECIPE


SMALL_CASES: List[SmallCase] = [
    SmallCase("n1_row_posture", 1, (1,), True, needs=("vertex",), lds_bytes=23264, waves_per_cu=2),
    SmallCase("n1_posture_only", 1, (), True, needs=("vertex",), lds_bytes=22736, waves_per_cu=2),                 # n_dense = 0: lenA == 0
    # n_sel = 0.  Rank-one H + regulariser on the skipped seeds: the oracle's own x moves by 1.4e-6 .. 1.8e-5 under one ulp of its inputs
    SmallCase("n2_two_rows", 2, (2,), False, needs=("vertex",), lds_bytes=23792, waves_per_cu=2, skipped=(20, 31, 33, 65)),
    SmallCase("n3", 3, (6,), True, lds_bytes=25904, waves_per_cu=2),
    SmallCase("n4", 4, (6,), True, lds_bytes=25904, waves_per_cu=2),
    SmallCase("n6", 6, (6,), True, needs=("drop",), lds_bytes=25904, waves_per_cu=2),
    SmallCase("n7", 7, (6,), True, needs=("drop",), lds_bytes=25904, waves_per_cu=2),
    SmallCase("n8", 8, (6,), True, needs=("drop",), lds_bytes=25904, waves_per_cu=2),                              # the last n of one elimination block
    SmallCase("n9", 9, (6,), True, needs=("drop",), lds_bytes=25904, waves_per_cu=2),                              # the first of two
    SmallCase("n16_full", 16, (4, 4, 4, 4), True, needs=("drop_positions",), lds_bytes=31184, waves_per_cu=2),     # r1 = 32, nin2 = 32, lenA = 256
    # posture only: H is diagonal and every bound's normal a coordinate axis, so the active normals are H^-1-orthogonal and no step ever drops a
    # constraint, whatever the noise (tried up to task_noise 300, p_bnd 1): this stack covers adds only ...
    SmallCase("n16_posture_only", 16, (), True, needs=("adds_only",), lds_bytes=22736, waves_per_cu=2),
    # ... and with every bound tight it adds until iq = n = 16: the full step onto a vertex at the largest n (RI, A, U filled to their last entry)
    SmallCase("n16_posture_only_tight", 16, (), True, recipe=dict(task_noise=30.0, p_bnd=1.0), needs=("adds_only", "vertex"), lds_bytes=22736, waves_per_cu=2),
    SmallCase("n16_rows_only", 16, (4, 4, 4, 4), False, needs=("drop_positions",), lds_bytes=31184, waves_per_cu=2),
    SmallCase("n16_no_bounds", 16, (4, 4, 4, 4), True, bounds=False, lds_bytes=31184, waves_per_cu=2),             # nin2 = 0: the `else` of the loop
    SmallCase("n16_sixteen_tasks", 16, (1,) * 16, False, needs=("drop",), lds_bytes=31184, waves_per_cu=2),        # n_tasks = 16
]


# ---- B: the compact envelope --------------------------------------------------------------------------------------------------------

COMPACT_BATCH = 48
COMPACT_RECIPE = dict(task_noise=1.5, p_act=0.3, p_bnd=0.2)  # tests/test_gpu_layout_variants.py's
COMPACT_SEED = 14_000_000


def in_compact_envelope(st) -> bool:
    """derive_compact's eligibility (csrc/wbcqp_host_derive.hpp), restated: what the table's `layout` column is checked against."""
    one_act_block = sum(1 for k, _ in st.ineq_blocks if k == S.INEQ_ACTUATION) == 1
    return (not st.dense_h and st.n <= 78 and st.neq <= 22 and st.nv <= 52 and st.nc <= 2 and st.nu <= 8 and st.na <= 64 and st.n_bound <= 64 and
            st.nin2 <= 256 and st.r1 <= 128 and st.n_tasks <= 64 and (not st.act_bounds or one_act_block) and st.n - st.neq <= 64 and
            not (st.act_bounds and st.n <= 62 and st.nv - 41 >= st.neq))  # (the last clause: the published actuation row's padding, below)


@dataclasses.dataclass(frozen=True)
class CompactCase:
    id: str
    nv: int
    na: int
    nc: int
    act: bool
    why: str
    layout: str                    # "compact" | "full" | "refused": what wbcqp_layout_of / wbcqp_set_structure answer
    lds_bytes: int = 0
    waves_per_cu: int = 0
    error: str = ""                # refused: a fragment of the error text (the code is UNSUPPORTED)
    recipe: Optional[dict] = None  # None: COMPACT_RECIPE
    bound_all: bool = False        # acceleration bounds on every velocity column, the base's included (n_bound = nv)
    fmax: float = 1500.0           # the contacts' largest normal force
    skipped: Tuple[int, ...] = ()  # seeds (offsets from the case's first) the batch leaves out: batch_of's rule

    batch = COMPACT_BATCH

    def stack(self):
        st = stack("edge_" + self.id, self.nv, self.na, self.nc, self.act, self.fmax)
        if self.bound_all:
            st = dataclasses.replace(st, bound_col=np.arange(self.nv, dtype=np.int32))
        return st

    def seed0(self):
        return COMPACT_SEED + 1000 * COMPACT_CASES.index(self)

    def recipe_(self):
        return self.recipe or COMPACT_RECIPE


# A stack is admitted only if its FULL layout fits the 160 KiB of a CU (derive runs before derive_compact, and FLAG_FULL_LDS must have a layout to run):
# with two contacts and a floating base that ends just above Talos' size (nv 50: 163 472 bytes of 163 840), so the envelope's corners nv = 52 with
# nin2 = 256 or nu = 8 are refused although derive_compact would take them.  The library's answer is what is recorded; the limits themselves -- row 255,
# nu = 8 -- are reached by the largest stacks that are admitted (the two *_talos_size cases).
FULL_OVER = "QP does not fit the 160 KiB LDS of one CU"
TIGHT_BOUNDS = dict(task_noise=1.5, p_act=0.3, p_bnd=0.5)  # stacks without actuation bounds drop once or twice per batch at p_bnd = 0.2
COMPACT_CASES: List[CompactCase] = [
    CompactCase("nin2_256", 52, 47, 2, True, "nin2 = 4 x 47 + 68 = 256: one-sided row 255 exists", "refused", error=FULL_OVER),
    # (row 255 is the last contact's normal force against fmax: 650 N is just above the 640 N synth's feasible point can carry, so the QPs stay feasible
    # by construction and the unconstrained minimiser of a few of them asks for more)
    CompactCase("nin2_256_talos_size", 50, 44, 2, True, "nin2 = 2 x 50 + 2 x 44 + 68 = 256 on the largest floating-base stack admitted", "compact", 71616, 2, bound_all=True,
                fmax=650.0),
    CompactCase("nin2_260", 52, 48, 2, True, "the first stack past it", "refused", error=FULL_OVER),
    CompactCase("nu8", 52, 44, 2, True, "nu = 8, nv = 52, n = 76", "refused", error=FULL_OVER),
    CompactCase("nu8_nv48", 48, 40, 2, True, "nu = 8 on the largest such stack admitted: n = 72, neq = 20", "compact", 68768, 2),
    CompactCase("nu9", 38, 29, 2, False, "nu = 9, neq = 21", "full", 135008, 1),
    CompactCase("nu0_free64", 52, 52, 2, False, "fully actuated with contacts; n - neq = 64 exactly", "compact", 78400, 2, recipe=TIGHT_BOUNDS),
    CompactCase("free65", 53, 53, 1, False, "nv = 53 > 52, the first nv past the envelope (n = 65, n - neq = 59: with nv <= 52 and nc <= 2 no stack has n - neq > 64)", "full", 132176, 1, recipe=TIGHT_BOUNDS),
    CompactCase("flight_act", 38, 32, 0, True, "floating base, no contact: neq = nu = 6, k = 0", "compact", 39520, 2),
    CompactCase("flight", 38, 32, 0, False, "... without actuation bounds", "compact", 38496, 2, recipe=TIGHT_BOUNDS),
    CompactCase("one_contact_nu0", 30, 30, 1, True, "neq = 6 from the contact alone", "compact", 42416, 2),
    # A fixed base at nv = 52 is inside every limit of the envelope, and the compact loop was wrong on it (dv off by 2.1 of |x| on the device): publishing an
    # actuation row stores its padding up to entry nv + 23 of np, which with 64-entry slots (n <= 62) and nv > 40 reaches the first nv - 40 entries of the
    # slot behind it, d -- live from entry neq on.  derive_compact now leaves such a stack (actuation bounds, n <= 62, nv - 41 >= neq) on the full layout.
    CompactCase("fixed52", 52, 52, 0, True, "fixed base at nv = 52, nin2 = 208: kept on the full layout (the published row's padding)", "full", 102976, 1),
    CompactCase("fixed40", 40, 40, 0, True, "the largest fixed base with actuation bounds the compact layout takes: entry nv + 23 ends its slot", "compact", 42176, 2),
]
ROW_255_CASE = "nin2_256_talos_size"


# ---- shared: batches and reference runs, computed once and left unchanged ---------------------------------------------------------------
#
# A batch is the first `batch` seeds from the case's first on whose QP the REFERENCE ITSELF keeps what the parity bar measures: under the oracle's eight
# one-ulp perturbations (solver_branches.classify) the status stays and, where OPTIMAL, dv, contact wrench and tau move by at most TOL_CLASS_B = 1e-10, a
# hundredth of the bar.  A seed that does not is skipped (the table records which: `skipped`); no figure of the device enters the choice.  Why at all: a
# stack with fewer level-1 rows than variables has an H of rank < n plus the 1e-8 regulariser -- n2_two_rows draws QPs with cond(H) = 1e11 on which one ulp
# of the inputs moves the oracle's own x by 1.8e-5 of its size; nothing can be held to 1e-8 of a number its definition leaves open at 1e-5.
MAX_SKIPPED = 4  # per batch: one QP in sixteen (A), one in twelve (B)

# class-A QPs by the perturbations on which a loop's count differed from the oracle's and the paths part at a pick whose two candidates' s differ by less
# than solver_branches.NEAR_TIE relative (1e-9): the last bits of s decide and eight perturbations happened not to flip them -- solver_branches.RECLASSIFIED's
# rule.  Filed as not class A; tests/test_size_edges_host.py checks that the near tie is there.  (case, seed): what was seen
RECLASSIFIED: Dict[Tuple[str, int], str] = {
    ("one_contact_nu0", 14_010_019): "compact layout: 31 iterations against the oracle's 32; pick 9 takes friction facet 143 where the oracle takes facet 142 of the same "
                                     "contact point: s = -26.061201423109768 against -26.061201423109488, 1.1e-14 relative",
}

_REF: Dict[str, tuple] = {}


def batch_of(case, oracle):
    """(inputs [batch, len], class A [batch] bool, skipped seed offsets, seeds) of a case: see above."""
    st = case.stack()
    ones, cls_a, skipped, seeds = [], [], [], []
    k = 0
    while len(ones) < case.batch:
        seed = case.seed0() + k
        one = synth.generate(st, 1, seed, **case.recipe_())
        cls, fig = sb.classify(st, one, seed, oracle)
        if cls != "unused" and fig.get("max_move", np.inf) <= sb.TOL_CLASS_B:
            ones.append(one)
            cls_a.append(cls == "A" and (case.id, seed) not in RECLASSIFIED)
            seeds.append(seed)
        else:
            skipped.append(k)
            assert len(skipped) <= MAX_SKIPPED, (case.id, skipped)
        k += 1
    inputs = {f: np.concatenate([o[f] for o in ones], axis=0) for f in synth.FIELDS}
    return inputs, np.asarray(cls_a, bool), tuple(skipped), seeds


def reference(case, oracle):
    """(st, inputs, oracle outputs) of a case's batch."""
    if case.id not in _REF:
        st = case.stack()
        inputs, cls_a, skipped, seeds = batch_of(case, oracle)
        ref = oracle.tick_batch(st, inputs)
        for v in list(inputs.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)] + [cls_a]:
            v.setflags(write=False)
        _REF[case.id] = (st, inputs, ref, cls_a, skipped, seeds)
    return _REF[case.id][:3]


def class_a(case, oracle) -> np.ndarray:
    """bool [batch]: the QPs on which the oracle keeps status, count and event log under its eight one-ulp perturbations (solver_branches.classify)."""
    reference(case, oracle)
    return _REF[case.id][3]


def skipped_seeds(case, oracle) -> Tuple[int, ...]:
    reference(case, oracle)
    return _REF[case.id][4]


def seeds_of(case, oracle) -> List[int]:
    reference(case, oracle)
    return _REF[case.id][5]


_CENSUS: Dict[str, tuple] = {}


def censuses(case, oracle):
    """(event logs, per-QP censuses, their sum) of a case's batch."""
    if case.id not in _CENSUS:
        st, inputs, ref = reference(case, oracle)
        B = len(ref["status"])
        logs = [oracle.tick_log(st, inputs, i, ref) for i in range(B)] if st.nin2 else []
        cs = [sb.census(st, lg, oracle) for lg in logs]
        _CENSUS[case.id] = (logs, cs, sb.census_sum(cs))
    return _CENSUS[case.id]


def rows_seen(logs, oracle) -> np.ndarray:
    """every row an event log picks, adds or drops (sorted, unique)"""
    rows = [r for lg in logs for code, r, _, _ in lg["events"].tolist() if r >= 0]
    return np.unique(np.asarray(rows, np.int64))


# ---- the one-wave kernel's staging arithmetic ---------------------------------------------------------------------------------------------

def small_div_is_exact() -> bool:
    """csrc/wbcqp_small.hpp stages element e of A (e < 256) in row (e * inv) >> 16 with inv = ceil(65536 / n): e / n for every n <= 16."""
    for n in range(1, 17):
        inv = (65536 + n - 1) // n
        for e in range(256):
            if (e * inv) >> 16 != e // n:
                return False
    return True


# ---- C: the dense seam --------------------------------------------------------------------------------------------------------------------

DENSE_SEED = 15_000_000
DENSE_N_MAX = 99  # the largest n wbcqp_solve_dense accepts (its LDS arithmetic: J n x odd(n), packed R, 36 vector slots, the int arrays <= 160 KiB); tests/test_gpu_size_edges.py holds the entry point to it


def dense_lds_bytes(n: int, neq: int) -> int:
    """wbcqp_solve_dense's LDS arithmetic (csrc/wbcqp_api.hip), restated."""
    odd = lambda v: v | 1
    even = lambda v: (v + 1) & ~1
    blocked = 1 <= neq <= 22 and n <= 80
    ldb = 2 * odd((4 * ((neq + 3) // 4) + 1) // 2)
    rsize = n * (n + 3) // 2 + 2
    if blocked:
        rsize = max(rsize, 256 + (n + 17) * ldb + 8)
    o = even(n * odd(n)) + even(rsize) + 36 * 128
    if blocked:
        o += even((n + 1) * ldb + 8) + even(neq * (neq + 1) + 4 * neq + 16)
    return 8 * (o + 1920 // 2 + 2)


# (n, neq, nin): four seeds each
DENSE_SIZES: List[Tuple[int, int, int]] = [
    (1, 0, 2), (1, 1, 0), (2, 2, 3), (3, 1, 6),
    (30, 30, 10),                       # neq = n
    (64, 0, 257), (80, 22, 512),        # the structured kernels' set-up (n <= 80), the blocked equality phase, a thread owning two rows
    (81, 23, 300),                      # the first n and neq past both switches
    (DENSE_N_MAX, 0, 512), (DENSE_N_MAX, 40, 512), (DENSE_N_MAX, DENSE_N_MAX, 0),
]
# seeds whose ORACLE count moves under one-ulp perturbations of the inputs, replaced by the next seed that keeps it (dense_seeds' rule; at most one per size)
DENSE_REPLACED: Dict[Tuple[int, int, int], Tuple[int, int]] = {}


def dense_qp(n: int, neq: int, nin: int, seed: int):
    """tests/test_gpu_dense.py's random recipe: H = G G' + 0.5 I, xs feasible, slack uniform(0, 1), g standard normal."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    H = G @ G.T + 0.5 * np.eye(n)
    g = rng.standard_normal(n)
    xs = rng.standard_normal(n)
    CE = rng.standard_normal((neq, n)); ce0 = -(CE @ xs)
    CI = rng.standard_normal((nin, n)); ci0 = -(CI @ xs) + rng.uniform(0.0, 1.0, nin)
    return H, g, CE, ce0, CI, ci0


def dense_perturbed(qp, k: int, seed: int):
    """Perturbation k of a dense QP: every non-zero element one ulp up or down (solver_branches.perturbed's rule), H symmetrised again."""
    rng = np.random.default_rng([seed, 78, k])
    out = []
    for a in qp:
        a = np.asarray(a, np.float64)
        up = rng.random(a.shape) < 0.5
        out.append(np.where(a == 0.0, a, np.nextafter(a, np.where(up, np.inf, -np.inf))))
    H = out[0]
    out[0] = np.tril(H) + np.tril(H, -1).T
    return tuple(out)


def dense_count_is_stable(qp, seed: int, oracle) -> bool:
    base = oracle.eiquadprog(*qp)
    return all(oracle.eiquadprog(*dense_perturbed(qp, k, seed))["iters"] == base["iters"] for k in range(sb.N_PERTURB))


# (64, 0, 257) has ONE row past the 256th: the first base at which the reference picks it (at DENSE_SEED + 500 none of the four seeds does)
DENSE_FIRST_SEED: Dict[Tuple[int, int, int], int] = {(64, 0, 257): DENSE_SEED + 504}


def dense_first_seed(size) -> int:
    return DENSE_FIRST_SEED.get(size, DENSE_SEED + 100 * DENSE_SIZES.index(size))


def dense_seeds(size, oracle) -> Tuple[List[int], Optional[Tuple[int, int]]]:
    """The rule: seeds s0 .. s0 + 3; the first of them whose oracle count moves under the perturbations gives way to the first later seed that keeps
    it.  Returns (seeds, (replaced, by) or None)."""
    n, neq, nin = size
    s0 = dense_first_seed(size)
    seeds = [s0 + j for j in range(4)]
    for j, s in enumerate(seeds):
        if not dense_count_is_stable(dense_qp(n, neq, nin, s), s, oracle):
            nxt = s0 + 4
            while not dense_count_is_stable(dense_qp(n, neq, nin, nxt), nxt, oracle):
                nxt += 1
            seeds[j] = nxt
            return seeds, (s, nxt)
    return seeds, None


def dense_table_seeds(size) -> List[int]:
    """the committed seeds of a size (no oracle): dense_seeds' answer as DENSE_REPLACED records it"""
    s0 = dense_first_seed(size)
    seeds = [s0 + j for j in range(4)]
    if size in DENSE_REPLACED:
        old, new = DENSE_REPLACED[size]
        seeds[seeds.index(old)] = new
    return seeds


# ---- D: refusals ------------------------------------------------------------------------------------------------------------------------

def refused_stacks():
    """(id, stack, documented code, fragment of the error text)"""
    big = small_stack("edge_five_bound_blocks", 64, (6,), True)
    big = dataclasses.replace(big, ineq_blocks=[(S.INEQ_BOUNDS, 0)] * 5)  # nin2 = 5 x 128
    rows = stack("edge_r1_289", 64, 64, 1, False)  # 27 dense rows + 6 + four posture tasks over the same 64 joints: r1 = 27 + 256 + 6
    rows = dataclasses.replace(rows, sel_col=np.tile(rows.sel_col, 4), sel_task=np.tile(rows.sel_task, 4))
    tall = small_stack("edge_nv65", 65, (6,), True)
    none = small_stack("edge_nv0", 1, (1,), True)
    none = dataclasses.replace(none, nv=0, na=0, sel_col=np.zeros(0, np.int32), sel_task=np.zeros(0, np.int32), bound_col=np.zeros(0, np.int32))
    many = dataclasses.replace(stack("edge_nc16", 30, 24, 16, False), ineq_blocks=[(S.INEQ_BOUNDS, 0)])  # (its 16 force blocks alone are one too many: INVALID)
    return [("n0", none, INVALID, "bad nv/na/nc"),
            ("nv65", tall, UNSUPPORTED, "nv exceeds 64"),
            ("nc16", many, UNSUPPORTED, "exceeds WBCQP_MAX_VARS"),  # 12 x 16 force variables: n > 126 stands in front of the contact count's own check
            ("nin2_640", big, UNSUPPORTED, "more than 512 one-sided inequality rows"),
            ("r1_289", rows, UNSUPPORTED, "more than 256 level-1 rows")]


# ---- what the tables record, printed ------------------------------------------------------------------------------------------------------

def main():
    from inria_wbc_amd import capi
    from oracle import oracle
    oracle.build()
    assert small_div_is_exact()
    for c in SMALL_CASES:
        st, inputs, ref = reference(c, oracle)
        L = capi.layout_of(st)
        logs, cs, tot = censuses(c, oracle)
        print("A", c.id, "n", st.n, "r1", st.r1, "nin2", st.nin2, "lenA", st.n_dense * st.nv, "n_tasks", st.n_tasks,
              "layout", {k: L[k] for k in ("lds_bytes", "waves_per_cu", "wave_per_qp")}, "optimal", float((ref["status"] == 0).mean()),
              "max_iters", int(ref["iters"].max()), {k: tot.get(k) for k in ("vertex", "partial_drop", "dual_drop", "drop_first", "drop_interior", "drop_last", "dependent")},
              "class A", int(class_a(c, oracle).sum()), "skipped", skipped_seeds(c, oracle), flush=True)
    for c in COMPACT_CASES:
        st = c.stack()
        try:
            L = capi.layout_of(st)
        except capi.WbcqpError as e:
            print("B", c.id, "n", st.n, "neq", st.neq, "nin2", st.nin2, "r1", st.r1, "REFUSED", e.code, str(e), "envelope", in_compact_envelope(st), flush=True)
            continue
        st, inputs, ref = reference(c, oracle)
        logs, cs, tot = censuses(c, oracle)
        print("B", c.id, "n", st.n, "neq", st.neq, "nu", st.nu, "nin2", st.nin2, "r1", st.r1, "envelope", in_compact_envelope(st),
              "layout", {k: L[k] for k in ("lds_bytes", "waves_per_cu", "wave_per_qp")}, "optimal", float((ref["status"] == 0).mean()),
              "max_iters", int(ref["iters"].max()), "drops", tot["partial_drop"] + tot["dual_drop"], "rows up to", int(rows_seen(logs, oracle).max(initial=-1)),
              "class A", int(class_a(c, oracle).sum()), "skipped", skipped_seeds(c, oracle), flush=True)
    for size in DENSE_SIZES:
        seeds, rep = dense_seeds(size, oracle)
        outs = [oracle.eiquadprog_log(*dense_qp(*size, s)) for s in seeds]
        print("C", size, "lds", dense_lds_bytes(size[0], size[1]), "seeds", seeds, "replaced", rep, "status", [o["status"] for o in outs], "iters", [o["iters"] for o in outs],
              "iq", [o["iq"] for o in outs], "drops", [int(np.isin(o["events"][:, 0], (oracle.EV_PARTIAL_DROP, oracle.EV_DUAL_DROP)).sum()) for o in outs],
              "max row", [int(o["events"][:, 1].max(initial=-1)) for o in outs], flush=True)
    for name, st, code, text in refused_stacks():
        try:
            capi.layout_of(st)
            print("D", name, "ACCEPTED")
        except capi.WbcqpError as e:
            print("D", name, e.code, str(e), "expected", code, text)


if __name__ == "__main__":
    main()
