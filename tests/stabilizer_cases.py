"""What the tests of the stabiliser share (tests/test_stabilizer_host.py, test_gpu_stabilize.py): the two stabilisers, a robot in balance, and the
sensor streams of the parity grid with the assertions that they decide every comparison clearly and reach every branch.  A plain module, in the
manner of tests/model_queries.py."""
import numpy as np

from inria_wbc_amd import model as mdl
from inria_wbc_amd import stabilizer as stb
from inria_wbc_amd import structure

WINDOWS = (1, 2, 7, 64)
NMAX = 67
DT = 2.0 ** -7  # a power of two: the hand-worked cases divide exactly
COM_GAINS = (0.5, 0.25, 0.25, 0.125, 0.125, 0.0625)
ANKLE_GAINS = (0.5, 0.25, 0.5, 0.25, 0.25, 0.125)
FFDA_GAINS = (2.0 ** -10, 0.5, 0.25)
LP, RP = (0.125, 0.25, 0.0625), (0.125, -0.25, 0.0625)  # the ankles of the hand-worked cases: dyadic, so sums of up to 64 of them are exact


def talos_stab(window, **kw):
    """The stabiliser of the Talos stack (nref 305) with the test gains (every law moves something); ankles = observed frames 0 and 1."""
    m = mdl.talos_like()
    tm = mdl.build_taskmap(m, structure.talos_structure(), mdl.talos_stack())
    s = stb.from_taskmap(m, tm, mdl.talos_stack(), window, COM_GAINS, ANKLE_GAINS, FFDA_GAINS)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def tree_stab(window):
    """The smallest shape: a 3-body random tree's map of the four required tasks and nothing else (nref 81, no contacts)."""
    m = mdl.random_tree(5, 3, True, nframe=4)
    stack = [dict(name="lf", type="se3", tracked=m.frame_names[0], kp=10.0, mask="111111"), dict(name="rf", type="se3", tracked=m.frame_names[1], kp=10.0, mask="111111"),
             dict(name="torso", type="se3", tracked=m.frame_names[2], kp=10.0, mask="000111"), dict(name="com", type="com", kp=10.0, mask="111")]
    st = structure._mk("stab_tree", m.nv, m.na, [], [("lf", 6, 1.0), ("rf", 6, 1.0), ("torso", 3, 1.0), ("com", 3, 1.0)], None, [], False, False, [])
    return stb.from_taskmap(m, mdl.build_taskmap(m, st, stack, dt=DT), stack, window, COM_GAINS, ANKLE_GAINS, FFDA_GAINS)


def mini_stab(window, **kw):
    """Six blocks and nothing else (nref 129), dt a power of two, x rows of 6 + 24."""
    s = stb.Stabilizer(window=window, dt=DT, mass=90.0, com_gains=COM_GAINS, ankle_gains=ANKLE_GAINS, ffda_gains=FFDA_GAINS, nref=129, com_ref=0, lf_ref=9,
                       rf_ref=33, torso_ref=57, lf_contact_ref=81, rf_contact_ref=105, lf_force_col=6, rf_force_col=18)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def se3_blocks(s):
    return [o for o in (s.lf_ref, s.rf_ref, s.torso_ref, s.lf_contact_ref, s.rf_contact_ref) if o >= 0]


def balanced(s, B=1, fz=400.0):
    """Inputs of a robot in balance: identity rotations, zero velocities, the CoP of each foot under its ankle, the combined CoP at the model's
    ZMP, and the previous solution's normal forces equal to the sensors'."""
    ref = np.zeros((B, s.nref))
    ref[:, s.com_ref:s.com_ref + 3] = (0.125, 0.0, 0.75)
    for o, p in zip((s.lf_ref, s.rf_ref, s.torso_ref, s.lf_contact_ref, s.rf_contact_ref), (LP, RP, (0.0, 0.0, 1.0), LP, RP)):
        if o >= 0:
            ref[:, o:o + 3] = p
            ref[:, o + 3:o + 12] = np.eye(3).reshape(9)
    wrench = np.zeros((B, 12))
    wrench[:, 2] = wrench[:, 8] = fz
    place = np.zeros((B, max(s.lf_pos, s.rf_pos) + 3))
    place[:, s.lf_pos:s.lf_pos + 3], place[:, s.rf_pos:s.rf_pos + 3] = LP, RP
    ldx = max(s.lf_force_col, s.rf_force_col, 0) + 12
    x = np.zeros((B, ldx))
    for col in (s.lf_force_col, s.rf_force_col):
        if col >= 0:
            x[:, col + 2:col + 12:3] = fz / 4
    return dict(ref=ref, wrench=wrench, com=np.tile((0.125, 0.0, 0.75), (B, 1)), acom=np.zeros((B, 3)), placement=place, x_prev=x)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def states_equal(a, b):
    """Two state arrays [B, state_bytes] agree in every byte, except that a NaN sample may be any NaN: the sign and payload of a NaN that
    arithmetic produced are the processor's, not the algorithm's.  (NaNs sit in the same places, and everything else is compared as bytes.)"""
    a, b = np.ascontiguousarray(a).copy(), np.ascontiguousarray(b).copy()
    fa, fb = a.view(np.float64)[:, stb.N_FILTERS:], b.view(np.float64)[:, stb.N_FILTERS:]
    na, nb = np.isnan(fa), np.isnan(fb)
    if not np.array_equal(na, nb):
        return False
    fa[na] = 0.0
    fb[nb] = 0.0
    return bits(a) == bits(b)


# ---- the streams of the parity grid ----------------------------------------------------------------------------------------------------------
BOTH, LEFT, RIGHT, NONE, SLIDE = range(5)  # which feet carry weight; SLIDE: fz below FMIN under a large tangential force (|f| > FMIN, no CoP)


def _schedule(rng, T, w):
    """A tick-by-tick pattern: runs of both feet long enough to fill a window, and runs of every other pattern between them."""
    out = []
    while len(out) < T:
        out += [BOTH] * int(rng.integers(w, w + 4))
        out += [int(rng.choice([LEFT, RIGHT, NONE, SLIDE, LEFT, RIGHT]))] * int(rng.integers(1, max(2, w // 2 + 2)))
        if rng.random() < 0.5:
            out += [int(rng.choice([LEFT, RIGHT]))] * int(rng.integers(w, w + 3))  # one foot long enough to become valid alone
    return out[:T]


def streams(s, seed, base_ref=None):
    """(inputs per tick [T] of dicts over NMAX instances, roles): T = 3 window + 5 ticks.  Instance 0 never leaves balance, 1 trips the CoP
    guard, 2 the force guard; the others walk through random schedules with a NaN sample here and there.  x_prev is None on the first tick."""
    rng = np.random.default_rng(seed)
    w, T, B = s.window, 3 * s.window + 5, NMAX
    bal = balanced(s, 1)
    if base_ref is None:
        base_ref = np.tile(bal["ref"], (B, 1))
        for i in range(3, B):  # rotations near the identity on both sides of Eigen's branch, and a few far from it
            for o in se3_blocks(s):
                e = rng.normal(0.0, 0.3 if i % 5 == 0 else 0.05, 3)
                R = mdl._rot(0, e[0]) @ mdl._rot(1, e[1]) @ mdl._rot(2, e[2])
                base_ref[i, o + 3:o + 12] = R.T.reshape(9)  # column-major
            base_ref[i, s.com_ref:s.com_ref + 3] += rng.normal(0.0, 0.02, 3)
    moving = np.concatenate([np.arange(s.com_ref + 3, s.com_ref + 9)] + [np.arange(o + 12, o + 24) for o in se3_blocks(s)])
    sched = [_schedule(rng, T, w) for _ in range(B)]
    ldx = bal["x_prev"].shape[1]
    ticks = []
    for t in range(T):
        ref = base_ref.copy()
        ref[3:, moving] = rng.normal(0.0, 0.01, (B - 3, moving.size))
        wrench = np.zeros((B, 12))
        place = np.tile(bal["placement"], (B, 1))
        place[3:, s.lf_pos:s.lf_pos + 3] += rng.normal(0.0, 0.01, (B - 3, 3))
        place[3:, s.rf_pos:s.rf_pos + 3] += rng.normal(0.0, 0.01, (B - 3, 3))
        com = np.tile(bal["com"], (B, 1))
        com[3:] += rng.normal(0.0, 0.03, (B - 3, 3))
        acom = np.zeros((B, 3))
        acom[3:] = rng.normal(0.0, 0.5, (B - 3, 3))
        x = rng.uniform(-5.0, 5.0, (B, ldx))
        for col in (s.lf_force_col, s.rf_force_col):
            if col >= 0:
                x[:, col + 2:col + 12:3] = rng.uniform(50.0, 150.0, (B, 4))
        for i in range(B):
            pat = BOTH if i < 3 else sched[i][t]
            for foot, down in ((0, pat in (BOTH, LEFT)), (1, pat in (BOTH, RIGHT))):
                f = wrench[i, 6 * foot:6 * foot + 3]
                if down:
                    f[:] = (rng.normal(0.0, 20.0), rng.normal(0.0, 20.0), rng.uniform(200.0, 600.0))
                else:
                    f[:] = (rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 15.0))
                    if pat == SLIDE:
                        f[0] = rng.uniform(50.0, 80.0)
                wrench[i, 6 * foot + 3:6 * foot + 6] = rng.normal(0.0, 10.0, 3)
        wrench[:3] = bal["wrench"]
        x[:3] = bal["x_prev"]
        # 1: feet and CoM sixteen metres away in x and y -- every CoP trips the guard once it is valid
        place[1, s.lf_pos:s.lf_pos + 2] += 16.0
        place[1, s.rf_pos:s.rf_pos + 2] += 16.0
        # 2: a ground force far beyond 10 M g = 98.1 M
        wrench[2, 2] = wrench[2, 8] = 100.0 * s.mass
        for i in range(3, B):  # a NaN sample: a torque (the CoP turns NaN for a window), a force (the foot counts as lifted)
            if i % 7 == 3 and t == w + 1:
                wrench[i, 4] = np.nan
            if i % 11 == 5 and t == w + 2:
                wrench[i, 8] = np.nan
        ticks.append(dict(ref=ref, wrench=wrench, com=com, acom=acom, placement=place, x_prev=x if t > 0 else None))
    return ticks


def reference_run(s, ticks):
    """The transcription over the whole stream: (outputs per tick, state after each tick [T][NMAX, bytes]).  Asserts, on the CPU, that no decision
    lies within 1e-9 relative of its threshold and that every branch occurs."""
    state = np.zeros((NMAX, stb.state_bytes(s.window)), np.uint8)
    outs, states, margins = [], [], []
    for inp in ticks:
        outs.append(stb.step(s, state, inp, margins))
        states.append(state.copy())
    stb.clear_margin(margins, 1e-9)
    flags = np.stack([o["flags"] for o in outs])  # [T][B]
    seen = {name: bool((flags & bit).any()) for name, bit in (("cop", stb.COP), ("lcop", stb.LCOP), ("rcop", stb.RCOP), ("com", stb.COM), ("err_cop", stb.ERR_COP))}
    valid = flags & (stb.COP | stb.LCOP | stb.RCOP)
    seen["fall back to left"] = bool((valid == stb.LCOP).any())
    seen["fall back to right"] = bool((valid == stb.RCOP).any())
    seen["no valid CoP"] = bool((valid[:, 3:] == 0).any())
    fz = np.stack([t["wrench"][:, [2, 8]] for t in ticks])
    for name, l, r in (("both feet", True, True), ("left only", True, False), ("right only", False, True), ("none", False, False)):
        seen[name] = bool((((fz[..., 0] > stb.FMIN) == l) & ((fz[..., 1] > stb.FMIN) == r)).any())
    seen["a NaN sample"] = bool(np.isnan(np.stack([t["wrench"] for t in ticks])).any())
    seen["balance kept"] = all(stb_bits_equal(o["ref_out"][0], t["ref"][0]) for o, t in zip(outs, ticks))
    decisions = [m for m in margins if m[0] == "r0 > 0"]
    if s.lf_contact_ref >= 0 and s.rf_contact_ref >= 0:  # (without contacts only the CoM law is left: no rotation is touched)
        seen["r0 > 0"] = any(m[1] > 0 for m in decisions)
        seen["r0 <= 0"] = any(m[1] <= 0 for m in decisions)
        for name, bit in (("left ankle", stb.LANKLE), ("right ankle", stb.RANKLE), ("ffda", stb.FFDA), ("err_force", stb.ERR_FORCE)):
            seen[name] = bool((flags & bit).any())
    missing = [k for k, v in seen.items() if not v]
    assert not missing, (s.window, missing)
    return outs, states


def stb_bits_equal(a, b):
    return bits(a) == bits(b)
