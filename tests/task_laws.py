"""A high-precision statement of the rows kernel's three piecewise task laws, and inputs that reach every branch of them.

Shared by tests/test_task_laws_host.py (the C oracle against this statement, on the CPU) and tests/test_gpu_task_laws.py (the device
against it).  Frame placements, velocities, classical accelerations, Jacobians, CoM and momentum terms come from oracle/rbd.py
(rbd_terms): they are held to parity elsewhere -- entry by entry against an mpmath statement of their own in tests/rbd_exact.py
(tests/test_rbd_exact_host.py for the oracle, tests/test_gpu_rbd_exact.py for the device).  What is stated here, in mpmath at 50 digits, is what the kernel and the oracle each
write in their own floating point:
  * errorInSE3's rotation part: the exact logarithm of oMf' R_ref (no angle thresholds, no branches);
  * tsid's computeAccLimits, returning per joint the eleven decisions it took and the margin of every inequality among them;
  * the 5PL self-collision repulsor as the reference writes it, with pow.

The bar (per entry):  |x - ref| <= TOL_ROWS max(1, |ref|) + 4 S,  S = the largest change of this statement's value when every element
of q and ref moves one ulp up, and one ulp down: no implementation can be closer than S to another that sees differently rounded
placements.  For the joint-bound rows S measures the law's own conditioning (q_j + dt dq_j is rounded before it meets the limit, and
the viability discriminants amplify that); a joint that sits on a limit EXACTLY is exact on purpose -- an ulp would move it to another
branch -- and has S = 0.  The inputs are chosen so that 4 S stays under TOL_ROWS max(1, |ref|) everywhere but near pi.
"""
from __future__ import annotations

import functools
import itertools
from typing import Dict, List, Optional, Tuple

import mpmath as mp
import numpy as np

from inria_wbc_amd import model as mdl
from inria_wbc_amd import structure

TOL_ROWS = 1e-10  # the project's bar for the rows kernel (tests/test_gpu_terms.py)
DPS = 50
PI = float(np.pi)
T_LOW, T_HIGH = 1.220703125e-4, PI - 1e-2  # log3's two thresholds

ANGLES = (0.0, 1e-9, 1.0e-4, 1.3e-4, 2e-4, 1e-3, 1e-2, 0.5, 2.0, 3.0, PI - 2e-2, PI - 5e-3, PI - 1e-3)
ANGLE_REGIME = ("taylor", "taylor", "taylor", "middle, low end", "middle, low end", "middle, low end", "middle, low end",
                "middle", "middle", "middle", "middle, top end", "near pi", "near pi")
NEAR_PI = (10, 11, 12)  # indices of the angles where S, not TOL_ROWS, may set the bar
assert all(abs(t / T_LOW - 1.0) >= 0.05 and abs(t - T_HIGH) >= 0.05 * 1e-2 for t in ANGLES)  # 5 % off both thresholds
# unit axes with every component at least 0.3 in magnitude, one per sign octant
OCTANTS = tuple(np.array(s) * np.array([0.5, 0.62, 0.6]) / np.linalg.norm([0.5, 0.62, 0.6]) for s in itertools.product((1.0, -1.0), repeat=3))
NCOMBO = len(ANGLES) * len(OCTANTS)  # combo c: angle c % 13, octant c // 13

_first = [(a % 8) * len(ANGLES) + a for a in range(len(ANGLES))]
_second = [o * len(ANGLES) + a for o in range(8) for a in NEAR_PI if o * len(ANGLES) + a not in _first]
SHORT_ORDER = _first + _second + [c for c in range(NCOMBO) if c not in _first + _second]

BANDS = ("-20 %", "-margin", "0", "+margin/2", "+margin", "+5 margin")
REGIMES = tuple(dict.fromkeys(ANGLE_REGIME)) + tuple("5PL " + b for b in BANDS) + ("5PL elsewhere", "bounds", "other")


# ---- the three laws, in mpmath ------------------------------------------------------------------------------------------

def exact_log3(R) -> List[mp.mpf]:
    """The rotation vector of the rotation nearest a 3 x 3 matrix of mpmath numbers (indexed [i, j]): through the unit quaternion, taking the largest of its four
    components first (accurate at every angle, pi included), angle = 2 atan2(|xyz|, w)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    cand = [1 + t, 1 + 2 * R[0, 0] - t, 1 + 2 * R[1, 1] - t, 1 + 2 * R[2, 2] - t]  # 4 w^2, 4 x^2, 4 y^2, 4 z^2
    k = max(range(4), key=lambda i: cand[i])
    a, b, c = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]  # 4 w (x, y, z)
    if k == 0:
        qw, qx, qy, qz = cand[0], a, b, c
    elif k == 1:
        qw, qx, qy, qz = a, cand[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]
    elif k == 2:
        qw, qx, qy, qz = b, R[0, 1] + R[1, 0], cand[2], R[1, 2] + R[2, 1]
    else:
        qw, qx, qy, qz = c, R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], cand[3]
    if qw < 0:
        qw, qx, qy, qz = -qw, -qx, -qy, -qz
    n = mp.sqrt(qx * qx + qy * qy + qz * qz)
    if n == 0:
        return [mp.mpf(0)] * 3
    f = 2 * mp.atan2(n, qw) / n
    return [f * qx, f * qy, f * qz]


def exp3(theta: float, axis: np.ndarray):
    """exp(theta [axis]x) as an mpmath matrix (Rodrigues)."""
    th = mp.mpf(float(theta))
    a = [mp.mpf(float(x)) for x in axis]
    nrm = mp.sqrt(sum(x * x for x in a))
    a = [x / nrm for x in a]
    K = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return mp.eye(3) + mp.sin(th) * K + (1 - mp.cos(th)) * (K * K)


def _mpmat(A: np.ndarray):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(A)])


DECISIONS = ("dq <= 0", "min_q3 < -dq/dt", "q != q_min", "fmax picks dq^2 / (2 (q - q_min))", "max_q3 > -dq/dt", "q != q_max",
             "fmin picks -dq^2 / (2 (q_max - q))", "delta_1 >= 0", "delta_2 >= 0", "ub < lb", "ub == ub_pos")
EXACT = (2, 5, 10)  # the equality decisions: exact on purpose, no margin
_T = lambda s: tuple(None if ch == "-" else ch == "1" for ch in s)
# Every combination of the eleven decisions a joint with q_min < q_max can take (found by a random search over (q, dq) in every regime
# of distance to a limit and of speed, 27 of them).  Both discriminants cannot be negative at once: delta_1 + delta_2 =
# dt^2 (2 dq_max^2 + 8 ddq_max (q_max - q_min)) > 0.  With dq <= 0 and min_q3 < -dq/dt, delta_2 = dt^2 (dq_max^2 + 4 |dq| dq_max +
# 8 ddq_max l) is positive because that condition puts l = q + dt dq - q_min above -dt |dq| / 2 (and the mirror image for dq > 0).
REACHABLE = tuple(_T(s) for s in (
    "0---00-0111", "0---00-1111", "0---010010-", "0---0100111", "0---010110-", "0---0110111", "0---011110-", "0---0111110", "0---0111111",
    "0---1--100-", "0---1--1010", "0---1--110-", "0---1--1110", "100----1010", "100----1110", "1010---100-", "1010---1010", "1010---110-",
    "1011---100-", "1011---1010", "1011---110-", "1011---1110", "11-----010-", "11-----0110", "11-----0111", "11-----110-", "11-----1110"))
assert len(set(REACHABLE)) == 27


def acc_limits(qj: float, dq: float, qmin: float, qmax: float, dqmax: float, dt: float):
    """tsid TaskJointPosVelAccBounds::computeAccLimits with ddq_max = dq_max / dt, in mpmath.  Returns (lb, ub, the eleven decisions as
    a tuple of True / False / None (not evaluated), the relative margin of every inequality evaluated (None elsewhere))."""
    qj, dq, qmin, qmax, dqmax, dt = (mp.mpf(float(x)) for x in (qj, dq, qmin, qmax, dqmax, dt))
    D: List[Optional[bool]] = [None] * 11
    G: List[Optional[float]] = [None] * 11

    def decide(i, a, b, op):
        D[i] = bool(op(a, b))
        s = max(abs(a), abs(b))
        G[i] = float("inf") if s == 0 else float(abs(a - b) / s)  # (0 against 0: both sides are exact zeros, nothing can round)
        return D[i]

    ddqmax = dqmax / dt
    two_dt_sq, mdq_dt = 2 / (dt * dt), -dq / dt
    max_q3, min_q3 = two_dt_sq * (qmax - qj - dt * dq), two_dt_sq * (qmin - qj - dt * dq)
    lt, gt, ge = (lambda a, b: a < b), (lambda a, b: a > b), (lambda a, b: a >= b)
    D[0] = bool(dq <= 0)
    G[0] = float("inf") if dq == 0 else 1.0  # the sign of an input: exact
    if D[0]:
        ub_pos = max_q3
        if decide(1, min_q3, mdq_dt, lt):
            lb_pos = min_q3
        else:
            D[2] = bool(qj != qmin)
            if D[2]:
                first = dq * dq / (2 * (qj - qmin))
                lb_pos = first if decide(3, first, mdq_dt, ge) else mdq_dt
            else:
                lb_pos = mp.mpf(10) ** 6
    else:
        lb_pos = min_q3
        if decide(4, max_q3, mdq_dt, gt):
            ub_pos = max_q3
        else:
            D[5] = bool(qj != qmax)
            if D[5]:
                first = -dq * dq / (2 * (qmax - qj))
                ub_pos = first if decide(6, mdq_dt, first, ge) else mdq_dt
            else:
                ub_pos = -mp.mpf(10) ** 6
    lb_vel, ub_vel = (-dqmax - dq) / dt, (dqmax - dq) / dt
    dt_dq, two_a, dt_ddq_dt = dt * dq, 2 * dt * dt, ddqmax * dt * dt
    b_1, b_2 = 2 * dt_dq + dt_ddq_dt, 2 * dt_dq - dt_ddq_dt
    c_1 = dq * dq - 2 * ddqmax * (qmax - (qj + dt_dq))
    c_2 = dq * dq - 2 * ddqmax * ((qj + dt_dq) - qmin)
    delta_1, delta_2 = b_1 * b_1 - 2 * two_a * c_1, b_2 * b_2 - 2 * two_a * c_2
    # (the margin of a discriminant's sign: against the larger of the two products it is the difference of)
    ub_via = (-b_1 + mp.sqrt(delta_1)) / two_a if decide(7, b_1 * b_1, 2 * two_a * c_1, ge) else mdq_dt
    lb_via = (-b_2 - mp.sqrt(delta_2)) / two_a if decide(8, b_2 * b_2, 2 * two_a * c_2, ge) else mdq_dt
    lb = max(lb_pos, lb_via, lb_vel, -ddqmax)
    ub = min(ub_pos, ub_via, ub_vel, ddqmax)
    if decide(9, ub, lb, lt):
        D[10] = bool(ub == ub_pos)
        if D[10]:
            lb = ub
        else:
            ub = lb
    return lb, ub, tuple(D), tuple(G)


@functools.lru_cache(maxsize=None)
def _five_pl_constants(margin: float, m: float):
    m, margin = mp.mpf(m), mp.mpf(margin)
    k5 = -mp.log(mp.power(1 - mp.mpf("1e-5"), -1 / m) - 1) / margin
    s_p = -1 / k5 * mp.log(-1 + mp.power(2, 1 / m))
    return m, k5, s_p


def five_pl(norm, aa, margin, m):
    """The 5PL repulsor of task-self-collision.cpp:147-156 at distance `norm`, as written there: C, the gradient's scale along diff
    (also the Hessian's isotropic part) and the Hessian's diff diff' coefficient."""
    m, k5, s_p = _five_pl_constants(float(margin), float(m))
    x = k5 * (norm - aa + s_p)
    e_p = mp.exp(-x)
    C = 1 - mp.power(1 + e_p, -m)
    pw1, pw2 = mp.power(e_p + 1, -m - 1), mp.power(e_p + 1, -m - 2)  # (the reference calls pow for each occurrence; the values are these)
    gscale = -1 / norm * k5 * m * e_p * pw1
    sn = norm * norm
    hh = (1 / sn * k5 ** 2 * (-m - 1) * m * mp.exp(-2 * x) * pw2 + 1 / sn * k5 ** 2 * m * e_p * pw1
          + 1 / mp.power(norm, mp.mpf("1.5")) * k5 * m * e_p * pw1)  # (pow(norm, 1.5), as the reference has it)
    return C, gscale, hh


# ---- the rows b1 / bc / blb / bub of one instance -----------------------------------------------------------------------------

def _se3_rhs(oMf12, vf, af, rf, kp, kd) -> np.ndarray:
    R, p = oMf12[:9].reshape(3, 3), oMf12[9:]
    Rref = rf[3:12].reshape(3, 3).T
    A, Bm = [[mp.mpf(float(x)) for x in r] for r in R], [[mp.mpf(float(x)) for x in r] for r in Rref]
    w = exact_log3({(i, j): A[0][i] * Bm[0][j] + A[1][i] * Bm[1][j] + A[2][i] * Bm[2][j] for i in range(3) for j in range(3)})
    perr = np.concatenate([R.T @ (rf[0:3] - p), [float(x) for x in w]])
    vref = np.concatenate([R.T @ rf[12:15], R.T @ rf[15:18]])
    aref = np.concatenate([R.T @ rf[18:21], R.T @ rf[21:24]])
    return (kp * perr + kd * (vref - vf) + aref) - af


def reference_rows(rbd, m, tm, st, q: np.ndarray, v: np.ndarray, ref: np.ndarray, bounds: bool = True) -> Dict[str, np.ndarray]:
    """b1, bc (and blb, bub, the decisions and their margins when `bounds`) of one instance, to the statement above."""
    mp.mp.dps = DPS
    T = rbd.rbd_terms(m, q, v)
    nv, na, nq = m.nv, m.na, m.nq
    b1 = []
    for B in tm.blocks:
        if B.kind == mdl.T_SE3:
            rhs = _se3_rhs(T["oMf"][B.frame], T["vf"][B.frame], T["af"][B.frame], ref[B.ref:B.ref + 24], B.kp, B.kd)
            b1 += [rhs[i] for i in range(6) if (B.mask >> i) & 1]
        elif B.kind == mdl.T_COM:
            r = ref[B.ref:B.ref + 9]
            b1 += [(-B.kp * (T["com"][i] - r[i]) - B.kd * (T["vcom"][i] - r[3 + i]) + r[6 + i]) - T["acom"][i] for i in range(3) if (B.mask >> i) & 1]
        elif B.kind == mdl.T_MOMENTUM:
            r, L = ref[B.ref:B.ref + 12], T["Ag"] @ v
            b1 += [(-B.kp * (L[i] - r[i]) + r[6 + i]) - T["dAgv"][i] for i in range(6) if (B.mask >> i) & 1]
        else:
            Bs = mp.mpf(0)
            pos = T["oMf"][B.frame][9:]
            for fa, r0 in B.avoided:
                diff = [mp.mpf(float(x)) for x in pos - T["oMf"][fa][9:]]
                drift = [mp.mpf(float(x)) for x in T["af"][B.frame][:3] - T["af"][fa][:3]]
                Jv = [mp.mpf(float(x)) for x in (T["Jw"][B.frame][:3] - T["Jw"][fa][:3]) @ v]
                norm = mp.sqrt(sum(x * x for x in diff))
                C, gscale, hh = five_pl(norm, mp.mpf(float(r0)) + mp.mpf(float(B.radius)), B.margin, B.m)
                dJv = sum(a * b for a, b in zip(diff, Jv))
                quad = hh * dJv * dJv + gscale * sum(x * x for x in Jv)
                gd = sum(gscale * d * (-dr + mp.mpf(float(B.kd)) * j) for d, dr, j in zip(diff, drift, Jv))
                Bs += -(quad + gd + mp.mpf(float(B.kp)) * C)
            b1.append(float(Bs))
    for c in tm.sel_col:
        ja = int(c) - (nv - na)
        b1.append(-tm.posture_kp * (q[nq - na + ja] - ref[tm.posture_ref + ja]) - tm.posture_kd * v[int(c)])
    b1 += [0.0] * (6 * tm.ncontact + tm.n_acteq + (3 if tm.cop else 0))
    bc = []
    for c in range(tm.ncontact):
        f = int(tm.contact_frame[c])
        bc += list(_se3_rhs(T["oMf"][f], T["vf"][f], T["af"][f], ref[tm.contact_ref[c]:tm.contact_ref[c] + 24], tm.contact_kp[c], tm.contact_kd[c]))
    out = dict(b1=np.array(b1, dtype=np.float64), bc=np.array(bc, dtype=np.float64))
    if bounds:
        res = [acc_limits(q[nq - na + j], v[nv - na + j], m.q_lb[j], m.q_ub[j], m.dq_max[j], tm.dt) for j in range(tm.n_bound)]
        out["blb"] = np.array([float(r[0]) for r in res])
        out["bub"] = np.array([float(r[1]) for r in res])
        out["decisions"] = [r[2] for r in res]
        out["margins"] = [r[3] for r in res]
    return out


def pair_gaps(rbd, m, tm, q: np.ndarray) -> List[List[Tuple[float, float, float]]]:
    """Per self-collision block, per pair: (norm - (r0 + radius), r0 + radius, margin) at q."""
    T = rbd.rbd_terms(m, q, np.zeros(m.nv))
    out = []
    for B in tm.blocks:
        if B.kind == mdl.T_SELFCOLLISION:
            out.append([(float(np.linalg.norm(T["oMf"][B.frame][9:] - T["oMf"][fa][9:])) - (r0 + B.radius), r0 + B.radius, B.margin) for fa, r0 in B.avoided])
    return out


def band_targets(aa: float, margin: float) -> Tuple[float, ...]:
    return (-0.2 * aa, -margin, 0.0, 0.5 * margin, margin, 5.0 * margin)


def band_of(gap: float, aa: float, margin: float) -> Optional[int]:
    """Which of the six distances a pair sits at (to a millionth of its margin), or None."""
    for k, t in enumerate(band_targets(aa, margin)):
        if abs(gap - t) <= 1e-6 * margin:
            return k
    return None


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def _models():
    def talos():
        m = mdl.talos_like()
        st = structure.talos_structure()
        return m, st, mdl.build_taskmap(m, st, mdl.talos_stack())

    def franka():
        m = mdl.franka_like()
        st = structure.franka_structure()
        return m, st, mdl.build_taskmap(m, st, mdl.franka_stack())

    def tree():
        m = mdl.random_tree(21, 30, True, nframe=12)
        st, stack = mdl.random_stack(m, 121, 2)
        return m, st, mdl.build_taskmap(m, st, stack, dt=2e-3)

    return {"talos": talos, "franka": franka, "tree": tree}


MODELS = _models()
BATCH = {"talos": 52, "franka": 64, "tree": 64}  # (Talos: 52 instances x 2 contacts = every angle x octant on a contact)

def _decisions_f64(q, dq, lo, hi, vm, dt):
    """The eleven decisions of acc_limits for arrays of (q, dq), in float64 (-1: not evaluated), the smallest margin among the
    inequalities, lb and ub: only to SEARCH for placements -- the mpmath statement above is what the tests hold anything to."""
    with np.errstate(all="ignore"):
        n = q.size
        D = np.full((n, 11), -1)
        G = np.full(n, np.inf)

        def decide(i, a, b, val, where):
            D[where, i] = val[where]
            sc = np.maximum(np.abs(a), np.abs(b))
            g = np.where(sc == 0, np.inf, np.abs(a - b) / np.where(sc == 0, 1.0, sc))
            G[where] = np.minimum(G[where], g[where])

        acc = vm / dt
        mdq = -dq / dt
        max_q3, min_q3 = 2 / dt ** 2 * (hi - q - dt * dq), 2 / dt ** 2 * (lo - q - dt * dq)
        neg = dq <= 0
        D[:, 0] = neg
        c1 = min_q3 < mdq
        decide(1, min_q3, mdq, c1, neg)
        w2 = neg & ~c1
        D[w2, 2] = (q != lo)[w2]
        first = dq * dq / (2 * (q - lo))
        w3 = w2 & (q != lo)
        decide(3, first, mdq, first >= mdq, w3)
        lb_pos = np.where(neg, np.where(c1, min_q3, np.where(q != lo, np.fmax(first, mdq), 1e6)), min_q3)
        c4 = max_q3 > mdq
        decide(4, max_q3, mdq, c4, ~neg)
        w5 = ~neg & ~c4
        D[w5, 5] = (q != hi)[w5]
        second = -dq * dq / (2 * (hi - q))
        w6 = w5 & (q != hi)
        decide(6, mdq, second, mdq >= second, w6)
        ub_pos = np.where(~neg, np.where(c4, max_q3, np.where(q != hi, np.fmin(second, mdq), -1e6)), max_q3)
        b_1, b_2 = 2 * dt * dq + acc * dt * dt, 2 * dt * dq - acc * dt * dt
        c_1, c_2 = dq * dq - 2 * acc * (hi - (q + dt * dq)), dq * dq - 2 * acc * ((q + dt * dq) - lo)
        d1, d2 = b_1 * b_1 - 4 * dt * dt * c_1, b_2 * b_2 - 4 * dt * dt * c_2
        every = np.ones(n, bool)
        decide(7, b_1 * b_1, 4 * dt * dt * c_1, d1 >= 0, every)
        decide(8, b_2 * b_2, 4 * dt * dt * c_2, d2 >= 0, every)
        ub_via = np.where(d1 >= 0, (-b_1 + np.sqrt(np.abs(d1))) / (2 * dt * dt), mdq)
        lb_via = np.where(d2 >= 0, (-b_2 - np.sqrt(np.abs(d2))) / (2 * dt * dt), mdq)
        lb = np.maximum(np.maximum(lb_pos, lb_via), np.maximum((-vm - dq) / dt, -acc))
        ub = np.minimum(np.minimum(ub_pos, ub_via), np.minimum((vm - dq) / dt, acc))
        decide(9, ub, lb, ub < lb, every)
        w10 = ub < lb
        D[w10, 10] = (ub == ub_pos)[w10]
        lb, ub = np.where(w10 & (ub == ub_pos), ub, lb), np.where(w10 & (ub != ub_pos), lb, ub)
    return D, G, lb, ub


def _joint_pool(rng, lo: float, hi: float, vm: float, dt: float, still: bool, n: int = 20000):
    """Candidate (q, dq) of one joint from its own limits -- anywhere in the range, on a limit exactly, a little inside or outside one
    (1e-8 to 1), within a few steps or a braking distance of one, speeds from a thousandth of dq_max to four times it, either sign
    (still: dq = +0.0 or -0.0) -- grouped by the decisions they lead to; those with a margin under 1e-4 and those where an ulp of q shows in the result are left out."""
    s = rng.choice([-1.0, 1.0], n)
    L = np.where(s < 0, lo, hi)
    dq = rng.choice([-1.0, 1.0], n) * vm * 10 ** rng.uniform(-3, 0.6, n)
    if still:
        dq = np.where(dq > 0, 0.0, -0.0)
    kind = rng.integers(0, 7, n)
    step = dt * np.abs(dq)
    q = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                  [rng.uniform(lo, hi, n), L, L - s * 10 ** rng.uniform(-8, 0, n), L + s * 10 ** rng.uniform(-8, 0, n),
                   L - s * rng.uniform(0, 4, n) * step, L - s * rng.uniform(0, 3, n) * step * 0.5 * (1 + np.abs(dq) / vm)],
                  L - s * rng.uniform(-1, 1, n) * step)
    D, G, lb, ub = _decisions_f64(q, dq, lo, hi, vm, dt)
    ok = G > 1e-4
    for to in (np.inf, -np.inf):  # well conditioned: an ulp of q moves lb and ub by 2e-12 (relative, at least absolute) at the most
        _, _, lb1, ub1 = _decisions_f64(np.nextafter(q, to), dq, lo, hi, vm, dt)
        with np.errstate(all="ignore"):
            ok &= (kind == 1) | ((np.abs(lb1 - lb) <= 2e-12 * np.maximum(1.0, np.abs(lb))) & (np.abs(ub1 - ub) <= 2e-12 * np.maximum(1.0, np.abs(ub))))
    q, dq, D = q[ok], dq[ok], D[ok]
    code = (D + 1) @ (3 ** np.arange(11))
    pool: Dict[tuple, List[Tuple[float, float]]] = {}
    for c in np.unique(code):
        w = np.where(code == c)[0][:8]
        pool[tuple(None if x < 0 else bool(x) for x in D[w[0]])] = [(q[i], dq[i]) for i in w]
    return pool


def _place_joints(rng, m, tm, q, v, still_rows):
    """Overwrites the actuated joints' (q_j, dq_j) of the batch: joint j of instance i takes the next of the decision tuples its pool
    reaches (so every tuple is taken in turn, on every joint)."""
    na, nq, nv = m.na, m.nq, m.nv
    for j in range(tm.n_bound):
        for still in (False, True):
            pool = _joint_pool(rng, m.q_lb[j], m.q_ub[j], m.dq_max[j], tm.dt, still, 4000 if still else 20000)
            keys = sorted(pool, key=str)
            for n, i in enumerate(np.where(still_rows == still)[0]):
                cand = pool[keys[(n + j) % len(keys)]]
                q[i, nq - na + j], v[i, nv - na + j] = cand[int(rng.integers(0, len(cand)))]


def _path_joints(m, ba: int, bb: int) -> List[int]:
    """Actuated bodies whose joint moves exactly one of the two bodies (the chain between them)."""
    last = m.subtree_last()
    sup = lambda j, b: j <= b <= last[j]
    return [j for j in range(1 if m.floating_base else 0, m.nbody) if sup(j, ba) != sup(j, bb)]


@functools.lru_cache(maxsize=None)
def _oracle_model(name: str):
    from oracle import rbd
    return rbd.OracleModel(MODELS[name]()[0])


def _distance(m, q: np.ndarray, ft: int, fa: int) -> float:
    """Distance of two frames' origins, from the oracle's placements (the ones the laws are stated on)."""
    from oracle import rbd
    oMf = rbd.rbd_terms(_oracle_model("tree") if m.name.startswith("random_tree") else m, q, np.zeros(m.nv))["oMf"]
    return float(np.linalg.norm(oMf[ft, 9:] - oMf[fa, 9:]))


def _chain_extremes(m, q, ft: int, fa: int, free: List[int]) -> Tuple[np.ndarray, np.ndarray]:
    """Values of the chain's joints that bring two frames together, and apart (coordinate descent over the joints' ranges: the distance of two frames depends on the joints between them only)."""
    off = 1 if m.floating_base else 0

    dist = lambda qq: _distance(m, qq, ft, fa)

    out = []
    for sign in (1.0, -1.0):
        qq = q.copy()
        best = sign * dist(qq)
        for _ in range(2):
            for j in free:
                for x in np.linspace(0.98 * m.q_lb[j - off], 0.98 * m.q_ub[j - off], 9):
                    old = qq[m.idx_q(j)]
                    qq[m.idx_q(j)] = x
                    d = sign * dist(qq)
                    if d < best:
                        best = d
                    else:
                        qq[m.idx_q(j)] = old
        out.append(qq)
    return out[0], out[1]


def _aim_pair(m, q, ft: int, fa: int, aa: float, target: float, free: List[int], near: np.ndarray, far: np.ndarray) -> Optional[np.ndarray]:
    """The chain's joints at which the two frames' distance is aa + target: bisection along the segment from the instance's own values
    (or the far ones, when it is already closer than that) to the near ones.  None when the segment does not cross the distance."""
    idx = [m.idx_q(j) for j in free]

    def gap(x):
        qq = q.copy()
        qq[idx] = x
        return _distance(m, qq, ft, fa) - aa - target

    x0, x1 = q[idx].copy(), near[idx]
    if gap(x0) <= 0.0:
        x0 = far[idx]
    if not (gap(x0) > 0.0 and gap(x1) < 0.0):
        return None
    for _ in range(36):
        xm = 0.5 * (x0 + x1)
        if gap(xm) > 0.0:
            x0 = xm
        else:
            x1 = xm
    return 0.5 * (x0 + x1)


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """The batch of one model: states from sample_states, then joints placed on every branch of the bounds law, self-collision pairs
    moved to the six distances (trees), every SE(3) and contact reference set to R_frame(q) exp(theta a), and v = 0 with zero velocity
    and acceleration references in the odd rows."""
    mp.mp.dps = DPS
    m, st, tm = MODELS[name]()
    B = BATCH[name]
    s = mdl.sample_states(m, tm, B, 73_000, q_noise=0.3, v_noise=0.5, ref_noise=0.05)
    q, v, ref = s["q"], s["v"], s["ref"]
    rng = np.random.default_rng(4242)
    still = np.arange(B) % 2 == 1
    v[still] = 0.0
    _place_joints(rng, m, tm, q, v, still)
    # self-collision pairs: instance i aims pair (i // 6) % npairs at distance i % 6, with a joint of the chain between the two frames
    pairs = [(bi, B_.frame, fa, r0 + B_.radius, B_.margin) for bi, B_ in enumerate(tm.blocks) if B_.kind == mdl.T_SELFCOLLISION for fa, r0 in B_.avoided]
    aimed = []
    if name == "tree":
        chains = []
        for bi, ft, fa, aa, margin in pairs:
            free = _path_joints(m, int(m.frame_body[ft]), int(m.frame_body[fa]))
            chains.append((free,) + _chain_extremes(m, m.q0, ft, fa, free))
        for i in range(B):
            p = (i // 6) % len(pairs)
            bi, ft, fa, aa, margin = pairs[p]
            free, near, far = chains[p]
            hit = _aim_pair(m, q[i], ft, fa, aa, band_targets(aa, margin)[i % 6], free, near, far)
            if hit is not None:
                q[i, [m.idx_q(j) for j in free]] = hit
                aimed.append((i, p, i % 6))
    # law lanes: SE(3) blocks with an angular row, then contacts; lane slot n of the batch takes combo n % NCOMBO
    lanes = [("se3", k, B_.frame, B_.ref, B_.mask, B_.kp) for k, B_ in enumerate(tm.blocks) if B_.kind == mdl.T_SE3 and (B_.mask >> 3)]
    full = [l for l in lanes if l[4] == 63]
    part = [l for l in lanes if l[4] != 63]
    cont = [("contact", c, int(tm.contact_frame[c]), int(tm.contact_ref[c]), 63, float(tm.contact_kp[c])) for c in range(tm.ncontact)]
    combos = {}
    for group in (full, part, cont):
        per_state = (B // 2) * len(group)
        for i in range(B):
            for k, lane in enumerate(group):
                n = (i // 2) * len(group) + k
                if per_state >= NCOMBO:  # every angle x octant in the moving rows and again in the still ones, half a table apart
                    c = (n + (NCOMBO // 2 if still[i] else 0)) % NCOMBO
                elif 2 * per_state >= NCOMBO:  # every angle x octant once, every angle in both kinds of row
                    c = (n + (per_state if still[i] else 0)) % NCOMBO
                else:  # too few lanes for that: every angle first, then the near-pi angles in every octant; still rows mirror the axis
                    c = SHORT_ORDER[n % NCOMBO]
                    if still[i]:
                        c = (7 - c // len(ANGLES)) * len(ANGLES) + c % len(ANGLES)
                combos[(i, lane[0], lane[1])] = c
    for i in range(B):
        Rf, _ = m.frame_placements(q[i])
        for lane in full + part + cont:
            c = combos[(i, lane[0], lane[1])]
            Rr = _mpmat(Rf[lane[2]]) * exp3(ANGLES[c % len(ANGLES)], OCTANTS[c // len(ANGLES)])
            r0 = lane[3]
            ref[i, r0 + 3:r0 + 12] = np.array([[float(Rr[a, b]) for a in range(3)] for b in range(3)]).reshape(9)  # column-major
            if still[i]:
                ref[i, r0 + 12:r0 + 24] = 0.0
            elif lane[0] == "contact":
                ref[i, r0 + 12:r0 + 24] = 0.05 * rng.standard_normal(12)  # (a behaviour may set them, tasks.cpp:359-362)
        if still[i]:
            for B_ in tm.blocks:
                if B_.kind == mdl.T_SE3:
                    ref[i, B_.ref + 12:B_.ref + 24] = 0.0
                elif B_.kind == mdl.T_COM:
                    ref[i, B_.ref + 3:B_.ref + 9] = 0.0
    return dict(m=m, st=st, tm=tm, q=q, v=v, ref=ref, still=still, lanes=full + part + cont, full=full, part=part, cont=cont,
                combos=combos, pairs=pairs, aimed=aimed)


def _nudge(a: np.ndarray, up: bool) -> np.ndarray:
    return np.nextafter(a, np.inf if up else -np.inf)


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """inputs(name) with the reference rows, S per entry and the regime of every entry."""
    from oracle import rbd
    I = inputs(name)
    m, st, tm, q, v, ref = (I[k] for k in ("m", "st", "tm", "q", "v", "ref"))
    B = q.shape[0]
    rows = [reference_rows(rbd, m, tm, st, q[i], v[i], ref[i]) for i in range(B)]
    out = {k: np.stack([r[k] for r in rows]) for k in ("b1", "bc", "blb", "bub") if k in rows[0] and rows[0][k].size}
    S = {k: np.zeros_like(a) for k, a in out.items()}
    for up in (True, False):
        for i in range(B):
            r = reference_rows(rbd, m, tm, st, _nudge(q[i], up), v[i], _nudge(ref[i], up))
            for k in out:
                S[k][i] = np.maximum(S[k][i], np.abs(r[k] - out[k][i]))
    if tm.n_bound:
        qa = q[:, m.nq - m.na:]
        on_a_limit = (qa == m.q_lb[None, :]) | (qa == m.q_ub[None, :])
        S["blb"][on_a_limit] = 0.0
        S["bub"][on_a_limit] = 0.0
    # regime of every entry
    regime = {k: np.full(a.shape, REGIMES.index("bounds" if k in ("blb", "bub") else "other")) for k, a in out.items()}
    row = 0
    sc = 0
    gaps = [pair_gaps(rbd, m, tm, q[i]) for i in range(B)]
    bands = np.full((B, len(I["pairs"])), -1)
    for k, B_ in enumerate(tm.blocks):
        if B_.kind == mdl.T_SE3:
            o = 0
            for bit in range(6):
                if (B_.mask >> bit) & 1:
                    if bit >= 3 and (B_.mask >> 3):
                        for i in range(B):
                            regime["b1"][i, row + o] = REGIMES.index(ANGLE_REGIME[I["combos"][(i, "se3", k)] % len(ANGLES)])
                    o += 1
        elif B_.kind == mdl.T_SELFCOLLISION:
            p0 = sum(len(b.avoided) for b in tm.blocks[:k] if b.kind == mdl.T_SELFCOLLISION)
            for i in range(B):
                hit = [band_of(*g) for g in gaps[i][sc]]
                for a, h in enumerate(hit):
                    bands[i, p0 + a] = -1 if h is None else h
                hits = [h for h in hit if h is not None]
                regime["b1"][i, row] = REGIMES.index("5PL " + BANDS[min(hits)] if hits else "5PL elsewhere")  # the deepest of the block's pairs
            sc += 1
        row += B_.rows
    for c in range(tm.ncontact):
        for i in range(B):
            regime["bc"][i, 6 * c + 3:6 * c + 6] = REGIMES.index(ANGLE_REGIME[I["combos"][(i, "contact", c)] % len(ANGLES)])
    return dict(I, rows=out, S=S, regime=regime, decisions=[r.get("decisions", []) for r in rows], margins=[r.get("margins", []) for r in rows],
                bands=bands, gaps=gaps)


def bar(ref: np.ndarray, S: np.ndarray) -> np.ndarray:
    return TOL_ROWS * np.maximum(1.0, np.abs(ref)) + 4.0 * S


def worst_per_regime(C: dict, got: Dict[str, np.ndarray]) -> Dict[str, Tuple[float, float, float]]:
    """regime -> (largest |got - ref| / max(1, |ref|), largest S / max(1, |ref|), largest |got - ref| / bar) over b1, bc, blb, bub."""
    w: Dict[str, Tuple[float, float, float]] = {}
    for k, r in C["rows"].items():
        sc = np.maximum(1.0, np.abs(r))
        err, S = np.abs(got[k] - r), C["S"][k]
        for g in np.unique(C["regime"][k]):
            sel = C["regime"][k] == g
            old = w.get(REGIMES[g], (0.0, 0.0, 0.0))
            w[REGIMES[g]] = (max(old[0], float((err / sc)[sel].max())), max(old[1], float((S / sc)[sel].max())),
                             max(old[2], float((err / bar(r, S))[sel].max())))
    return w


def report(what: str, w: Dict[str, Tuple[float, float, float]]) -> None:
    for g in REGIMES:
        if g in w:
            print("%-28s %-18s err %.2e  S %.2e  err / bar %.3f" % (what, g, w[g][0], w[g][1], w[g][2]))
