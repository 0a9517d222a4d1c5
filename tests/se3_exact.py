"""An exact statement of the state integration after the path (csrc/wbcqp_integrate.hpp: integrate_one; oracle/wbc_oracle.c: wbco_integrate), in
mpmath at 80 digits, and the writer of the fixtures under tests/golden/se3_exact/.  CPU only; needs mpmath.  `python -m tests.se3_exact --write`.

The kernel and the oracle share one formulation (pinocchio's: exp6 through a rotation matrix with a Taylor switch at t = 1e-4, M0 * exp6, rotation
-> quaternion by Shoemake's four cases, sign continuity, a first-order normalisation).  This statement shares none of it: quaternion algebra and
the closed forms of exp on SE(3), no rotation matrix, no switch, no cases.
    v_next    no statement: fl(dq + fl(dt dv)) in numpy, bit for bit; an F32 handle computes that in double and stores float32 of it.  Everything
              below starts from that double, v: for an F64 handle it IS v_next as stored.
    joints    fl(q + fl(dt v)), bit for bit (F32: float32 of it).
    base      M0 exp6(dt v), (dt v) the exact products, q0 as the input's numbers say, normalised here:
                  q1 = q0 (x) (sin(t/2) w/t, cos(t/2)), then the sign that keeps q1 . q0 >= 0         w = dt v[3:6], t = |w|
                  p1 = p + R(q0) (u + A w x u + B w x (w x u))                                         u = dt v[0:3]
              A = (1 - cos t) / t^2 = 2 sin^2(t/2) / t^2, B = (t - sin t) / t^3 (evaluated with as many more digits as the difference
              cancels), their limits 1/2 and 1/6 at t = 0.  R(q0) u is the quaternion sandwich q0 (x) (u, 0) (x) q0*.
    q_solver  the rotation vector of the result quaternion AS STORED IN float64: angle 2 atan2(|u|, |w|) in [0, pi], axis u / |u| with the sign of
              w; an exact +0 where u is exactly 0.  A kept state (status not OPTIMAL): the same of the input quaternion; position, joints and
              the whole of q_next and v_next are the inputs bit for bit.
    K ticks   at a constant body twist (dv = 0) the state after K ticks is M0 exp6(K dt v): a one-parameter subgroup.  No sign is chosen there:
              each tick keeps the sign continuous, and q0 (x) (sin(s t/2) w/t, cos(s t/2)) is continuous in s.

SCALES (tests/se3_exact_cases.py says how 0 and inf are read).  Quaternion entries 1; rotation-vector entries max(1, angle); position entry i
    |p_i| + sum_j |R0_ij| (|u_j| + c_j),       c_j = |(w x u)_j| / (2 t^2) where t > 1e-4, 0 where not:
the reference's own (1 - cos t) / t^2 loses eps / (2 t^2) on the closed-form side of its switch (cos t is within eps / 2 of 1), and that loss is
its formulation, not a defect.  The K-tick end state: the largest |p_i| of the K + 1 states on the way plus sum_j (|u_j| + c_j) (|R_ij| <= 1 on a
path along which R turns), held to K times the one-step bar.

A DRIFTED input quaternion (|q0| = 1 +- 1e-6) has no exact statement: the reference's semantics there are pinocchio's (the rotation matrix of a
non-unit quaternion is no rotation; a first-order normalisation follows), so that family's values are the oracle's own outputs and its scales those
of the normalised input."""
from __future__ import annotations

import argparse
import functools
import os
from typing import Dict, Optional, Sequence

import mpmath as mp
import numpy as np

from tests.se3_exact_cases import FAMILIES, GOLDEN, KSTEPS, SWITCH, W_MARGIN, flat, inputs, path

DPS = 80
mp.mp.dps = DPS


def _f(x):
    return mp.mpf(float(x))  # (a float64 is a dyadic rational: exact)


def _vec(a):
    return [_f(x) for x in a]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def _norm(a):
    return mp.sqrt(_dot(a, a))


def _qmul(a, b):
    """Hamilton product, (x, y, z, w)."""
    c = _cross(a[:3], b[:3])
    return [a[3] * b[i] + b[3] * a[i] + c[i] for i in range(3)] + [a[3] * b[3] - _dot(a[:3], b[:3])]


def _rotate(q, u):
    r = _qmul(_qmul(q, list(u) + [mp.mpf(0)]), [-q[0], -q[1], -q[2], q[3]])
    return r[:3]


def _coefficients(t):
    """A = (1 - cos t) / t^2, B = (t - sin t) / t^3."""
    if t == 0:
        return mp.mpf(1) / 2, mp.mpf(1) / 6
    extra = max(0, int(-3 * mp.log10(t)) + 10)  # t - sin t = t^3 / 6 cancels 2 log10(1/t) digits
    with mp.workdps(DPS + extra):
        s = mp.sin(t / 2)
        A, B = 2 * s * s / (t * t), (t - mp.sin(t)) / t ** 3
    return +A, +B


def exp6(u, w, s=1):
    """exp6 of s (u, w): (translation, unit quaternion)."""
    u, w = [s * x for x in u], [s * x for x in w]
    t = _norm(w)
    A, B = _coefficients(t)
    wu = _cross(w, u)
    wwu = _cross(w, wu)
    tr = [u[i] + A * wu[i] + B * wwu[i] for i in range(3)]
    h = mp.sin(t / 2) / t if t != 0 else mp.mpf(1) / 2
    return tr, [h * w[0], h * w[1], h * w[2], mp.cos(t / 2)]


def compose(p, q, tr, dq):
    """(p, q) * (tr, dq) on SE(3)."""
    r = _rotate(q, tr)
    return [p[i] + r[i] for i in range(3)], _qmul(q, dq)


def rotvec(quat):
    """(rotation vector, angle, all exact zeros) of a quaternion that need not be of unit norm: 2 atan2(|u|, |w|) u / |u|, the sign of w."""
    u, w = quat[:3], quat[3]
    n = _norm(u)
    if n == 0:
        return [mp.mpf(0)] * 3, mp.mpf(0), True
    angle = 2 * mp.atan2(n, abs(w))
    s = -1 if w < 0 else 1
    return [angle * x / (s * n) for x in u], angle, False


def _np(v):
    return np.array([float(x) for x in v], dtype=np.float64)  # (mpf -> float rounds to nearest)


def base_step(p, quat, v6, dt, steps=1):
    """One instance's base: values (mpf lists) and scales (floats).  steps = K: the subgroup statement of K ticks."""
    dt_ = _f(dt)
    u, w = [dt_ * _f(x) for x in v6[:3]], [dt_ * _f(x) for x in v6[3:6]]
    q0 = _vec(quat)
    n0 = _norm(q0)
    q0 = [x / n0 for x in q0]
    p0 = _vec(p)
    t = _norm(w)
    tr, dq = exp6(u, w, steps)
    p1, q1 = compose(p0, q0, tr, dq)
    dot = _dot(q1, q0)
    if steps == 1 and dot < 0:
        q1 = [-x for x in q1]
    closed = t > _f(SWITCH)
    wu = _cross(w, u)
    c = [abs(x) / (2 * t * t) if closed else mp.mpf(0) for x in wu]
    R0 = [_rotate(q0, e) for e in ([1, 0, 0], [0, 1, 0], [0, 0, 1])]  # R0[j][i] = R_ij: for the scale alone
    reach = [abs(u[j]) + c[j] for j in range(3)]
    scale_p = [abs(p0[i]) + mp.fsum(abs(R0[j][i]) * reach[j] for j in range(3)) for i in range(3)]
    return dict(p=p1, q=q1, scale_p=_np(scale_p), reach=float(mp.fsum(reach)))


def solver_rotvec(stored_quat):
    """The rotation-vector entries of q_solver for a stored quaternion (float64 numbers): (values, scales)."""
    rv, angle, zero = rotvec(_vec(stored_quat))
    if zero:
        return np.zeros(3), np.zeros(3)  # exact +0
    scale = float(max(mp.mpf(1), angle))
    if abs(stored_quat[3]) < W_MARGIN * float(np.linalg.norm(stored_quat)):
        scale = np.inf  # the axis flips at w = 0: not judged
    return _np(rv), np.full(3, scale)


def statement(G) -> Dict[str, np.ndarray]:
    """The statement of one group: q_next, v_next, q_solver as float64 arrays, and their scales.  One statement for both handles: an F32
    handle computes in double and rounds once, so what is bit for bit there is float32 of these numbers."""
    fb, nv, dt = bool(G["fb"]), int(G["nv"]), float(G["dt"])
    q, dq, x = G["q"], G["dq"], G["x"]
    B = q.shape[0]
    kept = (G["status"] != 0) if "status" in G else np.zeros(B, dtype=bool)
    with np.errstate(invalid="ignore"):
        v = dq + dt * x[:, :nv]  # two roundings, unfused
        j0, off = (6, 1) if fb else (0, 0)
        joints = q[:, j0 + off:] + dt * v[:, j0:]
    q_next, q_solver = np.zeros_like(q), np.zeros_like(dq)
    s_next, s_solver = np.zeros_like(q), np.zeros_like(dq)
    v_next = np.where(kept[:, None], dq, v)
    q_next[:, j0 + off:] = np.where(kept[:, None], q[:, j0 + off:], joints)
    q_solver[:, j0:] = q_next[:, j0 + off:]
    if fb:
        for i in range(B):
            if kept[i]:
                q_next[i, :7] = q[i, :7]
                q_solver[i, :3] = q[i, :3]
                q_solver[i, 3:6], s_solver[i, 3:6] = solver_rotvec(q[i, 3:7])
                continue
            r = base_step(q[i, :3], q[i, 3:7], v[i, :6], dt)
            q_next[i, :3], q_next[i, 3:7] = _np(r["p"]), _np(r["q"])
            s_next[i, :3], s_next[i, 3:7] = r["scale_p"], 1.0
            q_solver[i, :3], s_solver[i, :3] = q_next[i, :3], r["scale_p"]
            q_solver[i, 3:6], s_solver[i, 3:6] = solver_rotvec(q_next[i, 3:7])
    return {"q_next": q_next, "v_next": v_next, "q_solver": q_solver, "scale.q_next": s_next, "scale.q_solver": s_solver}


def k_steps(G, K=KSTEPS) -> Dict[str, np.ndarray]:
    """The state after K ticks at the group's constant twist (dv = 0, floating base, no joints): values and scales of q_next."""
    q, dq, dt = G["q"], G["dq"], float(G["dt"])
    assert int(G["nv"]) == 6 and not np.any(G["x"])
    end, scale = np.zeros_like(q), np.ones_like(q)
    for i in range(q.shape[0]):
        r = base_step(q[i, :3], q[i, 3:7], dq[i], dt, K)
        end[i, :3], end[i, 3:7] = _np(r["p"]), _np(r["q"])
        way = np.abs(np.array([_np(base_step(q[i, :3], q[i, 3:7], dq[i], dt, k)["p"]) for k in range(K + 1)])).max(axis=0)
        scale[i, :3] = way + r["reach"]
    return {"end.q_next": end, "end.scale.q_next": scale, "K": np.int32(K)}


def _oracle_values(G) -> Dict[str, np.ndarray]:
    from oracle import oracle
    oracle.build()
    return oracle.integrate(bool(G["fb"]), float(G["dt"]), G["q"], G["dq"], G["x"][:, :int(G["nv"])])


def compute(family) -> Dict[str, np.ndarray]:
    """The fixture of a family, flat ("<group>.<key>")."""
    out = {}
    for g, G in inputs(family).items():
        F = dict(G)
        F.update(statement(G))
        if family == "drifted":  # no exact statement: the oracle's own outputs, the scales of the normalised input
            F.update(_oracle_values(G))
        if family == "ksteps":
            F.update(k_steps(G))
        out[g] = F
    return flat(out)


@functools.lru_cache(maxsize=None)
def computed(family) -> Dict[str, np.ndarray]:
    return compute(family)


def identities() -> Dict[str, float]:
    """The statement against itself: the result's norm, exp6(a) exp6(b) = exp6(a + b) for parallel twists, K ticks one by one against the
    subgroup statement.  The largest defect of each."""
    rng = np.random.default_rng(5)
    worst = {"norm": mp.mpf(0), "parallel": mp.mpf(0)}
    for t in (0.0, 1e-170, 1e-8, 0.9e-4, 1e-4, 1.1e-4, 1e-3, 1.0, 2.5, 4.0):
        ax = rng.standard_normal(3)
        w = _vec(ax / np.linalg.norm(ax) * t)
        u = _vec(rng.standard_normal(3))
        q0 = _vec(rng.standard_normal(4))
        n0 = _norm(q0)
        q0 = [x / n0 for x in q0]
        p0 = _vec(rng.standard_normal(3))
        a, b = mp.mpf("0.3"), mp.mpf("1.9")
        pa, qa = compose(p0, q0, *exp6(u, w, a))
        pab, qab = compose(pa, qa, *exp6(u, w, b))
        ps, qs = compose(p0, q0, *exp6(u, w, a + b))
        worst["norm"] = max(worst["norm"], abs(_norm(qab) - 1))
        worst["parallel"] = max(worst["parallel"], max(abs(x - y) for x, y in zip(pab + qab, ps + qs)))
    return {k: float(v) for k, v in worst.items()}


def write(families: Optional[Sequence[str]] = None) -> None:
    os.makedirs(GOLDEN, exist_ok=True)
    for f in families or FAMILIES:
        np.savez_compressed(path(f), **compute(f))
        print("%-10s %7d bytes" % (f, os.path.getsize(path(f))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="write tests/golden/se3_exact/*.npz")
    ap.add_argument("families", nargs="*")
    a = ap.parse_args()
    if a.write:
        write(a.families or None)
