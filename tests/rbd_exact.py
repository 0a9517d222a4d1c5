"""An exact statement of the rigid-body terms on a kinematic tree, entry by entry, with the scale of every entry.

Shared by tests/test_rbd_exact_host.py (the C oracle and the numpy statements of inria_wbc_amd/*.py against this statement, on the CPU) and
tests/test_gpu_rbd_exact.py (the device against the committed fixtures).  tests/task_laws.py states the three task laws; this is the statement of
what it takes from elsewhere: placements, Jacobians, CoM, momentum, M, nle and the inverse dynamics.

Nothing here is a recursive spatial-algebra algorithm.  The module reads `Model`'s tables and the joint conventions of `Model.body_placements`
(the quaternion-to-rotation formula applied to the quaternion as given, not renormalised) and uses mpmath at DPS = 80 digits:
  * placements are computed directly;
  * first derivatives are central differences (step STEP = 1e-20) of the placement map along the tangent: q_j + e for a joint; p + R e v and
    R exp(e w^) for the free-flyer, v and w in the base's own axes.  From them the frame Jacobians in the three conventions of
    wbcqp_reference_frame, the body-CoM and angular Jacobians, Jcom and Ag (linear, then angular about the CoM, world axes);
  * second derivatives are differences along the curve q_j + t v_j + t^2 a_j / 2, M0 exp(t xi + t^2 xi' / 2): body and frame velocities, the
    frames' classical accelerations at a = 0 (drift), vcom, acom, Ag v and d(Ag v)/dt at a = 0;
  * M is the Hessian of the kinetic energy, sum_b m Jc_b' Jc_b + Jw_b' R I_c R' Jw_b; nle and the inverse dynamics are d'Alembert's principle,
    tau_j = sum_b Jc_bj . m (a_c,b - g) + Jw_bj . (I_w alpha_b + w_b x I_w w_b) - sum_k (J_k' w_k)_j.
A central difference of step 1e-20 is off by 1e-40 of the value and, at 80 digits, rounds at 1e-60; a second difference rounds at 1e-80 / 1e-40.
check_steps() asserts that halving the step moves nothing by more than 1e-25 of its scale.

THE SCALE of an entry is what its exact computation sums with every elementary product replaced by its magnitude, down to the model's tables:
  * a rotation: SR_b = SR_parent |R_placement| |R_joint| (the quaternion formula term by term); a position: Sp_b = Sp_parent + SR_parent |link|;
  * a Jacobian column at a point: |axis| for a translation, the two terms of |axis| x |lever| for a rotation, the lever's components being the
    sum of the |link vectors| along the chain from the joint to the point; turned into a frame's axes with SR_frame';
  * M(i, j): sum_b m sum_k SJc_bi[k] SJc_bj[k] + sum_kl SJw_bi[k] SI_w[k, l] SJw_bj[l], SI_w = SR |I_c| SR';
  * velocities: sum_j (column scale) |v_j|; accelerations: sum_j (column scale) |a_j| plus the magnitudes of w x (w x r) and 2 w x v pair by pair (an angular
    acceleration: also the products of R_ddot R' itself, whose rotations are orthogonal to rounding only);
  * a generalised force: the d'Alembert sum over the dof's subtree with every factor's scale.
An entry whose scale is under ZERO_REL = 1e-20 of the array's largest is a STRUCTURAL ZERO: its scale is reported as 0 and every implementation must
give an exact 0 there.  The bar of a comparison is K eps scale, entry by entry (worst_ratio below).

`scale_total` (M, nle, tau_a, tau_aw, Agv) is the scale of an algorithm that forms a subtree's total as a difference of whole-robot running totals
about one common origin -- the floating base (csrc/wbcqp_rnea.hpp, wbcqp_terms.hpp), the world's origin for a fixed base: |S_i|' (sum over ALL
bodies of |Y_b about the origin|, entry by entry) |S_j| for M, the same with the bodies' momentum rates in place of Y_b S_j for a force.

`scale_world` and `scale_base` (every quantity but placement, com and the forces) are the local sums for an algorithm that forms every column about
one common origin and moves it to the point: a rotation's lever is then two, origin to joint and origin to point, each with its magnitude.  They are
what a zero lever (local scale 0, an exact zero for a body-local recursion) and the rates cost a common-origin formulation (tests/test_gpu_rbd_exact.py).

THE SECOND-ORDER KINEMATICS (what wbcqp_kinematic_hessians computes; fixtures of their own, <case>.hessians.npz, for hessian_frames(case)):
  * H_world, H_local, H_lwa [states, frames, 6, nv, nv]: H[f, r, j, k] is the central difference (step STEP again) along dof k in the tangent space
    of the frame's Jacobian entry J[f, r, j] in that convention, J being the central difference of the placement map above, formed anew at either
    displaced configuration -- a nested difference: it rounds at 1e-80 / 1e-40 and is off by 1e-40, check_steps_hessians() halves either step;
  * dJ_world, dJ_local, dJ_lwa [states, frames, 6, nv]: the same difference of J along the curve q (+) t v (a = 0), on its own -- H is not contracted;
  * no table of cross products is used.  `scale` of an H entry is the motion cross product (l1, w1) x_m (l2, w2) = (w1 x l2 + l1 x w2, w1 x w2) of the
    two columns' J_<c>.scale with every term of every component added; in LOCAL_WORLD_ALIGNED the linear rows have one term, not two: l_j = w_j x
    (frame - joint j), a dof k of j's body or above it turns all of it (w_k x l_j), one under it moves the frame's origin alone (w_j x l_k);
    `scale_world`: the same of the columns' scale_world.  dJ.scale = sum_k H.scale[..., j, k] |v_k|; dJ.scale_world is what
    csrc/wbcqp_hessians.hpp sums, (|V|(frame's body) + |V|(bodyof(j))) x_m |S_j| about the world's origin, |V|(b) = sum over the chain to b of
    |S_k| |v_k|, moved to the frame and turned with SR_frame' for LOCAL_WORLD_ALIGNED and LOCAL: the difference V(frame) - V(body) counts both;
  * the STRUCTURAL ZEROS of H are decided from the values (dependence()): scale and scale_world are 0 where the exact value is under ZERO_REL of
    its magnitude sum in every state of the case and in generic(case), a second model of generic geometry at a generic state -- there J[f, r, j]
    does not depend on q_k at all.  The decision is made with exact_rotations: it is a statement about rigid bodies.  The fixture's value is 0 there
    (with the tables' own rotations it is 1e-16 of the magnitude sum).  tests/test_rbd_exact_host.py asserts that inria_wbc_amd/hessians.py's
    structure_masks says the same.

The identities the statement is held to (tests/test_rbd_exact_host.py): M symmetric, (Ag of the first derivatives) v = the bodies' momenta on the curve,
and v' nle(q, v, g = 0) = v' M_dot v / 2 -- the last with the tables' rotations orthogonalised in mpmath (exact_rotations), because it is an identity of
rigid bodies and the tables' own rotations are orthogonal to 1e-16 only.  The second-order quantities: second_order_identities().

Cases: the smallest at which the tree kernels can go wrong (CASES).  Their statements are committed under tests/golden/rbd_exact/ as compressed
.npz: `python -m tests.rbd_exact --write` makes them, <case>.npz and <case>.hessians.npz.
"""
from __future__ import annotations

import copy
import functools
import os
import sys
import time
from typing import Dict, List, Optional, Sequence

import mpmath as mp
import numpy as np

from inria_wbc_amd import model as mdl
from tests.rbd_exact_cases import (CASES, CONVENTIONS, EPS, FULL_ONLY, GOLDEN, HESSIANS, K_ORACLE, NO_ORIGIN, ORIGINS, QUANTITIES,  # noqa: F401
                                   RATES, SECOND_ORDER, SMALL, TOTALS, hessian_frames, hessians_path, load, load_hessians, model, path, ratios,
                                   states, worst_ratio, wrench_frames)

DPS = 80
STEP = "1e-20"
ZERO_REL = 1e-20
CHECKS = ("check.M_asymmetry", "check.Agv_identity")  # the statement's own identities, per state: computed with it, kept out of the fixtures


# ---- 3-vectors and 3 x 3 matrices of mpmath numbers, as lists ------------------------------------------------------------------------------
def _f(x):
    return mp.mpf(float(x))


def _vec(a):
    return [_f(x) for x in a]


def _mat(a):
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    return [[_f(a[i, j]) for j in range(3)] for i in range(3)]


def _zero3():
    return [mp.mpf(0), mp.mpf(0), mp.mpf(0)]


def _eye():
    return [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]


def _mv(A, x):
    return [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(3)]


def _mtv(A, x):
    return [A[0][i] * x[0] + A[1][i] * x[1] + A[2][i] * x[2] for i in range(3)]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mmt(A, B):
    return [[A[i][0] * B[j][0] + A[i][1] * B[j][1] + A[i][2] * B[j][2] for j in range(3)] for i in range(3)]


def _add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _sc(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _cmag(a, b):
    """The two terms of every component of a cross product, added: for vectors of magnitudes."""
    return [a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]]


def _vabs(a):
    return [abs(x) for x in a]


def _mabs(A):
    return [[abs(x) for x in r] for r in A]


def _madd(A, B):
    return [[A[i][j] + B[i][j] for j in range(3)] for i in range(3)]


def _msub(A, B):
    return [[A[i][j] - B[i][j] for j in range(3)] for i in range(3)]


def _msc(s, A):
    return [[s * x for x in r] for r in A]


def _col(A, k):
    return [A[0][k], A[1][k], A[2][k]]


def _vee(W):
    return [(W[2][1] - W[1][2]) / 2, (W[0][2] - W[2][0]) / 2, (W[1][0] - W[0][1]) / 2]


def _hat(w):
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def _rot(axis: int, a):
    """model._rot in mpmath."""
    c, s = mp.cos(a), mp.sin(a)
    R = _eye()
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i][i], R[i][j], R[j][i], R[j][j] = c, -s, s, c
    return R


def _quat_rot(x, y, z, w):
    """model.quat_to_rot in mpmath, on the quaternion as given."""
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _quat_rot_scale(x, y, z, w):
    x, y, z, w = abs(x), abs(y), abs(z), abs(w)
    return [[1 + 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 + 2 * (x * x + z * z), 2 * (y * z + x * w)],
            [2 * (x * z + y * w), 2 * (y * z + x * w), 1 + 2 * (x * x + y * y)]]


def _exp6(rho, phi):
    """exp of a small twist (linear rho, angular phi) of SE(3): (R, p), by the series (the arguments are of the size of the step)."""
    t2 = _dot(phi, phi)
    A = 1 - t2 / 6 + t2 * t2 / 120 - t2 ** 3 / 5040
    B = mp.mpf(1) / 2 - t2 / 24 + t2 * t2 / 720 - t2 ** 3 / 40320
    Cc = mp.mpf(1) / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880
    K = _hat(phi)
    K2 = _mm(K, K)
    R = _madd(_eye(), _madd(_msc(A, K), _msc(B, K2)))
    Vm = _madd(_eye(), _madd(_msc(B, K), _msc(Cc, K2)))
    return R, _mv(Vm, rho)


# ---- the model's tables ---------------------------------------------------------------------------------------------------------------------
class _Tables:
    def __init__(self, m):
        self.m = m
        nb = m.nbody
        self.nb, self.nv, self.nf, self.fb = nb, m.nv, m.nframe, bool(m.floating_base)
        self.parent = [int(x) for x in m.parent]
        self.last = [int(x) for x in m.subtree_last()]
        self.jtype = [int(x) for x in m.jtype]
        self.Rp = [_mat(m.placement[b, :9]) for b in range(nb)]
        self.pp = [_vec(m.placement[b, 9:]) for b in range(nb)]
        self.mass = [_f(m.inertia[b, 0]) for b in range(nb)]
        self.c = [_vec(m.inertia[b, 1:4]) for b in range(nb)]
        Y = m.inertia
        self.I = [_mat([[Y[b, 4], Y[b, 5], Y[b, 6]], [Y[b, 5], Y[b, 7], Y[b, 8]], [Y[b, 6], Y[b, 8], Y[b, 9]]]) for b in range(nb)]
        self.fbody = [int(x) for x in m.frame_body]
        self.fR = [_mat(m.frame_placement[f, :9]) for f in range(self.nf)]
        self.fp = [_vec(m.frame_placement[f, 9:]) for f in range(self.nf)]
        self.g = _vec(m.gravity)
        # dofs: (body, kind, axis); kind: "fl" / "fa" the free-flyer's linear / angular, "r" revolute, "p" prismatic
        self.dofs = []
        for b in range(nb):
            jt = self.jtype[b]
            if jt == mdl.J_FREEFLYER:
                self.dofs += [(b, "fl", k) for k in range(3)] + [(b, "fa", k) for k in range(3)]
            elif jt <= mdl.J_RZ:
                self.dofs.append((b, "r", jt - mdl.J_RX))
            else:
                self.dofs.append((b, "p", jt - mdl.J_PX))
        assert len(self.dofs) == self.nv
        self.sup = [[j for j, (a, _, _) in enumerate(self.dofs) if a <= b <= self.last[a]] for b in range(nb)]  # the dofs that move body b
        self.own = [[j for j, (a, _, _) in enumerate(self.dofs) if a == b] for b in range(nb)]

    def local(self, b, x):
        """Body b's placement in its parent from its joint's coordinate x (the free-flyer: x = (R, p)), as Model.body_placements composes it."""
        jt = self.jtype[b]
        if jt == mdl.J_FREEFLYER:
            return _mm(self.Rp[b], x[0]), _add(_mv(self.Rp[b], x[1]), self.pp[b])
        if jt <= mdl.J_RZ:
            return _mm(self.Rp[b], _rot(jt - mdl.J_RX, x)), list(self.pp[b])
        return [list(r) for r in self.Rp[b]], _add(_sc(x, _col(self.Rp[b], jt - mdl.J_PX)), self.pp[b])

    def forward(self, loc, R=None, p=None, start=0):
        """World placements of the bodies start .. last[start] from the local ones (the others are taken from R, p)."""
        R = {} if R is None else R
        p = {} if p is None else p
        outR, outp = {}, {}
        for b in range(start, self.last[start] + 1):
            par = self.parent[b]
            if par < 0:
                outR[b], outp[b] = loc[b]
            else:
                Rq, pq = (outR[par], outp[par]) if par in outR else (R[par], p[par])
                outR[b], outp[b] = _mm(Rq, loc[b][0]), _add(_mv(Rq, loc[b][1]), pq)
        return outR, outp


def _coords(T, q):
    """Per body: the joint's coordinate in mpmath (the free-flyer: (R, p) of the quaternion as given)."""
    m = T.m
    out = []
    for b in range(T.nb):
        i = m.idx_q(b)
        if T.jtype[b] == mdl.J_FREEFLYER:
            out.append((_quat_rot(*_vec(q[i + 3:i + 7])), _vec(q[i:i + 3])))
        else:
            out.append(_f(q[i]))
    return out


def _moved(T, x, b, kind, k, e):
    """The joint coordinate of body b moved by e along dof (kind, k)."""
    if kind == "fl":
        return x[0], _add(x[1], _sc(e, _col(x[0], k)))
    if kind == "fa":
        w = _zero3()
        w[k] = e
        return _mm(x[0], _exp6(_zero3(), w)[0]), x[1]
    return x + e


def _on_curve(T, x, b, v, a, t):
    """The joint coordinate of body b at time t of the curve with velocity v and velocity derivative a at 0."""
    iv = T.m.idx_v(b)
    if T.jtype[b] == mdl.J_FREEFLYER:
        xi = [t * v[iv + i] + t * t * a[iv + i] / 2 for i in range(6)]
        Re, pe = _exp6(xi[:3], xi[3:])
        return _mm(x[0], Re), _add(x[1], _mv(x[0], pe))
    return x + t * v[iv] + t * t * a[iv] / 2


def _hi_lo(a):
    """An array of mpmath numbers as two float64 arrays: the rounded value, and what rounding left."""
    a = np.array(a, dtype=object)
    if not a.size:
        return np.zeros(a.shape), np.zeros(a.shape)
    hi = np.vectorize(float, otypes=[np.float64])(a)
    lo = np.vectorize(lambda x, h_: float(x - mp.mpf(h_)), otypes=[np.float64])(a, hi)
    return hi, lo


def statement(m, q, v, a, wframes: Sequence[int], wrench, step: str = STEP, **kw) -> Dict[str, np.ndarray]:
    """_statement, and beside every quantity's `scale` its `scale_world` and `scale_base` (but NO_ORIGIN): the same sums for an algorithm that forms
    every column about ONE common origin -- the world's (csrc/wbcqp_observe.hpp, wbcqp_jacobians.hpp) or the floating base (wbcqp_fdyn.hpp,
    wbcqp_terms.hpp; a fixed base: the world's) -- so that a rotation's lever is two, origin to joint and origin to point, each with its magnitude."""
    out = _statement(m, q, v, a, wframes, wrench, step, **kw)
    plain = not (kw.get("want_M_only") or kw.get("raw") or kw.get("exact_rotations") or kw.get("shift") is not None or kw.get("gravity") is False)
    if plain:  # (the scales of the other origins: for the plain statement only, the one the fixtures hold)
        for origin in ORIGINS:
            alt = _statement(m, q, v, a, wframes, wrench, step, origin=origin)
            for k in QUANTITIES:
                if k not in NO_ORIGIN:
                    assert np.array_equal(alt[k], out[k]) and (alt[k + ".scale"] >= out[k + ".scale"]).all(), k
                    out[k + ".scale_" + origin] = alt[k + ".scale"]
    return out


def _statement(m, q, v, a, wframes: Sequence[int], wrench, step: str = STEP, want_M_only: bool = False, gravity: bool = True, shift=None,
               raw: bool = False, exact_rotations: bool = False, origin: Optional[str] = None, hessian_frames: Optional[Sequence[int]] = None,
               step2: str = STEP, values: bool = True) -> Dict[str, np.ndarray]:
    """Every quantity of QUANTITIES for one state as float64 arrays: out[name], out[name + ".scale"] and, for TOTALS, out[name + ".scale_total"].
    wrench [len(wframes), 6]: linear, angular in the frames' own axes.  shift: evaluate at time `shift` of the curve that leaves q with the constant
    velocity v.  exact_rotations: the tables' rotations replaced by the nearest orthogonal matrices and the quaternion by the unit one, in mpmath
    (what the identities of rigid bodies presume; the tables' own are orthogonal to 1e-16).  raw: also out[name + ".lo"], what rounding to float64 left of every value, and out["_mp"], M, nle, the frame Jacobians and the drifts as mpmath numbers.
    hessian_frames: return _second_order's arrays for those frames instead (step2: the step of the difference of the Jacobian; values False: the
    magnitude sums alone), as soon as the Jacobians and their scales stand."""
    mp.mp.dps = DPS
    T = _tables(m, exact_rotations)
    nb, nv, nf = T.nb, T.nv, T.nf
    h = mp.mpf(step)
    zero = mp.mpf(0)
    x0 = _coords(T, q)
    if exact_rotations and T.fb:
        n_ = mp.sqrt(sum(_f(x) ** 2 for x in q[3:7]))
        x0[0] = (_quat_rot(*[_f(x) / n_ for x in q[3:7]]), x0[0][1])
    if shift is not None:
        x0 = [_on_curve(T, x0[b], b, [_f(x) for x in v], [mp.mpf(0)] * nv, shift) for b in range(nb)]
    loc0 = [T.local(b, x0[b]) for b in range(nb)]
    R, p = T.forward(loc0)
    vv, aa = [_f(x) for x in v], [_f(x) for x in a]
    av, ab = [abs(x) for x in vv], [abs(x) for x in aa]
    g = T.g if gravity else _zero3()

    # ---- scales of the placements ----------------------------------------------------------------------------------------------------------
    SR, Sp, Spre = [None] * nb, [None] * nb, [None] * nb
    for b in range(nb):
        par = T.parent[b]
        SRpar = _eye() if par < 0 else SR[par]
        Sppar = _zero3() if par < 0 else Sp[par]
        Spre[b] = _mm(SRpar, _mabs(T.Rp[b]))  # magnitude of the axes the joint moves about
        jt = T.jtype[b]
        link = _mv(SRpar, _vabs(T.pp[b]))
        if jt == mdl.J_FREEFLYER:
            i = m.idx_q(b)
            SR[b] = _mm(Spre[b], _quat_rot_scale(*_vec(q[i + 3:i + 7])))
            link = _add(link, _mv(Spre[b], _vabs(x0[b][1])))
        elif jt <= mdl.J_RZ:
            SR[b] = _mm(Spre[b], _mabs(_rot(jt - mdl.J_RX, x0[b])))
        else:
            SR[b] = Spre[b]
            link = _add(link, _sc(abs(x0[b]), _col(Spre[b], jt - mdl.J_PX)))
        Sp[b] = _add(Sppar, link)

    def axis_scale(j):
        b, kind, k = T.dofs[j]
        return _col(SR[b], k) if kind in ("fl", "fa") else _col(Spre[b], k)

    SZ = [axis_scale(j) for j in range(nv)]

    def column_scale(j, b, ax):
        """(linear, angular) scale of dof j's column at the point of body b whose offset has the magnitudes ax in the body's axes."""
        a_, kind, _ = T.dofs[j]
        if kind in ("fl", "p"):
            return SZ[j], _zero3()
        if origin is None:
            lever = _add(_sub(Sp[b], Sp[a_]), _mv(SR[b], ax))
            return _cmag(SZ[j], lever), SZ[j]
        So = Sp[0] if (origin == "base" and T.fb) else _zero3()
        return _add(_cmag(SZ[j], _sub(Sp[a_], So)), _cmag(SZ[j], _sub(_add(Sp[b], _mv(SR[b], ax)), So))), SZ[j]

    # ---- first derivatives -------------------------------------------------------------------------------------------------------------------
    dP: List[dict] = []  # per dof: body -> (dp, dR)
    for j, (b0, kind, k) in enumerate(T.dofs):
        side = []
        for e in (h, -h):
            loc = list(loc0)
            loc[b0] = T.local(b0, _moved(T, x0[b0], b0, kind, k, e))
            side.append(T.forward(loc, R, p, b0))
        (Ra, pa), (Rb, pb) = side
        dP.append({b: (_sc(1 / (2 * h), _sub(pa[b], pb[b])), _msc(1 / (2 * h), _msub(Ra[b], Rb[b]))) for b in range(b0, T.last[b0] + 1)})
    Jw = [{j: _vee(_mmt(dP[j][b][1], R[b])) for j in T.sup[b]} for b in range(nb)]  # angular Jacobian of body b, world axes

    def point(b, x):
        """Jacobian of a point of body b (offset x in its axes), linear, world axes: values and scales per supporting dof."""
        ax = _vabs(x)
        val = {j: _add(dP[j][b][0], _mv(dP[j][b][1], x)) for j in T.sup[b]}
        scl = {j: column_scale(j, b, ax)[0] for j in T.sup[b]}
        return val, scl

    SJw = [{j: column_scale(j, b, _zero3())[1] for j in T.sup[b]} for b in range(nb)]
    Jc, SJc = zip(*[point(b, T.c[b]) for b in range(nb)])
    Iw = [_mm(R[b], _mmt(T.I[b], R[b])) for b in range(nb)]
    SIw = [_mm(SR[b], _mmt(_mabs(T.I[b]), SR[b])) for b in range(nb)]
    cw = [_add(_mv(R[b], T.c[b]), p[b]) for b in range(nb)]
    Scw = [_add(_mv(SR[b], _vabs(T.c[b])), Sp[b]) for b in range(nb)]
    mtot = sum(T.mass)
    com = _sc(1 / mtot, functools.reduce(_add, [_sc(T.mass[b], cw[b]) for b in range(nb)]))
    Scom = _sc(1 / mtot, functools.reduce(_add, [_sc(T.mass[b], Scw[b]) for b in range(nb)]))

    out: Dict[str, np.ndarray] = {}

    def put(name, val, scale, total=None):
        (val, lo), scale = _hi_lo(val), _hi_lo(scale)[0]
        if raw:
            out[name + ".lo"] = lo
        big = scale.max() if scale.size else 0.0
        structural = scale < ZERO_REL * big
        # (a numerical derivative of an exact zero is the differences' own rounding, not 0)
        assert (np.abs(val[structural]) <= 1e-30 * max(big, 1.0)).all(), (name, "a structural zero has a value")
        out[name], out[name + ".scale"] = np.where(structural, 0.0, val), np.where(structural, 0.0, scale)
        if total is not None:
            out[name + ".scale_total"] = _hi_lo(total)[0]

    keep = {}

    # ---- M from the kinetic energy ----------------------------------------------------------------------------------------------------------
    Mv = [[zero] * nv for _ in range(nv)]
    Ms = [[zero] * nv for _ in range(nv)]
    for b in range(nb):
        IJ = {j: _mv(Iw[b], Jw[b][j]) for j in T.sup[b]}
        SIJ = {j: _mv(SIw[b], SJw[b][j]) for j in T.sup[b]}
        mb = T.mass[b]
        for i in T.sup[b]:
            for j in T.sup[b]:
                Mv[i][j] += mb * _dot(Jc[b][i], Jc[b][j]) + _dot(Jw[b][i], IJ[j])
                Ms[i][j] += mb * _dot(SJc[b][i], SJc[b][j]) + _dot(SJw[b][i], SIJ[j])
    # scale_total: the dofs' motion subspaces about the common origin, and the bodies' inertias about it
    common = list(p[0]) if T.fb else _zero3()
    S6 = []
    for j, (b0, kind, k) in enumerate(T.dofs):
        S6.append(_vabs(_add(dP[j][b0][0], _cross(Jw[b0][j], _sub(common, p[b0])))) + _vabs(Jw[b0][j]))
    Y = [[zero] * 6 for _ in range(6)]
    rb = [_sub(cw[b], common) for b in range(nb)]
    for b in range(nb):
        r = _hat(rb[b])
        mr = _msc(T.mass[b], r)
        Io = _msub(Iw[b], _mm(mr, r))
        for i in range(3):
            Y[i][i] += T.mass[b]
            for k in range(3):
                Y[i][3 + k] += abs(mr[i][k])
                Y[3 + i][k] += abs(mr[i][k])
                Y[3 + i][3 + k] += abs(Io[i][k])
    YS = [[sum(Y[r_][c_] * S6[j][c_] for c_ in range(6)) for r_ in range(6)] for j in range(nv)]
    Mt = [[sum(S6[i][r_] * YS[j][r_] for r_ in range(6)) for j in range(nv)] for i in range(nv)]
    put("M", Mv, Ms, Mt)
    out["check.M_asymmetry"] = np.array(float(max(abs(Mv[i][j] - Mv[j][i]) / max(Ms[i][j], mp.mpf(10) ** -300) for i in range(nv) for j in range(nv))))
    keep["M"] = Mv
    if raw:
        out["_mp"] = keep
    if want_M_only:
        return out

    # ---- placements, Jacobians ---------------------------------------------------------------------------------------------------------------
    Rf = [_mm(R[T.fbody[f]], T.fR[f]) for f in range(nf)]
    pf = [_add(_mv(R[T.fbody[f]], T.fp[f]), p[T.fbody[f]]) for f in range(nf)]
    SRf = [_mm(SR[T.fbody[f]], _mabs(T.fR[f])) for f in range(nf)]
    Spf = [_add(_mv(SR[T.fbody[f]], _vabs(T.fp[f])), Sp[T.fbody[f]]) for f in range(nf)]
    put("placement", [[x for r in Rf[f] for x in r] + list(pf[f]) for f in range(nf)], [[x for r in SRf[f] for x in r] + list(Spf[f]) for f in range(nf)])
    put("com", com, Scom)
    Jf, SJf = zip(*[point(T.fbody[f], T.fp[f]) for f in range(nf)]) if nf else ((), ())
    Jval = {k: np.full((nf, 6, nv), zero, dtype=object) for k in ("J_world", "J_local", "J_lwa")}
    Jscl = {k: np.full((nf, 6, nv), zero, dtype=object) for k in Jval}
    Jloc_mp = [dict() for _ in range(nf)]  # frame -> dof -> (6 values, 6 scales), LOCAL: the wrenches' Jacobians
    for f in range(nf):
        b = T.fbody[f]
        for j in T.sup[b]:
            lin, ang, slin, sang = Jf[f][j], Jw[b][j], SJf[f][j], SJw[b][j]
            loc = _mtv(Rf[f], lin) + _mtv(Rf[f], ang)
            sloc = _mtv(SRf[f], slin) + _mtv(SRf[f], sang)
            Jloc_mp[f][j] = (loc, sloc)
            for name, val, scl in (("J_lwa", lin + ang, slin + sang), ("J_local", loc, sloc),
                                   ("J_world", _add(lin, _cross(pf[f], ang)) + ang, _add(slin, _cmag(Spf[f], sang)) + sang)):
                for i in range(6):
                    Jval[name][f, i, j], Jscl[name][f, i, j] = val[i], scl[i]
    for k in Jval:
        put(k, Jval[k], Jscl[k])
        keep[k] = Jval[k]
    if hessian_frames is not None:
        return _second_order(T, x0, loc0, vv, h, mp.mpf(step2), list(hessian_frames), Jscl, Sp, SZ, SRf, Spf, values)
    # Jcom, Ag
    Ag = [[zero] * nv for _ in range(6)]
    SAg = [[zero] * nv for _ in range(6)]
    arm = [_sub(cw[b], com) for b in range(nb)]
    Sarm = [_add(Scw[b], Scom) for b in range(nb)]
    for b in range(nb):
        mb = T.mass[b]
        for j in T.sup[b]:
            lin, slin = _sc(mb, Jc[b][j]), _sc(mb, SJc[b][j])
            ang = _add(_mv(Iw[b], Jw[b][j]), _cross(arm[b], lin))
            sang = _add(_mv(SIw[b], SJw[b][j]), _cmag(Sarm[b], slin))
            for i in range(3):
                Ag[i][j] += lin[i]
                SAg[i][j] += slin[i]
                Ag[3 + i][j] += ang[i]
                SAg[3 + i][j] += sang[i]
    put("Ag", Ag, SAg)
    put("Jcom", [[x / mtot for x in r] for r in Ag[:3]], [[x / mtot for x in r] for r in SAg[:3]])

    # ---- second derivatives along the curve --------------------------------------------------------------------------------------------------
    def along(acc):
        """Per body: (dp, ddp, dR, ddR, w, alpha) on the curve with velocity v and velocity derivative acc."""
        side = []
        for t in (h, -h):
            side.append(T.forward([T.local(b, _on_curve(T, x0[b], b, vv, acc, t)) for b in range(nb)]))
        (Ra, pa), (Rb, pb) = side
        res = []
        for b in range(nb):
            dp, ddp = _sc(1 / (2 * h), _sub(pa[b], pb[b])), _sc(1 / (h * h), _add(_sub(pa[b], _sc(2, p[b])), pb[b]))
            dR = _msc(1 / (2 * h), _msub(Ra[b], Rb[b]))
            ddR = _msc(1 / (h * h), _madd(_msub(Ra[b], _msc(2, R[b])), Rb[b]))
            # the tables' rotations are orthogonal to rounding only, so R_ddot R' has an antisymmetric part of 1e-16 of its own products even where
            # the structure says alpha = 0: those products' magnitudes are part of alpha's scale
            G = _mmt(_mabs(ddR), _mabs(R[b]))
            floor = [(G[2][1] + G[1][2]) / 2, (G[0][2] + G[2][0]) / 2, (G[1][0] + G[0][1]) / 2]
            res.append((dp, ddp, dR, ddR, _vee(_mmt(dR, R[b])), _vee(_mmt(ddR, R[b])), floor))
        return res

    # scales of a point's velocity and acceleration, and of a body's angular ones
    Sw_own = [functools.reduce(_add, [_sc(av[j], column_scale(j, b, _zero3())[1]) for j in T.own[b]], _zero3()) for b in range(nb)]
    Sw = [None] * nb
    for b in range(nb):
        Sw[b] = _add(Sw_own[b], Sw[T.parent[b]] if T.parent[b] >= 0 else _zero3())

    def rate_scales(b, slin, acc_abs):
        """(velocity, acceleration) scale of a point of body b from its columns' scales: sum_j S_j |a_j|, and pair by pair the magnitudes of
        w_j x (w_k x r), twice where dof j is of an ancestor of dof k's body (2 w x v for a translation k), once within one joint."""
        sv, sa = _zero3(), _zero3()
        for k in T.sup[b]:
            a_ = T.dofs[k][0]
            par = T.parent[a_]
            turn = _add(_sc(2, Sw[par]) if par >= 0 else _zero3(), Sw_own[a_])
            sv = _add(sv, _sc(av[k], slin[k]))
            sa = _add(sa, _add(_sc(acc_abs[k], slin[k]), _sc(av[k], _cmag(turn, slin[k]))))
        return sv, sa

    def alpha_scale(b, acc_abs, curve):
        sa = list(curve[b][6])
        for k in T.sup[b]:
            a_ = T.dofs[k][0]
            par = T.parent[a_]
            sk = SJw[b][k]
            turn = _sub(_add(Sw[par] if par >= 0 else _zero3(), Sw_own[a_]), _sc(av[k], sk))
            sa = _add(sa, _add(_sc(acc_abs[k], sk), _sc(av[k], _cmag(turn, sk))))
        return sa

    zeros = [zero] * nv
    free = along(zeros)  # a = 0
    # frames: velocity (LOCAL), drift (LOCAL, LOCAL_WORLD_ALIGNED)
    vel, svel, dl, sdl, dw, sdw = ([] for _ in range(6))
    for f in range(nf):
        b = T.fbody[f]
        dp, ddp, dR, ddR, w, al, _ = free[b]
        xd, xdd = _add(dp, _mv(dR, T.fp[f])), _add(ddp, _mv(ddR, T.fp[f]))
        sv, sa = rate_scales(b, SJf[f], zeros)
        sal = alpha_scale(b, zeros, free)
        vel.append(_mtv(Rf[f], xd) + _mtv(Rf[f], w))
        svel.append(_mtv(SRf[f], sv) + _mtv(SRf[f], Sw[b]))
        dl.append(_mtv(Rf[f], xdd) + _mtv(Rf[f], al))
        sdl.append(_mtv(SRf[f], sa) + _mtv(SRf[f], sal))
        dw.append(xdd + al)
        sdw.append(sa + sal)
    put("velocity", vel, svel)
    put("drift_local", dl, sdl)
    put("drift_lwa", dw, sdw)
    keep["drift_local"], keep["drift_lwa"], keep["sdrift_local"], keep["sdrift_lwa"] = dl, dw, sdl, sdw

    def bodies(curve, acc_abs, grav):
        """Per body: (m c_dot, its scale, momentum rate (force, moment about the body's CoM), their scales, w, I_w w and scales)."""
        res = []
        for b in range(nb):
            dp, ddp, dR, ddR, w, al, _ = curve[b]
            cd, cdd = _add(dp, _mv(dR, T.c[b])), _add(ddp, _mv(ddR, T.c[b]))
            sv, sa = rate_scales(b, SJc[b], acc_abs)
            sal = alpha_scale(b, acc_abs, curve)
            mb = T.mass[b]
            force, sforce = _sc(mb, _sub(cdd, grav)), _sc(mb, _add(sa, _vabs(grav)))
            Lw, SLw = _mv(Iw[b], w), _mv(SIw[b], Sw[b])
            mom = _add(_mv(Iw[b], al), _cross(w, Lw))
            smom = _add(_mv(SIw[b], sal), _cmag(Sw[b], SLw))
            res.append(dict(lin=_sc(mb, cd), slin=_sc(mb, sv), force=force, sforce=sforce, mom=mom, smom=smom, Lw=Lw, SLw=SLw))
        return res

    def centroidal(B, lin, slin, ang, sang):
        """Sum over the bodies of (lin, ang + arm x lin) and its scale."""
        tot, stot = [zero] * 6, [zero] * 6
        for b in range(nb):
            a_ = _add(B[b][ang], _cross(arm[b], B[b][lin]))
            sa_ = _add(B[b][sang], _cmag(Sarm[b], B[b][slin]))
            for i in range(3):
                tot[i] += B[b][lin][i]
                stot[i] += B[b][slin][i]
                tot[3 + i] += a_[i]
                stot[3 + i] += sa_[i]
        return tot, stot

    nog = bodies(free, zeros, _zero3())
    Agv, SAgv = centroidal(nog, "lin", "slin", "Lw", "SLw")
    # scale_total of the momentum: the whole robot's momentum about the common origin, moved to the CoM
    tot_lin = functools.reduce(_add, [_vabs(B["lin"]) for B in nog])
    tot_ang = functools.reduce(_add, [_add(_vabs(B["Lw"]), _vabs(_cross(rb[b], B["lin"]))) for b, B in enumerate(nog)])
    put("Agv", Agv, SAgv, tot_lin + _add(tot_ang, _cmag(_vabs(_sub(com, common)), tot_lin)))
    # (Ag from the first derivatives) v against the bodies' momenta from the curve's differences, over the scale
    out["check.Agv_identity"] = np.array(float(max(abs(sum(Ag[i][j] * vv[j] for j in range(nv)) - Agv[i]) / SAgv[i] for i in range(6))))
    put("vcom", _sc(1 / mtot, Agv[:3]), _sc(1 / mtot, SAgv[:3]))
    dAgv, SdAgv = centroidal(nog, "force", "sforce", "mom", "smom")
    put("dAgv", dAgv, SdAgv)
    put("acom", _sc(1 / mtot, dAgv[:3]), _sc(1 / mtot, SdAgv[:3]))

    # ---- d'Alembert: nle, the inverse dynamics with a, and with wrenches -----------------------------------------------------------------------
    def forces(B, wr):
        tau, stau = [zero] * nv, [zero] * nv
        for b in range(nb):
            for j in T.sup[b]:
                tau[j] += _dot(Jc[b][j], B[b]["force"]) + _dot(Jw[b][j], B[b]["mom"])
                stau[j] += _dot(SJc[b][j], B[b]["sforce"]) + _dot(SJw[b][j], B[b]["smom"])
        # scale_total: the bodies' momentum rates about the common origin, all of them, against the dof's motion subspace
        tl = functools.reduce(_add, [B[b]["sforce"] for b in range(nb)])
        ta = functools.reduce(_add, [_add(B[b]["smom"], _cmag(_vabs(rb[b]), B[b]["sforce"])) for b in range(nb)])
        if wr is not None:
            for k, f in enumerate(wframes):
                wk = [_f(x) for x in wr[k]]
                awk = _vabs(wk)
                for j, (col, scol) in Jloc_mp[f].items():
                    tau[j] -= sum(col[i] * wk[i] for i in range(6))
                    stau[j] += sum(scol[i] * awk[i] for i in range(6))
                fw, mw = _mv(SRf[f], awk[:3]), _mv(SRf[f], awk[3:])
                tl = _add(tl, fw)
                ta = _add(ta, _add(mw, _cmag(_vabs(_sub(pf[f], common)), fw)))
        ttot = [sum(S6[j][i] * tl[i] + S6[j][3 + i] * ta[i] for i in range(3)) for j in range(nv)]
        return tau, stau, ttot

    nle = forces(bodies(free, zeros, g), None)
    keep["nle"], keep["v"] = nle[0], vv
    put("nle", *nle)
    driven = bodies(along(aa), ab, g)
    put("tau_a", *forces(driven, None))
    put("tau_aw", *forces(driven, np.asarray(wrench, dtype=np.float64)))
    return out


def _compose(A, B):
    """The placement A followed by B, each (R, p); None is the identity."""
    if A is None or B is None:
        return B if A is None else A
    return _mm(A[0], B[0]), _add(_mv(A[0], B[1]), A[1])


def _second_order(T, x0, loc0, vv, h, h2, frames, Jscl, Sp, SZ, SRf, Spf, values):
    """The second-order kinematics of the frames `frames` for one state, as arrays of mpmath numbers: H_<c> [F, 6, nv, nv] and dJ_<c> [F, 6, nv]
    (values: asked for), H_<c>.mag, the magnitude sums of H before the structural zeros are decided, and dJ_<c>.mag_world; c of CONVENTIONS.
    h is the step of the Jacobian's own difference, h2 the step of the difference of the Jacobian.  Jscl: the Jacobians' scales of the pass
    (the local ones, or those of a common origin)."""
    nv, nF, zero = T.nv, len(frames), mp.mpf(0)
    av = [abs(x) for x in vv]
    zeros = [zero] * nv
    out = {}
    for c in CONVENTIONS:
        out["H_%s.mag" % c] = np.full((nF, 6, nv, nv), zero, dtype=object)
        out["dJ_%s.mag_world" % c] = np.full((nF, 6, nv), zero, dtype=object)
        if values:
            out["H_" + c], out["dJ_" + c] = np.full((nF, 6, nv, nv), zero, dtype=object), np.full((nF, 6, nv), zero, dtype=object)

    def about_origin(k):
        """|S_k|: the magnitudes of dof k's world column about the world's origin, (linear, angular)."""
        a, kind, _ = T.dofs[k]
        return (SZ[k], _zero3()) if kind in ("fl", "p") else (_cmag(Sp[a], SZ[k]), SZ[k])

    def path_sum(body):
        """|V|(body) = sum over the chain to the body of |S_k| |v_k|."""
        lin, ang = _zero3(), _zero3()
        for k in T.sup[body]:
            sl, sw = about_origin(k)
            lin, ang = _add(lin, _sc(av[k], sl)), _add(ang, _sc(av[k], sw))
        return lin, ang

    for fi, f in enumerate(frames):
        b = T.fbody[f]
        dofs = T.sup[b]
        # ---- magnitudes: H from the two columns' scales, the motion cross product with every term of every component added ------------------
        cols = {c: {j: [Jscl["J_" + c][f, r, j] for r in range(6)] for j in dofs} for c in CONVENTIONS}
        for j in dofs:
            for k in dofs:
                for c in ("world", "local"):
                    cj, ck = cols[c][j], cols[c][k]
                    s = _add(_cmag(ck[3:], cj[:3]), _cmag(ck[:3], cj[3:])) + _cmag(ck[3:], cj[3:])
                    for r in range(6):
                        out["H_%s.mag" % c][fi, r, j, k] = s[r]
                # world axes at the frame's origin: l_j = w_j x (frame - joint j).  A dof k of j's body or above it turns the whole of it,
                # w_k x l_j; one under it moves the frame's origin alone, w_j x l_k; the angular rows are w_k x w_j either way, if anything
                cj, ck = cols["lwa"][j], cols["lwa"][k]
                s = (_cmag(ck[3:], cj[:3]) if T.dofs[k][0] <= T.dofs[j][0] else _cmag(cj[3:], ck[:3])) + _cmag(ck[3:], cj[3:])
                for r in range(6):
                    out["H_lwa.mag"][fi, r, j, k] = s[r]
        # ---- dJ as an algorithm about the world's origin sums it: (|V|(frame's body) + |V|(bodyof(j))) x_m |S_j|, moved to the frame -----------
        Vf = path_sum(b)
        for j in dofs:
            Vj = path_sum(T.dofs[j][0])
            Wl, Ww = _add(Vf[0], Vj[0]), _add(Vf[1], Vj[1])
            sl, sw = about_origin(j)
            Yl, Yw = _add(_cmag(Ww, sl), _cmag(Wl, sw)), _cmag(Ww, sw)
            at_frame = _add(Yl, _cmag(Yw, Spf[f]))
            for c, s in (("world", Yl + Yw), ("lwa", at_frame + Yw), ("local", _mtv(SRf[f], at_frame) + _mtv(SRf[f], Yw))):
                for r in range(6):
                    out["dJ_%s.mag_world" % c][fi, r, j] = s[r]
        if not values:
            continue
        # ---- values: differences of the frame's Jacobian, itself the difference of the placement map --------------------------------------------
        chain = []
        a = b
        while a >= 0:
            chain.append(a)
            a = T.parent[a]
        chain.reverse()
        d = len(chain)
        pos = {a: i for i, a in enumerate(chain)}
        seg = [[None] * (d + 1) for _ in range(d + 1)]  # seg[i][j]: the chain's bodies i .. j - 1 as they stand, composed
        for i in range(d):
            acc = None
            for i2 in range(i, d):
                acc = _compose(acc, loc0[chain[i2]])
                seg[i][i2 + 1] = acc

        def placed(mods):
            """The frame's body in the world with the local placements `mods` (place on the chain -> (R, p)) in place of those as they stand."""
            acc, at = None, 0
            for pz in sorted(mods):
                acc = _compose(_compose(acc, seg[at][pz]), mods[pz])
                at = pz + 1
            return _compose(acc, seg[at][d])

        plain = {}  # dof j moved alone, either way: its local placement, and that composed with the chain above it and with the chain under it

        def alone(j, e):
            if (j, e) not in plain:
                bj, kind, kk = T.dofs[j]
                L = T.local(bj, _moved(T, x0[bj], bj, kind, kk, e))
                plain[(j, e)] = (L, _compose(seg[0][pos[bj]], L), _compose(L, seg[pos[bj] + 1][d]))
            return plain[(j, e)]

        def columns(over, mods, centre, j, one=None):
            """Column j of the frame's Jacobian in the three conventions where the coordinates `over` (body -> coordinate; mods: their local
            placements) replace those of the state: the module's central difference of the placement map along dof j, formed there.
            one: where a single body is moved, its place on the chain and its local placement composed with the chain above and under it
            (the same products as placed(), the shared ones formed once)."""
            bj, kind, kk = T.dofs[j]
            side = []
            for e in (h, -h):
                if bj in over:
                    there = dict(mods)
                    there[pos[bj]] = T.local(bj, _moved(T, over[bj], bj, kind, kk, e))
                    side.append(placed(there))
                elif one is not None:
                    (pk, above, under), pj = one, pos[bj]
                    side.append(_compose(_compose(above, seg[pk + 1][pj]), alone(j, e)[2]) if pj > pk else
                                _compose(_compose(alone(j, e)[1], seg[pj + 1][pk]), under))
                else:
                    there = dict(mods)
                    there[pos[bj]] = alone(j, e)[0]
                    side.append(placed(there))
            (Ra, pa), (Rb, pb) = side
            Rc, pc = centre
            dp, dR = _sc(1 / (2 * h), _sub(pa, pb)), _msc(1 / (2 * h), _msub(Ra, Rb))
            lin, ang = _add(dp, _mv(dR, T.fp[f])), _vee(_mmt(dR, Rc))
            Rf, pf = _mm(Rc, T.fR[f]), _add(_mv(Rc, T.fp[f]), pc)
            return {"lwa": lin + ang, "local": _mtv(Rf, lin) + _mtv(Rf, ang), "world": _add(lin, _cross(pf, ang)) + ang}

        for k in dofs:
            bk, kind, kk = T.dofs[k]
            side = []
            for e in (h2, -h2):
                xk = _moved(T, x0[bk], bk, kind, kk, e)
                Lk, pk = T.local(bk, xk), pos[bk]
                over, mods = {bk: xk}, {pk: Lk}
                one = (pk, _compose(seg[0][pk], Lk), _compose(Lk, seg[pk + 1][d]))
                centre = _compose(one[1], seg[pk + 1][d])
                side.append({j: columns(over, mods, centre, j, one) for j in dofs})
            for j in dofs:
                for c in CONVENTIONS:
                    for r in range(6):
                        out["H_" + c][fi, r, j, k] = (side[0][j][c][r] - side[1][j][c][r]) / (2 * h2)
        side = []
        for t in (h2, -h2):
            over = {a: _on_curve(T, x0[a], a, vv, zeros, t) for a in chain}
            mods = {pos[a]: T.local(a, over[a]) for a in chain}
            centre = placed(mods)
            side.append({j: columns(over, mods, centre, j) for j in dofs})
        for j in dofs:
            for c in CONVENTIONS:
                for r in range(6):
                    out["dJ_" + c][fi, r, j] = (side[0][j][c][r] - side[1][j][c][r]) / (2 * h2)
    return out


def _orthogonal(R):
    """The orthogonal matrix nearest R (Newton's iteration for the polar factor)."""
    A = mp.matrix(R)
    for _ in range(10):
        A = (A + mp.inverse(A).T) / 2
    return [[A[i, j] for j in range(3)] for i in range(3)]


_TABLES: dict = {}


def _tables(m, exact_rotations=False):
    """The model's tables in mpmath, kept per CONTENT of the tables (a model changed in place gets its own)."""
    mp.mp.dps = DPS
    key = (bool(exact_rotations), bool(m.floating_base), tuple(m.gravity)) + tuple(
        np.ascontiguousarray(a).tobytes() for a in (m.parent, m.jtype, m.placement, m.inertia, m.frame_body, m.frame_placement))
    if key not in _TABLES:
        T = _Tables(m)
        if exact_rotations:
            T.Rp, T.fR = [_orthogonal(R) for R in T.Rp], [_orthogonal(R) for R in T.fR]
        _TABLES[key] = T
    return _TABLES[key]


def compute(name, step: str = STEP, raw: bool = False) -> Dict[str, np.ndarray]:
    """The statement of every state of a case, stacked; the inputs ride along.  raw: with what rounding left of every value (name + ".lo")."""
    m, s = model(name), states(name)
    per = [statement(m, s["q"][i], s["v"][i], s["a"][i], wrench_frames(name), s["wrench"][i], step, raw=raw) for i in range(s["q"].shape[0])]
    out = {k: np.stack([r[k] for r in per]) for k in per[0] if k != "_mp"}
    out.update({"in." + k: a for k, a in s.items()})
    out["in.wrench_frames"] = np.array(wrench_frames(name), dtype=np.int32)
    return out


@functools.lru_cache(maxsize=None)
def computed(name) -> Dict[str, np.ndarray]:
    """compute(name), once per process (the fixtures' test and the identities' test share it)."""
    return compute(name)


def _moves(a, b, quantities) -> float:
    worst = 0.0
    for k in quantities:
        s = a[k + ".scale"]
        with np.errstate(divide="ignore", invalid="ignore"):
            mv = np.where(s > 0, np.abs((a[k] - b[k]) + (a[k + ".lo"] - b[k + ".lo"])) / s, 0.0)
        worst = max(worst, float(mv.max()) if mv.size else 0.0)
    return worst


def check_steps(name) -> float:
    """Halving the step moves no value by more than 1e-25 of its scale; returns the largest move over scale."""
    worst = _moves(compute(name, STEP, raw=True), compute(name, "5e-21", raw=True), QUANTITIES)
    assert worst <= 1e-25, (name, worst)
    return worst


# ---- the second-order kinematics of a case: H = dJ/dq and dJ/dt ------------------------------------------------------------------------------
def second_order(m, q, v, frames, step: str = STEP, step2: str = STEP, **kw):
    """_second_order for one state (the statement's first part runs ahead of it: placements, scales, the Jacobians)."""
    return _statement(m, q, v, np.zeros(m.nv), [], None, step, hessian_frames=frames, step2=step2, **kw)


def _floats(a):
    return np.vectorize(float, otypes=[np.float64])(a)


def generic(name):
    """A second model and state for deciding the structural zeros: the case's tree with generic geometry, at a generic q and v.  Every frame is
    off its body's origin and every link off its parent's by a generic vector, every placement's rotation is off the table's by a generic one
    (exact_rotations takes the nearest orthogonal matrix).  What is zero there is zero because the Jacobian's entry does not depend on q_k; a
    frame ON its joint's origin, parallel axes, an axis through the base's origin give zeros of the values that no dependence explains."""
    m = copy.deepcopy(model(name))
    rng = np.random.default_rng(19_000 + list(CASES).index(name))
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    m.frame_placement[:, 9:] = rng.uniform(0.1, 0.4, (m.nframe, 3)) * sign((m.nframe, 3))
    m.placement[:, 9:] = rng.uniform(0.1, 0.4, (m.nbody, 3)) * sign((m.nbody, 3))
    m.frame_placement[:, :9] += rng.uniform(0.05, 0.2, (m.nframe, 9)) * sign((m.nframe, 9))
    m.placement[:, :9] += rng.uniform(0.05, 0.2, (m.nbody, 9)) * sign((m.nbody, 9))
    q = m.q0.copy()
    q[m.nq - m.na:] += rng.uniform(-1.0, 1.0, m.na)
    if m.floating_base:
        q[0:3] = rng.uniform(0.5, 1.5, 3)
        u = rng.standard_normal(4)
        q[3:7] = u / np.linalg.norm(u)
    return m, q, rng.uniform(0.5, 1.5, m.nv) * sign(m.nv)


@functools.lru_cache(maxsize=None)
def dependence(name) -> Dict[str, np.ndarray]:
    """H_<c> -> [frames, 6, nv, nv] bool: True where the Jacobian's entry (f, r, j) depends on q_k.  Decided from the values alone: False where
    the exact value is under ZERO_REL of its magnitude sum in every state of the case and in generic(name).  It is a statement about RIGID bodies,
    so the tables' rotations are orthogonalised (exact_rotations, as for the energy identity): with the tables' own, orthogonal to 1e-16, such an
    entry holds 1e-16 of its magnitude sum -- the relative placements between the two dofs do not quite drop out of R' R."""
    s, frames = states(name), hessian_frames(name)
    gm, gq, gv = generic(name)
    passes = [second_order(model(name), s["q"][i], s["v"][i], frames, exact_rotations=True) for i in range(s["q"].shape[0])]
    passes.append(second_order(gm, gq, gv, frames, exact_rotations=True))
    out = {}
    for k in HESSIANS:
        seen = [(_floats(abs(r[k])), _floats(r[k + ".mag"])) for r in passes]
        out[k] = np.any([(val > ZERO_REL * mag) & (mag > 0) for val, mag in seen], axis=0)
        for val, mag in seen:  # decided with room: nothing lies between 1e-35 of its magnitude sum and ZERO_REL of it
            assert not ((val > 1e-35 * mag) & (val <= ZERO_REL * mag)).any(), (name, k)
    return out


def compute_hessians(name, step: str = STEP, step2: str = STEP, raw: bool = False) -> Dict[str, np.ndarray]:
    """The six second-order quantities of every state of a case, stacked, each with `scale` and `scale_world`; in.hessian_frames beside them.
    raw: with what rounding left of every value (name + ".lo")."""
    m, s, frames = model(name), states(name), hessian_frames(name)
    n = s["q"].shape[0]
    per = [second_order(m, s["q"][i], s["v"][i], frames, step, step2) for i in range(n)]
    world = [second_order(m, s["q"][i], s["v"][i], frames, step, step2, origin="world", values=False) for i in range(n)]
    dep = dependence(name)
    out: Dict[str, np.ndarray] = {}

    def put(k, val, scale, scale_world, tiny):
        """Values outside the scale: zeros.  tiny: what the tables' rotations leave there, over the magnitude sum."""
        (hi, lo) = _hi_lo(val)
        with np.errstate(divide="ignore", invalid="ignore"):
            floor = 1e-30 * max(1.0, float(tiny.max()))  # (a difference of an exact zero is the differences' own rounding)
            assert (np.abs(hi[scale == 0.0]) <= 1e-14 * tiny[scale == 0.0] + floor).all(), (name, k, "a structural zero has a value")
            assert (np.abs(hi) <= scale * (1 + 1e-12))[scale > 0.0].all(), (name, k, "a value is larger than its magnitude sum")
        assert (scale_world >= scale).all() or k in RATES, (name, k)
        out[k], out[k + ".scale"], out[k + ".scale_world"] = np.where(scale > 0.0, hi, 0.0), scale, scale_world
        if raw:
            out[k + ".lo"] = np.where(scale > 0.0, lo, 0.0)

    av = np.abs(s["v"])
    for c in CONVENTIONS:
        H, dJ = "H_" + c, "dJ_" + c
        mag = np.stack([_floats(r[H + ".mag"]) for r in per])
        mag_world = np.stack([_floats(r[H + ".mag"]) for r in world])
        scale = np.where(dep[H][None], mag, 0.0)
        put(H, np.stack([r[H] for r in per]), scale, np.where(dep[H][None], mag_world, 0.0), mag_world)
        rate = np.zeros(scale.shape[:-1])
        for k in range(m.nv):  # (one dof after the other: the same sum on every machine)
            rate = rate + scale[..., k] * av[:, None, None, None, k]
        rate_world = np.stack([_floats(r[dJ + ".mag_world"]) for r in per])
        put(dJ, np.stack([r[dJ] for r in per]), rate, rate_world, rate_world)
    out["in.hessian_frames"] = np.array(frames, dtype=np.int32)
    return out


@functools.lru_cache(maxsize=None)
def computed_hessians(name) -> Dict[str, np.ndarray]:
    return compute_hessians(name)


def second_order_identities(name, i: int = 0) -> Dict[str, float]:
    """What ties the second-order quantities of state i to one another and to the first part of the statement, in mpmath, each as the largest
    |defect| over the magnitude sum of what it compares:
      * sum_k H[..., k] v_k = dJ in each convention (dJ is differenced along the curve, H along one dof at a time);
      * dJ_lwa v = drift_lwa, the frames' classical acceleration at a = 0 of the statement's first part;
      * dJ_local v + (w_f x l_f, 0) = drift_local, (l_f, w_f) = J_local v;
      * in WORLD, H[j][k] - H[k][j] = J_k x_m J_j where dof k's body is above dof j's, the bracket of the two columns from J_world; and TWICE
        that between two dofs of the free-flyer, each of which is <= the other (the base's own axes turn with it: d_k J_j = J_k x_m J_j both ways).
    The first two hold for the tables as they are.  The last two are identities of RIGID bodies (R' R_dot is a cross product only where R is
    orthogonal) and are formed with exact_rotations, as the energy identity is."""
    m, s, frames = model(name), states(name), hessian_frames(name)
    q, v = s["q"][i], s["v"][i]
    vv = [_f(x) for x in v]
    av = [abs(x) for x in vv]
    nv, zero = m.nv, mp.mpf(0)
    tiny = mp.mpf(10) ** -35  # (a difference of an exact zero is the differences' own rounding)
    first = {x: _statement(m, q, v, np.zeros(nv), [], None, raw=True, exact_rotations=x)["_mp"] for x in (False, True)}
    second = {x: second_order(m, q, v, frames, exact_rotations=x) for x in (False, True)}
    worst, dofs = {}, _tables(m).dofs

    def hold(what, defect, scale):
        assert scale > 0 or abs(defect) <= tiny, (name, what)
        worst[what] = max(worst.get(what, 0.0), float(abs(defect) / scale) if scale > 0 else 0.0)

    for fi, f in enumerate(frames):
        for c in CONVENTIONS:
            H, Hs, dJ = second[False]["H_" + c][fi], second[False]["H_%s.mag" % c][fi], second[False]["dJ_" + c][fi]
            for r in range(6):
                for j in range(nv):
                    hold("H v = dJ, " + c, sum((H[r, j, k] * vv[k] for k in range(nv)), zero) - dJ[r, j],
                         sum((Hs[r, j, k] * av[k] for k in range(nv)), zero))
        dJ = second[False]["dJ_lwa"][fi]
        for r in range(6):
            hold("dJ_lwa v = drift_lwa", sum((dJ[r, j] * vv[j] for j in range(nv)), zero) - first[False]["drift_lwa"][f][r],
                 first[False]["sdrift_lwa"][f][r])
        dJ, J = second[True]["dJ_local"][fi], first[True]["J_local"][f]
        vf = [sum((J[r, j] * vv[j] for j in range(nv)), zero) for r in range(6)]
        wl, swl = _cross(vf[3:], vf[:3]) + _zero3(), _cmag(_vabs(vf[3:]), _vabs(vf[:3])) + _zero3()
        for r in range(6):
            hold("dJ_local v + (w x l, 0) = drift_local", sum((dJ[r, j] * vv[j] for j in range(nv)), zero) + wl[r] - first[True]["drift_local"][f][r],
                 first[True]["sdrift_local"][f][r] + swl[r])
        H, Hs, J = second[True]["H_world"][fi], second[True]["H_world.mag"][fi], first[True]["J_world"][f]
        for j in range(nv):
            for k in range(j):
                ck, cj = list(J[:, k]), list(J[:, j])
                bracket = _add(_cross(ck[3:], cj[:3]), _cross(ck[:3], cj[3:])) + _cross(ck[3:], cj[3:])
                twice = dofs[k][0] == dofs[j][0]
                for r in range(6):
                    hold("H_world[j][k] - H_world[k][j] = %sJ_k x_m J_j" % ("2 " if twice else ""),
                         H[r, j, k] - H[r, k, j] - (2 if twice else 1) * bracket[r], Hs[r, j, k])
    return worst


def check_steps_hessians(name) -> float:
    """check_steps for the second-order quantities: either step halved, the Jacobian's own and that of the difference of the Jacobian."""
    a = compute_hessians(name, raw=True)
    worst = max(_moves(a, compute_hessians(name, "5e-21", STEP, raw=True), SECOND_ORDER),
                _moves(a, compute_hessians(name, STEP, "5e-21", raw=True), SECOND_ORDER))
    assert worst <= 1e-25, (name, worst)
    return worst


def energy_identity(name, i: int = 0, exact_rotations: bool = True) -> float:
    """|v' nle(q, v, g = 0) - v' M_dot v / 2| over sum |v_i| (scale of nle_i) for state i of a case, M_dot from differencing M along the curve that
    leaves q with the constant velocity v: the power of the forces that hold the accelerations at zero is the rate of the kinetic energy, + v' M_dot v / 2
    (M_dot - 2 C is skew).  It is an identity of RIGID bodies: with the tables' rotations as float64 holds them (orthogonal to 1e-16) it is met to about
    1e-22 only, with exact_rotations to the differences' own accuracy."""
    m, s = model(name), states(name)
    args = (m, s["q"][i], s["v"][i], s["a"][i], wrench_frames(name), s["wrench"][i])
    here = statement(*args, gravity=False, raw=True, exact_rotations=exact_rotations)
    h = mp.mpf(STEP)
    Ma, Mb = (statement(*args, want_M_only=True, shift=t, raw=True, exact_rotations=exact_rotations)["_mp"]["M"] for t in (h, -h))
    v, nle, nv = here["_mp"]["v"], here["_mp"]["nle"], m.nv
    power = sum(v[j] * nle[j] for j in range(nv))
    rate = sum(v[i_] * (Ma[i_][j] - Mb[i_][j]) / (2 * h) * v[j] for i_ in range(nv) for j in range(nv)) / 2
    scale = sum(abs(v[j]) * mp.mpf(float(here["nle.scale"][j])) for j in range(nv))
    return float(abs(power - rate) / scale)


def write(names: Optional[Sequence[str]] = None) -> None:
    os.makedirs(GOLDEN, exist_ok=True)
    for name in names or CASES:
        t0 = time.time()
        np.savez_compressed(path(name), **{k: a for k, a in compute(name).items() if k not in CHECKS})  # values and scales only
        print("%-28s %6.1f s  %8d bytes" % (name, time.time() - t0, os.path.getsize(path(name))))
        t0 = time.time()
        np.savez_compressed(hessians_path(name), **compute_hessians(name))
        print("%-28s %6.1f s  %8d bytes (second order)" % (name, time.time() - t0, os.path.getsize(hessians_path(name))))


if __name__ == "__main__":
    if "--write" in sys.argv:
        write([a for a in sys.argv[1:] if a in CASES] or None)
    else:
        print(__doc__)
