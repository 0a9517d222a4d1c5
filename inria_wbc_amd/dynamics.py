"""The numpy statement of what wbcqp_inverse_dynamics computes on the device (include/wbcqp.h, csrc/wbcqp_rnea.hpp):

    tau = M(q) a + nle(q, v) - sum_k J_k(q)' w_k

the reference's RobotModel (src/utils/robot_model.cpp there: pinocchio::rnea, nonLinearEffects, computeGeneralizedGravity,
compute_rnea_double_support).  A plain recursive Newton-Euler pass over `Model` in every BODY's own axes (Featherstone's form: velocities and
accelerations outward, forces inward), with the wrenches entering as external forces on their frames' bodies -- which is -J' w for the LOCAL
frame Jacobian.  Independent of the oracle (oracle/rbd_oracle.c) and of the kernel, which works in one common world-aligned frame with prefix
sums.  Host code for tests and tools: the hot path is the HIP kernel.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .model import J_FREEFLYER, J_RZ, J_RX, J_PX, Model


def _joint_vectors(jt: int, x: np.ndarray):
    """(linear, angular) part of S x for a joint of type jt, in the joint's own axes; x: the joint's entries of v or a."""
    if jt == J_FREEFLYER:
        return x[0:3].copy(), x[3:6].copy()
    if jt <= J_RZ:
        return np.zeros(3), np.eye(3)[jt - J_RX] * x[0]
    return np.eye(3)[jt - J_PX] * x[0], np.zeros(3)


def _inertia_times(Y: np.ndarray, lin: np.ndarray, ang: np.ndarray):
    """The spatial inertia Y = (m, c, I_c xx xy xz yy yz zz) about the joint frame's origin, applied to a motion vector."""
    m, c = Y[0], Y[1:4]
    Ic = np.array([[Y[4], Y[5], Y[6]], [Y[5], Y[7], Y[8]], [Y[6], Y[8], Y[9]]])
    f = m * (lin + np.cross(ang, c))
    return f, Ic @ ang + np.cross(c, f)


def rnea_one(model: Model, q: np.ndarray, v: np.ndarray, a: np.ndarray, frames: Sequence[int] = (), wrench: Optional[np.ndarray] = None) -> np.ndarray:
    """tau [nv] for one state.  frames: indices into the model's frame table (repeats allowed); wrench [n_frames, 6]: linear (3), angular (3)
    in each frame's OWN axes."""
    nb = model.nbody
    R, p = model.body_placements(q)
    vl, w = np.zeros((nb, 3)), np.zeros((nb, 3))   # spatial velocity of every body, in its own axes
    al, aw = np.zeros((nb, 3)), np.zeros((nb, 3))  # spatial acceleration (gravity as the root's acceleration)
    fl, fa = np.zeros((nb, 3)), np.zeros((nb, 3))  # force on every body, about its joint frame's origin
    rel = [None] * nb
    g = np.asarray(model.gravity, dtype=np.float64)
    for i in range(nb):
        jt, iv = int(model.jtype[i]), model.idx_v(i)
        vj, wj = _joint_vectors(jt, v[iv:])
        aj, alj = _joint_vectors(jt, a[iv:])
        par = int(model.parent[i])
        if par >= 0:
            Rrel = R[par].T @ R[i]             # child axes -> parent axes
            prel = R[par].T @ (p[i] - p[par])  # child origin in the parent's axes
            rel[i] = (Rrel, prel)
            pv, pw = Rrel.T @ (vl[par] + np.cross(w[par], prel)), Rrel.T @ w[par]
            pa, pal = Rrel.T @ (al[par] + np.cross(aw[par], prel)), Rrel.T @ aw[par]
        else:
            pv, pw = np.zeros(3), np.zeros(3)
            pa, pal = R[i].T @ (-g), np.zeros(3)
        vl[i], w[i] = pv + vj, pw + wj
        # a_i = X a_parent + S a_j + v_i x S v_j  (motion cross product)
        al[i] = pa + aj + np.cross(w[i], vj) + np.cross(vl[i], wj)
        aw[i] = pal + alj + np.cross(w[i], wj)
        hl, ha = _inertia_times(model.inertia[i], vl[i], w[i])
        fl[i], fa[i] = _inertia_times(model.inertia[i], al[i], aw[i])
        fl[i] += np.cross(w[i], hl)
        fa[i] += np.cross(w[i], ha) + np.cross(vl[i], hl)
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    if frames.size:
        wrench = np.asarray(wrench, dtype=np.float64).reshape(frames.size, 6)
        for k, f in enumerate(frames):
            b = int(model.frame_body[f])
            Rp, pp = model.frame_placement[f, :9].reshape(3, 3), model.frame_placement[f, 9:]
            F = Rp @ wrench[k, :3]
            fl[b] -= F
            fa[b] -= Rp @ wrench[k, 3:] + np.cross(pp, F)
    tau = np.zeros(model.nv)
    for i in range(nb - 1, -1, -1):
        jt, iv = int(model.jtype[i]), model.idx_v(i)
        if jt == J_FREEFLYER:
            tau[iv:iv + 3], tau[iv + 3:iv + 6] = fl[i], fa[i]
        elif jt <= J_RZ:
            tau[iv] = fa[i][jt - J_RX]
        else:
            tau[iv] = fl[i][jt - J_PX]
        par = int(model.parent[i])
        if par >= 0:
            Rrel, prel = rel[i]
            F = Rrel @ fl[i]
            fl[par] += F
            fa[par] += Rrel @ fa[i] + np.cross(prel, F)
    return tau


def inverse_dynamics(model: Model, q: np.ndarray, v: Optional[np.ndarray] = None, a: Optional[np.ndarray] = None, frames: Sequence[int] = (),
                     wrench: Optional[np.ndarray] = None) -> np.ndarray:
    """tau [B, nv], the output of wbcqp_inverse_dynamics: q [B, nq]; v [B, nv] or None (zero); a [B, >= nv] or None (zero), its first nv columns are
    read; wrench [B, n_frames, 6] or None.  v = a = None: generalized gravity; a = None: the non-linear effects."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B, nv = q.shape[0], model.nv
    v = np.zeros((B, nv)) if v is None else np.atleast_2d(np.asarray(v, dtype=np.float64))
    a = np.zeros((B, nv)) if a is None else np.atleast_2d(np.asarray(a, dtype=np.float64))[:, :nv]
    if wrench is None:
        frames = ()
    else:
        wrench = np.asarray(wrench, dtype=np.float64).reshape(B, -1, 6)
    return np.stack([rnea_one(model, q[i], v[i], a[i], frames, None if wrench is None else wrench[i]) for i in range(B)])


def algorithmic_bytes(model: Model, n_frames: int = 0, itemsize: int = 8) -> int:
    """What one instance must move: q, v, a and the wrenches in, tau out."""
    return (model.nq + 2 * model.nv + 6 * n_frames + model.nv) * itemsize
