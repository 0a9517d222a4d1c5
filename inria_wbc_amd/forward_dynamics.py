"""The numpy statement of what wbcqp_mass_matrix, wbcqp_forward_dynamics and wbcqp_spd_commands compute on the device (include/wbcqp.h,
csrc/wbcqp_fdyn.hpp):

    M(q);    (M(q) + diag(damping)) a = tau - nle(q, v) + sum_k J_k(q)' w_k;    the reference's compute_spd

the reference's RobotModel::inertia_matrix() and inria_wbc::robot_dart::compute_spd (include/inria_wbc/robot_dart/cmd.hpp:10-38 there).
The mass matrix is the composite-rigid-body algorithm in every BODY's own axes (Featherstone's form: composite inertias inward, then each
joint's force carried down to the root), independent of the oracle (oracle/rbd_oracle.c) and of the kernel, which works in one common
world-aligned frame at the base and folds every body's inertia into its parent's, last body first.  The bias is dynamics.inverse_dynamics
with a = 0; the solve is a plain Cholesky factorisation with LAPACK's potrf convention for a pivot that is not > 0.  Host code for tests and tools: the hot path is the HIP kernel.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from . import dynamics
from .model import J_FREEFLYER, J_PX, J_RX, J_RZ, Model


def _skew(c: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]])


def _inertia6(Y: np.ndarray) -> np.ndarray:
    """The spatial inertia Y = (m, c, I_c xx xy xz yy yz zz) about the joint frame's origin as a 6 x 6 on motion vectors (linear, angular)."""
    m, cx = Y[0], _skew(Y[1:4])
    Ic = np.array([[Y[4], Y[5], Y[6]], [Y[5], Y[7], Y[8]], [Y[6], Y[8], Y[9]]])
    out = np.zeros((6, 6))
    out[:3, :3] = m * np.eye(3)
    out[:3, 3:] = -m * cx
    out[3:, :3] = m * cx
    out[3:, 3:] = Ic + m * cx @ cx.T
    return out


def _subspace(jt: int) -> np.ndarray:
    """The joint's motion subspace in its own axes, [6, dofs of the joint]."""
    if jt == J_FREEFLYER:
        return np.eye(6)
    return np.eye(6)[:, [(3 + jt - J_RX) if jt <= J_RZ else (jt - J_PX)]]


def mass_matrix_one(model: Model, q: np.ndarray) -> np.ndarray:
    """M [nv, nv] for one state; a floating base's six rows and columns are in the base's own axes (pinocchio's convention)."""
    nb = model.nbody
    R, p = model.body_placements(q)
    Yc = [_inertia6(model.inertia[i]) for i in range(nb)]
    Xf = [None] * nb  # a force on body i, about its origin in its axes -> the same force about the parent's origin in the parent's axes
    for i in range(nb - 1, 0, -1):
        par = int(model.parent[i])
        Rrel, prel = R[par].T @ R[i], R[par].T @ (p[i] - p[par])
        X = np.zeros((6, 6))
        X[:3, :3] = X[3:, 3:] = Rrel
        X[3:, :3] = _skew(prel) @ Rrel
        Xf[i] = X
        Xinv = X.T  # a motion of the parent, in the child's axes about the child's origin: the transpose of the force transform
        Yc[par] = Yc[par] + Xinv.T @ Yc[i] @ Xinv
    M = np.zeros((model.nv, model.nv))
    for i in range(nb):
        S = _subspace(int(model.jtype[i]))
        iv = model.idx_v(i)
        F = Yc[i] @ S
        own = np.triu(S.T @ F)  # (a free-flyer's 6 x 6: the upper triangle, mirrored -- both triangles hold the same bits)
        M[iv:iv + S.shape[1], iv:iv + S.shape[1]] = own + np.triu(own, 1).T
        j = i
        while model.parent[j] >= 0:
            F = Xf[j] @ F
            j = int(model.parent[j])
            Sj = _subspace(int(model.jtype[j]))
            jv = model.idx_v(j)
            blk = Sj.T @ F
            M[jv:jv + Sj.shape[1], iv:iv + S.shape[1]] = blk
            M[iv:iv + S.shape[1], jv:jv + Sj.shape[1]] = blk.T
    return M


def mass_matrix(model: Model, q: np.ndarray) -> np.ndarray:
    """M [B, nv, nv], the output of wbcqp_mass_matrix: q [B, nq]."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    return np.stack([mass_matrix_one(model, q[i]) for i in range(q.shape[0])])


def cholesky_solve(A: np.ndarray, b: np.ndarray) -> Tuple[np.ndarray, int]:
    """(x, info) with A x = b by A = L L': info = 0, or k + 1 when the k-th pivot is not > 0 (then x is all NaN)."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        s = A[k:, k] - L[k:, :k] @ L[k, :k]
        if not s[0] > 0.0:
            return np.full(n, np.nan), k + 1
        L[k:, k] = s / np.sqrt(s[0])
        L[k, k] = np.sqrt(s[0])
    y = np.array(b, dtype=np.float64)
    for k in range(n):
        y[k] /= L[k, k]
        y[k + 1:] -= L[k + 1:, k] * y[k]
    for k in range(n - 1, -1, -1):
        y[k] /= L[k, k]
        y[:k] -= L[k, :k] * y[k]
    return y, 0


def forward_dynamics(model: Model, q: np.ndarray, v: Optional[np.ndarray] = None, tau: Optional[np.ndarray] = None, frames: Sequence[int] = (),
                     wrench: Optional[np.ndarray] = None, damping: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(a [B, nv], info [B]), the outputs of wbcqp_forward_dynamics: q [B, nq]; v [B, nv] or None (zero); tau [B, >= nv] or None (zero), its
    first nv columns are read; wrench [B, n_frames, 6] or None; damping [nv] or None."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B, nv = q.shape[0], model.nv
    tau = np.zeros((B, nv)) if tau is None else np.atleast_2d(np.asarray(tau, dtype=np.float64))[:, :nv]
    D = np.zeros(nv) if damping is None else np.asarray(damping, dtype=np.float64).reshape(nv)
    bias = dynamics.inverse_dynamics(model, q, v, None, frames, wrench)
    M = mass_matrix(model, q)
    a, info = np.zeros((B, nv)), np.zeros(B, np.int32)
    for i in range(B):
        a[i], info[i] = cholesky_solve(M[i] + np.diag(D), tau[i] - bias[i])
    return a, info


def spd_gains(dt: float) -> Tuple[np.float32, np.float32]:
    """(stiffness, damping) of the reference's compute_spd: computed in double, stored in a float (cmd.hpp:15-16)."""
    return np.float32(10000 / (dt * 1000)), np.float32(100 / (dt * 1000))


def spd_commands(model: Model, q: np.ndarray, v: Optional[np.ndarray], target: np.ndarray, dt: float, kp: Optional[float] = None,
                 kd: Optional[float] = None, frames: Sequence[int] = (), wrench: Optional[np.ndarray] = None) -> dict:
    """dict(commands [B, nv], qddot [B, nv], info [B]), the outputs of wbcqp_spd_commands: target [B, >= na], its first na columns are read;
    kp, kd None: spd_gains(dt).  A floating base's six dofs have no gains (the reference's floating_base = true)."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B, nv, na = q.shape[0], model.nv, model.na
    g = spd_gains(dt)
    kp, kd = float(g[0] if kp is None else kp), float(g[1] if kd is None else kd)
    v = np.zeros((B, nv)) if v is None else np.atleast_2d(np.asarray(v, dtype=np.float64))
    target = np.atleast_2d(np.asarray(target, dtype=np.float64))[:, :na]
    nbase = nv - na
    Kp, Kd = np.zeros(nv), np.zeros(nv)
    Kp[nbase:], Kd[nbase:] = kp, kd
    qa = np.zeros((B, nv))
    qa[:, nbase:] = q[:, model.nq - na:]
    tg = np.zeros((B, nv))
    tg[:, nbase:] = target
    p = -Kp * (qa + v * dt - tg)
    d = -Kd * v
    qddot, info = forward_dynamics(model, q, v, p + d, frames, wrench, Kd * dt)
    return {"commands": p + d - Kd * qddot * dt, "qddot": qddot, "info": info}


def algorithmic_bytes(model: Model, call: str = "forward_dynamics", n_frames: int = 0, itemsize: int = 8) -> int:
    """What one instance must move.  call: "mass_matrix" (q in, M out), "forward_dynamics" (q, v, tau and the wrenches in, a and info out) or
    "spd_commands" (q, v, target and the wrenches in, commands, qddot and info out)."""
    nq, nv, na = model.nq, model.nv, model.na
    if call == "mass_matrix":
        return (nq + nv * nv) * itemsize
    if call == "forward_dynamics":
        return (nq + 2 * nv + 6 * n_frames + nv) * itemsize + 4
    if call == "spd_commands":
        return (nq + nv + na + 6 * n_frames + 2 * nv) * itemsize + 4
    raise ValueError(call)
