"""The numpy statement of what wbcqp_inverse_dynamics_derivatives computes on the device (include/wbcqp.h, csrc/wbcqp_idderiv.hpp): the
linearisation of the inverse dynamics

    tau = M(q) a + nle(q, v) - sum_k J_k(q)' w_k

in q and in v -- pinocchio's computeRNEADerivatives -- for a batch of states.  dtau_dq[i, j] is the derivative of tau_i along dof j in the
tangent space, d/de at e = 0 of tau(q (+) e e_j) with the SE(3) integration of the library (the convention of hessians.py); the wrenches act
at their frames, in each frame's own axes, and stay fixed in those axes.  dtau_dv[i, j] = d tau_i / d v_j.  d tau / d a is M.

A plain transcription about the TRUE world origin, world axes.  Motion vectors X = (l, w), forces F = (f, n), X . F = l . f + w . n,
    X x_m Y = (w_X x l_Y + l_X x w_Y, w_X x w_Y),     X x_f F = (w x f, w x n + l x f).
Per body b: the velocity V_b, the acceleration A_b (gravity as the root's acceleration: -g on its linear part), the inertia about the origin Y_b
as a 6 x 6 matrix, the momentum H_b = Y_b V_b = (hl, ha), the force f_b = Y_b A_b + V_b x_f H_b minus the wrenches on b, and
    N_b = V_b x_f Y_b - (Y_b V_b) x_m = [[0, -[hl]x], [[hl]x, D_b]],   D_b = [w]x I_o - I_o [w]x - [l]x [h]x - [h]x [l]x.
A composite X^c is the direct sum of X_b over the subtree of c (numpy's sum over the slice: no fold).  Per dof j with column S_j, body beta and
parent body lambda (at the root V = 0, A = (-g, 0)):
    U_j = S_j x_m V_lambda,   W_j = S_j x_m A_lambda - U_j x_m V_lambda,   Z_j = S_j x_m (V_lambda + V_beta).
For dofs i, j whose bodies lie on one path (two dofs of the free-flyer do), c the deeper of the two bodies:
    dtau_dq[i, j] = S_i . (-Y^c W_j - N^c U_j - U_j x_f H^c)  +  [body(i) a strict ancestor of beta]  S_i . (S_j x_f F^beta)
    dtau_dv[i, j] = S_i . ( N^c S_j + S_j x_f H^c - Y^c Z_j)
and +0.0 everywhere else.  tests/test_id_derivatives_host.py holds this to an 80-digit statement (tests/id_derivatives_exact.py) and to central
differences of the C oracle.  The kernel works about the floating base, folds its composites leaf to root and maps dofs to lanes: it differs
from this in origin, order and mapping.  Host code for tests and tools: the hot path is the HIP kernel.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from .jacobians import dof_bodies, supports
from .model import J_FREEFLYER, J_PX, J_RX, J_RZ, Model

OUTPUTS = ("dtau_dq", "dtau_dv")


class CIdDerivativeOutputs(ctypes.Structure):
    """wbcqp_id_derivative_outputs (include/wbcqp.h): one pointer per output, NULL where it is not asked for.  capi binds the entry points with it."""
    _fields_ = [(k, ctypes.c_void_p) for k in OUTPUTS]


def structure_mask(model: Model) -> np.ndarray:
    """[nv, nv] bool: True where the bodies of dofs i and j lie on one path from the root -- M's pattern.  Everything else is +0.0 in both
    matrices (and so are columns 0..2 of dtau_dq on a floating base, which this mask does not say)."""
    body, sup = dof_bodies(model), supports(model)
    on = sup[body[:, None], body[None, :]]
    return on | on.T


def _hat(x: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])


def _xm(X: np.ndarray, Y: np.ndarray) -> np.ndarray:
    """X x_m Y."""
    return np.concatenate([np.cross(X[3:], Y[:3]) + np.cross(X[:3], Y[3:]), np.cross(X[3:], Y[3:])])


def _xf(X: np.ndarray, F: np.ndarray) -> np.ndarray:
    """X x_f F."""
    return np.concatenate([np.cross(X[3:], F[:3]), np.cross(X[3:], F[3:]) + np.cross(X[:3], F[:3])])


def derivatives_one(model: Model, q: np.ndarray, v: np.ndarray, a: np.ndarray, frames: Sequence[int] = (), wrench: Optional[np.ndarray] = None):
    """(dtau_dq, dtau_dv), each [nv, nv], for one state."""
    nb, nv = model.nbody, model.nv
    R, p = model.body_placements(q)
    body, last, sup = dof_bodies(model), model.subtree_last(), supports(model)
    g = np.asarray(model.gravity, dtype=np.float64)
    # the dofs' columns about the world origin, world axes
    S = np.zeros((nv, 6))
    for b in range(nb):
        jt, iv = int(model.jtype[b]), model.idx_v(b)
        if jt == J_FREEFLYER:
            for k in range(3):
                S[iv + k, :3] = R[b][:, k]
                S[iv + 3 + k] = np.concatenate([np.cross(p[b], R[b][:, k]), R[b][:, k]])
        elif jt <= J_RZ:
            ax = R[b][:, jt - J_RX]
            S[iv] = np.concatenate([np.cross(p[b], ax), ax])
        else:
            S[iv, :3] = R[b][:, jt - J_PX]
    own = [np.flatnonzero(body == b) for b in range(nb)]
    # velocities and accelerations down the tree
    V, A = np.zeros((nb, 6)), np.zeros((nb, 6))
    root_A = np.concatenate([-g, np.zeros(3)])
    for b in range(nb):
        par = int(model.parent[b])
        Vj = S[own[b]].T @ v[own[b]]
        V[b] = (V[par] if par >= 0 else 0.0) + Vj
        A[b] = (A[par] if par >= 0 else root_A) + S[own[b]].T @ a[own[b]] + _xm(V[b], Vj)
    # per body: inertia about the origin, momentum, N, force
    Y, H, N, F = np.zeros((nb, 6, 6)), np.zeros((nb, 6)), np.zeros((nb, 6, 6)), np.zeros((nb, 6))
    for b in range(nb):
        Yb = model.inertia[b]
        m, c = Yb[0], R[b] @ Yb[1:4] + p[b]
        Ic = np.array([[Yb[4], Yb[5], Yb[6]], [Yb[5], Yb[7], Yb[8]], [Yb[6], Yb[8], Yb[9]]])
        ch = _hat(m * c)
        Io = R[b] @ Ic @ R[b].T - m * _hat(c) @ _hat(c)
        Y[b, :3, :3], Y[b, :3, 3:], Y[b, 3:, :3], Y[b, 3:, 3:] = m * np.eye(3), -ch, ch, Io
        H[b] = Y[b] @ V[b]
        lx, wx, hlx = _hat(V[b, :3]), _hat(V[b, 3:]), _hat(H[b, :3])
        N[b, :3, 3:], N[b, 3:, :3] = -hlx, hlx
        N[b, 3:, 3:] = wx @ Io - Io @ wx - lx @ ch - ch @ lx
        F[b] = Y[b] @ A[b] + _xf(V[b], H[b])
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    if frames.size:
        wrench = np.asarray(wrench, dtype=np.float64).reshape(frames.size, 6)
        for k, f in enumerate(frames):
            b = int(model.frame_body[f])
            Rf = R[b] @ model.frame_placement[f, :9].reshape(3, 3)
            pf = R[b] @ model.frame_placement[f, 9:] + p[b]
            fw = Rf @ wrench[k, :3]
            F[b] -= np.concatenate([fw, Rf @ wrench[k, 3:] + np.cross(pf, fw)])
    # composites: direct sums over each subtree
    sub = [slice(c, int(last[c]) + 1) for c in range(nb)]
    Yc = np.stack([Y[s].sum(axis=0) for s in sub])
    Hc = np.stack([H[s].sum(axis=0) for s in sub])
    Nc = np.stack([N[s].sum(axis=0) for s in sub])
    Fc = np.stack([F[s].sum(axis=0) for s in sub])
    # per dof
    zero6 = np.zeros(6)
    U, W, Z = np.zeros((nv, 6)), np.zeros((nv, 6)), np.zeros((nv, 6))
    for j in range(nv):
        par = int(model.parent[body[j]])
        Vl, Al = (V[par], A[par]) if par >= 0 else (zero6, root_A)
        U[j] = _xm(S[j], Vl)
        W[j] = _xm(S[j], Al) - _xm(U[j], Vl)
        Z[j] = _xm(S[j], Vl + V[body[j]])
    dq, dv = np.zeros((nv, nv)), np.zeros((nv, nv))
    for i in range(nv):
        for j in range(nv):
            bi, bj = int(body[i]), int(body[j])
            if not (sup[bi, bj] or sup[bj, bi]):
                continue
            c = max(bi, bj)  # (depth-first numbering: of two bodies on one path the deeper has the larger index)
            x = S[i] @ (-Yc[c] @ W[j] - Nc[c] @ U[j] - _xf(U[j], Hc[c]))
            if bi != bj and sup[bi, bj]:
                x += S[i] @ _xf(S[j], Fc[bj])
            dq[i, j] = x
            dv[i, j] = S[i] @ (Nc[c] @ S[j] + _xf(S[j], Hc[c]) - Yc[c] @ Z[j])
    if model.floating_base:
        dq[:, :3] = 0.0  # nothing depends on where the base is: written as zeros, as on the device
    return dq, dv


def derivatives(model: Model, q: np.ndarray, v: Optional[np.ndarray] = None, a: Optional[np.ndarray] = None, frames: Sequence[int] = (),
                wrench: Optional[np.ndarray] = None, which: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """The outputs of wbcqp_inverse_dynamics_derivatives named in `which`: q [B, nq]; v [B, nv] or None (zero); a [B, >= nv] or None (zero), its
    first nv columns are read; wrench [B, n_frames, 6] or None at the frame indices `frames`.  dtau_dq, dtau_dv [B, nv, nv].  which None:
    dtau_dq and, with v, dtau_dv.  Refuses what the library refuses: nothing asked for, dtau_dv without v."""
    if which is None:
        which = ["dtau_dq"] + (["dtau_dv"] if v is not None else [])
    which = list(which)
    if not which or any(k not in OUTPUTS for k in which):
        raise ValueError("which: a non-empty choice of %r" % (OUTPUTS,))
    if "dtau_dv" in which and v is None:
        raise ValueError("dtau_dv needs v")
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B, nv = q.shape[0], model.nv
    v = np.zeros((B, nv)) if v is None else np.atleast_2d(np.asarray(v, dtype=np.float64))
    a = np.zeros((B, nv)) if a is None else np.atleast_2d(np.asarray(a, dtype=np.float64))[:, :nv]
    if wrench is None:
        frames = ()
    else:
        wrench = np.asarray(wrench, dtype=np.float64).reshape(B, -1, 6)
    both = [derivatives_one(model, q[i], v[i], a[i], frames, None if wrench is None else wrench[i]) for i in range(B)]
    out = {"dtau_dq": np.stack([d[0] for d in both]), "dtau_dv": np.stack([d[1] for d in both])}
    return {k: out[k] for k in which}


def algorithmic_bytes(model: Model, n_frames: int = 0, which: Sequence[str] = OUTPUTS, itemsize: int = 8) -> int:
    """What one instance must move for the outputs named in `which`: q, v, a and the wrenches in, the matrices out."""
    for k in which:
        if k not in OUTPUTS:
            raise ValueError(k)
    return (model.nq + 2 * model.nv + 6 * n_frames + len(set(which)) * model.nv * model.nv) * itemsize
