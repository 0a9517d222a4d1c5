"""The numpy statement of what wbcqp_jacobians computes on the device (include/wbcqp.h, csrc/wbcqp_jacobians.hpp): the Jacobians of chosen model
frames, the CoM Jacobian, the centroidal momentum matrix and their drift terms, for a batch of states -- what the reference's
RobotModel::update(..., update_jacobians = true) fills one robot at a time (src/utils/robot_model.cpp:92-98, 115-126 there).

Written in every BODY's own axes, unlike the kernel (one world frame): a frame's LOCAL column is the joint's motion subspace carried from the
joint's body to the frame by the relative placement of the two, and the other two conventions are made from it (LOCAL_WORLD_ALIGNED: turned by
R_f; WORLD: Ad(oMf)).  Column j of Ag is the momentum of the robot when dof j alone moves at unit speed -- observe.body_velocities on a unit
vector, summed over the bodies about the CoM -- and Jcom its linear rows over the total mass.  The drift terms come from
observe.body_bias_accelerations.  Host code for tests and tools: the hot path is the HIP kernel.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .model import J_FREEFLYER, J_PX, J_RX, J_RZ, Model
from .observe import body_bias_accelerations, body_velocities

WORLD, LOCAL, LOCAL_WORLD_ALIGNED = 0, 1, 2  # wbcqp_reference_frame: pinocchio's values
OUTPUTS = ("J", "Jcom", "Ag", "drift", "dAgv")


def _subspace(jt: int) -> np.ndarray:
    """The joint's motion subspace in its own axes, [6 (linear, angular), dofs of the joint]."""
    if jt == J_FREEFLYER:
        return np.eye(6)
    return np.eye(6)[:, [(3 + jt - J_RX) if jt <= J_RZ else (jt - J_PX)]]


def dof_bodies(model: Model) -> np.ndarray:
    """[nv] the body whose joint dof j belongs to."""
    out = np.zeros(model.nv, np.int64)
    for b in range(model.nbody):
        iv = model.idx_v(b)
        out[iv:iv + _subspace(int(model.jtype[b])).shape[1]] = b
    return out


def supports(model: Model) -> np.ndarray:
    """[nbody, nbody] bool: [a, b] is True where body a is b itself or one of its ancestors (a's joint moves b)."""
    nb = model.nbody
    out = np.zeros((nb, nb), bool)
    for b in range(nb):
        a = b
        while a >= 0:
            out[a, b] = True
            a = int(model.parent[a])
    return out


def _inertia3(Y: np.ndarray) -> np.ndarray:
    return np.array([[Y[4], Y[5], Y[6]], [Y[5], Y[7], Y[8]], [Y[6], Y[8], Y[9]]])


def frame_jacobian_local(model: Model, R: np.ndarray, p: np.ndarray, frame: int, sup: np.ndarray) -> np.ndarray:
    """[6, nv] the LOCAL Jacobian of model frame `frame` from the world placements (R, p) of `Model.body_placements`."""
    fb = int(model.frame_body[frame])
    Rp, pp = model.frame_placement[frame, :9].reshape(3, 3), model.frame_placement[frame, 9:]
    J = np.zeros((6, model.nv))
    for b in range(model.nbody):
        if not sup[b, fb]:
            continue
        # the frame seen from body b: b's axes -> the frame's body's axes -> the frame's
        Rrel = R[b].T @ R[fb] @ Rp
        prel = R[b].T @ (R[fb] @ pp + p[fb] - p[b])
        S = _subspace(int(model.jtype[b]))
        iv = model.idx_v(b)
        J[:3, iv:iv + S.shape[1]] = Rrel.T @ (S[:3] - np.cross(prel, S[3:], axis=0))
        J[3:, iv:iv + S.shape[1]] = Rrel.T @ S[3:]
    return J


def jacobians(model: Model, q: np.ndarray, v: Optional[np.ndarray] = None, frames: Sequence[int] = (), reference_frame: int = LOCAL,
              which: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """The outputs of wbcqp_jacobians named in `which` for the states q [B, nq], v [B, nv] and the frame indices `frames` (repeats allowed):
    J [B, n_frames, 6, nv] (rows: linear, angular; a floating base's six columns in the base's own axes), Jcom [B, 3, nv], Ag [B, 6, nv] (linear,
    then angular about the CoM, world axes), drift [B, n_frames, 6] (the frame's classical acceleration at zero joint accelerations, LOCAL or
    LOCAL_WORLD_ALIGNED axes) and dAgv [B, 6].  which None: J, Jcom, Ag and, with v, dAgv and (not WORLD) drift."""
    if reference_frame not in (WORLD, LOCAL, LOCAL_WORLD_ALIGNED):
        raise ValueError("unknown reference_frame %r" % (reference_frame,))
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B, nv, nb = q.shape[0], model.nv, model.nbody
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    nf = frames.size
    if which is None:
        which = ["J", "Jcom", "Ag"] + (["dAgv"] if v is not None else []) + (["drift"] if v is not None and reference_frame != WORLD else [])
    if ("drift" in which or "dAgv" in which) and v is None:
        raise ValueError("drift / dAgv need v")
    if "drift" in which and reference_frame == WORLD:
        raise ValueError("drift is LOCAL or LOCAL_WORLD_ALIGNED")
    if v is not None:
        v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    shape = {"J": (B, nf, 6, nv), "Jcom": (B, 3, nv), "Ag": (B, 6, nv), "drift": (B, nf, 6), "dAgv": (B, 6)}
    out = {k: np.zeros(shape[k]) for k in which}
    m, c = model.inertia[:, 0], model.inertia[:, 1:4]
    I3 = [_inertia3(model.inertia[i]) for i in range(nb)]
    sup = supports(model)
    fb = model.frame_body[frames]
    Rp = model.frame_placement[frames, :9].reshape(nf, 3, 3)
    pp = model.frame_placement[frames, 9:]
    for i in range(B):
        R, p = model.body_placements(q[i])
        Rf = np.einsum("fij,fjk->fik", R[fb], Rp)
        pf = np.einsum("fij,fj->fi", R[fb], pp) + p[fb]
        if "J" in out:
            for k, f in enumerate(frames):
                Jl = frame_jacobian_local(model, R, p, int(f), sup)
                if reference_frame != LOCAL:
                    lin, ang = Rf[k] @ Jl[:3], Rf[k] @ Jl[3:]
                    if reference_frame == WORLD:
                        lin = lin + np.cross(pf[k], ang, axis=0)
                    Jl = np.concatenate([lin, ang])
                out["J"][i, k] = Jl
        cw = np.einsum("bij,bj->bi", R, c) + p
        com = (m[:, None] * cw).sum(axis=0) / m.sum()
        if "Jcom" in out or "Ag" in out:
            Ag = np.zeros((6, nv))
            for j in range(nv):
                vl, w = body_velocities(model, R, p, np.eye(nv)[j])
                pv = m[:, None] * np.einsum("bij,bj->bi", R, vl + np.cross(w, c))  # the bodies' linear momenta, world axes
                Lw = np.stack([R[b] @ (I3[b] @ w[b]) for b in range(nb)])       # ... angular momenta about their own centres of mass
                Ag[:3, j] = pv.sum(axis=0)
                Ag[3:, j] = (Lw + np.cross(cw - com, pv)).sum(axis=0)
            if "Ag" in out:
                out["Ag"][i] = Ag
            if "Jcom" in out:
                out["Jcom"][i] = Ag[:3] / m.sum()
        if v is None or ("drift" not in out and "dAgv" not in out):
            continue
        vl, w = body_velocities(model, R, p, v[i])
        al, aw = body_bias_accelerations(model, R, p, vl, w, v[i])
        if "drift" in out:
            # the body's spatial acceleration carried to the frame, plus w x v there: the classical acceleration of the frame's origin
            vf = np.einsum("fji,fj->fi", Rp, vl[fb] + np.cross(w[fb], pp))
            wf = np.einsum("fji,fj->fi", Rp, w[fb])
            af = np.einsum("fji,fj->fi", Rp, al[fb] + np.cross(aw[fb], pp)) + np.cross(wf, vf)
            awf = np.einsum("fji,fj->fi", Rp, aw[fb])
            if reference_frame == LOCAL_WORLD_ALIGNED:
                af, awf = np.einsum("fij,fj->fi", Rf, af), np.einsum("fij,fj->fi", Rf, awf)
            out["drift"][i, :, :3], out["drift"][i, :, 3:] = af, awf
        if "dAgv" in out:
            # Newton-Euler of every body about the CoM: m a_c, and I alpha + w x I w turned into the world plus the arm's moment
            ac = np.einsum("bij,bj->bi", R, al + np.cross(aw, c) + np.cross(w, vl + np.cross(w, c)))
            f = m[:, None] * ac
            nw = np.stack([R[b] @ (I3[b] @ aw[b] + np.cross(w[b], I3[b] @ w[b])) for b in range(nb)])
            out["dAgv"][i, :3] = f.sum(axis=0)
            out["dAgv"][i, 3:] = (nw + np.cross(cw - com, f)).sum(axis=0)
    return out


def algorithmic_bytes(model: Model, n_frames: int = 0, which: Sequence[str] = OUTPUTS, itemsize: int = 8) -> int:
    """What one instance must move for the outputs named in `which`: q in (and v, where drift or dAgv is asked for), the outputs out."""
    nq, nv = model.nq, model.nv
    per = {"J": n_frames * 6 * nv, "Jcom": 3 * nv, "Ag": 6 * nv, "drift": n_frames * 6, "dAgv": 6}
    for k in which:
        if k not in per:
            raise ValueError(k)
    reads = nq + (nv if ("drift" in which or "dAgv" in which) else 0)
    return (reads + sum(per[k] for k in set(which))) * itemsize
