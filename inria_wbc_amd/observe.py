"""The numpy statement of what wbcqp_observe computes on the device (include/wbcqp.h, csrc/wbcqp_observe.hpp): centre of mass, its
velocity, and the world placement and local velocity of chosen model frames, for a batch of states.

Positions come from `Model.body_placements`; velocities from the recursion written here (a body's spatial velocity in its own axes:
v_i = X_i^-1 v_parent + S_i qdot_i).  Host code for tests, tools and initialisation: the hot path is the HIP kernel.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from .model import J_FREEFLYER, J_RZ, J_RX, J_PX, Model


def frame_ids(model: Model, names: Sequence[str]) -> np.ndarray:
    """Indices into the model's frame table for wbcqp_set_observed_frames, e.g. frame_ids(model, ["leg_left_6_joint", "gripper_right_joint"]).
    An unknown name raises KeyError, as the reference does (tasks.cpp:68-69)."""
    return np.array([model.frame(n) for n in names], dtype=np.int32)


def body_velocities(model: Model, R: np.ndarray, p: np.ndarray, v: np.ndarray):
    """Linear and angular velocity of every body's joint frame in the BODY's own axes, from the world placements (R, p) of
    `Model.body_placements` and the velocity vector v."""
    nb = model.nbody
    vl = np.zeros((nb, 3))
    w = np.zeros((nb, 3))
    for i in range(nb):
        jt, iv = int(model.jtype[i]), model.idx_v(i)
        if jt == J_FREEFLYER:
            vj, wj = v[iv:iv + 3], v[iv + 3:iv + 6]
        elif jt <= J_RZ:
            vj, wj = np.zeros(3), np.eye(3)[jt - J_RX] * v[iv]
        else:
            vj, wj = np.eye(3)[jt - J_PX] * v[iv], np.zeros(3)
        par = int(model.parent[i])
        if par >= 0:
            Rrel = R[par].T @ R[i]            # child axes -> parent axes
            prel = R[par].T @ (p[i] - p[par])  # child origin in the parent's axes
            vl[i] = Rrel.T @ (vl[par] + np.cross(w[par], prel)) + vj
            w[i] = Rrel.T @ w[par] + wj
        else:
            vl[i], w[i] = vj, wj
    return vl, w


def body_bias_accelerations(model: Model, R: np.ndarray, p: np.ndarray, vl: np.ndarray, w: np.ndarray, v: np.ndarray):
    """Spatial acceleration (linear, angular) of every body's joint frame in the BODY's own axes with zero joint accelerations and no gravity,
    from the placements and the velocities of `body_velocities`: a_i = X_i^-1 a_parent + v_i x S_i qdot_i (the motion cross product)."""
    nb = model.nbody
    al = np.zeros((nb, 3))
    aw = np.zeros((nb, 3))
    for i in range(nb):
        jt, iv = int(model.jtype[i]), model.idx_v(i)
        if jt == J_FREEFLYER:
            vj, wj = v[iv:iv + 3], v[iv + 3:iv + 6]
        elif jt <= J_RZ:
            vj, wj = np.zeros(3), np.eye(3)[jt - J_RX] * v[iv]
        else:
            vj, wj = np.eye(3)[jt - J_PX] * v[iv], np.zeros(3)
        # (v, w) x (vj, wj) = (w x vj + v x wj, w x wj)
        bl, bw = np.cross(w[i], vj) + np.cross(vl[i], wj), np.cross(w[i], wj)
        par = int(model.parent[i])
        if par >= 0:
            Rrel = R[par].T @ R[i]
            prel = R[par].T @ (p[i] - p[par])
            al[i] = Rrel.T @ (al[par] + np.cross(aw[par], prel)) + bl
            aw[i] = Rrel.T @ aw[par] + bw
        else:
            al[i], aw[i] = bl, bw
    return al, aw


def observe(model: Model, q: np.ndarray, v: Optional[np.ndarray] = None, frames: Sequence[int] = (), acom: bool = False) -> Dict[str, np.ndarray]:
    """dict(com [B, 3], placement [B, n_frames, 12]) and, with v, vcom [B, 3] and velocity [B, n_frames, 6]: the four outputs of
    wbcqp_observe for the states q [B, nq], v [B, nv] and the frame indices `frames` (repeats allowed).  placement: rotation row-major
    (9), translation (3); velocity: linear (3), angular (3) in the frame's own axes.  acom=True (needs v) adds acom [B, 3]: the CoM's
    acceleration with zero joint accelerations and no gravity, in the world's axes (tsid's data.acom[0], the drift of the CoM task)."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B = q.shape[0]
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    nf = frames.size
    m = model.inertia[:, 0]
    c = model.inertia[:, 1:4]
    out = {"com": np.zeros((B, 3)), "placement": np.zeros((B, nf, 12))}
    if v is not None:
        v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        out["vcom"] = np.zeros((B, 3))
        out["velocity"] = np.zeros((B, nf, 6))
        if acom:
            out["acom"] = np.zeros((B, 3))
    else:
        assert not acom, "acom needs v"
    fb = model.frame_body[frames]
    Rp = model.frame_placement[frames, :9].reshape(nf, 3, 3)
    pp = model.frame_placement[frames, 9:]
    for i in range(B):
        R, p = model.body_placements(q[i])
        cw = np.einsum("bij,bj->bi", R, c) + p
        out["com"][i] = (m[:, None] * cw).sum(axis=0) / m.sum()
        Rf = np.einsum("fij,fjk->fik", R[fb], Rp)
        out["placement"][i, :, :9] = Rf.reshape(nf, 9)
        out["placement"][i, :, 9:] = np.einsum("fij,fj->fi", R[fb], pp) + p[fb]
        if v is None:
            continue
        vl, w = body_velocities(model, R, p, v[i])
        # velocity of a body's centre of mass, in the world's axes
        vc = np.einsum("bij,bj->bi", R, vl + np.cross(w, c))
        out["vcom"][i] = (m[:, None] * vc).sum(axis=0) / m.sum()
        # the frame's velocity in its own axes: the body's, moved to the frame's origin and turned into the frame's axes
        out["velocity"][i, :, :3] = np.einsum("fji,fj->fi", Rp, vl[fb] + np.cross(w[fb], pp))
        out["velocity"][i, :, 3:] = np.einsum("fji,fj->fi", Rp, w[fb])
        if acom:
            # classical acceleration of a body's centre of mass: the spatial one moved to c, plus w x (velocity of c)
            al, aw = body_bias_accelerations(model, R, p, vl, w, v[i])
            ac = np.einsum("bij,bj->bi", R, al + np.cross(aw, c) + np.cross(w, vl + np.cross(w, c)))
            out["acom"][i] = (m[:, None] * ac).sum(axis=0) / m.sum()
    return out
