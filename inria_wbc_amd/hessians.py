"""The numpy statement of what wbcqp_kinematic_hessians computes on the device (include/wbcqp.h, csrc/wbcqp_hessians.hpp): the kinematic Hessian
H = dJ/dq of chosen model frames and the Jacobian's time variation dJ = sum_k H[..., k] v_k, for a batch of states, in pinocchio's three
conventions -- what the reference's RobotModel::hessian(name, reference_frame) hands out one robot at a time (src/utils/robot_model.cpp:92-98,
128-135 there: computeJointKinematicHessians, getJointKinematicHessian).

Made from the columns J_j = (l_j, w_j) of jacobians.jacobians in the convention asked for, with masks over (j, k) and einsum; "k <= j" below
says that dof k's body is dof j's body or one of its ancestors (two dofs of a free-flyer are each <= the other), and x_m is the motion cross
product (l1, w1) x_m (l2, w2) = (w1 x l2 + l1 x w2, w1 x w2).  Where both j and k move the frame's body:

    WORLD                 k <= j: J_k x_m J_j                  otherwise: +0.0
    LOCAL                 k <= j: +0.0                         otherwise: J_j x_m J_k
    LOCAL_WORLD_ALIGNED   k <= j: (w_k x l_j, w_k x w_j)       otherwise: (w_j x l_k, +0.0)

and +0.0 everywhere else -- and for the free-flyer's TWINS, its translation and its rotation along one axis e of the base (dofs i and i + 3): both
columns are made of the one vector R e, whose product with itself is written as +0.0 like the diagonal's (WORLD: all six rows, either order;
LOCAL_WORLD_ALIGNED: the linear rows; the angular ones are a product with the translation's w = 0).  d/dq_k is the derivative along dof k in the tangent space, d/de at 0 of J(q (+) e e_k) with the SE(3) integration of
the library: tests/test_hessians_host.py holds the table to central differences of jacobians.py.  dJ is formed from partial sums of v_k J_k
along the chain, never from H.  Host code for tests and tools: the hot path is the HIP kernel.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from .jacobians import LOCAL, LOCAL_WORLD_ALIGNED, WORLD, dof_bodies, jacobians, supports
from .model import Model

OUTPUTS = ("H", "dJ")


class CHessianOutputs(ctypes.Structure):
    """wbcqp_hessian_outputs (include/wbcqp.h): one pointer per output, NULL where it is not asked for.  capi binds the entry points with it."""
    _fields_ = [(k, ctypes.c_void_p) for k in OUTPUTS]


def precedes(model: Model) -> np.ndarray:
    """[nv, nv] bool: [j, k] is True where k <= j -- dof k's body is dof j's body or one of its ancestors."""
    body = dof_bodies(model)
    return supports(model)[body[None, :], body[:, None]]


def moves(model: Model, frames: Sequence[int]) -> np.ndarray:
    """[n_frames, nv] bool: dof j moves the body of frame f."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    return supports(model)[dof_bodies(model)[None, :], model.frame_body[frames][:, None]]


def twins(model: Model) -> np.ndarray:
    """[nv, nv] bool: the free-flyer's translation and rotation along one axis of the base.  Two different dofs that are each <= the other are the
    free-flyer's (every other joint has one dof), v = (linear, angular): twins lie three apart."""
    pre, d = precedes(model), np.arange(model.nv)
    return pre & pre.T & (np.abs(d[:, None] - d[None, :]) == 3)


def structure_masks(model: Model, frames: Sequence[int], reference_frame: int):
    """(lin, ang): [n_frames, nv, nv] bool, True where the table above has a cross product in H's linear and angular rows at (f, j, k); every
    other element of H is +0.0.  The diagonal k = j is +0.0 too wherever the product is of a vector with itself, and so are the twins."""
    mv, pre = moves(model, frames), precedes(model)
    both = mv[:, :, None] & mv[:, None, :]
    off = ~np.eye(model.nv, dtype=bool) & ~twins(model)
    if reference_frame == WORLD:
        lin = both & pre[None] & off[None]
        return lin, lin
    if reference_frame == LOCAL:
        lin = both & ~pre[None]
        return lin, lin
    return both & ~twins(model)[None], both & pre[None] & off[None]


def _cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a x b along axis -3 of [..., 3, j, k] operands (broadcast)."""
    return np.stack([a[..., 1, :, :] * b[..., 2, :, :] - a[..., 2, :, :] * b[..., 1, :, :],
                     a[..., 2, :, :] * b[..., 0, :, :] - a[..., 0, :, :] * b[..., 2, :, :],
                     a[..., 0, :, :] * b[..., 1, :, :] - a[..., 1, :, :] * b[..., 0, :, :]], axis=-3)


def hessians(model: Model, q: np.ndarray, v: Optional[np.ndarray] = None, frames: Sequence[int] = (), reference_frame: int = LOCAL,
             which: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """The outputs of wbcqp_kinematic_hessians named in `which` for the states q [B, nq], v [B, nv] and the frame indices `frames` (repeats
    allowed): H [B, n_frames, 6, nv, nv] (H[b, f, r, j, k] = d J[b, f, r, j] / d q_k) and dJ [B, n_frames, 6, nv] (needs v).  which None: H
    and, with v, dJ.  Refuses what the library refuses: no frames, nothing asked for, an unknown reference_frame, dJ without v."""
    if reference_frame not in (WORLD, LOCAL, LOCAL_WORLD_ALIGNED):
        raise ValueError("unknown reference_frame %r" % (reference_frame,))
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    if frames.size == 0:
        raise ValueError("no frames are selected")
    if which is None:
        which = ["H"] + (["dJ"] if v is not None else [])
    which = list(which)
    if not which or any(k not in OUTPUTS for k in which):
        raise ValueError("which: a non-empty choice of %r" % (OUTPUTS,))
    if "dJ" in which and v is None:
        raise ValueError("dJ needs v")
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    J = jacobians(model, q, None, frames, reference_frame, which=["J"])["J"]
    l, w = J[:, :, :3], J[:, :, 3:]  # [B, F, 3, nv]
    pre = precedes(model)
    out = {}
    if "H" in which:
        lin_mask, ang_mask = structure_masks(model, frames, reference_frame)
        lj, wj, lk, wk = l[..., :, None], w[..., :, None], l[..., None, :], w[..., None, :]  # [B, F, 3, j, k]: column j, column k
        if reference_frame == WORLD:
            lin, ang = _cross(wk, lj) + _cross(lk, wj), _cross(wk, wj)
        elif reference_frame == LOCAL:
            lin, ang = _cross(wj, lk) + _cross(lj, wk), _cross(wj, wk)
        else:
            lin, ang = np.where(pre[None, None, None], _cross(wk, lj), _cross(wj, lk)), _cross(wk, wj)
        out["H"] = np.concatenate([np.where(lin_mask[None, :, None], lin, 0.0), np.where(ang_mask[None, :, None], ang, 0.0)], axis=2)
    if "dJ" in which:
        v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        mv = moves(model, frames)
        # the chain's motion up to and with dof j's body, and what lies between that body and the frame (J is +0.0 off the chain)
        upto = np.einsum("jk,bfrk,bk->bfrj", pre.astype(np.float64), J, v)
        below = np.einsum("jk,bfrk,bk->bfrj", (~pre).astype(np.float64), J, v)
        c = lambda a, b: np.cross(a, b, axis=2)  # noqa: E731
        if reference_frame == WORLD:
            lin, ang = c(upto[:, :, 3:], l) + c(upto[:, :, :3], w), c(upto[:, :, 3:], w)
        elif reference_frame == LOCAL:
            lin, ang = c(w, below[:, :, :3]) + c(l, below[:, :, 3:]), c(w, below[:, :, 3:])
        else:
            lin, ang = c(upto[:, :, 3:], l) + c(w, below[:, :, :3]), c(upto[:, :, 3:], w)
        out["dJ"] = np.where(mv[None, :, None], np.concatenate([lin, ang], axis=2), 0.0)
    return out


def algorithmic_bytes(model: Model, n_frames: int, which: Sequence[str] = OUTPUTS, itemsize: int = 8) -> int:
    """What one instance must move for the outputs named in `which`: q in (and v, where dJ is asked for), the outputs out."""
    nq, nv = model.nq, model.nv
    per = {"H": n_frames * 6 * nv * nv, "dJ": n_frames * 6 * nv}
    for k in which:
        if k not in per:
            raise ValueError(k)
    return (nq + (nv if "dJ" in which else 0) + sum(per[k] for k in set(which))) * itemsize
