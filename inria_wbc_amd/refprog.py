"""Reference programs (wbcqp_program, include/wbcqp.h): a behaviour's reference streams as data, expanded on the device by refgen_kernel.

`Program` builds one; `expand` is the numpy reference of the expansion, built on trajs.py (the closed forms of
/root/reference/include/inria_wbc/trajs/trajectory_generator.hpp:23-156); `move_com_program`, `cartesian_program` and `walk_on_spot_program`
are the streams of trajs.move_com_stream, trajs.cartesian_stream and model.WalkOnSpotPlan as programs.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import trajs

TRACK_VEC, TRACK_SE3 = 0, 1
POSE_ONLY, RELATIVE = 1, 2
MAX_TRACKS = 16


@dataclass
class Segment:
    n_steps: int
    T: float
    x0: np.ndarray                      # [3] (a VEC track of dim 1 uses entry 0)
    xf: np.ndarray
    R0: np.ndarray = field(default_factory=lambda: np.eye(3))
    axis: np.ndarray = field(default_factory=lambda: np.array([1.0, 0.0, 0.0]))
    angle: float = 0.0


@dataclass
class Track:
    kind: int
    dim: int
    flags: int
    dst: Tuple[int, int]                # (offset, second offset or -1)
    segments: List[Segment]

    @property
    def ncomp(self) -> int:
        return 24 if self.kind == TRACK_SE3 else (9 if self.dim == 3 else 1)


def _dst(dst) -> Tuple[int, int]:
    d = [int(x) for x in np.atleast_1d(dst)]
    assert 1 <= len(d) <= 2, dst
    return (d[0], d[1] if len(d) == 2 else -1)


class Program:
    """One behaviour timeline: n_intro ticks played once, then n_cycle ticks repeated (0: hold the last sample).  A move is given by its ends and its
    duration T; it lasts floor(T / dt) ticks (trajectory_generator.hpp:73,152) unless n_steps is given."""

    def __init__(self, nref: int, dt: float, n_intro: int, n_cycle: int = 0, set_of: Optional[Sequence[int]] = None):
        self.nref, self.dt, self.n_intro, self.n_cycle = int(nref), float(dt), int(n_intro), int(n_cycle)
        self.set_of = None if set_of is None else np.ascontiguousarray(set_of, dtype=np.int32)
        self.tracks: List[Track] = []

    @property
    def length(self) -> int:
        return self.n_intro + self.n_cycle

    def steps(self, T: float) -> int:
        return int(np.floor(T / self.dt))

    def add_vec(self, dst, moves: Sequence[tuple], dim: int = 3, pose_only: bool = False, relative: bool = False) -> Track:
        """moves: (x0, xf, T) or (x0, xf, T, n_steps), consecutive; a hold has xf = x0."""
        segs = []
        for mv in moves:
            x0, xf = np.zeros(3), np.zeros(3)
            x0[:dim], xf[:dim] = np.asarray(mv[0], dtype=np.float64).reshape(-1)[:dim], np.asarray(mv[1], dtype=np.float64).reshape(-1)[:dim]
            T = float(mv[2])
            segs.append(Segment(int(mv[3]) if len(mv) > 3 else self.steps(T), T, x0, xf))
        t = Track(TRACK_VEC, int(dim), (POSE_ONLY if pose_only else 0) | (RELATIVE if relative else 0), _dst(dst), segs)
        self.tracks.append(t)
        return t

    def add_se3(self, dst, moves: Sequence[tuple], pose_only: bool = False, relative: bool = False) -> Track:
        """moves: (R0, p0, R1, p1, T) or (..., n_steps); axis and angle are those of R0' R1 (Eigen::AngleAxisd(Matrix3d), trajs._angle_axis)."""
        segs = []
        for mv in moves:
            R0, p0, R1, p1 = (np.asarray(a, dtype=np.float64) for a in mv[:4])
            T = float(mv[4])
            angle, axis = trajs._angle_axis(R0.T @ R1)
            segs.append(Segment(int(mv[5]) if len(mv) > 5 else self.steps(T), T, p0.copy(), p1.copy(), R0.copy(), np.asarray(axis, dtype=np.float64), float(angle)))
        t = Track(TRACK_SE3, 3, (POSE_ONLY if pose_only else 0) | (RELATIVE if relative else 0), _dst(dst), segs)
        self.tracks.append(t)
        return t


def index(prog: Program, tau: np.ndarray) -> np.ndarray:
    """Behaviour tick tau (< 0: not started) -> sample of the timeline (model.WalkOnSpotPlan.index)."""
    tau = np.asarray(tau)
    n0, nc = prog.n_intro, prog.n_cycle
    if nc > 0:
        return np.where(tau < 0, 0, np.where(tau < n0, tau, n0 + (tau - n0) % nc))
    return np.clip(tau, 0, max(n0 - 1, 0))


def _vec_table(seg: Segment, dt: float, dim: int) -> np.ndarray:
    """[n_steps, 3 dim] pos | vel | acc of one segment (trajs.min_jerk_trajectory per order, for the segment's own n_steps)."""
    return np.stack([np.concatenate([trajs.minimum_jerk_polynom(seg.x0[:dim], seg.xf[:dim], dt * i, seg.T, order) for order in range(3)])
                     for i in range(seg.n_steps)])


def _se3_table(seg: Segment, dt: float):
    """(R [n,3,3], p [n,3], d1 [n,6], d2 [n,6]) of one segment: trajs.min_jerk_se3 with the segment's own axis, angle and n_steps."""
    n, axis, angle, R0 = seg.n_steps, seg.axis, seg.angle, seg.R0
    Rs, ps, d1, d2 = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 6))
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    for i in range(n):
        t = dt * i
        ps[i] = trajs.minimum_jerk_polynom(seg.x0, seg.xf, t, seg.T, 0)
        a = trajs.minimum_jerk_polynom([0.0], [angle], t, seg.T, 0)[0]
        Rs[i] = R0 @ (np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K))
        for order, out in ((1, d1), (2, d2)):
            out[i, :3] = trajs.minimum_jerk_polynom(seg.x0, seg.xf, t, seg.T, order)
            out[i, 3:] = R0 @ (trajs.minimum_jerk_polynom([0.0], [angle], t, seg.T, order)[0] * axis)
    return Rs, ps, d1, d2


def track_table(prog: Program, tr: Track):
    """The samples of a track over the whole timeline, before the RELATIVE origin: VEC [L, 3 dim]; SE3 (R [L,3,3], p [L,3], d1 [L,6], d2 [L,6])."""
    if tr.kind == TRACK_VEC:
        return np.concatenate([_vec_table(s, prog.dt, tr.dim) for s in tr.segments])
    parts = [_se3_table(s, prog.dt) for s in tr.segments]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def expand(prog: Program, base: np.ndarray, offsets: Sequence[int], tick0: int, n_ticks: int):
    """(ref [n_ticks][B][nref] float64, schedule [n_ticks][B] int32 or None without set_of): what wbcqp_reference_samples writes and the schedule
    wbcqp_rollout_mixed_program makes, for call ticks [0, n_ticks) of a call at tick0.  base: [B][nref] or [nref]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    B = offsets.size
    base = np.asarray(base, dtype=np.float64)
    base = np.broadcast_to(base, (B, prog.nref))
    tau = np.arange(tick0, tick0 + n_ticks, dtype=np.int64)[:, None] - offsets[None, :]
    idx = index(prog, tau)
    ref = np.broadcast_to(base[None], (n_ticks, B, prog.nref)).copy()
    for tr in prog.tracks:
        d0 = tr.dst[0]
        rel, pose = bool(tr.flags & RELATIVE), bool(tr.flags & POSE_ONLY)
        val = np.zeros((n_ticks, B, tr.ncomp))
        if tr.kind == TRACK_VEC:
            tab = track_table(prog, tr)[idx]
            dim = tr.dim
            val[..., :dim] = base[None, :, d0:d0 + dim] + tab[..., :dim] if rel else tab[..., :dim]
            if dim == 3 and not pose:
                val[..., 3:] = tab[..., 3:]
        else:
            Rs, ps, d1, d2 = (a[idx] for a in track_table(prog, tr))
            if rel:
                Rb = base[:, d0 + 3:d0 + 12].reshape(B, 3, 3).transpose(0, 2, 1)  # the row holds the rotation column-major
                ps = base[None, :, d0:d0 + 3] + ps
                Rs = np.einsum("bij,tbjk->tbik", Rb, Rs)
                d1 = np.concatenate([d1[..., :3], np.einsum("bij,tbj->tbi", Rb, d1[..., 3:])], axis=-1)
                d2 = np.concatenate([d2[..., :3], np.einsum("bij,tbj->tbi", Rb, d2[..., 3:])], axis=-1)
            val[..., :3] = ps
            val[..., 3:12] = np.swapaxes(Rs, -1, -2).reshape(n_ticks, B, 9)
            if not pose:
                val[..., 12:18], val[..., 18:24] = d1, d2
        for d in tr.dst:
            if d >= 0:
                ref[..., d:d + tr.ncomp] = val
    schedule = None if prog.set_of is None else prog.set_of[idx].astype(np.int32)
    return ref, schedule


# ---- ready-made programs ----------------------------------------------------------------------------------------------------------------------

def move_com_program(nref: int, dst: int, task_init, targets, mask: str, dt: float, duration: float, loop: bool = True, absolute: bool = False,
                     relative: bool = False) -> Program:
    """trajs.move_com_stream (behaviors::humanoid::MoveCom, move_com.cpp:22-60) as a program: one VEC track of dim 3 at the CoM task's reference.
    Looping, the stream repeats (n_intro = 0); otherwise its last sample is held.  relative: the moves are displacements from the CoM position each
    instance's base row holds (task_init is then the zero vector of `absolute: false`)."""
    task_init = np.zeros(3) if relative else np.asarray(task_init, dtype=np.float64)
    targets = [list(t) for t in targets]
    if loop:
        targets.append(list(task_init) if absolute else [0.0, 0.0, 0.0])
    moves, start = [], task_init.copy()
    for tgt in targets:
        end = task_init.copy()
        for j in range(3):
            if mask[j] == "1":
                end[j] = tgt[j] if absolute else tgt[j] + task_init[j]
        moves.append((start, end, duration))
        start = end
    n = len(moves) * int(np.floor(duration / dt))
    prog = Program(nref, dt, 0 if loop else n, n if loop else 0)
    prog.add_vec(dst, moves, dim=3, relative=relative)
    return prog


def cartesian_program(nref: int, dst, R_init: np.ndarray, p_init: np.ndarray, rel_pos, dt: float, duration: float, loop: bool = True, rel_rpy=None,
                      relative: bool = False) -> Program:
    """trajs.cartesian_stream (generic::cartesian, cartesian.cpp:28-61) as a program: one SE3 track, init -> target (-> init when looping).
    relative: R_init / p_init are taken per instance from the base row (pass the identity and zeros)."""
    R_init, p_init = np.asarray(R_init, dtype=np.float64), np.asarray(p_init, dtype=np.float64)
    Rf, pf = R_init.copy(), p_init + np.asarray(rel_pos, dtype=np.float64)
    if rel_rpy is not None and len(rel_rpy) == 3:
        r, pch, y = rel_rpy
        cz, sz, cy, sy, cx, sx = np.cos(y), np.sin(y), np.cos(pch), np.sin(pch), np.cos(r), np.sin(r)
        rot = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Rf = rot @ R_init
    moves = [(R_init, p_init, Rf, pf, duration)]
    if loop:
        moves.append((Rf, pf, R_init, p_init, duration))
    n = len(moves) * int(np.floor(duration / dt))
    prog = Program(nref, dt, 0 if loop else n, n if loop else 0)
    prog.add_se3(dst, moves, relative=relative)
    return prog


def walk_on_spot_program(plan) -> Program:
    """model.WalkOnSpotPlan as a program: INIT once, then the six phases of the cycle; the feet's streams (pose only) feed the feet's tasks and
    their contacts' references, the CoM's its task; set_of is the plan's.  The base row is plan.base."""
    prog = Program(plan.nref, plan.dt, plan.phase_len[0], plan.cycle, set_of=plan.set_of)
    for dst, R, moves in (((plan.lf_ref, plan.cl_ref), plan.Rl, plan.moves["lf"]), ((plan.rf_ref, plan.cr_ref), plan.Rr, plan.moves["rf"])):
        prog.add_se3(dst, [(R, a, R, b, T, n) for a, b, T, n in moves], pose_only=True)
    prog.add_vec(plan.com_ref, plan.moves["com"], dim=3, pose_only=True)
    return prog
