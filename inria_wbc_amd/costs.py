"""Per-task costs of a solved QP record, in numpy: the reference for wbcqp_task_costs and the cost field of the traced roll-outs.

cost[i][t] = || A_t x_i - b_t ||_2 over the level-1 rows of task t exactly as they enter H and g (include/wbcqp.h, "Per-task costs").  The
torque task's rows are formed from the record (M, h, Ac and the structure's force generators: tau = h_a + M_a dv - J_a' f, J = T' Ac), so
this does not depend on the tau a solver wrote.  For the dense and selection rows it is the reference's Controller::cost(task)
(controller.hpp:148-152)."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from .structure import Structure


def _sym(Mp: np.ndarray, nv: int) -> np.ndarray:
    """[B, nv(nv+1)/2] packed lower triangle -> [B, nv, nv]."""
    B = Mp.shape[0]
    M = np.zeros((B, nv, nv))
    il = np.tril_indices(nv)
    M[:, il[0], il[1]] = Mp
    M[:, il[1], il[0]] = Mp
    return M


def decode_tau(st: Structure, rows: Dict[str, np.ndarray], x: np.ndarray) -> np.ndarray:
    """tau = h_a + M_a dv - J_a' f of every instance (getActuatorForces, controller.cpp:250), [B, na]."""
    x = np.asarray(x, np.float64)
    B, nv, na, nu = x.shape[0], st.nv, st.na, st.nu
    M = _sym(np.asarray(rows["M"], np.float64).reshape(B, -1), nv)
    h = np.asarray(rows["h"], np.float64).reshape(B, nv)
    dv = x[:, :nv]
    tau = h[:, nu:] + np.einsum("bij,bj->bi", M[:, nu:, :], dv)
    if st.nc:
        Ac = np.asarray(rows["Ac"], np.float64).reshape(B, st.nc, 6, nv)
        T = st.force_gen()  # [nc][6][12]
        Jc = np.einsum("crm,bcrj->bcmj", T, Ac)  # [B][nc][12][nv]
        f = x[:, nv:nv + st.k].reshape(B, st.nc, 12)
        tau -= np.einsum("bcmj,bcm->bj", Jc[:, :, :, nu:], f)
    return tau


def task_rows(st: Structure, rows: Dict[str, np.ndarray], x: np.ndarray) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Per level-1 row r of every instance: (task index [r1], residual [B, r1]) -- the rows in b1's order."""
    x = np.asarray(x, np.float64)
    B, nv = x.shape[0], st.nv
    b1 = np.asarray(rows["b1"], np.float64).reshape(B, st.r1)
    dv, f = x[:, :nv], x[:, nv:nv + st.k]
    res, task = [], []
    if st.n_dense:
        A = np.asarray(rows["A"], np.float64).reshape(B, st.n_dense, nv)
        res.append(np.einsum("brj,bj->br", A, dv))
        task.append(st.dense_row_task)
    if st.n_sel:
        res.append(dv[:, st.sel_col])
        task.append(st.sel_task)
    if st.nc:
        F = st.forcereg_mat()  # [nc][6][12] diag(w_f) T
        res.append(np.einsum("crm,bcm->bcr", F, f.reshape(B, st.nc, 12)).reshape(B, 6 * st.nc))
        task.append(np.repeat(st.forcereg_task, 6))
    if st.n_acteq:
        tau = decode_tau(st, rows, x)
        res.append(st.acteq_scale[None, :] * tau[:, st.acteq_joint])
        task.append(np.full(st.n_acteq, st.acteq_task))
    if st.cop_task >= 0:
        Acop = np.asarray(rows["Acop"], np.float64).reshape(B, 3, st.k)
        res.append(np.einsum("brm,bm->br", Acop, f))
        task.append(np.full(3, st.cop_task))
    Ax = np.concatenate(res, axis=1) if res else np.zeros((B, 0))
    return np.concatenate(task).astype(np.int64) if task else np.zeros(0, np.int64), Ax - b1


def task_costs(st: Structure, rows: Dict[str, np.ndarray], x: np.ndarray, tau=None) -> np.ndarray:
    """[B, n_tasks] ||A_t x - b_t|| (tau is not read: the torque rows come from the record; the argument mirrors wbcqp_task_costs)."""
    task, r = task_rows(st, rows, x)
    B = r.shape[0]
    out = np.zeros((B, st.n_tasks))
    for t in range(st.n_tasks):
        out[:, t] = np.sqrt((r[:, task == t] ** 2).sum(axis=1))
    return out


def rhs_norms2(st: Structure, rows: Dict[str, np.ndarray]) -> np.ndarray:
    """[B, n_tasks] ||b_t||^2 with b_t the right-hand side as it enters g: b1, except on the torque task's rows, whose b is
    scale_j tau_ref_j - scale_j h_a(joint_j) (b1 holds scale_j tau_ref_j)."""
    h = np.asarray(rows["h"], np.float64).reshape(-1, st.nv)
    task, _ = task_rows(st, rows, np.zeros((h.shape[0], st.n)))
    b1 = np.asarray(rows["b1"], np.float64).reshape(-1, st.r1).copy()
    if st.n_acteq:
        o = st.n_dense + st.n_sel + 6 * st.nc
        b1[:, o:o + st.n_acteq] -= st.acteq_scale[None, :] * h[:, st.nu + st.acteq_joint]
    out = np.zeros((b1.shape[0], st.n_tasks))
    for t in range(st.n_tasks):
        out[:, t] = (b1[:, task == t] ** 2).sum(axis=1)
    return out


def objective_from_costs(st: Structure, rows: Dict[str, np.ndarray], x: np.ndarray, cost: np.ndarray) -> np.ndarray:
    """The identity between the costs and the QP's objective 1/2 x'Hx + g'x, H = sum w A'A + reg I, g = -sum w A'b:
    objective = 1/2 sum_t w_t (cost_t^2 - ||b_t||^2) + 1/2 hessian_reg ||x||^2, [B]."""
    x = np.asarray(x, np.float64)
    w = np.asarray(rows["w"], np.float64).reshape(x.shape[0], st.n_tasks)
    c = np.asarray(cost, np.float64)
    return 0.5 * (w * (c ** 2 - rhs_norms2(st, rows))).sum(axis=1) + 0.5 * st.hessian_reg * (x[:, :st.n] ** 2).sum(axis=1)


def identity_scale(st: Structure, rows: Dict[str, np.ndarray]) -> np.ndarray:
    """sum_t w_t ||b_t||^2 per instance (b_t as in rhs_norms2): what the identity's error is measured against."""
    w = np.asarray(rows["w"], np.float64).reshape(-1, st.n_tasks)
    return (w * rhs_norms2(st, rows)).sum(axis=1)
