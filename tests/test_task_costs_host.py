"""Per-task costs on the host (no GPU): the numpy reference of inria_wbc_amd.costs against the oracle's solutions, and the C ABI's new
declarations (wbcqp_task_costs, wbcqp_rollout_traced, wbcqp_rollout_mixed_traced, wbcqp_trace)."""
import ctypes
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import capi, costs, structure, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(structure.STRUCTURES))
def test_costs_satisfy_the_objective_identity_on_every_stack(oracle_mod, name):
    st = structure.STRUCTURES[name]()
    rows = synth.generate(st, 12, 4242)
    o = oracle_mod.tick_batch(st, rows)
    c = costs.task_costs(st, rows, o["x"])
    assert c.shape == (12, st.n_tasks) and np.isfinite(c).all() and (c >= 0).all()
    obj = costs.objective_from_costs(st, rows, o["x"], c)
    scale = costs.identity_scale(st, rows)
    err = np.abs(obj - o["fval"]) / scale
    assert err.max() < 1e-9, (name, err.max(), o["status"])


@pytest.mark.parametrize("name", ["talos", "icub_single_support", "talos_torque_cop", "franka"])
def test_motion_task_costs_are_the_row_by_row_norm(oracle_mod, name):
    st = structure.STRUCTURES[name]()
    rows = synth.generate(st, 5, 777)
    x = oracle_mod.tick_batch(st, rows)["x"]
    c = costs.task_costs(st, rows, x)
    for i in range(5):
        dv = x[i, :st.nv]
        A = rows["A"][i].reshape(st.n_dense, st.nv)
        b1 = rows["b1"][i]
        for t in set(st.dense_row_task.tolist()) | set(st.sel_task.tolist()):
            r2 = 0.0
            for r in range(st.n_dense):
                if st.dense_row_task[r] == t:
                    r2 += (sum(A[r, j] * dv[j] for j in range(st.nv)) - b1[r]) ** 2
            for r in range(st.n_sel):
                if st.sel_task[r] == t:
                    r2 += (dv[st.sel_col[r]] - b1[st.n_dense + r]) ** 2
            assert abs(c[i, t] - np.sqrt(r2)) <= 1e-12 * max(1.0, np.sqrt(r2)), (name, i, t)


def test_torque_rows_use_the_decoded_tau(oracle_mod):
    st = structure.STRUCTURES["talos_torque"]()
    rows = synth.generate(st, 4, 99)
    o = oracle_mod.tick_batch(st, rows)
    tau = costs.decode_tau(st, rows, o["x"])
    assert np.allclose(tau, o["tau"], rtol=0, atol=1e-9 * max(1.0, np.abs(o["tau"]).max()))
    task, res = costs.task_rows(st, rows, o["x"])
    sel = task == st.acteq_task
    b = rows["b1"][:, sel]
    assert np.allclose(res[:, sel], st.acteq_scale[None, :] * o["tau"][:, st.acteq_joint] - b, rtol=0, atol=1e-8)


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    for sym in ("wbcqp_task_costs", "wbcqp_rollout_traced", "wbcqp_rollout_mixed_traced"):
        assert sym in declared and sym in capi.EXPORTS
        assert hasattr(capi.Handle, {"wbcqp_task_costs": "task_costs", "wbcqp_rollout_traced": "rollout_traced",
                                     "wbcqp_rollout_mixed_traced": "rollout_mixed_traced"}[sym])
    assert "} wbcqp_trace;" in hdr
    assert ctypes.sizeof(capi.CTrace) == 72
    assert [f for f, _ in capi.CTrace._fields_] == ["stride", "q", "v", "x", "tau", "status", "iters", "objective", "cost"]
