"""Per-task costs on the device (wbcqp_task_costs) and per-tick traces of roll-outs (wbcqp_rollout_traced, wbcqp_rollout_mixed_traced).

Yardsticks: the numpy costs of inria_wbc_amd.costs on the same record and x; the identity between the costs and the solver's own
objective; K calls of wbcqp_tick / wbcqp_tick_mixed, bit for bit, for every trace entry; the untraced roll-outs, bit for bit."""
import dataclasses

import numpy as np
import pytest

from inria_wbc_amd import capi, costs, structure, synth, trajs
from inria_wbc_amd import model as mdl
from tests.test_gpu_mixed_contacts import _fleet, _mixed_tick, _outputs, _set_weights, _walk_plan

pytestmark = pytest.mark.gpu
DT = 1e-3  # the Talos task map's dt


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _check_costs(st, rows_np, x, c_gpu, tol):
    """GPU costs against numpy on the same record and x, per task, with an absolute floor scaled by the task's right-hand side."""
    want = costs.task_costs(st, rows_np, x)
    floor = 10 * tol * (1.0 + np.sqrt(costs.rhs_norms2(st, rows_np)) + np.abs(want))
    err = np.abs(c_gpu - want)
    assert (err <= tol * np.abs(want) + floor).all(), (st.name, float((err / (np.abs(want) + 1e-300)).max()), np.argwhere(err > tol * np.abs(want) + floor)[:5])


@pytest.mark.parametrize("dtype", [capi.F64, capi.F32])
@pytest.mark.parametrize("name", sorted(structure.STRUCTURES))
def test_task_costs_of_solve_batch_records_match_numpy(name, dtype):
    torch, dev = _torch()
    st = structure.STRUCTURES[name]()
    B = 257
    npd, td = (np.float64, torch.float64) if dtype == capi.F64 else (np.float32, torch.float32)
    rows_np = synth.generate(st, B, 31_000, dtype=npd)
    L = st.field_lengths()
    rows = {k: torch.from_numpy(np.ascontiguousarray(rows_np[k])).to(dev) for k in capi.FIELDS if L[k] > 0}
    out = dict(x=torch.zeros(B, st.n, dtype=td, device=dev), tau=torch.zeros(B, max(st.na, 1), dtype=td, device=dev),
               status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev),
               objective=torch.zeros(B, dtype=td, device=dev))
    h = capi.Handle(0, dtype)
    try:
        h.set_structure(0, st)
        stream = torch.cuda.current_stream().cuda_stream
        h.solve_batch(0, B, rows, out, stream=stream)
        c1 = torch.full((B, st.n_tasks), float("nan"), dtype=td, device=dev)
        c2 = torch.full((B, st.n_tasks), float("nan"), dtype=td, device=dev)
        h.task_costs(0, B, rows, out["x"], out["tau"] if st.na else None, c1, stream=stream)
        h.task_costs(0, B, rows, out["x"], out["tau"] if st.na else None, c2, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(c1, c2)
        x = _np(out["x"])
        rec = {k: rows_np[k].astype(np.float64) for k in rows_np}
        _check_costs(st, rec, x, _np(c1), 1e-12 if dtype == capi.F64 else 1e-5)
        if dtype == capi.F64:
            obj = costs.objective_from_costs(st, rec, x, _np(c1))
            err = np.abs(obj - _np(out["objective"])) / costs.identity_scale(st, rec)
            assert err.max() < 1e-9, err.max()
    finally:
        h.close()


@pytest.mark.parametrize("robot", ["talos", "icub", "franka"])
def test_task_costs_of_tick_records_match_numpy(robot):
    torch, dev = _torch()
    m = {"talos": mdl.talos_like, "icub": mdl.icub_like, "franka": mdl.franka_like}[robot]()
    st = {"talos": structure.talos_structure, "icub": structure.icub_structure, "franka": structure.franka_structure}[robot]()
    tm = mdl.build_taskmap(m, st, {"talos": mdl.talos_stack, "icub": mdl.icub_stack, "franka": mdl.franka_stack}[robot]())
    B = 257
    s = mdl.sample_states(m, tm, B, 32_000, q_noise=0.005, v_noise=0.02, ref_noise=0.005)
    L = st.field_lengths()
    rows = {k: torch.zeros(B, max(L[k], 1), dtype=torch.float64, device=dev) for k in capi.ROW_FIELDS}
    if st.act_bounds:
        rows["tlb"] = torch.from_numpy(np.tile(-m.tau_max, (B, 1))).to(dev)
        rows["tub"] = torch.from_numpy(np.tile(m.tau_max, (B, 1))).to(dev)
    rows["w"] = torch.from_numpy(np.tile(st.default_weights, (B, 1))).to(dev)
    out = dict(x=torch.zeros(B, st.n, dtype=torch.float64, device=dev), tau=torch.zeros(B, max(st.na, 1), dtype=torch.float64, device=dev),
               status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev),
               objective=torch.zeros(B, dtype=torch.float64, device=dev))
    state = {k: torch.from_numpy(s[k]).to(dev) for k in ("q", "v", "ref")}
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        stream = torch.cuda.current_stream().cuda_stream
        h.tick(0, B, state, rows, out, torch.zeros_like(state["q"]), torch.zeros_like(state["v"]), tm.dt, stream=stream)
        c = torch.zeros(B, st.n_tasks, dtype=torch.float64, device=dev)
        h.task_costs(0, B, rows, out["x"], out["tau"], c, stream=stream)
        torch.cuda.synchronize()
        rec = {k: _np(v)[:, :L[k]] for k, v in rows.items()}
        x = _np(out["x"])
        _check_costs(st, rec, x, _np(c), 1e-12)
        err = np.abs(costs.objective_from_costs(st, rec, x, _np(c)) - _np(out["objective"])) / costs.identity_scale(st, rec)
        assert err.max() < 1e-9, err.max()
    finally:
        h.close()


# ---- the single-slot roll-out ------------------------------------------------------------------------------------------------------------

def _squat(st_override=None, B=512, K=24, seed=93_000):
    torch, dev = _torch()
    m = mdl.talos_like()
    st = st_override or structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    s = mdl.sample_states(m, tm, B, seed, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    com_blk = next(b for b in tm.blocks if b.kind == mdl.T_COM)
    pos, vel, acc = trajs.move_com_stream(m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0, loop=True, absolute=False)
    refs = np.repeat(s["ref"][None], K, axis=0).copy()
    for t in range(K):
        for i in range(B):
            k = (t + 37 * i) % len(pos)
            refs[t, i, com_blk.ref:com_blk.ref + 9] = np.concatenate([pos[k], vel[k], acc[k]])
    lim = dict(tlb=torch.from_numpy(np.tile(-m.tau_max, (B, 1))).to(dev), tub=torch.from_numpy(np.tile(m.tau_max, (B, 1))).to(dev),
               w=torch.from_numpy(np.tile(st.default_weights, (B, 1))).to(dev))
    return m, st, tm, s, refs, lim


def _outs(st, B, dev, torch):
    return dict(x=torch.full((B, st.n), float("nan"), dtype=torch.float64, device=dev),
                tau=torch.full((B, st.na), float("nan"), dtype=torch.float64, device=dev),
                status=torch.full((B,), -99, dtype=torch.int32, device=dev), iters=torch.full((B,), -1, dtype=torch.int32, device=dev),
                objective=torch.full((B,), float("nan"), dtype=torch.float64, device=dev))


def _trace_bufs(na, B, n_rec, nq, nv, dev, torch, ldx, ldc):
    """Every field of a trace, filled with NaN / -99 / -1 (what no roll-out writes)."""
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    return dict(q=f(n_rec, B, nq), v=f(n_rec, B, nv), x=f(n_rec, B, ldx), tau=f(n_rec, B, na),
                status=torch.full((n_rec, B), -99, dtype=torch.int32, device=dev), iters=torch.full((n_rec, B), -1, dtype=torch.int32, device=dev),
                objective=f(n_rec, B), cost=f(n_rec, B, ldc))


def _tick_loop(h, st, m, s, refs, lim, K, dev, torch):
    """K calls of wbcqp_tick, state fed back: per tick q_next, v_next, x, tau, status, iters, objective and the costs of its record."""
    B = s["q"].shape[0]
    L = st.field_lengths()
    rows = {k: torch.zeros(B, max(L[k], 1), dtype=torch.float64, device=dev) for k in capi.ROW_FIELDS}
    rows.update(lim)
    q, v = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    per = []
    for t in range(K):
        o = _outs(st, B, dev, torch)
        qn, vn = torch.zeros_like(q), torch.zeros_like(v)
        h.tick(0, B, dict(q=q, v=v, ref=torch.from_numpy(refs[t]).to(dev)), rows, o, qn, vn, DT, stream=stream)
        c = torch.zeros(B, st.n_tasks, dtype=torch.float64, device=dev)
        h.task_costs(0, B, rows, o["x"], o["tau"], c, stream=stream)
        torch.cuda.synchronize()
        per.append(dict(q=qn.clone(), v=vn.clone(), cost=c, **o))
        q, v = qn, vn
    return per


def _rollout(h, st, s, refs, lim, K, dev, torch, trace=None, stride=1, traced=True):
    B = s["q"].shape[0]
    o = _outs(st, B, dev, torch)
    qn, vn = torch.zeros(B, s["q"].shape[1], dtype=torch.float64, device=dev), torch.zeros(B, s["v"].shape[1], dtype=torch.float64, device=dev)
    isum, tok = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    state = dict(q=torch.from_numpy(s["q"]).to(dev), v=torch.from_numpy(s["v"]).to(dev), ref=torch.from_numpy(np.ascontiguousarray(refs[:K])).to(dev))
    stream = torch.cuda.current_stream().cuda_stream
    if traced:
        h.rollout_traced(0, B, K, state, lim, o, qn, vn, DT, trace=trace, stride=stride, iters_sum=isum, ticks_ok=tok, stream=stream)
    else:
        h.rollout(0, B, K, state, lim, o, qn, vn, DT, iters_sum=isum, ticks_ok=tok, stream=stream)
    torch.cuda.synchronize()
    return dict(o, q_next=qn, v_next=vn, iters_sum=isum, ticks_ok=tok)


def _same(a, b, what):
    for k in a:
        assert torch_equal(a[k], b[k]), (what, k)


def torch_equal(a, b):
    x, y = a.cpu().numpy(), b.cpu().numpy()
    return x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")


def _check_trace(tr, per, stride, K):
    for r in range(K // stride):
        p = per[(r + 1) * stride - 1]
        for f, g in (("q", "q"), ("v", "v"), ("x", "x"), ("tau", "tau"), ("status", "status"), ("iters", "iters"), ("objective", "objective"),
                     ("cost", "cost")):
            assert torch_equal(tr[f][r], p[g]), ("trace entry", r, f)


@pytest.mark.parametrize("streams", ["1", "2"])
def test_rollout_traced_equals_the_tick_loop_bit_for_bit(streams, monkeypatch):
    torch, dev = _torch()
    monkeypatch.setenv("WBCQP_ROLLOUT_STREAMS", streams)
    m, st, tm, s, refs, lim = _squat()
    B, K = 512, 24
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        per = _tick_loop(h, st, m, s, refs, lim, K, dev, torch)
        plain = _rollout(h, st, s, refs, lim, K, dev, torch, traced=False)
        for stride in (1, 5):
            n_rec = K // stride
            tr = _trace_bufs(st.na, B, n_rec, m.nq, m.nv, dev, torch, st.n, st.n_tasks)
            got = _rollout(h, st, s, refs, lim, K, dev, torch, trace=tr, stride=stride)
            _same(plain, got, "final outputs, stride %d" % stride)
            _check_trace(tr, per, stride, K)
        # no trace, and a trace with every field NULL: the untraced call
        _same(plain, _rollout(h, st, s, refs, lim, K, dev, torch, trace=None), "trace = NULL")
        _same(plain, _rollout(h, st, s, refs, lim, K, dev, torch, trace={}, stride=3), "all-NULL trace")
        # the last tick's outputs agree with the tick loop's
        for f in ("x", "tau", "status", "iters", "objective"):
            assert torch_equal(plain[f], per[-1][f]), f
        assert torch_equal(plain["q_next"], per[-1]["q"]) and (plain["ticks_ok"] == K).all().item()
        # some fields only, the last tick not recorded (24 % 7 != 0)
        tr = dict(cost=torch.full((K // 7, B, st.n_tasks), float("nan"), dtype=torch.float64, device=dev),
                  q=torch.full((K // 7, B, m.nq), float("nan"), dtype=torch.float64, device=dev))
        _same(plain, _rollout(h, st, s, refs, lim, K, dev, torch, trace=tr, stride=7), "partial trace")
        for r in range(K // 7):
            assert torch_equal(tr["cost"][r], per[7 * r + 6]["cost"]) and torch_equal(tr["q"][r], per[7 * r + 6]["q"])
    finally:
        h.close()


def test_rollout_traced_shows_the_failed_ticks():
    """max_iter at the median of the stream's iteration counts: some ticks end on MAX_ITER_REACHED, and the trace says which."""
    torch, dev = _torch()
    m, st, tm, s, refs, lim = _squat(B=256, K=16, seed=94_000)
    B, K = 256, 16
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        it = dict(iters=torch.full((K, B), -1, dtype=torch.int32, device=dev))
        _rollout(h, st, s, refs, lim, K, dev, torch, trace=it, stride=1)
        st = dataclasses.replace(st, max_iter=max(1, int(np.median(it["iters"].cpu().numpy()))))
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        tr = _trace_bufs(st.na, B, K, m.nq, m.nv, dev, torch, st.n, st.n_tasks)
        got = _rollout(h, st, s, refs, lim, K, dev, torch, trace=tr, stride=1)
        status = tr["status"].cpu().numpy()
        assert (status == 3).any() and (status == 0).any(), np.unique(status)
        assert np.array_equal(got["ticks_ok"].cpu().numpy(), (status == 0).sum(axis=0))
        q = np.concatenate([s["q"][None], tr["q"].cpu().numpy()])
        v = np.concatenate([s["v"][None], tr["v"].cpu().numpy()])
        bad = status != 0
        assert np.array_equal(q[1:][bad], q[:-1][bad]) and np.array_equal(v[1:][bad], v[:-1][bad])  # a failed tick holds the state
        assert not np.array_equal(q[1:][~bad], q[:-1][~bad])
        per = _tick_loop(h, st, m, s, refs, lim, K, dev, torch)
        _check_trace(tr, per, 1, K)
    finally:
        h.close()


# ---- the mixed roll-out -------------------------------------------------------------------------------------------------------------------

def test_rollout_mixed_traced_equals_mixed_ticks_and_numpy_costs():
    torch, dev = _torch()
    h, m, sets, slots = _fleet("talos")
    try:
        B, K, stride = 256, 40, 1
        plan = _walk_plan(m, sets, 0.03, 0.01)
        offsets = 1 + np.arange(B) % 28
        k0 = 89 - 20  # the window [69, 109) crosses the left foot's touchdown at 89 for every instance
        full = sets["both"][1]
        s = mdl.sample_states(m, full, B, 6, q_noise=0.002, v_noise=0.01, ref_noise=0.0)
        w = _set_weights(sets, B, dev, torch)
        tlb, tub = torch.from_numpy(np.tile(-m.tau_max, (B, 1))).to(dev), torch.from_numpy(np.tile(m.tau_max, (B, 1))).to(dev)
        ldx = max(st.n for st, _ in sets.values())
        ldc = max(st.n_tasks for st, _ in sets.values())
        stream = torch.cuda.current_stream().cuda_stream
        sch, ref = plan.plan(offsets, k0, K)
        assert len(np.unique(sch)) >= 2 and any((np.diff(sch[:, i]) != 0).any() for i in range(B))
        ref_d = torch.from_numpy(ref).to(dev)
        q0, v0 = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)

        def run(trace, traced=True):
            ro, re = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=np.nan)
            isum, tok = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
            args = (slots, sch, dict(q=q0, v=v0, ref=ref_d, momentum=re["momentum"]), w, ro, re["q_next"], re["v_next"], full.dt)
            kw = dict(tlb=tlb, tub=tub, q_solver=re["q_solver"], iters_sum=isum, ticks_ok=tok, stream=stream)
            if traced:
                h.rollout_mixed_traced(*args, trace=trace, stride=stride, **kw)
            else:
                h.rollout_mixed(*args, **kw)
            torch.cuda.synchronize()
            return dict(ro, **re, iters_sum=isum, ticks_ok=tok)

        plain = run(None, traced=False)
        tr = _trace_bufs(m.na, B, K, m.nq, m.nv, dev, torch, ldx=ldx, ldc=ldc)
        _same(plain, run(tr), "final outputs")
        _same(plain, run(None), "trace = NULL")
        _same(plain, run({}), "all-NULL trace")
        # K mixed ticks; the host split of each tick gives the per-set records for the numpy costs
        cq, cv = q0.clone(), v0.clone()
        names = list(sets)
        for t in range(K):
            to, te = _mixed_tick(h, m, sets, slots, sch[t], dict(q=cq, v=cv, ref=ref_d[t].contiguous()), w, tlb, tub, full.dt, ldx, capi.F64, dev, torch)
            torch.cuda.synchronize()
            for f in ("x", "tau", "status", "iters", "objective"):
                assert torch_equal(tr[f][t], to[f]), (t, f)
            assert torch_equal(tr["q"][t], te["q_next"]) and torch_equal(tr["v"][t], te["v_next"]), t
            cost = tr["cost"][t].cpu().numpy()
            for k, name in enumerate(names):
                st, tmk = sets[name]
                idx = np.nonzero(sch[t] == k)[0]
                if idx.size == 0:
                    continue
                assert (cost[idx, st.n_tasks:] == 0).all(), (t, name)
                rec = h.problem_data_host(slots[k], cq.cpu().numpy()[idx], cv.cpu().numpy()[idx], ref[t][idx])
                rec["w"] = w[k][idx].cpu().numpy()
                _check_costs(st, rec, to["x"].cpu().numpy()[idx, :st.n], cost[idx, :st.n_tasks], 1e-12)
            cq, cv = te["q_next"], te["v_next"]
        _same({k: plain[k] for k in ("x", "tau", "status", "iters", "objective")}, to, "last tick")
    finally:
        h.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_and_empty_calls():
    torch, dev = _torch()
    m, st, tm, s, refs, lim = _squat(B=8, K=4, seed=95_000)
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        tr = _trace_bufs(st.na, 8, 4, m.nq, m.nv, dev, torch, st.n, st.n_tasks)
        with pytest.raises(capi.WbcqpError) as e:
            _rollout(h, st, s, refs, lim, 4, dev, torch, trace=tr, stride=0)
        assert e.value.code == 1
        assert tr["status"].eq(-99).all().item() and torch.isnan(tr["cost"]).all().item()
        # batch = 0 and n_ticks = 0: OK, nothing written
        o = _outs(st, 8, dev, torch)
        qn = torch.full((8, m.nq), np.nan, dtype=torch.float64, device=dev)
        vn = torch.full((8, m.nv), np.nan, dtype=torch.float64, device=dev)
        state = dict(q=torch.from_numpy(s["q"]).to(dev), v=torch.from_numpy(s["v"]).to(dev), ref=torch.from_numpy(np.ascontiguousarray(refs)).to(dev))
        h.rollout_traced(0, 0, 4, state, lim, o, qn, vn, 1e-3, trace=tr, stride=1)
        h.rollout_traced(0, 8, 0, state, lim, o, qn, vn, 1e-3, trace=tr, stride=1)
        c = torch.full((8, st.n_tasks), np.nan, dtype=torch.float64, device=dev)
        h.task_costs(0, 0, {}, o["x"], o["tau"], c)
        torch.cuda.synchronize()
        assert tr["status"].eq(-99).all().item() and torch.isnan(tr["cost"]).all().item() and torch.isnan(qn).all().item()
        assert torch.isnan(c).all().item() and o["status"].eq(-99).all().item()
        # a torque task's costs need tau
        stq = structure.STRUCTURES["talos_torque"]()
        h.set_structure(1, stq)
        rows = {k: torch.zeros(8, max(v, 1), dtype=torch.float64, device=dev) for k, v in stq.field_lengths().items()}
        with pytest.raises(capi.WbcqpError) as e:
            h.task_costs(1, 8, rows, o["x"], None, c)
        assert e.value.code == 1
    finally:
        h.close()
    # the mixed call: stride 0 refused; a warm-start handle is UNSUPPORTED, as for the untraced call
    for flags, code, stride in ((0, 1, 0), (capi.FLAG_WARM_START, 3, 1)):
        hm, mm, sets, slots = _fleet("talos", flags=flags)
        try:
            B, K = 4, 3
            sch = np.zeros((K, B), np.int32)
            full = sets["both"][1]
            sm = mdl.sample_states(mm, full, B, 7, q_noise=0.002, v_noise=0.01, ref_noise=0.0)
            w = _set_weights(sets, B, dev, torch)
            ldx = max(x.n for x, _ in sets.values())
            ro, re = _outputs(B, ldx, mm.na, mm.nq, mm.nv, capi.F64, dev, torch, fill=np.nan)
            ref = torch.from_numpy(np.repeat(sm["ref"][None], K, axis=0)).to(dev)
            trm = dict(status=torch.full((K, B), -99, dtype=torch.int32, device=dev))
            with pytest.raises(capi.WbcqpError) as e:
                hm.rollout_mixed_traced(slots, sch, dict(q=torch.from_numpy(sm["q"]).to(dev), v=torch.from_numpy(sm["v"]).to(dev), ref=ref), w, ro,
                                        re["q_next"], re["v_next"], full.dt, trace=trm, stride=stride,
                                        tlb=torch.from_numpy(np.tile(-mm.tau_max, (B, 1))).to(dev), tub=torch.from_numpy(np.tile(mm.tau_max, (B, 1))).to(dev))
            assert e.value.code == code
            torch.cuda.synchronize()
            assert trm["status"].eq(-99).all().item() and ro["status"].eq(-99).all().item()
        finally:
            hm.close()

