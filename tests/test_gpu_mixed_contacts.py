"""A fleet of one robot model whose instances sit in DIFFERENT contact sets, in one call (wbcqp_tick_mixed, wbcqp_rollout_mixed).

Yardsticks: (1) the same tick split on the host -- a torch gather into each contact set, wbcqp_tick on that set's slot, a scatter back --
bit for bit; (2) K mixed ticks, bit for bit; (3) the loop of the three oracles (rows, QP, integration) per contact set on the host, for a
staggered walk on the spot, and the physics of it (a lifted foot rises, a landed foot is back down, the support foot stays)."""
import numpy as np
import pytest

from inria_wbc_amd import capi, structure
from inria_wbc_amd import model as mdl

pytestmark = pytest.mark.gpu

OUT_FIELDS = ("x", "tau", "status", "iters", "objective", "n_active", "active_mask")


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _fleet(robot, dtype=capi.F64, flags=0, first_slot=0):
    """A handle with one slot per contact set of `robot` (structure + model on the shared reference layout)."""
    m = mdl.talos_like() if robot == "talos" else mdl.icub_like()
    sets = mdl.talos_contact_sets(m) if robot == "talos" else mdl.icub_contact_sets(m)
    h = capi.Handle(0, dtype, flags)
    slots = []
    for i, (name, (st, tm)) in enumerate(sets.items()):
        h.set_structure(first_slot + i, st)
        h.set_model(first_slot + i, m, tm)
        slots.append(first_slot + i)
    return h, m, sets, slots


def _inputs(m, sets, B, seed, dtype, dev, torch):
    """States and references by instance (the full map's layout), per-set weights by instance, torque limits by instance."""
    npd = np.float64 if dtype == capi.F64 else np.float32
    full = next(iter(sets.values()))[1]
    s = mdl.sample_states(m, full, B, seed, q_noise=0.005, v_noise=0.02, ref_noise=0.005)
    rng = np.random.default_rng(seed)
    scale = np.where(rng.random(B) < 0.5, 1.0, 1.0 + 0.2 * rng.random(B))  # half the instances on the default weights (the factor cache's case)
    w = [torch.from_numpy((scale[:, None] * st.default_weights[None, :]).astype(npd)).to(dev) for st, _ in sets.values()]
    lim = (1.0 + 0.1 * rng.random((B, 1))) * m.tau_max[None, :]
    tlb, tub = (torch.from_numpy((-lim).astype(npd)).to(dev), torch.from_numpy(lim.astype(npd)).to(dev)) if m.na and next(iter(sets.values()))[0].act_bounds else (None, None)
    state = {k: torch.from_numpy(s[k].astype(npd)).to(dev) for k in ("q", "v", "ref")}
    return state, w, tlb, tub


def _outputs(B, ldx, na, nq, nv, dtype, dev, torch, fill=0.0):
    td = torch.float64 if dtype == capi.F64 else torch.float32
    out = dict(x=torch.full((B, ldx), fill, dtype=td, device=dev), tau=torch.full((B, max(na, 1)), fill, dtype=td, device=dev),
               status=torch.full((B,), -99, dtype=torch.int32, device=dev), iters=torch.full((B,), -1, dtype=torch.int32, device=dev),
               objective=torch.full((B,), fill, dtype=td, device=dev), n_active=torch.full((B,), -1, dtype=torch.int32, device=dev),
               active_mask=torch.full((B, 8), -1, dtype=torch.int32, device=dev))
    ext = dict(q_next=torch.full((B, nq), fill, dtype=td, device=dev), v_next=torch.full((B, nv), fill, dtype=td, device=dev),
               q_solver=torch.full((B, nv), fill, dtype=td, device=dev), momentum=torch.full((B, 6), fill, dtype=td, device=dev))
    return out, ext


def _split_tick(h, m, sets, slots, which, state, w, tlb, tub, dt, ldx, dtype, dev, torch):
    """The host's way: gather each contact set's instances, wbcqp_tick on its slot, scatter the results back to instance order."""
    B = len(which)
    out, ext = _outputs(B, ldx, m.na, m.nq, m.nv, dtype, dev, torch, fill=0.0)
    stream = torch.cuda.current_stream().cuda_stream
    for k, (st, tm) in enumerate(sets.values()):
        idx = np.nonzero(which == k)[0]
        if idx.size == 0:
            continue
        ii = torch.from_numpy(idx).to(dev)
        nb = idx.size
        L = st.field_lengths()
        rows = {f: torch.zeros(nb, max(L[f], 1), dtype=state["q"].dtype, device=dev) for f in capi.ROW_FIELDS}
        rows["w"] = w[k][ii].contiguous()
        if st.act_bounds:
            rows["tlb"], rows["tub"] = tlb[ii].contiguous(), tub[ii].contiguous()
        o, e = _outputs(nb, st.n, st.na, m.nq, m.nv, dtype, dev, torch)
        sub = dict(q=state["q"][ii].contiguous(), v=state["v"][ii].contiguous(), ref=state["ref"][ii].contiguous(), momentum=e["momentum"])
        h.tick(slots[k], nb, sub, rows, o, e["q_next"], e["v_next"], dt, q_solver=e["q_solver"], stream=stream)
        for f in OUT_FIELDS:
            if f == "x":
                out["x"][ii, :st.n] = o["x"]
            else:
                out[f][ii] = o[f]
        for f in ext:
            ext[f][ii] = e[f]
    return out, ext


def _mixed_tick(h, m, sets, slots, which, state, w, tlb, tub, dt, ldx, dtype, dev, torch, fill=0.0):
    B = len(which)
    out, ext = _outputs(B, ldx, m.na, m.nq, m.nv, dtype, dev, torch, fill=fill)
    st_ = dict(state, momentum=ext["momentum"])
    h.tick_mixed(slots, which, st_, w, out, ext["q_next"], ext["v_next"], dt, tlb=tlb, tub=tub, q_solver=ext["q_solver"],
                 stream=torch.cuda.current_stream().cuda_stream)
    return out, ext


def _assert_same(a, b, what):
    for f in a:
        x, y = a[f].cpu().numpy(), b[f].cpu().numpy()
        assert np.array_equal(x, y), (what, f, np.argwhere(x != y)[:5])


@pytest.mark.parametrize("robot,dtype,Bs", [("talos", capi.F64, (1, 37, 1000)), ("icub", capi.F64, (1, 37, 1000)), ("talos", capi.F32, (37,))])
def test_mixed_tick_equals_per_set_ticks_bit_for_bit(robot, dtype, Bs):
    torch, dev = _torch()
    h, m, sets, slots = _fleet(robot, dtype)
    try:
        ldx = max(st.n for st, _ in sets.values())
        dt = next(iter(sets.values()))[1].dt
        K = len(sets)
        for B in Bs:
            rng = np.random.default_rng(B)
            which = rng.integers(0, K, B).astype(np.int32)
            if B >= 37 and K >= 3:
                which[which == K - 1] = 0  # a set with no instance
            state, w, tlb, tub = _inputs(m, sets, B, 1000 + B, dtype, dev, torch)
            mo, me = _mixed_tick(h, m, sets, slots, which, state, w, tlb, tub, dt, ldx, dtype, dev, torch, fill=np.nan)
            so, se = _split_tick(h, m, sets, slots, which, state, w, tlb, tub, dt, ldx, dtype, dev, torch)
            torch.cuda.synchronize()
            _assert_same(mo, so, (robot, B))
            _assert_same(me, se, (robot, B))
            # x: each instance's row in its own set's layout, zeros past its n
            x = mo["x"].cpu().numpy()
            for k, (st, _) in enumerate(sets.values()):
                assert (x[which == k, st.n:] == 0).all()
            assert (mo["status"].cpu().numpy() == 0).mean() > 0.9
            assert len(set(which.tolist())) >= min(B, 2)
    finally:
        h.close()


def _walk_plan(m, sets, T, step):
    return mdl.WalkOnSpotPlan(m, {k: tm for k, (_, tm) in sets.items()}, T, T, step)


def _set_weights(sets, B, dev, torch):
    """walk_on_spot.yaml's customize_task_weights (momentum: 0) on every set, by instance."""
    out = []
    for st, _ in sets.values():
        w = st.default_weights.copy()
        if "momentum" in st.task_names:
            w[st.task_names.index("momentum")] = 0.0
        out.append(torch.from_numpy(np.tile(w, (B, 1))).to(dev))
    return out


def test_rollout_mixed_equals_mixed_ticks_bit_for_bit():
    torch, dev = _torch()
    h, m, sets, slots = _fleet("talos")
    try:
        B, K = 64, 60
        plan = _walk_plan(m, sets, 0.03, 0.01)  # 30-tick phases: the left foot lifts at tau 30 and lands at 89, the right one lifts at 120
        offsets = 1 + np.arange(B) % 28  # instance i: behaviour ticks [89 - o, 149 - o) in the window, across the touchdown at 89 and the lift at 120
        k0 = 89
        full = sets["both"][1]
        s = mdl.sample_states(m, full, B, 5, q_noise=0.002, v_noise=0.01, ref_noise=0.0)
        q, v = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)
        w = _set_weights(sets, B, dev, torch)
        tlb, tub = torch.from_numpy(np.tile(-m.tau_max, (B, 1))).to(dev), torch.from_numpy(np.tile(m.tau_max, (B, 1))).to(dev)
        ldx = max(st.n for st, _ in sets.values())
        stream = torch.cuda.current_stream().cuda_stream
        # walk up to tick k0 (one roll-out), then the window [k0, k0 + K) two ways
        sch0, ref0 = plan.plan(offsets, 0, k0)
        out, ext = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch)
        h.rollout_mixed(slots, sch0, dict(q=q, v=v, ref=torch.from_numpy(ref0).to(dev)), w, out, ext["q_next"], ext["v_next"], full.dt,
                        tlb=tlb, tub=tub, stream=stream)
        q0, v0 = ext["q_next"].clone(), ext["v_next"].clone()
        sch, ref = plan.plan(offsets, k0, K)
        assert all(int((np.diff(sch[:, i]) != 0).sum()) >= 2 for i in range(B)), "every instance switches its contact set at least twice"
        ref_d = torch.from_numpy(ref).to(dev)
        ro, re = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=np.nan)
        isum, tok = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
        h.rollout_mixed(slots, sch, dict(q=q0, v=v0, ref=ref_d, momentum=re["momentum"]), w, ro, re["q_next"], re["v_next"], full.dt, tlb=tlb,
                        tub=tub, q_solver=re["q_solver"], iters_sum=isum, ticks_ok=tok, stream=stream)
        cq, cv = q0.clone(), v0.clone()
        it_sum, ok_sum = np.zeros(B, np.int64), np.zeros(B, np.int64)
        for t in range(K):
            to, te = _mixed_tick(h, m, sets, slots, sch[t], dict(q=cq, v=cv, ref=ref_d[t].contiguous()), w, tlb, tub, full.dt, ldx, capi.F64,
                                 dev, torch)
            torch.cuda.synchronize()
            it_sum += to["iters"].cpu().numpy()
            ok_sum += (to["status"].cpu().numpy() == 0)
            cq, cv = te["q_next"], te["v_next"]
        torch.cuda.synchronize()
        _assert_same(ro, to, "last tick's outputs")
        _assert_same(re, te, "state")
        assert np.array_equal(isum.cpu().numpy(), it_sum) and np.array_equal(tok.cpu().numpy(), ok_sum)
        assert (tok.cpu().numpy() == K).all()
    finally:
        h.close()


def test_fleet_walk_on_spot_matches_oracle_loop_and_lifts_and_lands_feet():
    """Six Talos-like robots walking on the spot at different phase offsets, rolled out in chunks, against the oracles' loop per contact set.
    200-tick phases: the left foot lifts at tau 200 and its contact comes back at tau 599.  Physics: the lifted foot rises (the references
    have no feed-forward, so it lags its 5 cm: about 1.7 cm at touchdown), after touchdown it comes back down under the contact's own
    motion task, and the support foot never moves by more than 2 mm."""
    from oracle import oracle as orc
    from oracle import rbd
    torch, dev = _torch()
    h, m, sets, slots = _fleet("talos")
    try:
        B, chunk, n_chunks = 6, 50, 18
        plan = _walk_plan(m, sets, 0.2, 0.05)
        n = plan.n_foot
        offsets = np.array([0, 20, 40, 60, 80, 100])
        names = list(sets)
        full = sets["both"][1]
        s = mdl.sample_states(m, full, B, 1, q_noise=0.0, v_noise=0.0, ref_noise=0.0)
        q, v = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)
        w = _set_weights(sets, B, dev, torch)
        wn = [t.cpu().numpy() for t in w]
        tl, tu = np.tile(-m.tau_max, (B, 1)), np.tile(m.tau_max, (B, 1))
        tlb, tub = torch.from_numpy(tl).to(dev), torch.from_numpy(tu).to(dev)
        ldx = max(st.n for st, _ in sets.values())
        stream = torch.cuda.current_stream().cuda_stream
        oq, ov = s["q"].copy(), s["v"].copy()
        lf, rf = m.frame("leg_left_6_joint"), m.frame("leg_right_6_joint")
        pf0 = m.frame_placements(m.q0)[1]
        dz = {i: [] for i in range(B)}  # (behaviour tick, height of the left foot above its start) at every chunk end
        switched, prev = np.zeros(B, int), None
        for c in range(n_chunks):
            sch, ref = plan.plan(offsets, c * chunk, chunk)
            seq = sch if prev is None else np.concatenate([prev[None], sch])
            switched += (np.diff(seq, axis=0) != 0).sum(axis=0)
            prev = sch[-1]
            out, ext = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch)
            h.rollout_mixed(slots, sch, dict(q=q, v=v, ref=torch.from_numpy(ref).to(dev)), w, out, ext["q_next"], ext["v_next"], full.dt,
                            tlb=tlb, tub=tub, stream=stream)
            q, v = ext["q_next"], ext["v_next"]
            for t in range(chunk):  # the oracles, one contact set at a time
                nq_, nv_ = oq.copy(), ov.copy()
                for k, nm in enumerate(names):
                    idx = np.nonzero(sch[t] == k)[0]
                    if idx.size == 0:
                        continue
                    st, tm = sets[nm]
                    rows = rbd.task_rows(m, tm, st, oq[idx], ov[idx], ref[t][idx], n_threads=4)
                    oo = orc.tick_batch(st, dict(rows, tlb=tl[idx], tub=tu[idx], w=wn[k][idx]), nthreads=4)
                    assert (oo["status"] == 0).all(), (c, t, nm, oo["status"])
                    nxt = orc.integrate(True, full.dt, oq[idx], ov[idx], oo["x"][:, :st.nv])
                    nq_[idx], nv_[idx] = nxt["q_next"], nxt["v_next"]
                oq, ov = nq_, nv_
            torch.cuda.synchronize()
            assert (out["status"].cpu().numpy() == 0).all()
            gq = q.cpu().numpy()
            assert np.abs(gq - oq).max() < 1e-5, (c, np.abs(gq - oq).max())
            for i in range(B):
                p = m.frame_placements(gq[i])[1]
                tau = (c + 1) * chunk - offsets[i]
                if tau < 4 * n:  # (the right foot lifts from tau 800 on)
                    assert np.abs(p[rf] - pf0[rf]).max() < 2e-3, (c, i, p[rf] - pf0[rf])  # the support foot stays
                dz[i].append((tau, p[lf][2] - pf0[lf][2]))
        assert (switched >= 2).all(), switched  # every instance lifted its left foot and put it down
        for i in range(B):
            up = max(z for tau, z in dz[i] if tau <= 3 * n)
            at_touchdown = [z for tau, z in dz[i] if 3 * n - chunk < tau <= 3 * n][0]
            last_tau, last = dz[i][-1]
            assert up > 0.01 and at_touchdown > 0.01, (i, dz[i])  # the lifted foot rose
            assert last_tau >= 4 * n - chunk and last < 0.85 * at_touchdown, (i, dz[i])  # the landed foot comes back down
    finally:
        h.close()


def test_failing_qp_in_one_set_keeps_that_instance_state():
    """Mirror of test_tick_keeps_the_state_of_an_instance_whose_qp_fails (test_gpu_rollout.py): an instance whose torque limits cannot hold
    it keeps q and v, the others move; ticks_ok counts it."""
    torch, dev = _torch()
    h, m, sets, slots = _fleet("talos")
    try:
        B = 12
        which = (np.arange(B) % 3).astype(np.int32)
        state, w, tlb, tub = _inputs(m, sets, B, 4242, capi.F64, dev, torch)
        bad = 4  # set 1 (no left foot)
        tlb[bad] = 1.0
        tub[bad] = -1.0  # torque limits that contradict each other: its QP is infeasible
        ldx = max(st.n for st, _ in sets.values())
        dt = sets["both"][1].dt
        out, ext = _mixed_tick(h, m, sets, slots, which, state, w, tlb, tub, dt, ldx, capi.F64, dev, torch)
        torch.cuda.synchronize()
        status = out["status"].cpu().numpy()
        assert status[bad] != 0 and (np.delete(status, bad) == 0).all(), status
        q, qn = state["q"].cpu().numpy(), ext["q_next"].cpu().numpy()
        v, vn = state["v"].cpu().numpy(), ext["v_next"].cpu().numpy()
        assert np.array_equal(qn[bad], q[bad]) and np.array_equal(vn[bad], v[bad])
        assert all(not np.array_equal(qn[i], q[i]) for i in range(B) if i != bad)
        # the same through a roll-out of two ticks: ticks_ok counts the failures
        ref2 = torch.stack([state["ref"], state["ref"]]).contiguous()
        o2, e2 = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch)
        isum, tok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        h.rollout_mixed(slots, np.stack([which, which]), dict(state, ref=ref2), w, o2, e2["q_next"], e2["v_next"], dt, tlb=tlb, tub=tub,
                        iters_sum=isum, ticks_ok=tok, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        tok = tok.cpu().numpy()
        assert tok[bad] == 0 and (np.delete(tok, bad) == 2).all(), tok
        assert np.array_equal(e2["q_next"].cpu().numpy()[bad], q[bad])
    finally:
        h.close()


def test_refusals_leave_the_outputs_untouched():
    torch, dev = _torch()
    h, m, sets, slots = _fleet("talos")
    ic = mdl.icub_like()
    st_ic, tm_ic = mdl.icub_contact_sets(ic)["both"]
    h.set_structure(5, st_ic)
    h.set_model(5, ic, tm_ic)
    # a Talos slot whose map has a different reference length (the single-support map on its own layout)
    st_ss = structure.talos_structure(single_support=True)
    tm_own = mdl.build_taskmap(m, st_ss, [n for n in mdl.talos_stack() if n["name"] != "contact_lfoot"])
    assert tm_own.nref != sets["both"][1].nref
    h.set_structure(6, st_ss)
    h.set_model(6, m, tm_own)
    try:
        B = 8
        which = (np.arange(B) % 3).astype(np.int32)
        state, w, tlb, tub = _inputs(m, sets, B, 7, capi.F64, dev, torch)
        ldx = max(st.n for st, _ in sets.values())
        dt = sets["both"][1].dt
        out, ext = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=3.5)
        before = {k: t.clone() for k, t in list(out.items()) + list(ext.items())}
        stream = torch.cuda.current_stream().cuda_stream

        def call(sl, wh, ww, handle=h):
            handle.tick_mixed(sl, wh, dict(state, momentum=ext["momentum"]), ww, out, ext["q_next"], ext["v_next"], dt, tlb=tlb, tub=tub,
                              q_solver=ext["q_solver"], stream=stream)

        cases = [("another model", [slots[0], 5, slots[2]], which, w),
                 ("another nref", [slots[0], 6, slots[2]], which, w),
                 ("which out of range", slots, np.where(np.arange(B) == 3, 3, which).astype(np.int32), w),
                 ("negative which", slots, np.where(np.arange(B) == 3, -1, which).astype(np.int32), w),
                 ("no slot", [], np.zeros(B, np.int32), []),
                 ("nine slots", [slots[0]] * 9, which, [w[0]] * 9),
                 ("NULL w", slots, which, [w[0], None, w[2]])]
        for what, sl, wh, ww in cases:
            with pytest.raises(capi.WbcqpError) as e:
                call(sl, wh, ww)
            assert e.value.code == 1, (what, e.value)
        # a warm-start handle: UNSUPPORTED, from both calls
        hw, _, _, wslots = _fleet("talos", flags=64)
        try:
            with pytest.raises(capi.WbcqpError) as e:
                call(wslots, which, w, handle=hw)
            assert e.value.code == 3
            with pytest.raises(capi.WbcqpError) as e:
                hw.rollout_mixed(wslots, np.stack([which]), dict(state, ref=state["ref"][None].contiguous()), w, out, ext["q_next"], ext["v_next"],
                                 dt, tlb=tlb, tub=tub, stream=stream)
            assert e.value.code == 3
        finally:
            hw.close()
        with pytest.raises(capi.WbcqpError) as e:
            h.rollout_mixed(slots, np.stack([which, np.full(B, 7, np.int32)]), dict(state, ref=torch.stack([state["ref"]] * 2).contiguous()), w, out,
                            ext["q_next"], ext["v_next"], dt, tlb=tlb, tub=tub, stream=stream)
        assert e.value.code == 1
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal({**out, **ext}[k], t), k
        # a NULL w for a slot no instance uses is not an error
        call(slots, np.where(which == 1, 0, which).astype(np.int32), [w[0], None, w[2]])
        torch.cuda.synchronize()
        assert (out["status"].cpu().numpy() == 0).all()
    finally:
        h.close()
