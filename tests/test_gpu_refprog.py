"""References generated on the device from a reference program (refgen_kernel: wbcqp_reference_samples, wbcqp_rollout_program,
wbcqp_rollout_mixed_program).

Yardsticks: the numpy expansion inria_wbc_amd.refprog.expand -- holds and untouched entries bit for bit, moving samples within bounds DERIVED from the
closed forms (below); the existing roll-outs fed the generated rows as an array, bit for bit; the kernel's own output under other chunk lengths and
other splits of the ticks into calls, bit for bit.

Bounds of a moving sample (eps = 2^-52).  Host and device evaluate the same polynomial of the same td = (dt i) / T in a different order of fewer than
eight rounded operations each, on terms whose absolute values sum to c_k = (31, 120, 360) for derivative order k: |error| <= 256 eps c_k |xf - x0| / T^k,
plus eps |x0| for the final sum of order 0 (plus eps |origin| where a RELATIVE track adds the instance's origin).  A rotation entry is a product of
entries <= 1 with sin / cos of an angle that carries the polynomial's error: 256 eps (1 + 31 |angle|).  An F32 handle stores the double result rounded
to float: within one float ulp of expand(...).astype(float32)."""
import atexit
import os
import subprocess
import sys

import numpy as np
import pytest

from inria_wbc_amd import capi, refprog, structure
from inria_wbc_amd import model as mdl
from tests.test_gpu_mixed_contacts import _fleet, _outputs, _set_weights, _walk_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
C_K = (31.0, 120.0, 360.0)
MEASURED = []  # (what, figure): printed when the session's process ends


def _print_measured():
    print("\n==== reference programs: measured maxima (tests/test_gpu_refprog.py) ====")
    for what, fig in MEASURED:
        print("%-72s %s" % (what, fig))


def _measured(what, fig):
    """Keeps a figure for the end of the session (after pytest has given the terminal back) and prints it now, before the assertion it belongs to."""
    if not MEASURED:
        atexit.register(_print_measured)
    MEASURED.append((what, fig))
    print("%s: %s" % (what, fig))


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _td(dtype, torch):
    return (np.float64, torch.float64) if dtype == capi.F64 else (np.float32, torch.float32)


def _eq(a, b):
    x, y = a.cpu().numpy(), b.cpu().numpy()
    return x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert _eq(a[k], b[k]), (what, k)


# ---- 5. the expansion against numpy ------------------------------------------------------------------------------------------------------------

def _everything(nref=305, dt=1e-3):
    """Every kind of track on a Talos-sized row: a full CoM stream, a posture entry, a full SE3 move with a rotation, a pose-only SE3 with two
    destinations and a hold in the middle, a RELATIVE SE3 and a RELATIVE VEC.  Intro 60 ticks, cycle 90."""
    p = refprog.Program(nref, dt, 60, 90)
    c0, c1, c2 = np.array([0.02, -0.01, 0.88]), np.array([0.02, 0.07, 0.68]), np.array([-0.03, 0.07, 0.80])
    p.add_vec(192, [(c0, c1, 0.06), (c1, c1, 0.03), (c1, c2, 0.06)])
    p.add_vec(213 + 5, [(0.1, 0.1, 0.06), (0.1, -0.4, 0.05), (-0.4, 0.1, 0.04)], dim=1)
    Ra, Rb = mdl._rot(2, 0.2) @ mdl._rot(0, -0.1), mdl._rot(1, 0.9) @ mdl._rot(2, -0.4)
    pa, pb = np.array([0.3, 0.2, 1.0]), np.array([0.35, 0.1, 1.2])
    p.add_se3(72, [(Ra, pa, Rb, pb, 0.075), (Rb, pb, Ra, pa, 0.075)])
    f0, f1 = np.array([0.0, 0.09, 0.1]), np.array([0.0, 0.09, 0.15])
    Rf = mdl._rot(2, 0.05)
    p.add_se3((144, 257), [(Rf, f0, Rf, f1, 0.05), (Rf, f1, Rf, f1, 0.05), (Rf, f1, Rf, f0, 0.05)], pose_only=True)
    Rr = mdl._rot(0, 0.5)
    z = np.zeros(3)
    p.add_se3(96, [(np.eye(3), z, np.eye(3), z, 0.06), (np.eye(3), z, Rr, np.array([0.0, 0.1, -0.05]), 0.09)], relative=True)
    p.add_vec(0, [(z, np.array([0.0, 0.0, -0.1]), 0.1), (np.array([0.0, 0.0, -0.1]), z, 0.05)], relative=True)
    assert all(sum(s.n_steps for s in t.segments) == 150 for t in p.tracks)
    return p


def _tolerances(prog, base, idx):
    """tol [n_ticks][B][nref] for expand's rows at the samples idx: 0 = bit for bit (untouched entries, holds), else the docstring's bound."""
    B = idx.shape[1]
    base = np.broadcast_to(np.asarray(base, dtype=np.float64), (B, prog.nref))
    tol = np.zeros(idx.shape + (prog.nref,))
    for tr in prog.tracks:
        rel, pose = bool(tr.flags & refprog.RELATIVE), bool(tr.flags & refprog.POSE_ONLY)
        tab = np.zeros((prog.length, tr.ncomp))
        org = np.zeros((B, tr.ncomp))  # the extra term of a RELATIVE track's final sum, by instance
        at = 0
        for sg in tr.segments:
            d = np.abs(sg.xf - sg.x0)
            rows = slice(at, at + sg.n_steps)
            if tr.kind == refprog.TRACK_VEC:
                for k in range(3 if tr.dim == 3 and not pose else 1):
                    tab[rows, k * tr.dim:(k + 1) * tr.dim] = 256 * EPS * C_K[k] * d[:tr.dim] / sg.T ** k + (EPS * np.abs(sg.x0[:tr.dim]) * (d[:tr.dim] > 0) if k == 0 else 0.0)
            else:
                tab[rows, 0:3] = 256 * EPS * C_K[0] * d + EPS * np.abs(sg.x0) * (d > 0)
                moving = sg.angle != 0.0
                tab[rows, 3:12] = 256 * EPS * (1 + 31 * abs(sg.angle)) if (moving or rel) else 0.0
                if not pose:
                    for k in (1, 2):
                        tab[rows, 6 + 6 * k:9 + 6 * k] = 256 * EPS * C_K[k] * d / sg.T ** k
                        tab[rows, 9 + 6 * k:12 + 6 * k] = 256 * EPS * C_K[k] * abs(sg.angle) / sg.T ** k
            at += sg.n_steps
        t = tab[idx]
        if rel:  # origin + x: one more rounded sum where x moves (a hold adds the same two numbers on both sides)
            n = 3 if tr.kind == refprog.TRACK_SE3 else tr.dim
            org[:, :n] = EPS * np.abs(base[:, tr.dst[0]:tr.dst[0] + n])
            t = t + org[None] * (t > 0)
        for dst in tr.dst:
            if dst >= 0:
                tol[..., dst:dst + tr.ncomp] = t
    return tol


def _bases(prog, B, seed, npd):
    """Base rows by instance: random numbers, proper rotations at the origins of the RELATIVE SE3 tracks."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((B, prog.nref))
    for tr in prog.tracks:
        if tr.kind == refprog.TRACK_SE3 and tr.flags & refprog.RELATIVE:
            for i in range(B):
                base[i, tr.dst[0] + 3:tr.dst[0] + 12] = (mdl._rot(i % 3, rng.uniform(-1, 1)) @ mdl._rot((i + 1) % 3, rng.uniform(-1, 1))).T.reshape(9)
    return base.astype(npd)


@pytest.mark.parametrize("dtype", [capi.F64, capi.F32])
def test_reference_samples_match_expand(dtype):
    torch, dev = _torch()
    npd, td = _td(dtype, torch)
    h = capi.Handle(0, dtype)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        m = mdl.talos_like()
        sets = mdl.talos_contact_sets(m)
        plan = _walk_plan(m, sets, 0.05, 0.02)
        cases = [("everything", _everything(), None, 37, -11, 420), ("walk on the spot", refprog.walk_on_spot_program(plan), plan.base, 64, 5, 500)]
        for name, prog, base, B, tick0, n in cases:
            base = _bases(prog, B, 11, npd) if base is None else base.astype(npd)
            offsets = np.random.default_rng(4).integers(-50, 120, B)
            out = torch.full((n, B, prog.nref), float("nan"), dtype=td, device=dev)
            h.reference_samples(prog, torch.from_numpy(base).to(dev), offsets, tick0, n, out, stream=stream)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want, _ = refprog.expand(prog, base.astype(np.float64), offsets, tick0, n)
            idx = refprog.index(prog, np.arange(tick0, tick0 + n)[:, None] - offsets[None, :])
            assert len(np.unique(idx)) == prog.length  # every sample of the timeline is played by some instance
            tol = _tolerances(prog, base.astype(np.float64), idx)
            if dtype == capi.F32:
                w32 = want.astype(np.float32)
                exact = tol == 0
                assert np.array_equal(got[exact], w32[exact]), name
                ulp = np.spacing(np.maximum(np.abs(got), np.abs(w32)))
                err = np.abs(got.astype(np.float64) - w32.astype(np.float64)) / ulp
                _measured("reference_samples F32, %s: max error in float ulps" % name, "%.2f" % err.max())
                assert (err <= 1.0).all(), (name, err.max())
                continue
            exact = tol == 0
            assert exact.mean() > 0.5
            assert np.array_equal(got[exact], want[exact]), (name, np.argwhere(exact & (got != want))[:5])
            err = np.abs(got - want)
            ratio = (err[~exact] / tol[~exact]).max() if (~exact).any() else 0.0
            _measured("reference_samples F64, %s: max |error| / bound (moving entries)" % name, "%.3g (largest |error| %.3g)" % (ratio, err.max()))
            assert (err <= tol).all(), (name, ratio, np.argwhere(err > tol)[:5])
    finally:
        h.close()


# ---- 6. chunking is invisible -------------------------------------------------------------------------------------------------------------------

def _chunk_case():
    prog = _everything()
    B = 19
    return prog, _bases(prog, B, 12, np.float64), np.random.default_rng(5).integers(-30, 90, B), 23, 100


def _child_samples(path):
    """Run in a fresh process (WBCQP_REFPROG_CHUNK is read at wbcqp_create): the chunk case's rows to `path`."""
    torch, dev = _torch()
    prog, base, offsets, tick0, n = _chunk_case()
    h = capi.Handle(0, capi.F64)
    out = torch.zeros(n, len(offsets), prog.nref, dtype=torch.float64, device=dev)
    h.reference_samples(prog, torch.from_numpy(base).to(dev), offsets, tick0, n, out)
    torch.cuda.synchronize()
    np.save(path, out.cpu().numpy())
    h.close()


def test_chunk_length_and_call_boundaries_do_not_change_a_bit(tmp_path):
    torch, dev = _torch()
    rows = {}
    for chunk in ("1", "7", None):
        env = dict(os.environ)
        env.pop("WBCQP_REFPROG_CHUNK", None)
        if chunk:
            env["WBCQP_REFPROG_CHUNK"] = chunk
        path = str(tmp_path / ("rows_%s.npy" % chunk))
        r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_refprog import _child_samples; _child_samples(%r)" % path], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        rows[chunk] = np.load(path)
    assert 100 % 7 != 0
    assert np.array_equal(rows["1"], rows[None]) and np.array_equal(rows["7"], rows[None])
    prog, base, offsets, tick0, n = _chunk_case()
    want, _ = refprog.expand(prog, base, offsets, tick0, n)
    assert np.allclose(rows[None], want, rtol=0, atol=1e-9)
    h = capi.Handle(0, capi.F64)
    try:
        b = torch.from_numpy(base).to(dev)
        f = lambda t0, k: h.reference_samples(prog, b, offsets, t0, k, torch.zeros(k, len(offsets), prog.nref, dtype=torch.float64, device=dev))  # noqa: E731
        one, lo, hi = f(0, 100), f(0, 50), f(50, 50)
        torch.cuda.synchronize()
        assert torch.equal(one, torch.cat([lo, hi]))
        assert np.array_equal(f(tick0, n).cpu().numpy(), rows[None])
    finally:
        h.close()


# ---- 7. / 9. the one-slot roll-out ----------------------------------------------------------------------------------------------------------------

def _robot(robot):
    m = {"talos": mdl.talos_like, "icub": mdl.icub_like}[robot]()
    st = {"talos": structure.talos_structure, "icub": structure.icub_structure}[robot]()
    return m, st, mdl.build_taskmap(m, st, {"talos": mdl.talos_stack, "icub": mdl.icub_stack}[robot]())


def _squat_case(robot, B, dtype, dev, torch, seed=97_000):
    """The squat (etc/talos/squat.yaml: CoM 0.2 down and back up, 2 s each, looping) as a program, instance i 37 i ticks into it."""
    npd, td = _td(dtype, torch)
    m, st, tm = _robot(robot)
    s = mdl.sample_states(m, tm, B, seed, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    com = next(b for b in tm.blocks if b.kind == mdl.T_COM)
    prog = refprog.move_com_program(tm.nref, com.ref, m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0, loop=True, absolute=False)
    offsets = -37 * np.arange(B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(npd)).to(dev)  # noqa: E731
    lim = dict(w=up(np.tile(st.default_weights, (B, 1))))
    if st.act_bounds:
        lim.update(tlb=up(np.tile(-m.tau_max, (B, 1))), tub=up(np.tile(m.tau_max, (B, 1))))
    return m, st, tm, prog, offsets, dict(q=up(s["q"]), v=up(s["v"])), up(s["ref"]), lim


def _bufs(st, m, B, n_rec, td, dev, torch):
    f = lambda *shape: torch.full(shape, float("nan"), dtype=td, device=dev)  # noqa: E731
    i = lambda fill, *shape: torch.full(shape, fill, dtype=torch.int32, device=dev)  # noqa: E731
    out = dict(x=f(B, st.n), tau=f(B, st.na), status=i(-99, B), iters=i(-1, B), objective=f(B))
    ext = dict(q_next=f(B, m.nq), v_next=f(B, m.nv), iters_sum=i(-7, B), ticks_ok=i(-7, B))
    trace = dict(q=f(n_rec, B, m.nq), v=f(n_rec, B, m.nv), x=f(n_rec, B, st.n), tau=f(n_rec, B, st.na), status=i(-99, n_rec, B), iters=i(-1, n_rec, B),
                 objective=f(n_rec, B), cost=f(n_rec, B, st.n_tasks)) if n_rec else None
    return out, ext, trace


def _run(h, st, m, tm, B, K, state, lim, td, dev, torch, stride=0, ref=None, prog=None, base=None, offsets=None, tick0=0):
    """One roll-out of K ticks: from the array `ref`, or by program.  -> every output and trace field."""
    out, ext, trace = _bufs(st, m, B, K // stride if stride else 0, td, dev, torch)
    stream = torch.cuda.current_stream().cuda_stream
    kw = dict(trace=trace, stride=max(stride, 1), iters_sum=ext["iters_sum"], ticks_ok=ext["ticks_ok"], stream=stream)
    if prog is None:
        h.rollout_traced(0, B, K, dict(state, ref=ref), lim, out, ext["q_next"], ext["v_next"], tm.dt, **kw)
    else:
        h.rollout_program(0, B, tick0, K, prog, base, offsets, state, lim, out, ext["q_next"], ext["v_next"], tm.dt, **kw)
    torch.cuda.synchronize()
    res = dict(out, **ext)
    res.update({"trace_" + k: v for k, v in (trace or {}).items()})
    return res


@pytest.mark.parametrize("robot,dtype,B,streams", [("talos", capi.F64, 512, "1"), ("talos", capi.F64, 512, "2"), ("icub", capi.F64, 96, None),
                                                   ("talos", capi.F32, 64, None)])
def test_rollout_program_equals_rollout_traced_on_the_generated_rows(robot, dtype, B, streams, monkeypatch):
    torch, dev = _torch()
    npd, td = _td(dtype, torch)
    if streams:
        monkeypatch.setenv("WBCQP_ROLLOUT_STREAMS", streams)
    monkeypatch.setenv("WBCQP_REFPROG_CHUNK", "7")
    K, tick0 = 24, 5  # three chunks of 7 and a remainder of 3
    m, st, tm, prog, offsets, state, base, lim = _squat_case(robot, B, dtype, dev, torch)
    h = capi.Handle(0, dtype)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        ref = h.reference_samples(prog, base, offsets, tick0, K, torch.zeros(K, B, tm.nref, dtype=td, device=dev), stream=torch.cuda.current_stream().cuda_stream)
        for stride in (0, 3):
            a = _run(h, st, m, tm, B, K, state, lim, td, dev, torch, stride=stride, ref=ref)
            b = _run(h, st, m, tm, B, K, state, lim, td, dev, torch, stride=stride, prog=prog, base=base, offsets=offsets, tick0=tick0)
            _same(a, b, "%s stride %d" % (robot, stride))
            assert a["ticks_ok"].sum().item() > 0.9 * B * K  # (the comparison is of solved ticks)
            if stride:
                assert not torch.isnan(b["trace_cost"]).any().item()
        # the references did something: the CoM rows move between instances and ticks
        com = next(blk for blk in tm.blocks if blk.kind == mdl.T_COM)
        z = ref[:, :, com.ref + 2].cpu().numpy()
        assert np.ptp(z[:, min(B - 1, 20)]) > 0 and np.ptp(z[0]) > 1e-3
    finally:
        h.close()


def test_two_rollout_program_calls_equal_one_of_twice_the_ticks(monkeypatch):
    torch, dev = _torch()
    monkeypatch.setenv("WBCQP_REFPROG_CHUNK", "7")
    B, K = 128, 17
    m, st, tm, prog, offsets, state, base, lim = _squat_case("talos", B, capi.F64, dev, torch, seed=98_000)
    td = torch.float64
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        args = dict(prog=prog, base=base, offsets=offsets)
        one = _run(h, st, m, tm, B, 2 * K, state, lim, td, dev, torch, tick0=0, **args)
        first = _run(h, st, m, tm, B, K, state, lim, td, dev, torch, tick0=0, **args)
        second = _run(h, st, m, tm, B, K, dict(q=first["q_next"], v=first["v_next"]), lim, td, dev, torch, tick0=K, **args)
        for f in ("x", "tau", "status", "iters", "objective", "q_next", "v_next"):
            assert _eq(one[f], second[f]), f
        assert _eq(one["iters_sum"], first["iters_sum"] + second["iters_sum"]) and _eq(one["ticks_ok"], first["ticks_ok"] + second["ticks_ok"])
        assert not _eq(first["q_next"], second["q_next"])
    finally:
        h.close()


# ---- 8. the mixed roll-out ---------------------------------------------------------------------------------------------------------------------------

def _mixed_case(B, K, dev, torch):
    h, m, sets, slots = _fleet("talos")
    plan = mdl.WalkOnSpotPlan(m, {k: tm for k, (_, tm) in sets.items()}, traj_com_duration=0.05, traj_foot_duration=0.02, step_height=0.05)
    full = sets["both"][1]
    s = mdl.sample_states(m, full, B, 8, q_noise=0.002, v_noise=0.01, ref_noise=0.0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return h, m, sets, slots, plan, full, dict(q=up(s["q"]), v=up(s["v"])), _set_weights(sets, B, dev, torch), up(np.tile(-m.tau_max, (B, 1))), up(np.tile(m.tau_max, (B, 1)))


def _run_mixed(h, m, sets, slots, full, B, K, state, w, tlb, tub, dev, torch, stride, sch=None, ref=None, prog=None, base=None, offsets=None, tick0=0):
    ldx, ldc = max(st.n for st, _ in sets.values()), max(st.n_tasks for st, _ in sets.values())
    ro, re = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=np.nan)
    isum, tok = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    n_rec = K // stride
    trace = dict(q=f(n_rec, B, m.nq), v=f(n_rec, B, m.nv), x=f(n_rec, B, ldx), tau=f(n_rec, B, m.na), objective=f(n_rec, B), cost=f(n_rec, B, ldc),
                 status=torch.full((n_rec, B), -99, dtype=torch.int32, device=dev), iters=torch.full((n_rec, B), -1, dtype=torch.int32, device=dev))
    kw = dict(trace=trace, stride=stride, tlb=tlb, tub=tub, q_solver=re["q_solver"], iters_sum=isum, ticks_ok=tok, stream=torch.cuda.current_stream().cuda_stream)
    st_ = dict(state, momentum=re["momentum"])
    if prog is None:
        h.rollout_mixed_traced(slots, sch, dict(st_, ref=ref), w, ro, re["q_next"], re["v_next"], full.dt, **kw)
    else:
        h.rollout_mixed_program(slots, B, tick0, K, prog, base, offsets, st_, w, ro, re["q_next"], re["v_next"], full.dt, **kw)
    torch.cuda.synchronize()
    res = dict(ro, **re, iters_sum=isum, ticks_ok=tok)
    res.update({"trace_" + k: v for k, v in trace.items()})
    return res


def test_rollout_mixed_program_equals_rollout_mixed_traced_on_expands_schedule():
    torch, dev = _torch()
    B, K, tick0, stride = 64, 300, 0, 3
    h, m, sets, slots, plan, full, state, w, tlb, tub = _mixed_case(B, K, dev, torch)
    try:
        assert plan.phase_len == [50, 20, 20, 50, 20, 20, 50]
        offsets = np.random.default_rng(3).integers(0, 100, B)
        prog = refprog.walk_on_spot_program(plan)
        base = torch.from_numpy(plan.base).to(dev)
        want_ref, sch = refprog.expand(prog, plan.base, offsets, tick0, K)
        # every contact set and every phase occurs, some ticks hold one, two and three sets, and instances pass the wrap
        tau = np.arange(tick0, tick0 + K)[:, None] - offsets[None, :]
        assert set(np.unique(sch)) == {0, 1, 2} and set(np.unique(plan.phase_of[plan.index(tau)])) == set(range(7))
        assert {len(np.unique(row)) for row in sch} == {1, 2, 3}
        assert (tau.max(axis=0) >= prog.length).sum() >= 1
        ref = h.reference_samples(prog, base, offsets, tick0, K, torch.zeros(K, B, plan.nref, dtype=torch.float64, device=dev), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.allclose(ref.cpu().numpy(), want_ref, rtol=0, atol=1e-12)  # (test_reference_samples_match_expand holds the bounds)
        a = _run_mixed(h, m, sets, slots, full, B, K, state, w, tlb, tub, dev, torch, stride, sch=sch, ref=ref)
        b = _run_mixed(h, m, sets, slots, full, B, K, state, w, tlb, tub, dev, torch, stride, prog=prog, base=base, offsets=offsets, tick0=tick0)
        _same(a, b, "mixed roll-out")
        assert not torch.isnan(b["trace_cost"]).any().item()
        _measured("rollout_mixed_program, 64 walkers x 300 ticks: ticks solved", "%d of %d" % (int(b["ticks_ok"].sum().item()), B * K))
    finally:
        h.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_launch():
    torch, dev = _torch()
    B, K = 8, 6
    m, st, tm, prog, offsets, state, base, lim = _squat_case("talos", B, capi.F64, dev, torch)
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        out, ext, trace = _bufs(st, m, B, K, torch.float64, dev, torch)

        def untouched():
            torch.cuda.synchronize()
            return (out["status"].eq(-99).all().item() and torch.isnan(out["x"]).all().item() and torch.isnan(ext["q_next"]).all().item()
                    and trace["status"].eq(-99).all().item() and ext["iters_sum"].eq(-7).all().item())

        def call(p, **kw):
            h.rollout_program(0, B, 0, K, p, base, offsets, state, lim, out, ext["q_next"], ext["v_next"], tm.dt, trace=trace, stride=kw.get("stride", 1),
                              iters_sum=ext["iters_sum"], ticks_ok=ext["ticks_ok"])

        short = refprog.move_com_program(tm.nref - 1, 0, m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0)
        for p, kw, needle in ((short, {}, "nref"), (prog, dict(stride=0), "stride")):
            with pytest.raises(capi.WbcqpError) as e:
                call(p, **kw)
            assert e.value.code == 1 and needle in str(e.value), str(e.value)
            assert untouched()
        overlap = refprog.move_com_program(tm.nref, 192, m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0)
        overlap.add_vec(195, [(np.zeros(3), np.zeros(3), 4.0)])
        with pytest.raises(capi.WbcqpError) as e:
            call(overlap)
        assert e.value.code == 1 and "overlaps track 0" in str(e.value) and untouched()
        with pytest.raises(capi.WbcqpError) as e:
            h.reference_samples(overlap, base, offsets, 0, K, torch.zeros(K, B, tm.nref, dtype=torch.float64, device=dev))
        assert e.value.code == 1
        call(prog)  # and the call itself goes through
        torch.cuda.synchronize()
        assert out["status"].ne(-99).all().item() and ext["ticks_ok"].sum().item() > 0
    finally:
        h.close()
    # the mixed call: nref mismatch, no set_of, a set_of entry >= n_slots
    h, m, sets, slots, plan, full, state, w, tlb, tub = _mixed_case(B, K, dev, torch)
    try:
        good = refprog.walk_on_spot_program(plan)
        base = torch.from_numpy(plan.base).to(dev)
        offsets = np.arange(B)
        no_set = refprog.walk_on_spot_program(plan)
        no_set.set_of = None
        bad_set = refprog.walk_on_spot_program(plan)
        bad_set.set_of = bad_set.set_of.copy()
        bad_set.set_of[60] = 3
        wrong = refprog.Program(plan.nref + 1, plan.dt, 50, 180, set_of=plan.set_of)
        for p, needle in ((wrong, "nref"), (no_set, "set_of"), (bad_set, "set_of[60] = 3")):
            ldx = max(st.n for st, _ in sets.values())
            ro, re = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=np.nan)
            b = base if p is not wrong else torch.zeros(plan.nref + 1, dtype=torch.float64, device=dev)
            with pytest.raises(capi.WbcqpError) as e:
                h.rollout_mixed_program(slots, B, 0, K, p, b, offsets, state, w, ro, re["q_next"], re["v_next"], full.dt, tlb=tlb, tub=tub)
            assert e.value.code == 1 and needle in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert ro["status"].eq(-99).all().item() and torch.isnan(ro["x"]).all().item() and torch.isnan(re["q_next"]).all().item()
        ro, re = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=np.nan)
        h.rollout_mixed_program(slots, B, 0, K, good, base, offsets, state, w, ro, re["q_next"], re["v_next"], full.dt, tlb=tlb, tub=tub)
        torch.cuda.synchronize()
        assert ro["status"].ne(-99).all().item()
    finally:
        h.close()
