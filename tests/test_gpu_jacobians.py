"""Differential kinematics on the device (wbcqp_set_jacobian_frames, wbcqp_jacobians; csrc/wbcqp_jacobians.hpp): frame Jacobians in the three
reference frames, the CoM Jacobian, the centroidal momentum matrix and the two drift terms, against oracle/rbd_oracle.c (rbd_terms' Jl, Jw, Jcom, Ag,
dAgv, af) through the C ABI, and against the library's other kernels through the identities that tie them together.

Bar: TOL_ROWS (1e-10, tests/test_gpu_observe.py, test_gpu_terms.py: two formulations in double -- one world frame and leaf-to-root composites on the
device, pinocchio-style local recursions and per-body sums in the oracle), relative to max(1, the array's largest entry); an F32 handle is held to
the F64 result rounded to float.  The oracle has no LOCAL_WORLD_ALIGNED Jacobian: the reference there is blockdiag(R, R) Jl and R af with R from the oracle's oMf
(tests/test_jacobians_host.py: reference).
The shapes are the ones at which the kernel can go wrong: one body (nv = 1), the lane limit (64 bodies fixed; 59 bodies floating = nv 64), a pure
chain (every doubling round), a star, Talos; batches that are no multiple of the four instances of a workgroup; no frame, one, all 64 slots."""
import ctypes as C
import functools

import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import jacobians as jac
from inria_wbc_amd import model as mdl
from inria_wbc_amd import observe as obs
from tests import model_queries as mq
from tests.model_queries import BATCHES, _torch
from tests.test_forward_dynamics_host import CASES, case_states
from tests.test_jacobians_host import SHAPES, oracle_terms, reference, selections

pytestmark = pytest.mark.gpu

TOL_ROWS = 1e-10
NMAX = max(BATCHES)
FIELDS = capi.JACOBIAN_OUTPUTS
RFS = {"WORLD": capi.RF_WORLD, "LOCAL": capi.RF_LOCAL, "LOCAL_WORLD_ALIGNED": capi.RF_LOCAL_WORLD_ALIGNED}


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


def _set(handle, name, slot=3):
    m, st, tm = CASES[name]()
    handle.set_structure(slot, st)
    handle.set_model(slot, m, tm)
    return m, st, tm


def _shape(k, B, nf, nv):
    return {"J": (B, nf, 6, nv), "Jcom": (B, 3, nv), "Ag": (B, 6, nv), "drift": (B, nf, 6), "dAgv": (B, 6)}[k]


def _admitted(nf, rf, v=True):
    """The outputs a call with nf selected frames, the convention rf and (without) v admits."""
    return tuple(k for k in FIELDS if (k not in ("J", "drift") or nf) and (k not in ("drift", "dAgv") or v) and (k != "drift" or rf != capi.RF_WORLD))


def _jac(h, slot, B, nf, nv, q, v, rf, dev, torch, which=None, td=None):
    """One launch on device tensors -> {name: numpy array}; every element that must be written is finite, nothing behind the end is touched.
    v None: passed as NULL."""
    td = td or torch.float64
    which = _admitted(nf, rf, v is not None) if which is None else which
    bufs = {k: mq.guarded(int(np.prod(_shape(k, B, nf, nv))), td, dev, torch) for k in which}
    h.jacobians(slot, B, q[:B].contiguous(), None if v is None else v[:B].contiguous(), rf, stream=torch.cuda.current_stream().cuda_stream,
                **{k: part for k, (_, part) in bufs.items()})
    torch.cuda.synchronize()
    return {k: mq.read_guarded(whole, part.numel(), k).reshape(_shape(k, B, nf, nv)) for k, (whole, part) in bufs.items()}


def _rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


def _want(terms, frames, rf):
    """The oracle's answer for a selection, in wbcqp_jacobians' names and shapes."""
    J, drift = reference(terms, frames, rf)
    out = {"J": J, "Jcom": terms["Jcom"], "Ag": terms["Ag"], "dAgv": terms["dAgv"]}
    if drift is not None:
        out["drift"] = drift
    return out


@pytest.mark.parametrize("name", SHAPES)
def test_jacobians_parity(handle, name):
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    nv = m.nv
    qn, vn, _ = case_states(m, tm, NMAX, 81_000)
    terms = oracle_terms(m, qn, vn)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    body, sup = jac.dof_bodies(m), jac.supports(m)
    worst = {k: 0.0 for k in FIELDS}
    for sel, frames in selections(m).items():
        handle.set_jacobian_frames(3, frames)
        nf = len(frames)
        for rfname, rf in RFS.items():
            want = _want(terms, frames, rf) if nf else {k: terms[k] for k in ("Jcom", "Ag", "dAgv")}
            big = _jac(handle, 3, NMAX, nf, nv, q, v, rf, dev, torch)
            assert set(big) == set(want), (name, sel, rfname)
            for k in big:
                e = _rel(big[k], want[k])
                worst[k] = max(worst[k], e)
                assert e <= TOL_ROWS, (name, sel, rfname, k, e)
            for B in BATCHES[:-1]:  # the same rows in a smaller batch: the same bits
                got = _jac(handle, 3, B, nf, nv, q, v, rf, dev, torch)
                for k in got:
                    assert np.array_equal(got[k], big[k][:B]), (name, sel, rfname, B, k)
            # the columns of dofs that do not move the frame's body: +0.0, bit for bit
            for k, f in enumerate(frames):
                off = big["J"][:, k][:, :, ~sup[body, m.frame_body[f]]]
                assert (off == 0.0).all() and not np.signbit(off).any(), (name, sel, rfname, f)
    print("jacobians parity, worst per array, %-26s %s" % (name, "  ".join("%s %.1e" % (k, worst[k]) for k in FIELDS)))
    if name in ("star_17_floating", "talos"):
        assert (~sup[body][:, m.frame_body]).any()  # (the zero-column check had something to look at)


@pytest.mark.parametrize("name", ["talos", "tree_59_floating_nv_limit", "chain_62"])
def test_identities_across_kernels(handle, name):
    """What ties the matrices to the library's other answers on the same states: J_local v = wbcqp_observe's velocity, Jcom v = vcom, Ag v = the
    rows kernel's momentum (Talos: the shipped stack carries the states' references), J_world = Ad(oMf) J_local with wbcqp_observe's placement,
    and tau(0) - tau(w) = J_local' w through wbcqp_inverse_dynamics with v = a = NULL."""
    m, st, tm = _set(handle, name)
    nv = m.nv
    n = 24
    s = mdl.sample_states(m, tm, n, 82_000, q_noise=0.2, v_noise=0.5, ref_noise=0.01)
    qn, vn = s["q"], s["v"]
    frames = selections(m)["sixty_four_with_repeats"][:6] + [0, 1]
    handle.set_jacobian_frames(3, frames)
    handle.set_observed_frames(3, frames)
    handle.set_wrench_frames(3, frames)
    seen = handle.observe_host(3, qn, vn)
    local = handle.jacobians_host(3, qn, vn, capi.RF_LOCAL)
    world = handle.jacobians_host(3, qn, None, capi.RF_WORLD, which=["J"])["J"]
    errs = {"J_local v = velocity": _rel(np.einsum("nfij,nj->nfi", local["J"], vn), seen["velocity"]),
            "Jcom v = vcom": _rel(np.einsum("nij,nj->ni", local["Jcom"], vn), seen["vcom"])}
    if name == "talos":
        mom = handle.problem_data_host(3, qn, vn, s["ref"])["momentum"]
        errs["Ag v = momentum"] = _rel(np.einsum("nij,nj->ni", local["Ag"], vn), mom)
    R, p = seen["placement"][:, :, :9].reshape(n, len(frames), 3, 3), seen["placement"][:, :, 9:]
    lin, ang = np.einsum("nfij,nfjk->nfik", R, local["J"][:, :, :3]), np.einsum("nfij,nfjk->nfik", R, local["J"][:, :, 3:])
    ad = np.concatenate([lin + np.cross(p[:, :, :, None], ang, axis=2), ang], axis=2)
    errs["J_world = Ad(oMf) J_local"] = _rel(world, ad)
    w = 50.0 * np.random.default_rng(82_500).standard_normal((n, len(frames), 6))
    diff = handle.inverse_dynamics_host(3, qn) - handle.inverse_dynamics_host(3, qn, wrench=w)
    errs["tau(0) - tau(w) = J_local' w"] = _rel(diff, np.einsum("nfij,nfi->nj", local["J"], w))
    print("identities across kernels, %-26s %s" % (name, "  ".join("%s %.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL_ROWS, errs


def test_each_output_is_optional_and_independent(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "talos")
    nv = m.nv
    frames = obs.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "base_link", "head_2_joint", "leg_left_6_joint"])
    handle.set_jacobian_frames(3, frames)
    nf, B = len(frames), 7
    qn, vn, _ = case_states(m, tm, B, 83_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    rf = capi.RF_LOCAL_WORLD_ALIGNED
    full = _jac(handle, 3, B, nf, nv, q, v, rf, dev, torch)
    assert set(full) == set(FIELDS)
    for left_out in FIELDS:  # (_jac: what is asked for is written whole, nothing behind a buffer's end is touched)
        which = tuple(k for k in FIELDS if k != left_out)
        got = _jac(handle, 3, B, nf, nv, q, v, rf, dev, torch, which=which)
        for k in which:
            assert np.array_equal(got[k], full[k]), (left_out, k)
    for k in FIELDS:  # one at a time
        assert np.array_equal(_jac(handle, 3, B, nf, nv, q, v, rf, dev, torch, which=(k,))[k], full[k]), k
    # J, Jcom and Ag need no v: with v NULL the bits of the call with v
    for which in (("J", "Jcom", "Ag"), ("J",), ("Jcom",), ("Ag",)):
        got = _jac(handle, 3, B, nf, nv, q, None, rf, dev, torch, which=which)
        for k in which:
            assert np.array_equal(got[k], full[k]), ("v NULL", k)
    assert np.array_equal(full["J"][:, 0], full["J"][:, 4]) and np.array_equal(full["drift"][:, 0], full["drift"][:, 4])  # a repeated frame
    assert _rel(full["Jcom"], full["Ag"][:, :3] / m.inertia[:, 0].sum()) <= TOL_ROWS  # Jcom: Ag's linear rows over the total mass
    # Jcom, Ag and dAgv do not depend on the convention, nor on the selection
    handle.set_jacobian_frames(3, [])
    for rf2 in RFS.values():
        got = _jac(handle, 3, B, 0, nv, q, v, rf2, dev, torch)
        assert set(got) == {"Jcom", "Ag", "dAgv"}
        for k in got:
            assert np.array_equal(got[k], full[k]), k
    handle.set_jacobian_frames(3, frames)
    host = handle.jacobians_host(3, qn, vn, rf)
    for k in FIELDS:
        assert np.array_equal(host[k], full[k]), k


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "tree_24_floating")
    frames = list(range(0, m.nframe, 2))
    handle.set_jacobian_frames(3, frames)
    qn, vn, _ = case_states(m, tm, NMAX, 84_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(
        lambda lo, hi: _jac(handle, 3, hi - lo, len(frames), m.nv, q[lo:hi], v[lo:hi], capi.RF_LOCAL, dev, torch), NMAX)
    assert set(a) == set(FIELDS)


def test_f32_handle_rounds_the_f64_result(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "talos")
    frames = obs.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "head_2_joint"])
    qn, vn, _ = case_states(m, tm, 9, 85_000)
    q32, v32 = qn.astype(np.float32), vn.astype(np.float32)
    handle.set_jacobian_frames(3, frames)
    h32 = capi.Handle(0, capi.F32)
    try:
        h32.set_structure(0, st)
        h32.set_model(0, m, tm)
        h32.set_jacobian_frames(0, frames)
        for rf in RFS.values():
            want = handle.jacobians_host(3, q32.astype(np.float64), v32.astype(np.float64), rf)
            got = _jac(h32, 0, 9, len(frames), m.nv, torch.from_numpy(q32).to(dev), torch.from_numpy(v32).to(dev), rf, dev, torch, td=torch.float32)
            host = h32.jacobians_host(0, q32, v32, rf)
            assert set(got) == set(want) == set(host)
            for k in got:
                assert got[k].dtype == np.float32 and np.array_equal(got[k], host[k]), k
                ulp = float(np.spacing(np.float32(np.abs(want[k]).max())))
                assert np.abs(got[k].astype(np.float64) - want[k].astype(np.float32).astype(np.float64)).max() <= ulp, (k, ulp)
    finally:
        h32.close()


def test_a_traced_squat_in_one_call():
    """The q / v arrays of a trace pass as they are, as [n_rec * batch] rows: one call answers every recorded tick, bit for bit what tick-by-tick
    calls give, and the oracle agrees on the recorded states."""
    torch, dev = _torch()
    B, K, stride = 8, 12, 3
    n_rec = K // stride
    names = ["leg_left_6_joint", "leg_right_6_joint", "gripper_left_joint", "base_link"]
    h, m, _, _, trace, _, _ = mq.traced_squat(B, K, stride, lambda h, m, tm: h.set_jacobian_frames(0, obs.frame_ids(m, names)))
    try:
        frames, nv = obs.frame_ids(m, names), m.nv
        trq, trv = trace["q"], trace["v"]
        whole = _jac(h, 0, n_rec * B, len(frames), nv, trq.reshape(n_rec * B, -1), trv.reshape(n_rec * B, -1), capi.RF_LOCAL, dev, torch)
        for r in range(n_rec):
            tick = _jac(h, 0, B, len(frames), nv, trq[r], trv[r], capi.RF_LOCAL, dev, torch)
            for k in FIELDS:
                assert np.array_equal(whole[k][r * B:(r + 1) * B], tick[k]), (k, r)
        qs, vs = trq.reshape(n_rec * B, -1).cpu().numpy(), trv.reshape(n_rec * B, -1).cpu().numpy()
        assert np.isfinite(qs).all() and np.isfinite(vs).all() and np.abs(qs[:B] - qs[-B:]).max() > 0  # recorded, and the robots moved
        want = _want(oracle_terms(m, qs, vs), frames, capi.RF_LOCAL)
        w = {k: _rel(whole[k], want[k]) for k in FIELDS}
        print("jacobians over a traced squat (4 x 8 states) against the oracle: %s" % {k: "%.1e" % e for k, e in w.items()})
        assert max(w.values()) <= TOL_ROWS, w
    finally:
        h.close()


def test_refusals_come_before_any_launch():
    torch, dev = _torch()
    m, st, tm = CASES["talos"]()
    h = capi.Handle(0, capi.F64)
    try:
        B, nf, nv = 4, 2, m.nv
        qn, vn, _ = case_states(m, tm, B, 86_000)
        q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
        bufs = {k: mq.guarded(int(np.prod(_shape(k, B, nf, nv))), torch.float64, dev, torch) for k in FIELDS}
        part = {k: b[1] for k, b in bufs.items()}
        refused = functools.partial(mq.refused, h)

        def raw_set(slot, n, arr):
            h._check(h.lib.wbcqp_set_jacobian_frames(h._h, slot, n, arr.ctypes.data_as(capi.c_i32_p) if arr is not None else None))

        def ask(slot, batch, qq, vv, rf, *ks):
            h.jacobians(slot, batch, qq, vv, rf, **{k: part[k] for k in ks})

        # a slot without a model: no structure at all, then a structure alone
        refused(lambda: h.set_jacobian_frames(9, [0]))
        refused(lambda: ask(9, B, q, v, capi.RF_LOCAL, "Jcom"))
        h.set_structure(0, st)
        refused(lambda: h.set_jacobian_frames(0, [0]))
        refused(lambda: ask(0, B, q, v, capi.RF_LOCAL, "Jcom"))
        h.set_model(0, m, tm)
        # J / drift while no frames are selected (never selected, and an empty selection); the observed and the wrench frames are other selections
        assert "no frames" in refused(lambda: ask(0, B, q, v, capi.RF_LOCAL, "J"))
        h.set_jacobian_frames(0, [])
        h.set_observed_frames(0, [3, 5])
        h.set_wrench_frames(0, [3, 5])
        assert "no frames" in refused(lambda: ask(0, B, q, v, capi.RF_LOCAL, "drift"))
        # frame indices outside the model, n_frames outside 0 .. 64, frames NULL
        refused(lambda: h.set_jacobian_frames(0, [0, m.nframe]))
        refused(lambda: h.set_jacobian_frames(0, [-1]))
        refused(lambda: raw_set(0, 65, np.zeros(65, np.int32)))
        refused(lambda: raw_set(0, -1, np.zeros(1, np.int32)))
        refused(lambda: raw_set(0, 2, None))
        h.set_jacobian_frames(0, [3, 5])
        # drift / dAgv without v; drift in WORLD; an unknown reference frame; every output NULL; a negative batch; q NULL
        assert "v is NULL" in refused(lambda: ask(0, B, q, None, capi.RF_LOCAL, "J", "drift"))
        assert "v is NULL" in refused(lambda: ask(0, B, q, None, capi.RF_LOCAL, "Jcom", "dAgv"))
        assert "WORLD" in refused(lambda: ask(0, B, q, v, capi.RF_WORLD, "J", "drift"))
        assert "reference_frame" in refused(lambda: ask(0, B, q, v, 3, "J"))
        assert "reference_frame" in refused(lambda: ask(0, B, q, v, -1, "Jcom"))
        assert "every output" in refused(lambda: ask(0, B, q, v, capi.RF_LOCAL))
        refused(lambda: ask(0, -1, q, v, capi.RF_LOCAL, *FIELDS))
        refused(lambda: ask(0, B, None, v, capi.RF_LOCAL, "Jcom"))
        refused(lambda: h._check(h.lib.wbcqp_jacobians(h._h, 0, B, q.data_ptr(), v.data_ptr(), capi.RF_LOCAL, None, None)))  # the struct itself NULL
        ask(0, 0, q, v, capi.RF_LOCAL, *FIELDS)  # batch == 0: WBCQP_OK, nothing launched
        torch.cuda.synchronize()
        for k, (whole, _) in bufs.items():
            assert mq.unwritten(whole.cpu().numpy()).all(), (k, "a refused call wrote something")
        got = _jac(h, 0, B, nf, nv, q, v, capi.RF_LOCAL, dev, torch)  # and the selection [3, 5] still stands
        want = jac.jacobians(m, qn, vn, [3, 5], jac.LOCAL)
        assert max(_rel(got[k], want[k]) for k in FIELDS) <= TOL_ROWS
    finally:
        h.close()


def _talos_both(handle, seed, B=4, nf=2):
    """Talos on slot 3 of the module's handle; B states and prefilled outputs for nf frames, each as a (device, host) pair."""
    m, st, tm = _set(handle, "talos")
    qn, vn, _ = case_states(m, tm, B, seed)
    out = {k: mq.prefilled_both(int(np.prod(_shape(k, B, nf, m.nv)))) for k in FIELDS}
    return m, mq.both(qn), mq.both(vn), out, lambda *ks: mq.Out(capi.CJacobianOutputs, **{k: out[k] for k in ks})


def test_a_refused_selection_keeps_the_one_before(handle):
    m, (_, qn), (_, vn), _, _ = _talos_both(handle, 87_100)

    def still_stands(frames):
        got = handle.jacobians_host(3, qn, vn, capi.RF_LOCAL)
        want = jac.jacobians(m, qn, vn, frames, jac.LOCAL)
        assert got["J"].shape == (4, len(frames), 6, m.nv) and max(_rel(got[k], want[k]) for k in FIELDS) <= TOL_ROWS

    mq.a_refused_selection_keeps_the_one_before(handle, "jacobian", m.nframe, 64, still_stands)


def test_host_refusals_are_the_device_refusals(handle):
    _, q, v, out, O = _talos_both(handle, 87_200)  # (no frames are selected)
    L, W = capi.RF_LOCAL, capi.RF_WORLD
    mq.host_refusals_match(handle, "jacobians", [(3, 4, q, v, L, O("J")),        # J asked for with no frames selected
                                                 (3, 4, q, v, L, O("drift"))],   # drift likewise
                           out.values())
    handle.set_jacobian_frames(3, [3, 5])
    mq.host_refusals_match(handle, "jacobians", [(9, 4, q, v, L, O("Jcom")),             # a slot without a model
                                                 (3, -1, q, v, L, O("Jcom")),            # a negative batch
                                                 (3, 4, q, None, L, O("J", "drift")),    # drift with v NULL
                                                 (3, 4, q, None, L, O("Ag", "dAgv")),    # dAgv with v NULL
                                                 (3, 4, q, v, W, O("J", "drift")),       # drift in WORLD
                                                 (3, 4, q, v, 3, O("J")),                # an unknown reference frame
                                                 (3, 4, q, v, -1, O("Jcom")),
                                                 (3, 4, q, v, L, O()),                   # every output NULL
                                                 (3, 4, q, v, L, None),                  # the struct itself NULL
                                                 (3, 4, None, v, L, O("Jcom"))],         # q NULL
                           out.values())


def test_batch_zero_through_the_host_entry_point(handle):
    _, q, v, out, O = _talos_both(handle, 87_300)
    handle.set_jacobian_frames(3, [3, 5])
    mq.host_batch_zero(handle, "jacobians", [(3, 0, q, v, capi.RF_LOCAL, O(*FIELDS)), (3, 0, None, v, capi.RF_LOCAL, O(*FIELDS))], out.values())  # (q is not looked at)
    mq.raw(handle, "jacobians", 0, 3, 0, q, v, capi.RF_LOCAL, O(*FIELDS))
    _torch()[0].cuda.synchronize()
    for dev_side, _ in out.values():
        assert mq.unwritten(dev_side.cpu().numpy()).all()


def test_set_structure_and_set_model_drop_the_selection():
    torch, dev = _torch()
    m, st, tm = CASES["franka"]()
    h = capi.Handle(0, capi.F64)
    try:
        qn, vn, _ = case_states(m, tm, 3, 88_000)
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_jacobian_frames(0, [1, 2])
        assert h.jacobians_host(0, qn, vn)["J"].shape == (3, 2, 6, m.nv)

        def and_then():
            assert set(h.jacobians_host(0, qn, vn)) == {"Jcom", "Ag", "dAgv"}  # these need no selection
            h.set_jacobian_frames(0, [1, 2])

        mq.set_structure_and_set_model_drop(h, (m, st, tm), lambda: torch.full((3 * 2 * 6 * m.nv,), float("nan"), dtype=torch.float64, device=dev),
                                            lambda buf: h.jacobians(0, 3, torch.from_numpy(qn).to(dev), None, capi.RF_LOCAL, J=buf), "no frames", and_then)
    finally:
        h.close()


def test_nothing_else_moves(handle):
    def query(s, tick):
        handle.set_jacobian_frames(3, list(range(40)))
        for rf in RFS.values():
            handle.jacobians_host(3, s["q"], s["v"], rf)

    mq.nothing_else_moves(handle, mq.talos_case(), 89_000, query, observed=[1, 4, 9])
