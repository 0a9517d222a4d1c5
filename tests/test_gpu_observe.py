"""Observables on the device (wbcqp_observe, csrc/wbcqp_observe.hpp): centre of mass, its velocity, world placements and local velocities
of chosen model frames from (q, v), against oracle/rbd_oracle.c through the C ABI.

Bar: TOL_ROWS of tests/test_gpu_terms.py (two formulations in double: ancestor doubling in the world frame on the device, pinocchio-style
local recursions in the oracle), relative to max(1, the array's largest entry).  The shapes are the ones at which the kernel can go wrong:
one body, the lane limit, a pure chain (every doubling round), batches that are no multiple of the four instances of a workgroup.

One case differs from what one would write down first.  A floating tree of 64 bodies has nv = 69, and wbcqp_set_structure refuses
nv > 64 (the dv block's 64 x 64 register grid), so no slot can hold it: the lane limit is tested on a FIXED tree of 64 bodies and the
floating base at its own limit, 59 bodies (nv = 64)."""
import ctypes as C
import functools

import numpy as np
import pytest

from inria_wbc_amd import capi, structure
from inria_wbc_amd import model as mdl
from inria_wbc_amd import observe as obs
from tests import model_queries as mq
from tests.model_queries import BATCHES, _torch

pytestmark = pytest.mark.gpu

TOL_ROWS = 1e-10
NMAX = max(BATCHES)
FIELDS = capi.OBSERVABLES
WIDTH = {"com": 3, "vcom": 3, "placement": 12, "velocity": 6}


def _tree(seed, nb, fb, chain=False):
    return mq.tree_case("observe_", seed, nb, fb, "chain" if chain else None)


CASES = {"talos": mq.talos_case,
         "icub": mq.shipped_case(mdl.icub_like, structure.icub_structure, mdl.icub_stack),
         "franka": mq.shipped_case(mdl.franka_like, structure.franka_structure, mdl.franka_stack),
         "tree_one_body": _tree(51, 1, False), "tree_30_floating": _tree(52, 30, True), "tree_62_fixed": _tree(53, 62, False),
         "tree_64_fixed_lane_limit": _tree(54, 64, False), "tree_59_floating_nv_limit": _tree(55, 59, True), "chain_62": _tree(56, 62, False, chain=True)}


def _states(m, tm, n, seed):
    s = mdl.sample_states(m, tm, n, seed, q_noise=0.3, v_noise=0.5)  # the noise tests/test_gpu_terms.py uses for trees
    return s["q"], s["v"]


def _selections(m):
    """none (CoM only), one frame, all 64 slots with repeats, a frame on body 0 and one on the last body."""
    nb = m.nbody
    on0 = int(np.nonzero(m.frame_body == 0)[0][0])
    onlast = int(np.nonzero(m.frame_body == nb - 1)[0][0])
    return {"none": [], "one": [m.nframe // 2], "all_64_slots": np.random.default_rng(7).integers(0, m.nframe, 64).tolist(), "first_and_last_body": [on0, onlast]}


def _oracle(m, q, v):
    """com, vcom, placement, velocity of EVERY frame of the model for the states q, v, in wbcqp_observe's names and shapes."""
    from oracle import rbd
    om = rbd.OracleModel(m)
    ts = [rbd.rbd_terms(om, q[i], v[i]) for i in range(q.shape[0])]
    return {"com": np.stack([t["com"] for t in ts]), "vcom": np.stack([t["vcom"] for t in ts]),
            "placement": np.stack([t["oMf"] for t in ts]), "velocity": np.stack([t["vf"] for t in ts])}


def _pick(ora, frames):
    return {k: (a if k in ("com", "vcom") else a[:, frames]) for k, a in ora.items()}


def _bufs(B, nf, td, dev, torch, which=FIELDS):
    """NaN-filled output buffers with GUARD elements behind each: {name: (whole buffer, the part wbcqp_observe may write)}."""
    return {k: mq.guarded(B * WIDTH[k] * (1 if k in ("com", "vcom") else nf), td, dev, torch) for k in which}


def _observe(h, slot, B, nf, q, v, dev, torch, which=FIELDS, td=None):
    """One launch on device tensors -> {name: numpy array}; every element that must be written is finite, nothing behind the end is touched."""
    td = td or torch.float64
    bufs = _bufs(B, nf, td, dev, torch, which)
    kw = {k: (bufs[k][1] if k in bufs and bufs[k][1].numel() else None) for k in FIELDS}
    need_v = "vcom" in which or ("velocity" in which and nf)
    h.observe(slot, B, q[:B].contiguous(), v[:B].contiguous() if need_v else None, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return {k: mq.read_guarded(whole, part.numel(), k).reshape((B, 3) if k in ("com", "vcom") else (B, nf, WIDTH[k])) for k, (whole, part) in bufs.items()}


def _worst(got, want):
    return {k: float(np.abs(got[k] - want[k]).max() / max(1.0, np.abs(want[k]).max())) if want[k].size else 0.0 for k in got}


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


@pytest.mark.parametrize("name", list(CASES))
def test_observe_parity(handle, name):
    torch, dev = _torch()
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    qn, vn = _states(m, tm, NMAX, 71_000)
    ora = _oracle(m, qn, vn)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    worst = {k: 0.0 for k in FIELDS}
    for sel, frames in _selections(m).items():
        handle.set_observed_frames(3, frames)
        want = _pick(ora, frames)
        big = None
        for B in BATCHES[::-1]:
            got = _observe(handle, 3, B, len(frames), q, v, dev, torch)
            w = _worst(got, {k: a[:B] for k, a in want.items()})
            worst = {k: max(worst[k], w[k]) for k in FIELDS}
            assert max(w.values()) <= TOL_ROWS, (name, sel, B, w)
            if big is None:
                big = got
            for k in FIELDS:  # the same rows in a smaller batch: the same bits
                assert np.array_equal(got[k], big[k][:B]), (name, sel, B, k)
    print("observe parity, worst per array, %-26s %s" % (name, "  ".join("%s %.1e" % (k, worst[k]) for k in FIELDS)))


def test_each_output_is_optional_and_independent(handle):
    torch, dev = _torch()
    m, st, tm = CASES["talos"]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    frames = obs.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "base_link", "head_2_joint", "leg_left_6_joint"])
    handle.set_observed_frames(3, frames)
    B = 7
    qn, vn = _states(m, tm, B, 72_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    full = _observe(handle, 3, B, len(frames), q, v, dev, torch)
    for left_out in FIELDS:
        which = tuple(k for k in FIELDS if k != left_out)
        got = _observe(handle, 3, B, len(frames), q, v, dev, torch, which=which)
        for k in which:
            assert np.array_equal(got[k], full[k]), (left_out, k)
    for k in FIELDS:  # one at a time
        assert np.array_equal(_observe(handle, 3, B, len(frames), q, v, dev, torch, which=(k,))[k], full[k]), k
    # positions alone need no v
    got = _observe(handle, 3, B, len(frames), q, v, dev, torch, which=("com", "placement"))
    assert np.array_equal(got["com"], full["com"]) and np.array_equal(got["placement"], full["placement"])
    assert np.array_equal(full["placement"][:, 0], full["placement"][:, 4])  # a repeated frame
    host = handle.observe_host(3, qn, vn)
    for k in FIELDS:
        assert np.array_equal(host[k], full[k]), k


def test_vcom_is_the_rows_kernels_momentum_over_the_mass(handle):
    m, st, tm = CASES["talos"]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    s = mdl.sample_states(m, tm, 24, 73_000, q_noise=0.2, v_noise=0.5)
    mom = handle.problem_data_host(3, s["q"], s["v"], s["ref"])["momentum"]
    got = handle.observe_host(3, s["q"], s["v"])
    want = mom[:, :3] / m.inertia[:, 0].sum()
    err = np.abs(got["vcom"] - want).max() / max(1.0, np.abs(want).max())
    print("vcom against momentum[:3] / mass: %.1e" % err)
    assert err <= TOL_ROWS


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    m, st, tm = CASES["icub"]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    frames = list(range(0, m.nframe, 3))
    handle.set_observed_frames(3, frames)
    qn, vn = _states(m, tm, NMAX, 74_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(lambda lo, hi: _observe(handle, 3, hi - lo, len(frames), q[lo:hi], v[lo:hi], dev, torch), NMAX)
    assert set(a) == set(FIELDS)


def _trace_checks(h, slots, m, frames, trq, trv, B, n_rec, dev, torch):
    """observe over the trace arrays in one call == one call per recorded tick, through every slot given; and the oracle on the states."""
    nf = len(frames)
    whole = [_observe(h, s, n_rec * B, nf, trq.reshape(n_rec * B, -1), trv.reshape(n_rec * B, -1), dev, torch) for s in slots]
    for k in FIELDS:
        for other in whole[1:]:
            assert np.array_equal(whole[0][k], other[k]), ("through another slot of the mix", k)
        for r in range(n_rec):
            tick = _observe(h, slots[0], B, nf, trq[r], trv[r], dev, torch)
            assert np.array_equal(whole[0][k][r * B:(r + 1) * B], tick[k]), (k, r)
    qs, vs = trq.reshape(n_rec * B, -1).cpu().numpy(), trv.reshape(n_rec * B, -1).cpu().numpy()
    assert np.isfinite(qs).all() and np.isfinite(vs).all() and np.abs(qs[:B] - qs[-B:]).max() > 0  # recorded, and the robots moved
    w = _worst(whole[0], _pick(_oracle(m, qs, vs), frames))
    assert max(w.values()) <= TOL_ROWS, w
    return w


def test_observe_over_a_trace():
    torch, dev = _torch()
    B, K, stride = 8, 12, 3
    names = ["leg_left_6_joint", "leg_right_6_joint", "gripper_left_joint", "gripper_right_joint", "base_link"]
    h, m, _, _, trace, _, _ = mq.traced_squat(B, K, stride, lambda h, m, tm: h.set_observed_frames(0, obs.frame_ids(m, names)))
    try:
        w = _trace_checks(h, [0], m, obs.frame_ids(m, names), trace["q"], trace["v"], B, K // stride, dev, torch)
        print("observe over a traced roll-out (4 x 8 states) against the oracle: %s" % {k: "%.1e" % e for k, e in w.items()})
    finally:
        h.close()


def test_observe_over_a_mixed_trace_through_either_slot():
    from tests.test_gpu_mixed_contacts import _fleet, _inputs, _outputs
    torch, dev = _torch()
    B, K, stride = 8, 12, 3
    n_rec = K // stride
    h, m, sets, slots = _fleet("talos")
    try:
        sets2 = dict(list(sets.items())[:2])  # two contact sets: both feet, no left foot
        slots2 = slots[:2]
        frames = obs.frame_ids(m, ["leg_left_6_joint", "leg_right_6_joint", "base_link"])
        for s in slots2:
            h.set_observed_frames(s, frames)
        state, w, tlb, tub = _inputs(m, sets2, B, 75_000, capi.F64, dev, torch)
        sch = np.random.default_rng(5).integers(0, 2, (K, B)).astype(np.int32)
        ref = state["ref"].unsqueeze(0).repeat(K, 1, 1).contiguous()
        ldx = max(st.n for st, _ in sets2.values())
        ro, re = _outputs(B, ldx, m.na, m.nq, m.nv, capi.F64, dev, torch, fill=np.nan)
        f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
        trace = dict(q=f(n_rec, B, m.nq), v=f(n_rec, B, m.nv))
        h.rollout_mixed_traced(slots2, sch, dict(q=state["q"], v=state["v"], ref=ref), w, ro, re["q_next"], re["v_next"], next(iter(sets2.values()))[1].dt,
                               trace=trace, stride=stride, tlb=tlb, tub=tub, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _trace_checks(h, slots2, m, frames, trace["q"], trace["v"], B, n_rec, dev, torch)
    finally:
        h.close()


def test_f32_handle_rounds_the_f64_result(handle):
    torch, dev = _torch()
    m, st, tm = CASES["talos"]()
    frames = obs.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "head_2_joint"])
    qn, vn = _states(m, tm, 9, 76_000)
    q32, v32 = qn.astype(np.float32), vn.astype(np.float32)
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    handle.set_observed_frames(3, frames)
    want = handle.observe_host(3, q32.astype(np.float64), v32.astype(np.float64))
    h32 = capi.Handle(0, capi.F32)
    try:
        h32.set_structure(0, st)
        h32.set_model(0, m, tm)
        h32.set_observed_frames(0, frames)
        got = _observe(h32, 0, 9, len(frames), torch.from_numpy(q32).to(dev), torch.from_numpy(v32).to(dev), dev, torch, td=torch.float32)
        host = h32.observe_host(0, q32, v32)
    finally:
        h32.close()
    for k in FIELDS:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], host[k]), k
        ulp = float(np.spacing(np.float32(np.abs(want[k]).max())))
        assert np.abs(got[k].astype(np.float64) - want[k].astype(np.float32).astype(np.float64)).max() <= ulp, (k, ulp)


def test_nothing_else_moves(handle):
    def query(s, tick):
        handle.set_observed_frames(3, list(range(40)))
        handle.observe_host(3, s["q"], s["v"])

    mq.nothing_else_moves(handle, CASES["talos"](), 77_000, query)


def test_refusals_come_before_any_launch():
    torch, dev = _torch()
    m, st, tm = CASES["talos"]()
    h = capi.Handle(0, capi.F64)
    try:
        B, nf = 4, 2
        qn, vn = _states(m, tm, B, 78_000)
        q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
        bufs = _bufs(B, nf, torch.float64, dev, torch)
        ptr = {k: b[1].data_ptr() for k, b in bufs.items()}
        stream = torch.cuda.current_stream().cuda_stream

        refused = functools.partial(mq.refused, h)

        def raw_set(slot, n, arr):
            h._check(h.lib.wbcqp_set_observed_frames(h._h, slot, n, arr.ctypes.data_as(capi.c_i32_p) if arr is not None else None))

        def raw_observe(slot, batch, qp, vp, **out):
            o = capi.CObservables(*[out.get(k) for k in FIELDS])
            h._check(h.lib.wbcqp_observe(h._h, slot, batch, qp, vp, C.byref(o), C.c_void_p(stream)))

        # a slot without a model: no structure at all, then a structure alone
        refused(lambda: h.set_observed_frames(9, [0]))
        refused(lambda: raw_observe(9, B, q.data_ptr(), v.data_ptr(), com=ptr["com"]))
        h.set_structure(0, st)
        refused(lambda: h.set_observed_frames(0, [0]))
        refused(lambda: raw_observe(0, B, q.data_ptr(), v.data_ptr(), com=ptr["com"]))
        h.set_model(0, m, tm)
        # placement / velocity while no frames are selected (never selected, and an empty selection)
        refused(lambda: raw_observe(0, B, q.data_ptr(), v.data_ptr(), placement=ptr["placement"]))
        h.set_observed_frames(0, [])
        refused(lambda: raw_observe(0, B, q.data_ptr(), v.data_ptr(), velocity=ptr["velocity"]))
        # frame indices outside the model, n_frames outside 0 .. 64
        refused(lambda: h.set_observed_frames(0, [0, m.nframe]))
        refused(lambda: h.set_observed_frames(0, [-1]))
        refused(lambda: raw_set(0, 65, np.zeros(65, np.int32)))
        refused(lambda: raw_set(0, -1, np.zeros(1, np.int32)))
        h.set_observed_frames(0, [3, 5])
        refused(lambda: h.set_observed_frames(0, [0, m.nframe]))  # (a refused selection leaves the one before in place: checked below)
        # a velocity output without v; a negative batch
        refused(lambda: raw_observe(0, B, q.data_ptr(), None, com=ptr["com"], vcom=ptr["vcom"]))
        refused(lambda: raw_observe(0, B, q.data_ptr(), None, placement=ptr["placement"], velocity=ptr["velocity"]))
        refused(lambda: raw_observe(0, -1, q.data_ptr(), v.data_ptr(), **ptr))
        refused(lambda: raw_observe(0, B, None, v.data_ptr(), com=ptr["com"]))  # q is required
        raw_observe(0, 0, q.data_ptr(), v.data_ptr(), **ptr)  # batch == 0: WBCQP_OK, nothing launched
        torch.cuda.synchronize()
        for k, (whole, _) in bufs.items():
            assert mq.unwritten(whole.cpu().numpy()).all(), (k, "a refused call wrote something")
        got = _observe(h, 0, B, nf, q, v, dev, torch)  # and the selection [3, 5] still stands
        want = obs.observe(m, qn, vn, [3, 5])
        assert max(_worst(got, want).values()) <= TOL_ROWS
    finally:
        h.close()


def _talos_both(handle, seed, B=4, nf=2):
    """Talos on slot 3 of the module's handle; B states and prefilled outputs for nf frames, each as a (device, host) pair."""
    m, st, tm = CASES["talos"]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    qn, vn = _states(m, tm, B, seed)
    out = {k: mq.prefilled_both(B * WIDTH[k] * (1 if k in ("com", "vcom") else nf)) for k in FIELDS}
    return m, mq.both(qn), mq.both(vn), out, lambda *ks: mq.Out(capi.CObservables, **{k: out[k] for k in ks})


def test_a_refused_selection_keeps_the_one_before(handle):
    m, (_, qn), (_, vn), _, _ = _talos_both(handle, 78_100)

    def still_stands(frames):
        got = handle.observe_host(3, qn, vn)
        assert got["placement"].shape == (4, len(frames), 12) and max(_worst(got, obs.observe(m, qn, vn, frames)).values()) <= TOL_ROWS

    mq.a_refused_selection_keeps_the_one_before(handle, "observed", m.nframe, 64, still_stands)


def test_host_refusals_are_the_device_refusals(handle):
    _, q, v, out, O = _talos_both(handle, 78_200)  # (no frames are selected)
    mq.host_refusals_match(handle, "observe", [(3, 4, q, v, O("placement")),    # placement asked for with no frames selected
                                               (3, 4, q, None, O("com", "vcom")),  # vcom asked for with v NULL
                                               (3, 4, None, v, O("com")),          # q NULL
                                               (3, -1, q, v, O("com")),            # a negative batch
                                               (9, 4, q, v, O("com"))],            # a slot without a model
                           out.values())


def test_batch_zero_through_the_host_entry_point(handle):
    _, q, v, out, O = _talos_both(handle, 78_300)
    handle.set_observed_frames(3, [3, 5])
    mq.host_batch_zero(handle, "observe", [(3, 0, q, v, O(*FIELDS)), (3, 0, None, v, O(*FIELDS))], out.values())  # (q is not looked at)


def test_set_structure_and_set_model_drop_the_selection():
    torch, dev = _torch()
    m, st, tm = CASES["franka"]()
    h = capi.Handle(0, capi.F64)
    try:
        qn, vn = _states(m, tm, 3, 79_000)
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_observed_frames(0, [1, 2])
        assert h.observe_host(0, qn, vn)["placement"].shape == (3, 2, 12)
        def and_then():
            assert set(h.observe_host(0, qn, vn)) == {"com", "vcom"}  # the CoM needs no selection
            h.set_observed_frames(0, [1, 2])

        mq.set_structure_and_set_model_drop(h, (m, st, tm), lambda: torch.full((3 * 2 * 12,), float("nan"), dtype=torch.float64, device=dev),
                                            lambda buf: h.observe(0, 3, torch.from_numpy(qn).to(dev), None, placement=buf), "no frames", and_then)
    finally:
        h.close()
