"""Self-collision on the device (wbcqp_check_collisions, csrc/wbcqp_collide.hpp) against the numpy statement inria_wbc_amd/collision.py (itself
checked against a transcription of the reference's four loops in tests/test_collision_host.py).

Bars.  centres: TOL_ROWS of tests/test_gpu_observe.py, the same kinematics in two formulations, relative to max(1, the array's largest entry).
colliding, n_pairs and first_pair are decisions on `distance < threshold`: they must be EQUAL on every state none of whose pairs lies within
TIE = 1e-9 of its threshold in the numpy statement (ten times TOL_ROWS: a centre moves by 1e-10 at the most, a distance by twice that).  The
tables and states below are chosen so that NO state is excluded and both outcomes occur; each test asserts that of its own inputs, so the exclusion
can never hide a failure.  clearance is a difference of two such distances' worth of error: 4 TOL_ROWS."""
import ctypes as C
import functools

import numpy as np
import pytest

from inria_wbc_amd import capi, collision, structure
from inria_wbc_amd import model as mdl
from tests import model_queries as mq
from tests.model_queries import UNSET, _torch
from tests.test_collision_host import FIXTURE, ordering_case, random_table

pytestmark = pytest.mark.gpu

TOL_ROWS = 1e-10
TIE = 1e-9
FIELDS = capi.COLLISIONS
INTS = ("colliding", "first_pair", "n_pairs")


def _states(m, n, seed, noise=0.5):
    rng = np.random.default_rng(seed)
    q = np.stack([m.q0] * n)
    q[:, (7 if m.floating_base else 0):] += noise * rng.standard_normal((n, m.na))
    if m.floating_base:
        q[:, :3] += rng.standard_normal((n, 3))
        q[:, 3:7] += 0.3 * rng.standard_normal((n, 4))
        q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    return q


def _margin(table, want):
    """Per state, the smallest |distance - threshold| over the cross-member pairs, from the numpy statement's centres (+inf without pairs)."""
    half = table.diameter * np.float32(0.5)
    thr = (half[None] + half[:, None]).astype(np.float64)
    cross = table.member[:, None] < table.member[None]
    c = want["centres"]
    if not cross.any():
        return np.full(c.shape[0], np.inf)
    d = np.linalg.norm(c[:, None, :, :] - c[:, :, None, :], axis=-1)
    return np.abs(d - thr)[:, cross].min(axis=1)


def _width(k, ns):
    return {"colliding": 1, "first_pair": 2, "n_pairs": 1, "clearance": 1, "centres": 3 * ns}[k]


def _bufs(B, ns, td, dev, torch, which=FIELDS):
    return {k: mq.guarded(B * _width(k, ns), torch.int32 if k in INTS else td, dev, torch) for k in which}


def _check(h, slot, B, ns, q, dev, torch, which=FIELDS, td=None):
    """One launch on device tensors -> {name: numpy array}; every element that must be written is, nothing behind the end is touched."""
    td = td or torch.float64
    bufs = _bufs(B, ns, td, dev, torch, which)
    h.check_collisions(slot, B, q[:B].contiguous(), stream=torch.cuda.current_stream().cuda_stream, **{k: b[1] for k, b in bufs.items()})
    torch.cuda.synchronize()
    return {k: mq.read_guarded(whole, part.numel(), k, finite=False).reshape({"first_pair": (B, 2), "centres": (B, ns, 3)}.get(k, (B,)))
            for k, (whole, part) in bufs.items()}  # (finite=False: a clearance of +inf is an answer)


def _agree(got, want, table, what):
    """The bars of the module's docstring; returns the worst centre deviation."""
    B = got["colliding"].shape[0]
    assert (_margin(table, want)[:B] > TIE).all(), (what, "a state lies on a threshold: choose other inputs")
    worst = float(np.abs(got["centres"] - want["centres"][:B]).max() / max(1.0, np.abs(want["centres"][:B]).max())) if table.n_spheres else 0.0
    assert worst <= TOL_ROWS, (what, worst)
    for k in INTS:
        assert np.array_equal(got[k], want[k][:B]), (what, k, got[k].tolist(), want[k][:B].tolist())
    inf = np.isinf(want["clearance"][:B])
    assert np.array_equal(np.isposinf(got["clearance"]), inf), what
    assert np.abs(got["clearance"][~inf] - want["clearance"][:B][~inf]).max(initial=0.0) <= 4 * TOL_ROWS, what
    return worst


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


def _bind(h, slot, m):
    st, tm = mq.minimal(m, "collide_")
    h.set_structure(slot, st)
    h.set_model(slot, m, tm)
    return st, tm


def test_exact_geometry_and_the_strict_comparison(handle):
    """Two bodies on a fixed base, both prismatic, one sphere of diameter 0.2 at each origin: the centres are q[1] apart, exactly."""
    torch, dev = _torch()
    m = mdl.random_tree(95, 2, False)
    m.parent, m.jtype = np.array([-1, 0], np.int32), np.array([mdl.J_PY, mdl.J_PX], np.int32)
    m.placement = np.stack([mdl.pack_se3(np.eye(3), (0, 0, 0))] * 2)
    m.validate()
    _bind(handle, 3, m)
    t = collision.SphereTable(body=np.array([0, 1], np.int32), member=np.array([0, 1], np.int32), centre=np.zeros((2, 3)),
                              diameter=np.full(2, 0.2, np.float32), member_names=["a", "b"])
    handle.set_collision_spheres(3, t)
    touching = float(np.float32(0.1) + np.float32(0.1))  # the threshold itself: 0.2f widened
    d = np.array([0.2 - 1e-6, 0.2 + 1e-6, 0.05, 1.0, touching])
    q = np.stack([np.zeros(5), d], axis=1)
    got = _check(handle, 3, 5, 2, torch.from_numpy(q).to(dev), dev, torch)  # batch 5: a partial last workgroup
    hit = [1, 0, 1, 0, 0]  # 0.2 - 1e-6 < 0.2f < 0.2 + 1e-6, and touching is no hit under the strict <
    assert got["colliding"].tolist() == hit and got["n_pairs"].tolist() == hit
    assert got["first_pair"].tolist() == [[0, 1] if x else [-1, -1] for x in hit]
    assert np.abs(got["clearance"] - (d - touching)).max() <= 1e-12 and got["clearance"][4] == 0.0
    assert np.array_equal(got["centres"][:, 1, 0], d) and np.count_nonzero(got["centres"]) == 5  # (every other coordinate is an exact zero)
    want = collision.check(m, t, q)
    for k in INTS:
        assert np.array_equal(got[k], want[k]), k


MODELS = {"tree24": lambda: mdl.random_tree(81, 24, True), "fixed64": lambda: mdl.random_tree(82, 64, False)}
# (table seed, diameter scale) per (model, n_spheres, members), found on the CPU: with _states(m, 7, 8100) both outcomes occur among the seven states and
# no pair of any state lies within TIE of its threshold.  One sphere, or one member, cannot collide: those cases only check that.
TABLES = {('tree24', 2, 2): (1, 3.0), ('tree24', 2, 16): (1, 3.0), ('tree24', 64, 2): (5, 0.3), ('tree24', 64, 16): (3, 0.3), ('tree24', 65, 2): (2, 0.3),
          ('tree24', 65, 16): (0, 0.3), ('tree24', 128, 2): (6, 0.3), ('tree24', 128, 16): (3, 0.1), ('tree24', 256, 2): (1, 0.1), ('tree24', 256, 16): (0, 0.1),
          ('fixed64', 2, 2): (7, 3.0), ('fixed64', 2, 16): (7, 3.0), ('fixed64', 64, 2): (0, 0.3), ('fixed64', 64, 16): (2, 0.3), ('fixed64', 65, 2): (3, 0.3),
          ('fixed64', 65, 16): (0, 0.3), ('fixed64', 128, 2): (0, 0.3), ('fixed64', 128, 16): (6, 0.3), ('fixed64', 256, 2): (1, 0.1), ('fixed64', 256, 16): (2, 0.1)}


@pytest.mark.parametrize("ns", [1, 2, 64, 65, 128, 256])
@pytest.mark.parametrize("name", list(MODELS))
def test_lane_round_edges(handle, name, ns):
    torch, dev = _torch()
    m = MODELS[name]()
    _bind(handle, 3, m)
    qn = _states(m, 7, 8100)
    q = torch.from_numpy(qn).to(dev)
    worst = 0.0
    for nm in (1, 2, 16):
        seed, scale = TABLES.get((name, ns, nm), (0, 1.0))
        t = random_table(m, ns, nm, seed, dmin=0.05 * scale, dmax=0.3 * scale)
        want = collision.check(m, t, qn)
        if min(nm, ns) < 2:
            assert not want["colliding"].any() and np.isposinf(want["clearance"]).all()
        else:
            assert 0 < want["colliding"].sum() < 7, "both outcomes must occur"
        handle.set_collision_spheres(3, t)
        big = None
        for B in (7, 4, 1):
            got = _check(handle, 3, B, ns, q, dev, torch)
            worst = max(worst, _agree(got, want, t, (name, ns, nm, B)))
            big = big or got
            for k in FIELDS:  # the same rows in a smaller batch: the same bits
                assert np.array_equal(got[k], big[k][:B]), (name, ns, nm, B, k)
    print("collision centres, worst deviation, %-8s n_spheres %3d: %.1e" % (name, ns, worst))


def test_first_pair_follows_the_reference_loops(handle):
    torch, dev = _torch()
    m, t, qn = ordering_case()
    _bind(handle, 3, m)
    handle.set_collision_spheres(3, t)
    got = _check(handle, 3, 1, 4, torch.from_numpy(qn).to(dev), dev, torch)
    assert got["n_pairs"].tolist() == [2] and got["first_pair"].tolist() == [[1, 2]]  # (A, 1)-(B, 0), not the smaller table pair (0, 3)
    assert collision.pair_names(t, got["first_pair"][0]) == (("A", 1), ("B", 0))


_talos = mq.talos_case


def _talos_states(m, tm):
    """64 sampled states, q0, and 8 states with the shoulders rolled inwards until the arms meet."""
    qs = [mdl.sample_states(m, tm, 64, 83_200, q_noise=0.2)["q"], m.q0[None]]
    for s in np.linspace(0.2, 1.6, 8):
        q = m.q0.copy()
        q[7 + m.joint_names.index("arm_left_2_joint") - 1] -= s
        q[7 + m.joint_names.index("arm_right_2_joint") - 1] += s
        qs.append(q[None])
    return np.concatenate(qs)


def test_talos_sphere_model(handle):
    torch, dev = _torch()
    m, st, tm = _talos()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    t = collision.sphere_table(m, FIXTURE)
    handle.set_collision_spheres(3, t)
    qn = _talos_states(m, tm)
    want = collision.check(m, t, qn)
    assert want["colliding"].sum() >= 8 and (1 - want["colliding"]).sum() >= 8 and want["colliding"][64] == 0  # (q0 is free)
    assert want["colliding"][65:].sum() >= 4 and collision.pair_names(t, want["first_pair"][-1])[0][0] == "arm_left"
    got = _check(handle, 3, qn.shape[0], t.n_spheres, torch.from_numpy(qn).to(dev), dev, torch)
    worst = _agree(got, want, t, "talos")
    host = handle.check_collisions_host(3, qn)
    for k in FIELDS:
        assert np.array_equal(host[k], got[k]), k
    print("collision centres, worst deviation, talos (112 spheres, 73 states, %d colliding): %.1e" % (want["colliding"].sum(), worst))


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    m = MODELS["tree24"]()
    _bind(handle, 3, m)
    t = random_table(m, 128, 16, 3, dmin=0.005, dmax=0.03)
    handle.set_collision_spheres(3, t)
    q = torch.from_numpy(_states(m, 67, 8200)).to(dev)
    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(lambda lo, hi: _check(handle, 3, hi - lo, 128, q[lo:hi], dev, torch), 67)
    assert set(a) == set(FIELDS) and 0 < a["colliding"].sum() < 67


def test_f32_handle(handle):
    """An F32 handle reads q as float and computes in double: on q rounded to float its flags are the F64 run's wherever no pair is within 1e-4 of
    its threshold, and its centres are the F64 centres rounded (1e-6)."""
    torch, dev = _torch()
    m, st, tm = _talos()
    t = collision.sphere_table(m, FIXTURE)
    q32 = _talos_states(m, tm).astype(np.float32)
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    handle.set_collision_spheres(3, t)
    want = handle.check_collisions_host(3, q32.astype(np.float64))
    h32 = capi.Handle(0, capi.F32)
    try:
        h32.set_structure(0, st)
        h32.set_model(0, m, tm)
        h32.set_collision_spheres(0, t)
        got = _check(h32, 0, q32.shape[0], t.n_spheres, torch.from_numpy(q32).to(dev), dev, torch, td=torch.float32)
        host = h32.check_collisions_host(0, q32)
    finally:
        h32.close()
    for k in FIELDS:
        assert np.array_equal(got[k], host[k]), k
    assert got["centres"].dtype == np.float32 and got["clearance"].dtype == np.float32
    assert np.abs(got["centres"].astype(np.float64) - want["centres"]).max() <= 1e-6
    clear = _margin(t, dict(centres=want["centres"])) > 1e-4
    assert clear.sum() >= 60
    for k in INTS:
        assert np.array_equal(got[k][clear], want[k][clear]), k
    assert np.abs(got["clearance"].astype(np.float64) - want["clearance"]).max() <= 1e-6


def test_each_output_is_optional_and_independent(handle):
    torch, dev = _torch()
    m = MODELS["tree24"]()
    _bind(handle, 3, m)
    t = random_table(m, 65, 16, 0, dmin=0.015, dmax=0.09)
    handle.set_collision_spheres(3, t)
    q = torch.from_numpy(_states(m, 7, 8100)).to(dev)
    full = _check(handle, 3, 7, 65, q, dev, torch)
    for left_out in FIELDS:
        which = tuple(k for k in FIELDS if k != left_out)
        got = _check(handle, 3, 7, 65, q, dev, torch, which=which)
        for k in which:
            assert np.array_equal(got[k], full[k]), (left_out, k)
    for k in FIELDS:  # one at a time
        assert np.array_equal(_check(handle, 3, 7, 65, q, dev, torch, which=(k,))[k], full[k]), k
    handle.check_collisions(3, 7, q)  # nothing asked for: WBCQP_OK, nothing written


def test_nothing_else_moves(handle):
    case = _talos()

    def query(s, tick):
        handle.set_collision_spheres(3, collision.sphere_table(case[0], FIXTURE))
        handle.check_collisions_host(3, s["q"])

    mq.nothing_else_moves(handle, case, 77_000, query, observed=[0, 5])


def test_a_traced_rollouts_q_in_one_call():
    torch, dev = _torch()
    B, K = 4, 8
    t = collision.sphere_table(mdl.talos_like(), FIXTURE)
    h, m, _, _, trace, _, _ = mq.traced_squat(B, K, 1, lambda h, m, tm: h.set_collision_spheres(0, t))
    try:
        whole = _check(h, 0, K * B, t.n_spheres, trace["q"].reshape(K * B, -1), dev, torch)
        for r in range(K):
            tick = _check(h, 0, B, t.n_spheres, trace["q"][r], dev, torch)
            for k in FIELDS:
                assert np.array_equal(whole[k][r * B:(r + 1) * B], tick[k]), (k, r)
        qs = trace["q"].reshape(K * B, -1).cpu().numpy()
        assert np.isfinite(qs).all() and np.abs(qs[:B] - qs[-B:]).max() > 0  # recorded, and the robots moved
        _agree(whole, collision.check(m, t, qs), t, "trace")
    finally:
        h.close()


def test_refusals_come_before_any_launch():
    torch, dev = _torch()
    m, st, tm = _talos()
    t = collision.sphere_table(m, FIXTURE)
    h = capi.Handle(0, capi.F64)
    try:
        B, ns = 4, t.n_spheres
        q = torch.from_numpy(_talos_states(m, tm)[:B]).to(dev)
        bufs = _bufs(B, ns, torch.float64, dev, torch)
        ptr = {k: b[1].data_ptr() for k, b in bufs.items()}
        stream = torch.cuda.current_stream().cuda_stream

        refused = functools.partial(mq.refused, h)

        def raw_check(slot, batch, qp, **out):
            o = capi.CCollisions(*[out.get(k) for k in FIELDS])
            h._check(h.lib.wbcqp_check_collisions(h._h, slot, batch, qp, C.byref(o), C.c_void_p(stream)))

        def changed(**kw):
            import copy
            c = copy.deepcopy(t)
            for k, (i, v) in kw.items():
                getattr(c, k)[i] = v
            return c

        # a slot without a model: no structure at all, then a structure alone
        refused(lambda: h.set_collision_spheres(9, t))
        refused(lambda: raw_check(9, B, q.data_ptr(), **ptr))
        h.set_structure(0, st)
        refused(lambda: h.set_collision_spheres(0, t))
        refused(lambda: raw_check(0, B, q.data_ptr(), **ptr))
        h.set_model(0, m, tm)
        # a slot without a sphere table (never set, and dropped by an empty one)
        refused(lambda: raw_check(0, B, q.data_ptr(), **ptr))
        h.set_collision_spheres(0, t)
        h.set_collision_spheres(0, None)
        refused(lambda: raw_check(0, B, q.data_ptr(), **ptr))
        # the table's own checks
        big = random_table(m, 257, 2, 0)
        sm = capi.CSphereModel(257, big.body.ctypes.data_as(capi.c_i32_p), big.member.ctypes.data_as(capi.c_i32_p), big.centre.ctypes.data_as(capi.c_f64_p),
                               big.diameter.ctypes.data_as(C.POINTER(C.c_float)))
        refused(lambda: h._check(h.lib.wbcqp_set_collision_spheres(h._h, 0, C.byref(sm))))
        sm.n_spheres = -1
        refused(lambda: h._check(h.lib.wbcqp_set_collision_spheres(h._h, 0, C.byref(sm))))
        for bad in (changed(body=(3, m.nbody)), changed(body=(3, -1)), changed(member=(-1, 16)), changed(member=(0, -1)), changed(member=(5, 4)),
                    changed(centre=((7, 1), np.nan)), changed(centre=((7, 2), np.inf)), changed(diameter=(2, 0.0)), changed(diameter=(2, -0.1)),
                    changed(diameter=(2, np.inf)), changed(diameter=(2, np.nan))):
            refused(lambda: h.set_collision_spheres(0, bad))
        h.set_collision_spheres(0, t)
        refused(lambda: h.set_collision_spheres(0, changed(body=(3, m.nbody))))  # (a refused table leaves the one before in place: checked below)
        refused(lambda: raw_check(0, -1, q.data_ptr(), **ptr))
        refused(lambda: raw_check(0, B, None, **ptr))  # q is required
        raw_check(0, 0, q.data_ptr(), **ptr)  # batch == 0: WBCQP_OK, nothing launched
        torch.cuda.synchronize()
        for k, (whole, _) in bufs.items():
            assert mq.unwritten(whole.cpu().numpy()).all(), (k, "a refused call wrote something")
        got = _check(h, 0, B, ns, q, dev, torch)  # and the table still stands
        _agree(got, collision.check(m, t, q.cpu().numpy()), t, "after the refusals")
    finally:
        h.close()


def _talos_both(handle, B=4):
    """Talos on slot 3 of the module's handle (no sphere table yet), its table; B states and prefilled outputs, each as a (device, host) pair."""
    m, st, tm = _talos()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    t = collision.sphere_table(m, FIXTURE)
    out = {k: mq.prefilled_both(B * _width(k, t.n_spheres), k in INTS) for k in FIELDS}
    return t, mq.both(np.ascontiguousarray(_talos_states(m, tm)[:B])), out, mq.Out(capi.CCollisions, **out)


def test_host_refusals_are_the_device_refusals(handle):
    t, q, out, O = _talos_both(handle)
    mq.host_refusals_match(handle, "check_collisions", [(3, 4, q, O)], out.values())  # a slot without a sphere table: never set,
    handle.set_collision_spheres(3, t)
    handle.set_collision_spheres(3, None)
    mq.host_refusals_match(handle, "check_collisions", [(3, 4, q, O)], out.values())  # and dropped by an empty one
    handle.set_collision_spheres(3, t)
    mq.host_refusals_match(handle, "check_collisions", [(3, -1, q, O),    # a negative batch
                                                        (3, 4, None, O),  # q NULL
                                                        (3, 4, q, None),  # no struct of outputs
                                                        (9, 4, q, O)],    # a slot without a model
                           out.values())


def test_batch_zero_through_the_host_entry_point(handle):
    t, q, out, O = _talos_both(handle)
    handle.set_collision_spheres(3, t)
    mq.host_batch_zero(handle, "check_collisions", [(3, 0, q, O), (3, 0, None, O)], out.values())  # (q is not looked at)


def test_set_structure_and_set_model_drop_the_table():
    torch, dev = _torch()
    m = mdl.franka_like()
    st = structure.franka_structure()
    tm = mdl.build_taskmap(m, st, mdl.franka_stack())
    t = random_table(m, 20, 3, 4)
    h = capi.Handle(0, capi.F64)
    try:
        qn = _states(m, 3, 8300)
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_collision_spheres(0, t)
        assert h.check_collisions_host(0, qn)["centres"].shape == (3, 20, 3)
        def and_then():
            h.set_collision_spheres(0, t)
            assert np.array_equal(h.check_collisions_host(0, qn)["colliding"], collision.check(m, t, qn)["colliding"])

        mq.set_structure_and_set_model_drop(h, (m, st, tm), lambda: torch.full((3,), UNSET, dtype=torch.int32, device=dev),
                                            lambda buf: h.check_collisions(0, 3, torch.from_numpy(qn).to(dev), colliding=buf), "no sphere table", and_then)
    finally:
        h.close()
