"""The inverse dynamics' derivatives on the device (wbcqp_inverse_dynamics_derivatives, csrc/wbcqp_idderiv.hpp) through the C ABI: dtau/dq and
dtau/dv against the committed 80-digit truth (tests/golden/id_derivatives/) where it exists and against the numpy statement
inria_wbc_amd/id_derivatives.py everywhere.

Bar: DEVICE_MARGIN (4) x K_STATEMENT of tests/id_derivatives_cases.py, in that module's measure max |x - truth| / max |truth| per state and
matrix.  K_STATEMENT is the numpy statement's own worst error against the truth, measured on the CPU; statement and kernel evaluate the same
formulas in float64 and differ in origin (the world's / the floating base), in the order of the sums (direct / folded leaf to root) and in the
mapping.  Nothing here is derived from the kernel's output.  The velocity identity against the library's own wbcqp_inverse_dynamics is held
to four times what the numpy statement leaves against inria_wbc_amd/dynamics.py on the same inputs, computed in the test.

Shapes: the smallest at which the kernel can go wrong -- one revolute body (1 x 1 matrices), prismatic + revolute, a chain of 8 (three doubling
rounds), a floating star of 9 (every subtree one lane), the light-leaf tree of 12, a random 24, the 59-body floating tree (nv = 64, the lane
limit), 64 fixed bodies, Talos; batches 1, 3, 5, 67."""
import functools

import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import id_derivatives as idd
from inria_wbc_amd import model as mdl
from tests import id_derivatives_cases as IC
from tests import model_queries as mq
from tests import rbd_exact_cases as RC
from tests.model_queries import BATCHES, _torch

pytestmark = pytest.mark.gpu

BAR = IC.DEVICE_MARGIN * IC.K_STATEMENT
NMAX = max(BATCHES)
PAD = 13  # lda = nv + PAD in the padded mode
OUT = capi.CIdDerivativeOutputs


def _exact_case(name):
    def f():
        m = RC.model(name)
        return (m,) + mq.minimal(m, "idd_")
    return f


CASES = {name: _exact_case(name) for name in RC.SMALL}
CASES.update({"tree_24_floating": mq.tree_case("idd_", 66, 24, True, two_on_one_body=True), "tree_59_floating": _exact_case("tree_59_floating"),
              "tree_64_fixed_lane_limit": mq.tree_case("idd_", 62, 64, False, two_on_one_body=True), "talos": mq.talos_case})
CHECKED = 4  # states per case that the numpy statement is evaluated on (the first ones and the last; the rest are held to them bit for bit)


def _wrench_frames(name, m):
    if name in RC.CASES:
        return RC.wrench_frames(name)
    return [2, 3, 1]  # two frames on one body, one on the last body


@functools.lru_cache(maxsize=None)
def _inputs(name, seed=71_000):
    """(q, v, a, wrench) for NMAX states drawn as tests/rbd_exact_cases.py draws the truth's states -- q within 0.5 of q0, a random unit
    quaternion, the base 1 to 3 m from the origin, v and a of order 1, wrenches of order 10 -- so that K_STATEMENT, measured on those, speaks for
    these; the fixture's own states (where the case has a fixture) in front."""
    m, st, tm = CASES[name]()
    n = NMAX
    rng = np.random.default_rng(seed)
    q = np.tile(m.q0, (n, 1))
    q[:, m.nq - m.na:] += rng.uniform(-0.5, 0.5, (n, m.na))
    if m.floating_base:
        d = rng.standard_normal((n, 3))
        q[:, 0:3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (n, 1))
        u = rng.standard_normal((n, 4))
        q[:, 3:7] = u / np.linalg.norm(u, axis=1, keepdims=True)
    v, a, w = rng.standard_normal((n, m.nv)), rng.standard_normal((n, m.nv)), 10.0 * rng.standard_normal((n, 3, 6))
    if name in IC.CASES:
        F = IC.load(name)
        k = F["in.q"].shape[0]
        q[:k], v[:k], a[:k], w[:k] = F["in.q"], F["in.v"], F["in.a"], F["in.wrench"]
    return q, v, a, w


def _selections(m):
    """none, one frame, all eight slots with repeats, two frames on one body, a frame on body 0 and one on the last body."""
    eight = np.random.default_rng(7).integers(0, m.nframe, 8)
    eight[5] = eight[2]
    return {"none": [], "one": [m.nframe // 2], "eight_with_repeats": eight.tolist(), "two_on_one_body": [2, 3], "first_and_last_body": [0, 1]}


MODES = ("full", "a_null", "v_a_null", "lda_padded")


def _padded(a, torch, dev, td=None):
    n, nv = a.shape
    wide = np.full((n, nv + PAD), np.nan)
    wide[:, :nv] = a
    t = torch.from_numpy(wide).to(dev)
    return t if td is None else t.to(td)


def _run(h, slot, B, nv, q, v, a, wrench, mode, which=IC.MATRICES, td=None):
    """One launch on device tensors -> {name: [B, nv, nv]} for the outputs in `which`: every element is written, nothing behind the end is
    touched.  a: [N, nv + PAD] with NaN in the padding; the modes pass it whole (lda = nv + PAD), as a contiguous copy of its first nv columns
    (lda = nv), or not at all.  v_a_null: v is not passed either (dtau_dq alone can be asked for)."""
    torch, dev = _torch()
    td = td or torch.float64
    bufs = {k: mq.guarded(B * nv * nv, td, dev, torch) for k in which}
    vv = None if mode == "v_a_null" else v[:B].contiguous()
    if mode in ("a_null", "v_a_null"):
        aa, lda = None, 0
    elif mode == "lda_padded":
        aa, lda = a[:B], nv + PAD
    else:
        aa, lda = a[:B, :nv].contiguous(), nv
    h.inverse_dynamics_derivatives(slot, B, q[:B].contiguous(), v=vv, a=aa, lda=lda, wrench=None if wrench is None else wrench[:B].contiguous(),
                                   stream=torch.cuda.current_stream().cuda_stream, **{k: part for k, (_, part) in bufs.items()})
    torch.cuda.synchronize()
    return {k: mq.read_guarded(whole, B * nv * nv, k).reshape(B, nv, nv) for k, (whole, _) in bufs.items()}


def _statement(m, q, v, a, frames, w, mode, rows, which=IC.MATRICES):
    q, v, a = q[rows], v[rows], a[rows]
    return idd.derivatives(m, q, None if mode == "v_a_null" else v, None if mode in ("a_null", "v_a_null") else a, frames,
                           w[rows][:, :len(frames)] if len(frames) else None, which=list(which))


def _up(t):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev)


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


def _zeros_are_plus_zero(m, got, name):
    mask = idd.structure_mask(m)
    for k, x in got.items():
        off = x[:, ~mask]
        assert (off == 0.0).all() and not np.signbit(off).any(), (name, k, "unrelated branches")
    if m.floating_base and "dtau_dq" in got:
        base = got["dtau_dq"][:, :, :3]
        assert (base == 0.0).all() and not np.signbit(base).any(), (name, "columns 0..2 of dtau_dq")


@pytest.mark.parametrize("name", list(CASES))
def test_device_against_truth_and_statement(handle, name):
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    frames = _wrench_frames(name, m)
    handle.set_wrench_frames(3, frames)
    qn, vn, an, wn = _inputs(name)
    q, v, a, w = _up(qn), _up(vn), _padded(an, *_torch()), _up(wn)
    big = _run(handle, 3, NMAX, m.nv, q, v, a, w, "full")
    for B in BATCHES[:-1]:
        got = _run(handle, 3, B, m.nv, q, v, a, w, "full")
        for k in got:
            assert np.array_equal(got[k], big[k][:B]), (name, k, B, "the same rows in a smaller batch: other bits")
    _zeros_are_plus_zero(m, big, name)
    if name in IC.CASES:
        F = IC.load(name)
        n = F["dtau_dq"].shape[0]
        e = IC.worst_error({k: big[k][:n] for k in big}, F)
        print("id derivatives, device against the truth, %-26s %.3e (bar %.2e)" % (name, e, BAR))
        assert e <= BAR, (name, "truth", e)
    rows = list(range(CHECKED - 1)) + [NMAX - 1]
    want = _statement(m, qn, vn, an, frames, wn, "full", rows)
    e = IC.worst_error({k: big[k][rows] for k in big}, want)
    print("id derivatives, device against the statement, %-26s %.3e (bar %.2e)" % (name, e, BAR))
    assert e <= BAR, (name, "statement", e)


@pytest.mark.parametrize("sel", ["none", "one", "eight_with_repeats", "two_on_one_body", "first_and_last_body"])
def test_modes_and_wrench_selections(handle, sel):
    """Every mode of the inputs with every kind of wrench selection on the random 24: against the statement at the bar; the padded a gives the
    bits of the contiguous one; each output alone has the bits it has beside the other."""
    name = "tree_24_floating"
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    frames = _selections(m)[sel]
    handle.set_wrench_frames(3, frames)
    qn, vn, an, _ = _inputs(name)
    wn = 50.0 * np.random.default_rng(72_000 + len(frames)).standard_normal((NMAX, max(len(frames), 1), 6))
    q, v, a, w = _up(qn), _up(vn), _padded(an, *_torch()), (_up(wn) if frames else None)
    B, rows, worst = 5, [0, 4], {}
    full = None
    for mode in MODES:
        which = ("dtau_dq",) if mode == "v_a_null" else IC.MATRICES
        got = _run(handle, 3, B, m.nv, q, v, a, w, mode, which)
        _zeros_are_plus_zero(m, got, (name, sel, mode))
        want = _statement(m, qn, vn, an, frames, wn, mode, rows, IC.MATRICES if mode != "v_a_null" else ("dtau_dq",))
        if mode == "v_a_null":  # (the measure's fallback scale: the statement's dtau_dv at v = 0)
            want["dtau_dv"] = idd.derivatives(m, qn[rows], np.zeros_like(vn[rows]), None, frames, wn[rows][:, :len(frames)] if frames else None)["dtau_dv"]
        worst[mode] = IC.worst_error({k: got[k][rows] for k in got}, want)
        assert worst[mode] <= BAR, (sel, mode, worst[mode])
        if mode == "full":
            full = got
        if mode == "lda_padded":  # the padding is never read: the bits of lda = nv
            for k in got:
                assert np.array_equal(got[k], full[k]), (sel, k)
        for k in which:  # each output alone: the bits it has when both are asked for
            assert np.array_equal(_run(handle, 3, B, m.nv, q, v, a, w, mode, (k,))[k], got[k]), (sel, mode, k)
    # v given or not makes no difference to dtau_dq at v = 0
    zero_v = _run(handle, 3, B, m.nv, q, 0.0 * v, a, w, "a_null", ("dtau_dq",))["dtau_dq"]
    assert np.array_equal(np.where(zero_v == 0.0, 0.0, zero_v), _run(handle, 3, B, m.nv, q, v, a, w, "v_a_null", ("dtau_dq",))["dtau_dq"])
    print("id derivatives, modes, %-20s %s" % (sel, "  ".join("%s %.1e" % kv for kv in worst.items())))


@pytest.mark.parametrize("name", ["tree_24_floating", "talos"])
def test_velocity_identity_against_the_librarys_inverse_dynamics(handle, name):
    """dtau_dv d = (tau(v + d) - tau(v - d)) / 2 with the library's own wbcqp_inverse_dynamics, for d of order 1: at four times what the numpy
    statement leaves against inria_wbc_amd/dynamics.py on the same inputs."""
    from inria_wbc_amd import dynamics
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    frames = _wrench_frames(name, m)
    handle.set_wrench_frames(3, frames)
    qn, vn, an, wn = (t[:3] for t in _inputs(name))
    d = np.random.default_rng(73_000).standard_normal(vn.shape)
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())  # noqa: E731
    want_np = (dynamics.inverse_dynamics(m, qn, vn + d, an, frames, wn) - dynamics.inverse_dynamics(m, qn, vn - d, an, frames, wn)) / 2
    left = rel(np.einsum("bij,bj->bi", idd.derivatives(m, qn, vn, an, frames, wn, which=["dtau_dv"])["dtau_dv"], d), want_np)
    want = (handle.inverse_dynamics_host(3, qn, vn + d, an, wn) - handle.inverse_dynamics_host(3, qn, vn - d, an, wn)) / 2
    got = handle.inverse_dynamics_derivatives_host(3, qn, vn, an, wn, which=["dtau_dv"])["dtau_dv"]
    e = rel(np.einsum("bij,bj->bi", got, d), want)
    print("id derivatives, velocity identity, %-20s device %.2e, statement with dynamics.py %.2e" % (name, e, left))
    assert 0.0 < left < 1e-12 and e <= 4.0 * left, (name, e, left)


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    name = "tree_24_floating"
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    handle.set_wrench_frames(3, _wrench_frames(name, m))
    qn, vn, an, wn = _inputs(name)
    q, v, a, w = _up(qn), _up(vn), _padded(an, *_torch()), _up(wn)
    mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(
        lambda lo, hi: _run(handle, 3, hi - lo, m.nv, q[lo:hi], v[lo:hi], a[lo:hi], w[lo:hi], "lda_padded"), NMAX)


def test_a_nan_stays_with_its_instance(handle):
    name = "light_leaf_12_floating"
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    handle.set_wrench_frames(3, _wrench_frames(name, m))
    qn, vn, an, wn = _inputs(name)
    clean = handle.inverse_dynamics_derivatives_host(3, qn, vn, an, wn)
    bad = qn.copy()
    bad[41, m.nq - 1] = np.nan
    got = handle.inverse_dynamics_derivatives_host(3, bad, vn, an, wn)
    others = np.arange(NMAX) != 41
    for k in IC.MATRICES:
        assert np.isfinite(clean[k]).all()
        assert np.array_equal(got[k][others], clean[k][others]), k
        assert np.isnan(got[k][41]).any(), k


def test_f32_handle_rounds_the_f64_result(handle):
    torch, dev = _torch()
    name = "talos"
    m, st, tm = CASES[name]()
    frames = _wrench_frames(name, m)
    qn, vn, an, wn = (t[:9] for t in _inputs(name))
    q32, v32, a32, w32 = (t.astype(np.float32) for t in (qn, vn, an, wn))
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    handle.set_wrench_frames(3, frames)
    want = handle.inverse_dynamics_derivatives_host(3, *(t.astype(np.float64) for t in (q32, v32, a32, w32)))
    h32 = capi.Handle(0, capi.F32)
    try:
        h32.set_structure(0, st)
        h32.set_model(0, m, tm)
        h32.set_wrench_frames(0, frames)
        got = _run(h32, 0, 9, m.nv, _up(q32), _up(v32), _padded(a32.astype(np.float64), torch, dev, torch.float32), _up(w32), "lda_padded",
                   td=torch.float32)
        host = h32.inverse_dynamics_derivatives_host(0, q32, v32, a32, w32)
    finally:
        h32.close()
    for k in IC.MATRICES:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], host[k])
        assert np.array_equal(got[k], want[k].astype(np.float32)), k  # float in, double inside, float out: the F64 result, rounded
    _zeros_are_plus_zero(m, got, "talos, F32")


def _talos_both(handle, seed=74_000, B=4):
    """Talos on slot 3 of the module's handle (no wrench frames yet); B states and wrenches at two frames as (device, host) pairs, and the two
    prefilled outputs."""
    m, st, tm = mq.talos_case()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    s = mdl.sample_states(m, tm, B, seed, q_noise=0.3, v_noise=0.5)
    a = np.random.default_rng(seed + 1).standard_normal((B, m.nv))
    dq, dv = mq.prefilled_both(B * m.nv * m.nv), mq.prefilled_both(B * m.nv * m.nv)
    return (m,) + tuple(mq.both(t) for t in (s["q"], s["v"], a, np.ones((B, 2, 6)))) + (dq, dv)


def test_refusals_are_the_same_through_both_entry_points_and_write_nothing(handle):
    m, q, v, a, w, dq, dv = _talos_both(handle)
    nv = m.nv
    out = mq.Out(OUT, dtau_dq=dq, dtau_dv=dv)
    msg = mq.refused(handle, lambda: mq.raw(handle, "inverse_dynamics_derivatives", 1, 3, 4, q, v, a, nv, w, out))
    assert "no frames are selected" in msg
    mq.host_refusals_match(handle, "inverse_dynamics_derivatives", [(3, 4, q, v, a, nv, w, out)], [dq, dv])  # a wrench while no frames are selected
    handle.set_wrench_frames(3, [3, 5])
    mq.host_refusals_match(handle, "inverse_dynamics_derivatives",
                           [(9, 4, q, v, a, nv, None, out),                        # a slot without a model
                            (3, -1, q, v, a, nv, w, out),                          # a negative batch
                            (3, 4, None, v, a, nv, w, out),                        # q NULL with batch > 0
                            (3, 4, q, v, a, nv, w, None),                          # the struct NULL
                            (3, 4, q, v, a, nv, w, mq.Out(OUT)),                   # both members NULL
                            (3, 4, q, None, a, nv, w, out),                        # dtau_dv without v
                            (3, 4, q, None, a, nv, w, mq.Out(OUT, dtau_dv=dv)),
                            (3, 4, q, v, a, nv - 1, w, out)],                      # lda < nv with a given
                           [dq, dv])
    mq.host_batch_zero(handle, "inverse_dynamics_derivatives", [(3, 0, q, v, a, nv, w, out), (3, 0, None, v, None, 0, None, out)], [dq, dv])
    for side in (0, 1):  # batch == 0 through the device entry point too; lda is not looked at without a
        mq.raw(handle, "inverse_dynamics_derivatives", side, 3, 0, q, v, a, nv, w, out)
    _torch()[0].cuda.synchronize()
    assert mq.unwritten(dq[0].cpu().numpy()).all() and mq.unwritten(dv[0].cpu().numpy()).all()
    # what is given is written whole, nothing else: dtau_dq alone leaves dtau_dv's buffer as it was, on both sides
    for side in (0, 1):
        mq.raw(handle, "inverse_dynamics_derivatives", side, 3, 4, q, None, None, 0, w, mq.Out(OUT, dtau_dq=dq))
    _torch()[0].cuda.synchronize()
    assert np.isfinite(dq[1]).all() and np.array_equal(dq[0].cpu().numpy(), dq[1])
    assert mq.unwritten(dv[0].cpu().numpy()).all() and mq.unwritten(dv[1]).all()


def test_set_model_drops_the_wrench_selection():
    torch, dev = _torch()
    m, st, tm = CASES["tree_24_floating"]()
    h = capi.Handle(0, capi.F64)
    try:
        qn, vn, an, wn = (t[:3] for t in _inputs("tree_24_floating"))
        wn = wn[:, :2]
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_wrench_frames(0, [1, 2])
        with_w = h.inverse_dynamics_derivatives_host(0, qn, vn, an, wn)

        def and_then():
            assert not np.array_equal(h.inverse_dynamics_derivatives_host(0, qn, vn, an)["dtau_dq"], with_w["dtau_dq"])  # no wrench: no selection needed
            h.set_wrench_frames(0, [1, 2])
            again = h.inverse_dynamics_derivatives_host(0, qn, vn, an, wn)
            assert all(np.array_equal(again[k], with_w[k]) for k in IC.MATRICES)

        mq.set_structure_and_set_model_drop(h, (m, st, tm), lambda: torch.full((3 * m.nv * m.nv,), float("nan"), dtype=torch.float64, device=dev),
                                            lambda buf: h.inverse_dynamics_derivatives(0, 3, _up(qn), wrench=_up(wn), dtau_dq=buf), "no frames", and_then)
    finally:
        h.close()


def test_the_neighbours_keep_their_bits(handle):
    """wbcqp_inverse_dynamics_host and wbcqp_mass_matrix_host return the same bits before and after a derivatives call."""
    name = "talos"
    m, st, tm = CASES[name]()
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    handle.set_wrench_frames(3, _wrench_frames(name, m))
    qn, vn, an, wn = (t[:6] for t in _inputs(name))
    before = handle.inverse_dynamics_host(3, qn, vn, an, wn), handle.mass_matrix_host(3, qn)
    got = handle.inverse_dynamics_derivatives_host(3, qn, vn, an, wn)
    assert np.isfinite(got["dtau_dq"]).all() and np.isfinite(got["dtau_dv"]).all()
    after = handle.inverse_dynamics_host(3, qn, vn, an, wn), handle.mass_matrix_host(3, qn)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # d tau / d a is M: tau(a + d) - tau(a) = M d, at the bar of two float64 formulations of tests/test_gpu_inverse_dynamics.py
    d = np.random.default_rng(75_000).standard_normal(an.shape)
    diff = handle.inverse_dynamics_host(3, qn, vn, an + d, wn) - before[0]
    assert np.abs(diff - np.einsum("bij,bj->bi", before[1], d)).max() <= 1e-10 * max(1.0, np.abs(diff).max())


def test_a_traced_squat_in_one_call():
    """A traced squat (batch 2, 8 recorded ticks): one call over n_rec * batch rows of the trace's arrays, a = the trace's x with lda = n, equals
    per-tick calls bit for bit."""
    torch, dev = _torch()
    B, K = 2, 8
    h, m, st, tm, trace, q0, v0 = mq.traced_squat(B, K, 1, lambda h, m, tm: h.set_wrench_frames(0, tm.contact_frame), more=("x", "status"))
    try:
        assert (trace["status"] == 0).all().item()
        nv = m.nv
        T = torch.from_numpy(np.asarray(st.force_gen()).reshape(st.nc, 6, 12)).to(dev)
        w = torch.einsum("cij,rbcj->rbci", T, trace["x"][..., st.nv:].reshape(K, B, st.nc, 12)).contiguous()

        def run(n, q, v, x, ww):
            bufs = {k: mq.guarded(n * nv * nv, torch.float64, dev, torch) for k in IC.MATRICES}
            h.inverse_dynamics_derivatives(0, n, q.contiguous(), v=v.contiguous(), a=x.contiguous(), lda=st.n, wrench=ww.contiguous(),
                                           stream=torch.cuda.current_stream().cuda_stream, **{k: part for k, (_, part) in bufs.items()})
            torch.cuda.synchronize()
            return {k: mq.read_guarded(whole, n * nv * nv, k).reshape(n, nv, nv) for k, (whole, _) in bufs.items()}

        whole = run(K * B, trace["q"].reshape(K * B, -1), trace["v"].reshape(K * B, -1), trace["x"].reshape(K * B, -1), w.reshape(K * B, st.nc, 6))
        for r in range(K):
            tick = run(B, trace["q"][r], trace["v"][r], trace["x"][r], w[r])
            for k in IC.MATRICES:
                assert np.array_equal(whole[k][r * B:(r + 1) * B], tick[k]), (r, k)
        assert np.abs(whole["dtau_dv"]).max() > 1e-3 and not np.array_equal(whole["dtau_dq"][:B], whole["dtau_dq"][-B:])
    finally:
        h.close()
