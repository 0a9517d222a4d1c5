"""Second-order kinematics on the device (wbcqp_kinematic_hessians; csrc/wbcqp_hessians.hpp): the kinematic Hessians H = dJ/dq of the frames of
wbcqp_set_jacobian_frames in the three reference frames and the Jacobians' time variation dJ, against the numpy statement
inria_wbc_amd/hessians.py (which tests/test_hessians_host.py holds to central differences of the Jacobians) through the C ABI, and against
wbcqp_jacobians' drift through the identities that tie the two calls together.

Bar: TOL_ROWS (1e-10, tests/test_gpu_jacobians.py: two formulations in double -- world columns and body velocities about the world's origin on
the device, body-local columns and partial sums of v_k J_k in the statement), relative to max(1, the array's largest entry); an F32 handle is held
to the F64 result rounded to float.  The shapes are the Jacobian tests': one body (nv = 1), the lane limit (64 bodies fixed; 59 bodies floating =
nv 64), a pure chain, a star, Talos -- odd and even nv; H's second store shape, which the library does not choose by itself, runs in a test of its
own; batches that are no multiple of the four instances of a workgroup."""
import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import hessians as hs
from inria_wbc_amd import model as mdl
from inria_wbc_amd import observe as obs
from tests import model_queries as mq
from tests.model_queries import BATCHES, _torch
from tests.test_forward_dynamics_host import CASES, case_states
from tests.test_jacobians_host import SHAPES, selections

pytestmark = pytest.mark.gpu

TOL_ROWS = 1e-10
NMAX = max(BATCHES)
FIELDS = capi.HESSIAN_OUTPUTS
RFS = {"WORLD": capi.RF_WORLD, "LOCAL": capi.RF_LOCAL, "LOCAL_WORLD_ALIGNED": capi.RF_LOCAL_WORLD_ALIGNED}
H_SELECTIONS = {"one": BATCHES[:-1], "first_and_last_body": BATCHES[:-1], "two_on_one_body": BATCHES[:-1], "sixty_four_with_repeats": (3,)}


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


def _set(handle, name, slot=3):
    m, st, tm = CASES[name]()
    handle.set_structure(slot, st)
    handle.set_model(slot, m, tm)
    return m, st, tm


def _shape(k, B, nf, nv):
    return {"H": (B, nf, 6, nv, nv), "dJ": (B, nf, 6, nv)}[k]


def _hes(h, slot, B, nf, nv, q, v, rf, dev, torch, which=None, td=None):
    """One launch on device tensors -> {name: numpy array}; every element that must be written is finite, nothing behind the end is touched.
    v None: passed as NULL."""
    td = td or torch.float64
    which = (("H",) if v is None else FIELDS) if which is None else which
    bufs = {k: mq.guarded(int(np.prod(_shape(k, B, nf, nv))), td, dev, torch) for k in which}
    h.kinematic_hessians(slot, B, q[:B].contiguous(), None if v is None else v[:B].contiguous(), rf, stream=torch.cuda.current_stream().cuda_stream,
                         **{k: part for k, (_, part) in bufs.items()})
    torch.cuda.synchronize()
    return {k: mq.read_guarded(whole, part.numel(), k).reshape(_shape(k, B, nf, nv)) for k, (whole, part) in bufs.items()}


def _rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


def _plus_zero(a, where):
    z = a[np.broadcast_to(where, a.shape)]
    return bool((z == 0.0).all() and not np.signbit(z).any())


@pytest.mark.parametrize("name", SHAPES)
def test_hessians_parity(handle, name):
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    nv = m.nv
    qn, vn, _ = case_states(m, tm, NMAX, 95_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    every = list(range(m.nframe))  # the statement once per convention, for every frame of the model: a selection is a gather of these
    nH = max(max(b) for b in H_SELECTIONS.values())
    worst = {k: 0.0 for k in FIELDS}
    for rfname, rf in RFS.items():
        want_dJ = hs.hessians(m, qn, vn, every, rf, which=["dJ"])["dJ"]
        want_H = hs.hessians(m, qn[:nH], None, every, rf, which=["H"])["H"]
        for sel, frames in selections(m).items():
            if not frames:
                continue
            handle.set_jacobian_frames(3, frames)
            nf = len(frames)
            moved = hs.moves(m, frames)
            big = _hes(handle, 3, NMAX, nf, nv, q, v, rf, dev, torch, which=("dJ",))["dJ"]
            e = _rel(big, want_dJ[:, frames])
            worst["dJ"] = max(worst["dJ"], e)
            assert e <= TOL_ROWS, (name, sel, rfname, "dJ", e)
            assert _plus_zero(big, ~moved[None, :, None]), (name, sel, rfname, "dJ")
            for B in BATCHES[:-1]:  # the same rows in a smaller batch: the same bits
                assert np.array_equal(_hes(handle, 3, B, nf, nv, q, v, rf, dev, torch, which=("dJ",))["dJ"], big[:B]), (name, sel, rfname, B)
            lin, ang = hs.structure_masks(m, frames, rf)
            first = None
            for B in H_SELECTIONS.get(sel, ()):
                got = _hes(handle, 3, B, nf, nv, q, v, rf, dev, torch)
                e = _rel(got["H"], want_H[:B][:, frames])
                worst["H"] = max(worst["H"], e)
                assert e <= TOL_ROWS, (name, sel, rfname, "H", B, e)
                assert np.array_equal(got["dJ"], big[:B]), (name, sel, rfname, B)
                # the table's zeros, and the entries k = j that are a vector's product with itself: +0.0, the sign bit clear
                assert _plus_zero(got["H"][:, :, :3], ~lin[None, :, None]) and _plus_zero(got["H"][:, :, 3:], ~ang[None, :, None]), (name, sel, rfname, B)
                first = got["H"] if first is None else first
                assert np.array_equal(got["H"][:min(B, first.shape[0])], first[:min(B, first.shape[0])]), (name, sel, rfname, B)
            if sel == "sixty_four_with_repeats":
                assert np.array_equal(first[:, 40], first[:, 7])  # a repeated frame: the same bits
    print("hessians parity, worst per array, %-26s %s" % (name, "  ".join("%s %.1e" % (k, worst[k]) for k in FIELDS)))
    if name in ("star_17_floating", "talos"):
        assert (~hs.moves(m, every)).any()  # (the zero check had rows and columns to look at)


@pytest.mark.parametrize("name", ["talos", "tree_59_floating_nv_limit", "chain_62"])
def test_identities_across_kernels(handle, name):
    """What ties the call to wbcqp_jacobians on the same states: dJ v is the frame's spatial acceleration at zero joint accelerations -- in
    LOCAL_WORLD_ALIGNED the drift itself, in LOCAL the drift less (w_f x l_f, 0) with (l_f, w_f) = J v, in WORLD Ad(oMf) of LOCAL's with
    wbcqp_observe's placement; sum_k H v_k contracted on the host is dJ; H needs no v."""
    m, st, tm = _set(handle, name)
    n = 24
    s = mdl.sample_states(m, tm, n, 96_000, q_noise=0.2, v_noise=0.5, ref_noise=0.01)
    qn, vn = s["q"], s["v"]
    frames = selections(m)["sixty_four_with_repeats"][:6] + [0, 1]
    handle.set_jacobian_frames(3, frames)
    handle.set_observed_frames(3, frames)
    seen = handle.observe_host(3, qn, vn)
    local = handle.jacobians_host(3, qn, vn, capi.RF_LOCAL, which=["J", "drift"])
    aligned = handle.jacobians_host(3, qn, vn, capi.RF_LOCAL_WORLD_ALIGNED, which=["drift"])
    got = {rf: handle.kinematic_hessians_host(3, qn, vn, rf) for rf in RFS.values()}
    dJv = {rf: np.einsum("nfrj,nj->nfr", g["dJ"], vn) for rf, g in got.items()}
    errs = {"dJ v = drift, aligned": _rel(dJv[capi.RF_LOCAL_WORLD_ALIGNED], aligned["drift"])}
    vf = np.einsum("nfrj,nj->nfr", local["J"], vn)
    errs["dJ v + (w x l, 0) = drift, local"] = _rel(dJv[capi.RF_LOCAL] + np.concatenate([np.cross(vf[..., 3:], vf[..., :3]), np.zeros_like(vf[..., 3:])], axis=-1),
                                                    local["drift"])
    R, p = seen["placement"][:, :, :9].reshape(n, len(frames), 3, 3), seen["placement"][:, :, 9:]
    lin, ang = np.einsum("nfij,nfj->nfi", R, dJv[capi.RF_LOCAL][..., :3]), np.einsum("nfij,nfj->nfi", R, dJv[capi.RF_LOCAL][..., 3:])
    errs["dJ_world v = Ad(oMf) dJ_local v"] = _rel(dJv[capi.RF_WORLD], np.concatenate([lin + np.cross(p, ang), ang], axis=-1))
    for rfname, rf in RFS.items():
        errs["H v = dJ, " + rfname] = _rel(np.einsum("nfrjk,nk->nfrj", got[rf]["H"], vn), got[rf]["dJ"])
    print("identities across kernels, %-26s %s" % (name, "  ".join("%s %.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL_ROWS, errs
    assert np.array_equal(handle.kinematic_hessians_host(3, qn, None, capi.RF_WORLD)["H"], got[capi.RF_WORLD]["H"])  # v NULL: the bits of the call with v


def test_each_output_is_optional_and_independent(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "talos")
    nv = m.nv
    frames = obs.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "base_link", "head_2_joint", "leg_left_6_joint"])
    handle.set_jacobian_frames(3, frames)
    nf, B = len(frames), 7
    qn, vn, _ = case_states(m, tm, B, 97_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    for rf in RFS.values():
        full = _hes(handle, 3, B, nf, nv, q, v, rf, dev, torch)
        assert set(full) == set(FIELDS)
        for k in FIELDS:  # one at a time (_hes: what is asked for is written whole, nothing behind a buffer's end is touched)
            assert np.array_equal(_hes(handle, 3, B, nf, nv, q, v, rf, dev, torch, which=(k,))[k], full[k]), k
        assert np.array_equal(_hes(handle, 3, B, nf, nv, q, None, rf, dev, torch)["H"], full["H"])  # H needs no v
        assert np.array_equal(full["H"][:, 0], full["H"][:, 4]) and np.array_equal(full["dJ"][:, 0], full["dJ"][:, 4])  # a repeated frame
        host = handle.kinematic_hessians_host(3, qn, vn, rf)
        for k in FIELDS:
            assert np.array_equal(host[k], full[k]), k
        # a buffer that starts at an odd element: H's rows cannot be stored two elements at a time, the bits stay
        whole, _ = mq.guarded(1 + full["H"].size, torch.float64, dev, torch)
        handle.kinematic_hessians(3, B, q, None, rf, H=whole[1:1 + full["H"].size], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        a = whole.cpu().numpy()
        assert np.isnan(a[0]) and np.isnan(a[1 + full["H"].size:]).all() and np.array_equal(a[1:1 + full["H"].size].reshape(full["H"].shape), full["H"])


@pytest.fixture(scope="module")
def wide_handle():
    """A handle that launches hessian_kernel's second store shape where it can: the library reads WBCQP_HESSIAN_STORE once, at wbcqp_create."""
    mp = pytest.MonkeyPatch()
    mp.setenv("WBCQP_HESSIAN_STORE", "wide")
    try:
        h = capi.Handle(0, capi.F64)
    finally:
        mp.undo()
    yield h
    h.close()


@pytest.mark.parametrize("name", ["talos", "tree_59_floating_nv_limit", "chain_62", "tree_64_fixed_lane_limit", "tree_24_floating", "one_body_fixed"])
def test_the_two_store_shapes_give_the_same_bits(handle, wide_handle, name):
    """H's rows go out one k per lane or, on a handle created with WBCQP_HESSIAN_STORE=wide, two consecutive k per lane where nv is even and H is
    aligned to two elements (two instantiations of the kernel; tools/hessians_bench.py times them side by side).  Even nv: Talos (50), the two
    trees of nv 64, chain_62.  Odd nv (29, 1), and H at an odd element: the wide handle falls back to one k per lane."""
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    _set(wide_handle, name)
    frames = selections(m)["sixty_four_with_repeats"][:5]
    handle.set_jacobian_frames(3, frames)
    wide_handle.set_jacobian_frames(3, frames)
    qn, vn, _ = case_states(m, tm, 5, 105_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    for rf in RFS.values():
        narrow = _hes(handle, 3, 5, len(frames), m.nv, q, v, rf, dev, torch)
        wide = _hes(wide_handle, 3, 5, len(frames), m.nv, q, v, rf, dev, torch)
        for k in FIELDS:
            assert np.array_equal(narrow[k], wide[k]), (name, rf, k)
        assert _rel(wide["H"], hs.hessians(m, qn, None, frames, rf)["H"]) <= TOL_ROWS
        # a buffer that starts at an odd element: rows cannot go out two elements at a time, the bits stay and nothing else is touched
        n = narrow["H"].size
        whole, _ = mq.guarded(1 + n, torch.float64, dev, torch)
        wide_handle.kinematic_hessians(3, 5, q[:5].contiguous(), None, rf, H=whole[1:1 + n], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        a = whole.cpu().numpy()
        assert np.isnan(a[0]) and np.isnan(a[1 + n:]).all() and np.array_equal(a[1:1 + n].reshape(narrow["H"].shape), narrow["H"]), (name, rf)


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "tree_24_floating")
    frames = [1, m.nframe // 2]
    handle.set_jacobian_frames(3, frames)
    qn, vn, _ = case_states(m, tm, NMAX, 98_000)
    q, v = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev)
    run = lambda lo, hi: _hes(handle, 3, hi - lo, len(frames), m.nv, q[lo:hi], v[lo:hi], capi.RF_LOCAL, dev, torch)  # noqa: E731
    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(run, NMAX)
    assert set(a) == set(FIELDS)
    for B in BATCHES[:-1]:
        got = run(0, B)
        for k in FIELDS:
            assert np.array_equal(got[k], a[k][:B]), (k, B)


def test_f32_handle_rounds_the_f64_result(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "talos")
    frames = obs.frame_ids(m, ["leg_left_6_joint", "gripper_right_joint", "head_2_joint"])
    qn, vn, _ = case_states(m, tm, 9, 99_000)
    q32, v32 = qn.astype(np.float32), vn.astype(np.float32)
    handle.set_jacobian_frames(3, frames)
    h32 = capi.Handle(0, capi.F32)
    try:
        h32.set_structure(0, st)
        h32.set_model(0, m, tm)
        h32.set_jacobian_frames(0, frames)
        for rf in RFS.values():
            want = handle.kinematic_hessians_host(3, q32.astype(np.float64), v32.astype(np.float64), rf)
            got = _hes(h32, 0, 9, len(frames), m.nv, torch.from_numpy(q32).to(dev), torch.from_numpy(v32).to(dev), rf, dev, torch, td=torch.float32)
            host = h32.kinematic_hessians_host(0, q32, v32, rf)
            assert set(got) == set(want) == set(host) == set(FIELDS)
            for k in got:
                assert got[k].dtype == np.float32 and np.array_equal(got[k], host[k]), k
                ulp = float(np.spacing(np.float32(np.abs(want[k]).max())))
                assert np.abs(got[k].astype(np.float64) - want[k].astype(np.float32).astype(np.float64)).max() <= ulp, (k, ulp)
    finally:
        h32.close()


def test_offsets_past_four_gigabytes(handle):
    """nv = 64, 64 frames, 342 instances of one state: H is 4.3 GB, so the last instances lie past a 32-bit byte offset.  Everything stays on the
    device; only the verdicts come down."""
    torch, dev = _torch()
    m, st, tm = _set(handle, "tree_59_floating_nv_limit")
    assert m.nv == 64
    frames = selections(m)["sixty_four_with_repeats"]
    handle.set_jacobian_frames(3, frames)
    B, per = 342, 64 * 6 * 64 * 64
    n = B * per
    assert (B - 1) * per * 8 < 2 ** 32 < n * 8  # (the last instance straddles the 32-bit boundary of byte offsets)
    qn, _, _ = case_states(m, tm, 1, 100_000)
    q = torch.from_numpy(np.repeat(qn, B, axis=0)).to(dev)
    whole, part = mq.guarded(n, torch.float64, dev, torch)
    handle.kinematic_hessians(3, B, q, None, capi.RF_WORLD, H=part, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    H = part.view(B, per)
    assert bool(torch.isfinite(H[0]).all().item()) and bool((H[0] != 0).any().item())
    assert torch.equal(H[B - 1], H[0]) and torch.equal(H[B - 2], H[0]) and torch.equal(H[B // 2], H[0])
    assert not bool(torch.isnan(part).any().item())        # every element written
    assert bool(torch.isnan(whole[n:]).all().item())       # the guard behind the end untouched
    del whole, part, H
    torch.cuda.empty_cache()


def _talos_both(handle, seed, B=4, nf=2):
    """Talos on slot 3 of the module's handle; B states and prefilled outputs for nf frames, each as a (device, host) pair."""
    m, st, tm = _set(handle, "talos")
    qn, vn, _ = case_states(m, tm, B, seed)
    out = {k: mq.prefilled_both(int(np.prod(_shape(k, B, nf, m.nv)))) for k in FIELDS}
    return m, mq.both(qn), mq.both(vn), out, lambda *ks: mq.Out(capi.CHessianOutputs, **{k: out[k] for k in ks})


def test_host_refusals_are_the_device_refusals(handle):
    _, q, v, out, O = _talos_both(handle, 101_000)  # (no frames are selected)
    L = capi.RF_LOCAL
    mq.host_refusals_match(handle, "kinematic_hessians", [(3, 4, q, v, L, O("H")), (3, 4, q, v, L, O("dJ"))], out.values())  # no frames selected
    assert "no frames" in mq.refused(handle, lambda: mq.raw(handle, "kinematic_hessians", 0, 3, 4, q, v, L, O("H", "dJ")))
    handle.set_jacobian_frames(3, [3, 5])
    mq.host_refusals_match(handle, "kinematic_hessians", [(9, 4, q, v, L, O("H")),             # a slot without a model
                                                          (3, -1, q, v, L, O("H")),            # a negative batch
                                                          (3, 4, q, None, L, O("H", "dJ")),    # dJ with v NULL
                                                          (3, 4, q, None, L, O("dJ")),
                                                          (3, 4, q, v, 3, O("H")),             # an unknown reference frame
                                                          (3, 4, q, v, -1, O("dJ")),
                                                          (3, 4, q, v, L, O()),                # both members NULL
                                                          (3, 4, q, v, L, None),               # the struct itself NULL
                                                          (3, 4, None, v, L, O("H"))],         # q NULL
                           out.values())
    assert "v is NULL" in mq.refused(handle, lambda: mq.raw(handle, "kinematic_hessians", 1, 3, 4, q, None, L, O("dJ")))
    assert "reference_frame" in mq.refused(handle, lambda: mq.raw(handle, "kinematic_hessians", 0, 3, 4, q, v, 7, O("H")))
    # batch == 0: WBCQP_OK through both entry points (q is not looked at), nothing launched, nothing written
    mq.host_batch_zero(handle, "kinematic_hessians", [(3, 0, q, v, L, O(*FIELDS)), (3, 0, None, v, L, O(*FIELDS))], out.values())
    mq.raw(handle, "kinematic_hessians", 0, 3, 0, q, v, L, O(*FIELDS))
    _torch()[0].cuda.synchronize()
    for dev_side, _ in out.values():
        assert mq.unwritten(dev_side.cpu().numpy()).all()


def test_a_refused_selection_keeps_the_one_before(handle):
    m, (_, qn), (_, vn), _, _ = _talos_both(handle, 102_000)

    def still_stands(frames):
        got = handle.kinematic_hessians_host(3, qn, vn, capi.RF_LOCAL)
        want = hs.hessians(m, qn, vn, frames, hs.LOCAL)
        assert got["H"].shape == (4, len(frames), 6, m.nv, m.nv) and max(_rel(got[k], want[k]) for k in FIELDS) <= TOL_ROWS

    mq.a_refused_selection_keeps_the_one_before(handle, "jacobian", m.nframe, 64, still_stands)


def test_set_structure_and_set_model_drop_the_selection():
    torch, dev = _torch()
    m, st, tm = CASES["franka"]()
    h = capi.Handle(0, capi.F64)
    try:
        qn, vn, _ = case_states(m, tm, 3, 103_000)
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_jacobian_frames(0, [1, 2])
        assert h.kinematic_hessians_host(0, qn, vn)["H"].shape == (3, 2, 6, m.nv, m.nv)
        mq.set_structure_and_set_model_drop(h, (m, st, tm), lambda: torch.full((3 * 2 * 6 * m.nv * m.nv,), float("nan"), dtype=torch.float64, device=dev),
                                            lambda buf: h.kinematic_hessians(0, 3, torch.from_numpy(qn).to(dev), None, capi.RF_LOCAL, H=buf), "no frames",
                                            lambda: h.set_jacobian_frames(0, [1, 2]))
    finally:
        h.close()


def test_nothing_else_moves(handle):
    def query(s, tick):
        handle.set_jacobian_frames(3, list(range(6)))
        for rf in RFS.values():
            handle.kinematic_hessians_host(3, s["q"], s["v"], rf)

    mq.nothing_else_moves(handle, mq.talos_case(), 104_000, query, observed=[1, 4, 9])


def test_a_traced_squat_in_one_call():
    """The q / v arrays of a trace pass as they are, as [n_rec * batch] rows: one call answers every recorded tick, bit for bit what tick-by-tick
    calls give, and the statement agrees on the recorded states."""
    torch, dev = _torch()
    B, K, stride = 8, 12, 3
    n_rec = K // stride
    names = ["leg_left_6_joint", "gripper_left_joint", "base_link"]
    h, m, _, _, trace, _, _ = mq.traced_squat(B, K, stride, lambda h, m, tm: h.set_jacobian_frames(0, obs.frame_ids(m, names)))
    try:
        frames, nv = obs.frame_ids(m, names), m.nv
        trq, trv = trace["q"], trace["v"]
        whole = _hes(h, 0, n_rec * B, len(frames), nv, trq.reshape(n_rec * B, -1), trv.reshape(n_rec * B, -1), capi.RF_LOCAL_WORLD_ALIGNED, dev, torch)
        for r in range(n_rec):
            tick = _hes(h, 0, B, len(frames), nv, trq[r], trv[r], capi.RF_LOCAL_WORLD_ALIGNED, dev, torch)
            for k in FIELDS:
                assert np.array_equal(whole[k][r * B:(r + 1) * B], tick[k]), (k, r)
        qs, vs = trq.reshape(n_rec * B, -1).cpu().numpy(), trv.reshape(n_rec * B, -1).cpu().numpy()
        assert np.isfinite(qs).all() and np.isfinite(vs).all() and np.abs(qs[:B] - qs[-B:]).max() > 0  # recorded, and the robots moved
        want = hs.hessians(m, qs, vs, frames, hs.LOCAL_WORLD_ALIGNED)
        w = {k: _rel(whole[k], want[k]) for k in FIELDS}
        print("hessians over a traced squat (4 x 8 states) against the statement: %s" % {k: "%.1e" % e for k, e in w.items()})
        assert max(w.values()) <= TOL_ROWS, w
    finally:
        h.close()
