"""Forward dynamics on the device (wbcqp_mass_matrix, wbcqp_forward_dynamics, wbcqp_spd_commands; csrc/wbcqp_fdyn.hpp) against
oracle/rbd_oracle.c (rbd_terms' M, nle and LOCAL frame Jacobians, rnea) through the C ABI.

Bars: TOL_ROWS (1e-10) relative to max(1, the array's largest entry); TOL_F32 (1e-6) for an F32 handle; tests/test_forward_dynamics_host.py says
why the accelerations are held to it in FORCE space (the round trip rnea(q, v, a_out) + damping a_out - sum J'w = tau_in, once through the
library's own wbcqp_inverse_dynamics -- an independent kernel -- and once through the oracle's rnea and Jacobians) and the SPD commands directly.
With tau NULL (zero) max(1, |tau|) is 1 and the bar is 1e-10 ABSOLUTE, while the forces the solve balances are the bias nle - sum J'w, up to
2.4e4 on the 62-body chain.  That bar is kept wherever the reference procedure itself (the oracle's M, LAPACK's Cholesky, the oracle's rnea back:
_reference_residual, computed here per case and wrench selection) stays REF_MULTIPLE = 4 times under it.  Where it does not -- the chain: 9.9e-11
with eight wrenches, 0.99 of the bar -- the bar is 4 times the reference procedure's own residual.  Four, because the round trip crosses between
two formulations in double (the device's common-frame recursion, the oracle's body-local one) and meets the rounding the reference procedure has
once, in the bias and in M a, once on either side.
The shapes are the ones at which the kernel can go wrong: one body, the lane limit (64 bodies fixed; 59 bodies floating = nv 64, the largest
LDS image), a pure chain, a star, a tree, Talos, a fixed-base arm; batches that are no multiple of the four instances of a workgroup."""
import ctypes as C

import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import forward_dynamics as fd
from tests import model_queries as mq
from tests.model_queries import BATCHES, _torch
from tests.test_forward_dynamics_host import CASES, DT, case_states, oracle_round_trip
from tests.test_gpu_inverse_dynamics import TOL_F32, TOL_ROWS, _padded, _rel, _selections

pytestmark = pytest.mark.gpu

NMAX = max(BATCHES)
TREES = [n for n in CASES if n != "franka"]  # the cases of tests/test_gpu_inverse_dynamics.py plus Talos
SELECTIONS = ("none", "one", "eight_with_repeats", "two_on_one_body")
MODES = ("v_null", "tau_null", "ldt_padded", "damping")
KP, KD = (float(g) for g in fd.spd_gains(DT))
REF_MULTIPLE = 4  # see the module's docstring


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _set(handle, name, slot=3):
    m, st, tm = CASES[name]()
    handle.set_structure(slot, st)
    handle.set_model(slot, m, tm)
    return m, st, tm


def _read(whole, B, width, what, nan_row=None):
    """mq.read_guarded for B rows; nan_row: the one row that may (here: must be free to) hold NaN, which a NaN-prefilled buffer cannot tell
    from an unwritten one -- every other row is written and finite, nothing behind the end is touched."""
    if nan_row is None:
        return mq.read_guarded(whole, B * width, what).reshape(B, width)
    a = whole.cpu().numpy()
    assert mq.unwritten(a[B * width:]).all(), (what, "written past the end")
    a = a[:B * width].reshape(B, width)
    assert np.isfinite(np.delete(a, nan_row, axis=0)).all(), (what, "an element was not written")
    return a


def _mass(h, slot, B, nv, q, torch, dev, td=None):
    whole, part = mq.guarded(B * nv * nv, td or torch.float64, dev, torch)
    h.mass_matrix(slot, B, q[:B].contiguous(), part, stream=_stream(torch))
    torch.cuda.synchronize()
    return mq.read_guarded(whole, B * nv * nv, "M").reshape(B, nv, nv)


def _fdyn(h, slot, B, nv, q, v, tau, w, damping, torch, dev, td=None, nan_row=None):
    """One launch on device tensors -> (a [B, nv], info [B]); tau: None, or [N, ldt] passed as it is (ldt = its row length)."""
    wa, pa = mq.guarded(B * nv, td or torch.float64, dev, torch)
    wi, pi = mq.guarded(B, torch.int32, dev, torch)
    h.forward_dynamics(slot, B, q[:B].contiguous(), pa, v=None if v is None else v[:B].contiguous(), tau=None if tau is None else tau[:B].contiguous(),
                       wrench=None if w is None else w[:B].contiguous(), damping=damping, info=pi, stream=_stream(torch))
    torch.cuda.synchronize()
    return _read(wa, B, nv, "a", nan_row), mq.read_guarded(wi, B, "info")


def _spd(h, slot, B, nv, q, v, target, ldtarget, w, torch, dev, td=None, nan_row=None, qddot=True):
    """One launch -> (commands [B, nv], qddot [B, nv] or None, info [B]); target is passed as it is, rows ldtarget apart."""
    wc, pc = mq.guarded(B * nv, td or torch.float64, dev, torch)
    wq, pq = mq.guarded(B * nv, td or torch.float64, dev, torch)
    wi, pi = mq.guarded(B, torch.int32, dev, torch)
    h.spd_commands(slot, B, (DT, KP, KD), q[:B].contiguous(), target, pc, v=None if v is None else v[:B].contiguous(),
                   ldtarget=ldtarget, wrench=None if w is None else w[:B].contiguous(), qddot=pq if qddot else None, info=pi, stream=_stream(torch))
    torch.cuda.synchronize()
    if not qddot:
        assert mq.unwritten(wq.cpu().numpy()).all()
    return _read(wc, B, nv, "commands", nan_row), _read(wq, B, nv, "qddot", nan_row) if qddot else None, mq.read_guarded(wi, B, "info")


def _inverse(h, slot, B, nv, q, v, a, w, torch, dev):
    whole, part = mq.guarded(B * nv, torch.float64, dev, torch)
    h.inverse_dynamics(slot, B, q[:B].contiguous(), part, v=None if v is None else v[:B].contiguous(), a=a, lda=nv,
                       wrench=None if w is None else w[:B].contiguous(), stream=_stream(torch))
    torch.cuda.synchronize()
    return mq.read_guarded(whole, B * nv, "tau").reshape(B, nv)


def _unrelated(m):
    """[nv, nv] bool: dofs whose bodies lie on different branches (neither in the other's subtree)."""
    last = m.subtree_last()
    body = np.zeros(m.nv, np.int64)
    for b in range(m.nbody):
        body[m.idx_v(b):m.idx_v(b) + (6 if b == 0 and m.floating_base else 1)] = b
    lo, hi = np.minimum.outer(body, body), np.maximum.outer(body, body)
    return hi > last[lo]


@pytest.mark.parametrize("name", list(CASES))
def test_mass_matrix_parity(handle, name):
    from oracle import rbd
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    qn, vn, _ = case_states(m, tm, NMAX, 91_000)
    om = rbd.OracleModel(m)
    want = np.stack([rbd.rbd_terms(om, qn[i], vn[i])["M"] for i in range(NMAX)])
    q = torch.from_numpy(qn).to(dev)
    big = _mass(handle, 3, NMAX, m.nv, q, torch, dev)
    e = _rel(big, want)
    print("mass matrix parity, %-26s %.1e (|M| up to %.3g)" % (name, e, np.abs(want).max()))
    assert e <= TOL_ROWS
    assert np.array_equal(big, big.transpose(0, 2, 1)), "the two triangles differ in bits"
    apart = _unrelated(m)
    assert (big[:, apart] == 0.0).all(), "an entry between unrelated branches is not an exact zero"
    if name in ("tree_24_floating", "talos", "star_17_floating"):
        assert apart.any()
    for B in BATCHES[:-1]:
        assert np.array_equal(_mass(handle, 3, B, m.nv, q, torch, dev), big[:B]), (B, "the same rows in a smaller batch: other bits")
    assert np.array_equal(handle.mass_matrix_host(3, qn[:5]), big[:5])  # the host-pointer entry point: the same kernel, the same bits


def _reference_residual(rbd, om, m, qn, vn, terms, frames, wn, Jl):
    """What the reference procedure itself leaves in the round trip with tau NULL, absolute: a = (the oracle's M)^-1 (-nle + sum J'w) by LAPACK's
    Cholesky factorisation and two triangular solves, then the oracle's rnea and Jacobians back."""
    a = np.zeros((qn.shape[0], m.nv))
    for i, t in enumerate(terms):
        b = -t["nle"]
        for k, f in enumerate(frames):
            b = b + t["Jl"][f].T @ wn[i, k]
        L = np.linalg.cholesky(t["M"])
        a[i] = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return float(np.abs(oracle_round_trip(rbd, om, m, qn, vn, a, frames, wn, None, Jl)).max())


@pytest.mark.parametrize("name", TREES)
def test_forward_dynamics_round_trip(handle, name):
    from oracle import rbd
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    nv = m.nv
    qn, vn, taun = case_states(m, tm, NMAX, 92_000)
    om = rbd.OracleModel(m)
    terms = [rbd.rbd_terms(om, qn[i], vn[i]) for i in range(NMAX)]
    Jl = np.stack([t["Jl"] for t in terms])
    q, v, tau = torch.from_numpy(qn).to(dev), torch.from_numpy(vn).to(dev), torch.from_numpy(taun).to(dev)
    wide = _padded(taun, torch, dev)
    dampn = np.linspace(0.0, 0.3, nv)
    worst = {}
    for sel in SELECTIONS:
        frames = _selections(m)[sel]
        handle.set_wrench_frames(3, frames)
        wn = 50.0 * np.random.default_rng(92_500 + len(frames)).standard_normal((NMAX, len(frames), 6))
        w = torch.from_numpy(wn).to(dev) if frames else None
        for mode in MODES:
            vv, vvn = (None, None) if mode == "v_null" else (v, vn)
            tt, ttn = (None, np.zeros_like(taun)) if mode == "tau_null" else (wide if mode == "ldt_padded" else tau, taun)
            dd = dampn if mode == "damping" else None
            big, info = _fdyn(handle, 3, NMAX, nv, q, vv, tt, w, dd, torch, dev)
            assert (info == 0).all(), (name, sel, mode)
            # through the library's own inverse dynamics, and through the oracle's
            back = _inverse(handle, 3, NMAX, nv, q, vv, torch.from_numpy(big).to(dev), w, torch, dev) + (0.0 if dd is None else dd * big)
            e_lib = _rel(back, ttn)
            e_ora = _rel(oracle_round_trip(rbd, om, m, qn, vvn, big, frames, wn, dd, Jl), ttn)
            bar = TOL_ROWS
            if mode == "tau_null":  # (max(1, |tau|) is 1: the figures are absolute; the module's docstring says where the bar is not the issue's)
                ref = _reference_residual(rbd, om, m, qn, vn, terms, frames, wn, Jl)
                bar = max(TOL_ROWS, REF_MULTIPLE * ref)
                print("tau NULL, %-26s %-18s device %.1e (library) %.1e (oracle), reference procedure %.1e, bar %.1e" % (name, sel, e_lib, e_ora, ref, bar))
            worst[mode] = max(worst.get(mode, 0.0), e_lib, e_ora)
            assert e_lib <= bar and e_ora <= bar, (name, sel, mode, e_lib, e_ora, bar)
            for B in BATCHES[:-1]:
                got, gi = _fdyn(handle, 3, B, nv, q, vv, tt, w, dd, torch, dev)
                assert np.array_equal(got, big[:B]) and (gi == 0).all(), (name, sel, mode, B, "the same rows in a smaller batch: other bits")
            if mode == "ldt_padded":  # the padding is never read: the bits of ldt = nv
                assert np.array_equal(big, _fdyn(handle, 3, NMAX, nv, q, vv, tau, w, dd, torch, dev)[0]), (name, sel)
    print("forward dynamics round trip, worst per mode, %-26s %s" % (name, "  ".join("%s %.1e" % kv for kv in worst.items())))


def _spd_inputs(m, tm, n, seed):
    qn, vn, _ = case_states(m, tm, n, seed)
    target = qn[:, m.nq - m.na:] + 0.05 * np.random.default_rng(seed + 7).standard_normal((n, m.na))
    return qn, vn, target


@pytest.mark.parametrize("name", ["talos", "tree_24_floating", "tree_59_floating_nv_limit", "franka"])
def test_spd_commands_parity(handle, name):
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    nv, na, nbase = m.nv, m.na, m.nv - m.na
    qn, vn, tn = _spd_inputs(m, tm, NMAX, 93_000)
    frames = _selections(m)["two_on_one_body"]
    handle.set_wrench_frames(3, frames)
    wn = 50.0 * np.random.default_rng(93_500).standard_normal((NMAX, 2, 6))
    q, v, t, w = (torch.from_numpy(x).to(dev) for x in (qn, vn, tn, wn))
    want = fd.spd_commands(m, qn, vn, tn, DT, KP, KD, frames, wn)
    cmd, qdd, info = _spd(handle, 3, NMAX, nv, q, v, t, na, w, torch, dev)
    e = float(np.abs(cmd - want["commands"]).max() / np.abs(want["commands"]).max())
    print("SPD commands parity, %-26s %.1e (|commands| up to %.3g)" % (name, e, np.abs(want["commands"]).max()))
    assert (info == 0).all() and e <= TOL_ROWS
    assert (cmd[:, :nbase] == 0.0).all()  # no gains on a floating base's six: no command there (none at all on a fixed base)
    # qddot is wbcqp_forward_dynamics with tau = p + d and damping = kd dt: the same kernel body, the same bits
    tau = np.zeros((NMAX, nv))
    tau[:, nbase:] = -KP * (qn[:, m.nq - na:] + vn[:, nbase:] * DT - tn) + -KD * vn[:, nbase:]
    damp = np.zeros(nv)
    damp[nbase:] = KD * DT
    a, ai = _fdyn(handle, 3, NMAX, nv, q, v, torch.from_numpy(tau).to(dev), w, damp, torch, dev)
    assert np.array_equal(qdd, a) and (ai == 0).all()
    for B in BATCHES[:-1]:
        c, qd, _ = _spd(handle, 3, B, nv, q, v, t[:B].contiguous(), na, w, torch, dev)
        assert np.array_equal(c, cmd[:B]) and np.array_equal(qd, qdd[:B]), B
    # qddot is optional; target rows may lie ldtarget apart: a q array as the target (pointer + nq - na, ldtarget = nq) is the zero position error
    c, none, _ = _spd(handle, 3, NMAX, nv, q, v, q[:, m.nq - na:], m.nq, w, torch, dev, qddot=False)
    c2, _, _ = _spd(handle, 3, NMAX, nv, q, v, q[:, m.nq - na:].contiguous(), na, w, torch, dev)
    assert none is None and np.array_equal(c, c2) and not np.array_equal(c, cmd)
    host = handle.spd_commands_host(3, (DT, KP, KD), qn[:5], vn[:5], tn[:5], wn[:5])
    assert np.array_equal(host["commands"], cmd[:5]) and np.array_equal(host["qddot"], qdd[:5]) and (host["info"] == 0).all()


def test_f32_handle(handle):
    """float in, double inside, float out.  M is the F64 result rounded; the accelerations are held to the F64 handle's on the same (float) inputs:
    the bias passes through a float on its way from rnea_kernel (include/wbcqp.h), so they are not its rounding."""
    from oracle import rbd
    torch, dev = _torch()
    m, st, tm = _set(handle, "talos")
    nv = m.nv
    frames = [m.frame("leg_left_6_joint"), m.frame("leg_right_6_joint")]
    handle.set_wrench_frames(3, frames)
    qn, vn, taun = case_states(m, tm, 9, 94_000)
    tn = qn[:, m.nq - m.na:] + 0.05
    wn = 50.0 * np.random.default_rng(94_500).standard_normal((9, 2, 6))
    q32, v32, tau32, w32, t32 = (x.astype(np.float32) for x in (qn, vn, taun, wn, tn))
    q64, v64, tau64, w64, t64 = (x.astype(np.float64) for x in (q32, v32, tau32, w32, t32))
    damp = np.full(nv, KD * DT)
    M64 = handle.mass_matrix_host(3, q64)
    a64, _ = handle.forward_dynamics_host(3, q64, v64, tau64, w64, damp)
    s64 = handle.spd_commands_host(3, (DT, KP, KD), q64, v64, t64, w64)
    h32 = capi.Handle(0, capi.F32)
    try:
        h32.set_structure(0, st)
        h32.set_model(0, m, tm)
        h32.set_wrench_frames(0, frames)
        up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
        M32 = _mass(h32, 0, 9, nv, up(q32), torch, dev, td=torch.float32)
        a32, i32 = _fdyn(h32, 0, 9, nv, up(q32), up(v32), up(tau32), up(w32), damp, torch, dev, td=torch.float32)
        c32, qd32, _ = _spd(h32, 0, 9, nv, up(q32), up(v32), up(t32), m.na, up(w32), torch, dev, td=torch.float32)
        hM, (ha, hi), hs = h32.mass_matrix_host(0, q32), h32.forward_dynamics_host(0, q32, v32, tau32, w32, damp), h32.spd_commands_host(
            0, (DT, KP, KD), q32, v32, t32, w32)
    finally:
        h32.close()
    assert M32.dtype == np.float32 and np.array_equal(M32, hM) and np.array_equal(a32, ha) and np.array_equal(c32, hs["commands"])
    assert np.array_equal(M32, M64.astype(np.float32))
    om = rbd.OracleModel(m)
    assert _rel(M32.astype(np.float64), np.stack([rbd.rbd_terms(om, q64[i], v64[i])["M"] for i in range(9)])) <= TOL_F32
    ea, ec = _rel(a32.astype(np.float64), a64), _rel(c32.astype(np.float64), s64["commands"])
    print("F32 handle against the F64 handle on the same inputs: a %.1e (|a| up to %.3g), commands %.1e (|commands| up to %.3g)" %
          (ea, np.abs(a64).max(), ec, np.abs(s64["commands"]).max()))
    assert (i32 == 0).all() and ea <= TOL_F32 and ec <= TOL_F32


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    m, st, tm = _set(handle, "tree_24_floating")
    frames = _selections(m)["eight_with_repeats"]
    handle.set_wrench_frames(3, frames)
    qn, vn, tn = _spd_inputs(m, tm, NMAX, 95_000)
    taun = case_states(m, tm, NMAX, 95_000)[2]
    wn = 50.0 * np.random.default_rng(95_500).standard_normal((NMAX, 8, 6))
    q, v, t, tau, w = (torch.from_numpy(x).to(dev) for x in (qn, vn, tn, taun, wn))

    def run(lo, hi):
        B = hi - lo
        a, _ = _fdyn(handle, 3, B, m.nv, q[lo:hi], v[lo:hi], tau[lo:hi], w[lo:hi], None, torch, dev)
        c, qd, _ = _spd(handle, 3, B, m.nv, q[lo:hi].contiguous(), v[lo:hi], t[lo:hi].contiguous(), m.na, w[lo:hi], torch, dev)
        return {"M": _mass(handle, 3, B, m.nv, q[lo:hi], torch, dev), "a": a, "commands": c, "qddot": qd}

    mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(run, NMAX)


def test_nothing_else_moves(handle):
    def query(s, tick):
        handle.set_wrench_frames(3, list(range(8)))
        B, nv = s["q"].shape[0], s["v"].shape[1]
        handle.mass_matrix_host(3, s["q"])
        handle.forward_dynamics_host(3, s["q"], s["v"], np.ones((B, nv)), np.ones((B, 8, 6)), np.full(nv, 0.1))
        handle.spd_commands_host(3, (DT, KP, KD), s["q"], s["v"], s["q"][:, 7:], np.ones((B, 8, 6)))

    mq.nothing_else_moves(handle, mq.talos_case(), 96_000, query, observed=[1, 4, 9])


@pytest.mark.parametrize("name", ["talos", "tree_59_floating_nv_limit"])
def test_a_bad_instance_stays_alone(handle, name):
    """NaN in one instance's q (a value, not a fault: no address depends on q): info != 0 and an all-NaN row there; every other row and info
    has the bits of the batch without the plant."""
    torch, dev = _torch()
    m, st, tm = _set(handle, name)
    nv = m.nv
    handle.set_wrench_frames(3, [2])
    qn, vn, tn = _spd_inputs(m, tm, NMAX, 97_000)
    taun = case_states(m, tm, NMAX, 97_000)[2]
    wn = 50.0 * np.random.default_rng(97_500).standard_normal((NMAX, 1, 6))
    bad = 41
    qb = qn.copy()
    qb[bad, m.nq - 3] = np.nan
    v, t, tau, w = (torch.from_numpy(x).to(dev) for x in (vn, tn, taun, wn))
    others = np.arange(NMAX) != bad
    res = {}
    for tag, qq in (("clean", qn), ("planted", qb)):
        q = torch.from_numpy(qq).to(dev)
        a, ai = _fdyn(handle, 3, NMAX, nv, q, v, tau, w, None, torch, dev, nan_row=None if tag == "clean" else bad)
        c, qd, ci = _spd(handle, 3, NMAX, nv, q, v, t, m.na, w, torch, dev, nan_row=None if tag == "clean" else bad)
        res[tag] = (a, ai, c, qd, ci)
    assert (res["clean"][1] == 0).all() and (res["clean"][4] == 0).all() and all(np.isfinite(x).all() for x in res["clean"])
    a, ai, c, qd, ci = res["planted"]
    assert ai[bad] != 0 and ci[bad] != 0
    assert np.isnan(a[bad]).all() and np.isnan(c[bad]).all() and np.isnan(qd[bad]).all()
    for got, want in zip(res["planted"], res["clean"]):
        assert np.array_equal(got[others], want[others])


def _both_case(handle, seed, B=4):
    m, st, tm = _set(handle, "talos")
    qn, vn, tn = _spd_inputs(m, tm, B, seed)
    taun = case_states(m, tm, B, seed)[2]
    return (m,) + tuple(mq.both(x) for x in (qn, vn, taun, tn, np.ones((B, 2, 6))))


def test_host_refusals_are_the_device_refusals(handle):
    m, q, v, tau, t, w = _both_case(handle, 98_000)
    nv, na = m.nv, m.na
    M, a, cmd, qdd = mq.prefilled_both(4 * nv * nv), mq.prefilled_both(4 * nv), mq.prefilled_both(4 * nv), mq.prefilled_both(4 * nv)
    info = mq.prefilled_both(4, int32=True)
    outs = [M, a, cmd, qdd, info]
    keep = [np.full(nv, 0.1), np.full(nv, -0.1), np.full(nv, np.inf), capi.CSpd(DT, KP, KD), capi.CSpd(0.0, KP, KD), capi.CSpd(DT, np.nan, KD),
            capi.CSpd(DT, KP, np.inf), capi.CSpd(np.nan, KP, KD)]
    good, neg, inf = (x.ctypes.data for x in keep[:3])
    law, dt0, kpnan, kdinf, dtnan = (C.addressof(x) for x in keep[3:])
    # a wrench while no frames are selected
    mq.host_refusals_match(handle, "forward_dynamics", [(3, 4, q, v, tau, nv, w, None, a, info)], outs)
    mq.host_refusals_match(handle, "spd_commands", [(3, 4, law, q, v, t, na, w, cmd, qdd, info)], outs)
    handle.set_wrench_frames(3, [3, 5])
    mq.host_refusals_match(handle, "mass_matrix", [(9, 4, q, M),      # a slot without a model
                                                   (3, -1, q, M),     # a negative batch
                                                   (3, 4, None, M),   # q NULL
                                                   (3, 4, q, None)],  # M NULL
                           outs)
    mq.host_refusals_match(handle, "forward_dynamics", [(9, 4, q, v, tau, nv, None, None, a, info),    # a slot without a model
                                                        (3, -1, q, v, tau, nv, w, good, a, info),      # a negative batch
                                                        (3, 4, None, v, tau, nv, w, good, a, info),    # q NULL
                                                        (3, 4, q, v, tau, nv, w, good, None, info),    # a NULL
                                                        (3, 4, q, v, tau, nv - 1, w, good, a, info),   # ldt < nv with tau given
                                                        (3, 4, q, v, tau, nv, w, neg, a, info),        # a negative damping
                                                        (3, 4, q, v, tau, nv, w, inf, a, info)],       # a non-finite damping
                           outs)
    mq.host_refusals_match(handle, "spd_commands", [(9, 4, law, q, v, t, na, None, cmd, qdd, info),    # a slot without a model
                                                    (3, -1, law, q, v, t, na, w, cmd, qdd, info),      # a negative batch
                                                    (3, 4, law, None, v, t, na, w, cmd, qdd, info),    # q NULL
                                                    (3, 4, law, q, v, t, na, w, None, qdd, info),      # commands NULL
                                                    (3, 4, law, q, v, None, na, w, cmd, qdd, info),    # target NULL
                                                    (3, 4, law, q, v, t, na - 1, w, cmd, qdd, info),   # ldtarget < na
                                                    (3, 4, None, q, v, t, na, w, cmd, qdd, info),      # law NULL
                                                    (3, 4, dt0, q, v, t, na, w, cmd, qdd, info),       # dt <= 0
                                                    (3, 4, dtnan, q, v, t, na, w, cmd, qdd, info),     # dt not finite
                                                    (3, 4, kpnan, q, v, t, na, w, cmd, qdd, info),     # kp not finite
                                                    (3, 4, kdinf, q, v, t, na, w, cmd, qdd, info)],    # kd not finite
                           outs)
    # batch == 0: WBCQP_OK through either entry point, nothing written
    for side in (0, 1):
        mq.raw(handle, "mass_matrix", side, 3, 0, q, M)
        mq.raw(handle, "forward_dynamics", side, 3, 0, q, v, tau, nv, w, good, a, info)
        mq.raw(handle, "spd_commands", side, 3, 0, law, q, v, t, na, w, cmd, qdd, info)
    mq.host_batch_zero(handle, "forward_dynamics", [(3, 0, q, None, None, 0, None, None, a, info)], outs)
    mq.host_batch_zero(handle, "spd_commands", [(3, 0, law, q, None, t, na, None, cmd, None, None)], outs)
    mq.host_batch_zero(handle, "mass_matrix", [(3, 0, q, M)], outs)
    # and what is not looked at: ldt without tau; info and qddot are optional
    mq.raw(handle, "forward_dynamics", 0, 3, 4, q, v, None, 0, w, None, a, None)
    mq.raw(handle, "spd_commands", 1, 3, 4, law, q, None, t, na, None, cmd, None, None)
    _torch()[0].cuda.synchronize()
    assert np.isfinite(a[0].cpu().numpy()).all() and np.isfinite(cmd[1]).all()
    assert mq.unwritten(info[0].cpu().numpy()).all() and mq.unwritten(qdd[1]).all() and mq.unwritten(info[1]).all()


def test_a_traced_squat_in_one_call():
    """A traced squat (batch 8, 12 ticks, stride 1): one call with batch = n_rec * batch answers every recorded tick, bit for bit what tick-by-tick
    calls give.  Entry r's tau and x go with entry r - 1's state (include/wbcqp.h); the decoded tau is zero-padded to nv and the QP's contact
    wrenches enter at the contact frames, so the round trip through wbcqp_inverse_dynamics gives the padded tau back."""
    torch, dev = _torch()
    B, K = 8, 12
    h, m, st, tm, trace, q0, v0 = mq.traced_squat(B, K, 1, lambda h, m, tm: h.set_wrench_frames(0, tm.contact_frame), more=("x", "tau", "status"))
    try:
        nv = m.nv
        assert (trace["status"] == 0).all().item()
        qb = torch.cat([q0[None], trace["q"][:-1]]).reshape(K * B, -1).contiguous()
        vb = torch.cat([v0[None], trace["v"][:-1]]).reshape(K * B, -1).contiguous()
        T = torch.from_numpy(np.asarray(st.force_gen()).reshape(st.nc, 6, 12)).to(dev)
        w = torch.einsum("cij,rbcj->rbci", T, trace["x"][..., st.nv:].reshape(K, B, st.nc, 12)).reshape(K * B, st.nc, 6).contiguous()
        tau = torch.zeros(K * B, nv, dtype=torch.float64, device=dev)
        tau[:, nv - m.na:] = trace["tau"].reshape(K * B, -1)[:, :m.na]
        whole, info = _fdyn(h, 0, K * B, nv, qb, vb, tau, w, None, torch, dev)
        assert (info == 0).all()
        for r in range(K):
            sl = slice(r * B, (r + 1) * B)
            tick, _ = _fdyn(h, 0, B, nv, qb[sl], vb[sl], tau[sl], w[sl], None, torch, dev)
            assert np.array_equal(whole[sl], tick), r
        back = _inverse(h, 0, K * B, nv, qb, vb, torch.from_numpy(whole).to(dev), w, torch, dev)
        e = _rel(back, tau.cpu().numpy())
        print("forward dynamics over a traced squat (12 x 8 ticks): round trip %.1e" % e)
        assert e <= TOL_ROWS
        cmd, _, ci = _spd(h, 0, K * B, nv, qb, vb, trace["q"].reshape(K * B, -1)[:, m.nq - m.na:], m.nq, w, torch, dev)  # target: the next state
        assert (ci == 0).all() and np.isfinite(cmd).all()
    finally:
        h.close()
