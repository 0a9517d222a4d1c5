"""CPU tests of the stabiliser (wbcqp_stabilize): the numpy transcription of the reference's CoP estimator, filters and admittance laws
(inria_wbc_amd/stabilizer.py) on hand-worked cases, both sides of Eigen's euler branch, the filters' semantics, the two guards, the library's
surface (symbols, state_bytes), the streams the GPU tests run, and observe.py's acom against the rigid-body oracle.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import stabilizer_cases as sc
from inria_wbc_amd import model as mdl
from inria_wbc_amd import stabilizer as stb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1  # WBCQP_ERR_INVALID (include/wbcqp.h)
TOL_ROWS = 1e-10  # tests/test_gpu_terms.py
DT = sc.DT


def run(s, ticks, state=None):
    """step() over a list of inputs with one state; the outputs per tick."""
    state = np.zeros((ticks[0]["ref"].shape[0], stb.state_bytes(s.window)), np.uint8) if state is None else state
    return [stb.step(s, state, t) for t in ticks], state


def with_(inp, **changes):
    out = {k: (v.copy() if v is not None else None) for k, v in inp.items()}
    for k, v in changes.items():
        out[k] = v
    return out


def cop_shift(inp, dx=0.0, dy=0.0, feet=(0, 1), fz=400.0):
    """The same inputs with the raw CoP of the given feet moved by (dx, dy) through the ankle torques: cop.x += -torque.y / fz, cop.y += torque.x / fz."""
    w = inp["wrench"].copy()
    for f in feet:
        w[:, 6 * f + 3] = dy * fz
        w[:, 6 * f + 4] = -dx * fz
    return with_(inp, wrench=w)


def lifted(inp, foot):
    w = inp["wrench"].copy()
    w[:, 6 * foot:6 * foot + 6] = 0.0
    return with_(inp, wrench=w)


# ---- a robot in balance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", sc.WINDOWS)
def test_a_robot_in_balance_is_left_alone(window):
    for s in (sc.mini_stab(window), sc.talos_stab(window)):
        inp = sc.balanced(s, 2)
        outs, state = run(s, [inp] * (window + 3))
        for t, o in enumerate(outs):
            assert sc.bits(o["ref_out"]) == sc.bits(inp["ref"]), (window, t)  # identity rotations included, bit for bit
            want = stb.COP | stb.LCOP | stb.RCOP | stb.COM | stb.LANKLE | stb.RANKLE | stb.FFDA if t >= window - 1 else 0
            assert (o["flags"] == want).all(), (window, t, o["flags"])
        assert np.array_equal(outs[-1]["cop"][0], [[0.125, 0.0], sc.LP[:2], sc.RP[:2]])
        assert np.isnan(outs[0]["cop"]).all() == (window > 1)


# ---- hand-worked numbers ---------------------------------------------------------------------------------------------------------------------
def test_a_cop_offset_moves_the_com_reference_by_the_gains():
    s = sc.mini_stab(2)
    inp = cop_shift(sc.balanced(s), dx=0.0625)  # both feet's CoP, hence the combined one, 1/16 m ahead: cor = zmp - cop = -1/16
    outs, _ = run(s, [inp, inp])
    r, r0 = outs[1]["ref_out"][0], inp["ref"][0]
    assert np.array_equal(outs[1]["cop"][0], [[0.1875, 0.0], [0.1875, 0.25], [0.1875, -0.25]])
    # pos -= p0 cor = +0.5/16; vel -= p2 cor / dt = +(0.25/16) 128; acc -= p4 cor / dt^2 = +(0.125/16) 16384; y: cor = 0
    assert r[0] == 0.125 + 0.03125 and r[3] == 2.0 and r[6] == 128.0
    assert r[1] == 0.0 and r[4] == 0.0 and r[7] == 0.0 and np.array_equal(r[[2, 5, 8]], r0[[2, 5, 8]])
    # ankles: pitch = 0.5 (cop.x - foot.x) = 1/32, roll = 0: vel[4] += 0.5 pitch / dt = 2, acc[4] += 0.25 pitch / dt^2 = 128
    for foot, contact in ((s.lf_ref, s.lf_contact_ref), (s.rf_ref, s.rf_contact_ref)):
        assert r[foot + 12 + 4] == 2.0 and r[foot + 18 + 4] == 128.0 and r[foot + 12 + 3] == 0.0 and r[foot + 18 + 3] == 0.0
        assert np.array_equal(r[foot:foot + 3], r0[foot:foot + 3]) and np.array_equal(r[contact:contact + 3], r0[contact:contact + 3])
        assert np.array_equal(r[contact + 12:contact + 24], r[foot + 12:foot + 24])  # the contact takes the FOOT TASK's velocity and acceleration
        R = r[foot + 3:foot + 12].reshape(3, 3).T  # column-major
        Ry = np.array([[math.cos(0.03125), 0, math.sin(0.03125)], [0, 1, 0], [-math.sin(0.03125), 0, math.cos(0.03125)]])
        assert np.abs(R - Ry).max() < 1e-15 and np.array_equal(r[contact + 3:contact + 12], r[foot + 3:foot + 12])
    assert outs[0]["flags"][0] == 0 and np.array_equal(outs[0]["ref_out"], inp["ref"])  # the window is not full yet
    # sideways: roll = 0.25 (cop.y - foot.y) = 1/64: vel[3] += 0.25 roll / dt = 0.5, acc[3] += 0.125 roll / dt^2 = 32
    inp = cop_shift(sc.balanced(s), dy=0.0625)
    r = run(s, [inp, inp])[0][1]["ref_out"][0]
    assert r[1] == 0.25 * 0.0625 and r[4] == (0.125 * 0.0625) / DT and r[7] == (0.0625 * 0.0625) / (DT * DT) and r[0] == 0.125
    assert r[s.lf_ref + 12 + 3] == 0.5 and r[s.lf_ref + 18 + 3] == 32.0 and r[s.lf_ref + 12 + 4] == 0.0
    assert abs(r[s.lf_ref + 3 + 5] - math.sin(1 / 64)) < 1e-15  # R(2,1) of Rx(roll)


def test_the_torso_rolls_by_the_difference_of_the_feet_normal_forces():
    s = sc.mini_stab(1)
    inp = sc.balanced(s)
    x = inp["x_prev"].copy()
    x[0, s.lf_force_col + 2::3][:4] = 125.0  # n_l = 500, n_r = 300 in the previous solution; the sensors read 400 and 400
    x[0, s.rf_force_col + 2::3][:4] = 75.0
    x[0, s.lf_force_col] = 1e3  # a tangential force: the normal is z, it counts for nothing
    o = stb.step(s, None, with_(inp, x_prev=x))
    r, t = o["ref_out"][0], s.torso_ref
    troll = 2.0 ** -10 * 200.0
    assert o["flags"][0] & stb.FFDA and r[t + 12 + 3] == 0.5 * troll / DT == 12.5 and r[t + 18 + 3] == 0.25 * troll / (DT * DT) == 800.0
    assert abs(r[t + 3 + 5] - math.sin(troll)) < 1e-15 and np.array_equal(r[t:t + 3], inp["ref"][0, t:t + 3])
    # no previous solution (the first tick), or a contact that is not active: no torso law, everything else as before
    for other in (stb.step(s, None, with_(inp, x_prev=None)), stb.step(sc.mini_stab(1, rf_force_col=-1), None, with_(inp, x_prev=x))):
        assert not other["flags"][0] & stb.FFDA and sc.bits(other["ref_out"][0, t:t + 24]) == sc.bits(inp["ref"][0, t:t + 24])
    # a foot whose contact is not active keeps its references, whatever its CoP says
    s1 = sc.mini_stab(1, lf_contact_ref=-1, lf_force_col=-1)
    o = stb.step(s1, None, cop_shift(inp, dx=0.0625))
    assert o["flags"][0] == stb.COP | stb.LCOP | stb.RCOP | stb.COM | stb.RANKLE
    assert sc.bits(o["ref_out"][0, s.lf_ref:s.lf_ref + 24]) == sc.bits(inp["ref"][0, s.lf_ref:s.lf_ref + 24])
    assert sc.bits(o["ref_out"][0, 81:105]) == sc.bits(inp["ref"][0, 81:105])


# ---- Eigen's eulerAngles(0, 1, 2) ------------------------------------------------------------------------------------------------------------
def test_both_sides_of_the_euler_branch_recompose_to_the_input():
    col = lambda R: R.T.reshape(9)  # noqa: E731
    ident = stb.euler_012(col(np.eye(3)))
    assert ident[3] is False and ident[:3] == (0.0, 0.0, 0.0) and sc.bits(np.array(stb.recompose(col(np.eye(3)), 0.0, 0.0))) == sc.bits(col(np.eye(3)))
    above, below = mdl._rot(0, 1e-3), mdl._rot(0, -1e-3)
    # Rx(a): atan2(R(1,2), R(2,2)) = -a, so a roll just BELOW zero takes the r0 > 0 side, where the first angle becomes pi - |a|
    ea, eb = stb.euler_012(col(above)), stb.euler_012(col(below))
    assert ea[3] is False and eb[3] is True and abs(ea[0] - 1e-3) < 1e-15 and abs(eb[0] - (math.pi - 1e-3)) < 1e-15 and 0 <= eb[0] <= math.pi
    rng = np.random.default_rng(5)
    worst, scale, flips = 0.0, 0.0, 0
    for k in range(400):
        e = rng.normal(0.0, 1.0, 3) if k >= 2 else (1e-3 * (1 - 2 * k), 0.0, 0.0)
        R = mdl._rot(0, e[0]) @ mdl._rot(1, e[1]) @ mdl._rot(2, e[2])
        back = np.array(stb.recompose(col(R), 0.0, 0.0))
        worst = max(worst, np.abs(back - col(R)).max())
        flips += stb.euler_012(col(R))[3]
        # the transcription's own rounding: its distance from the same formulas in extended precision, with a correction on top
        d0, d1 = rng.normal(0.0, 0.05, 2)
        long = np.array([float(x) for x in stb.recompose(col(R), d0, d1, stb.LONGDOUBLE)])
        scale = max(scale, np.abs(np.array(stb.recompose(col(R), d0, d1)) - long).max())
    print("euler round trip: %.1e; recompose in double against long double: %.1e (%d of 400 on the r0 > 0 side)" % (worst, scale, flips))
    assert worst < 5e-15 and scale < 5e-15 and 100 < flips < 300
    # on the r0 > 0 side an added pitch acts with the opposite sign (what the reference does)
    pa, pb = np.array(stb.recompose(col(above), 0.0, 0.01)), np.array(stb.recompose(col(below), 0.0, 0.01))
    assert pa[6] > 0.009 and pb[6] < -0.009  # R(0,2) = sin(pitch) on one side, -sin(pitch) on the other


# ---- the filters' semantics --------------------------------------------------------------------------------------------------------------------
def test_a_lifted_foot_resets_its_filter_and_not_the_combined_one():
    s = sc.mini_stab(3)
    a = sc.balanced(s)
    b = cop_shift(a, dx=0.1875)  # the CoPs three sixteenths ahead
    seq = [a, a, a, lifted(a, 0), b, b, b]
    outs, state = run(s, seq)
    V = stb.COP | stb.LCOP | stb.RCOP
    assert [int(o["flags"][0] & V) for o in outs] == [0, 0, V, stb.RCOP, stb.COP | stb.RCOP, stb.COP | stb.RCOP, V]
    # tick 3: the only valid CoP is the right one, and the CoM law takes it (cor = zmp - rcop = (0, 0.25))
    assert outs[3]["flags"][0] & stb.COM and outs[3]["ref_out"][0, 1] == -0.25 * 0.25 and outs[3]["ref_out"][0, 0] == 0.125
    # tick 4: touch-down.  The combined window still holds two samples from before the lift: (A + A + B) / 3, valid at once
    assert outs[4]["cop"][0, 0, 0] == ((0.125 + 0.125) + 0.3125) / 3.0 and np.isnan(outs[4]["cop"][0, 1]).all()
    assert outs[6]["cop"][0, 0, 0] == 0.3125 and outs[6]["cop"][0, 1, 0] == 0.3125
    counts = state.view(np.int32)[0, :10:2]
    assert counts.tolist() == [3, 3, 3, 3, 3]
    # the left filter was emptied at the lift; the left force filter was not fed at the lift but kept its samples (3 pushes before it: ready)
    st3 = np.zeros((1, stb.state_bytes(3)), np.uint8)
    run(s, seq[:4], st3)
    assert st3.view(np.int32)[0, :10:2].tolist() == [3, 0, 3, 3, 3]


def test_valid_cop_falls_back_from_combined_to_left_to_right():
    s = sc.mini_stab(2)
    a = cop_shift(cop_shift(sc.balanced(s), dx=0.0625, feet=(0,)), dx=-0.0625, feet=(1,))  # left CoP ahead, right behind, combined in the middle
    outs, _ = run(s, [a, a, lifted(a, 1), lifted(a, 0), lifted(lifted(a, 0), 1)])
    com_x = [float(o["ref_out"][0, 0]) for o in outs]
    # cor.x = 0.125 - cop.x: combined 0.125, left 0.1875 (after the right foot lifts), right 0.0625 ... one sample is not a window of two
    assert com_x[1] == 0.125 and com_x[2] == 0.125 - 0.5 * (0.125 - 0.1875)
    assert outs[2]["flags"][0] & (stb.COP | stb.LCOP | stb.RCOP) == stb.LCOP
    laws = stb.COP | stb.LCOP | stb.RCOP | stb.COM | stb.LANKLE | stb.RANKLE  # (the torso law does not look at the CoP)
    assert outs[3]["flags"][0] & laws == 0 and outs[4]["flags"][0] & laws == 0 and com_x[3] == com_x[4] == 0.125  # the right filter restarted at tick 3
    outs, _ = run(s, [a, a, lifted(a, 0)])
    assert outs[2]["flags"][0] & (stb.COP | stb.LCOP | stb.RCOP) == stb.RCOP and outs[2]["ref_out"][0, 0] == 0.125 - 0.5 * (0.125 - 0.0625)


@pytest.mark.parametrize("window", [1, 2, 7])
def test_a_nan_sample_invalidates_for_exactly_a_window(window):
    s = sc.mini_stab(window)
    a = sc.balanced(s)
    bad = a["wrench"].copy()
    bad[0, 4] = np.nan  # the left ankle's torque about y
    seq = [a] * window + [with_(a, wrench=bad)] + [a] * (window + 1)
    outs, _ = run(s, seq)
    V = stb.COP | stb.LCOP | stb.RCOP
    got = [int(o["flags"][0] & V) for o in outs[window - 1:]]
    assert got == [V] + [stb.RCOP] * window + [V] * (len(got) - window - 1), got
    assert np.isnan(outs[window]["cop"][0, :2]).all() and not np.isnan(outs[window]["cop"][0, 2]).any()
    assert all(o["flags"][0] & stb.COM for o in outs[window - 1:])  # the right foot's CoP carries the CoM law meanwhile


# ---- the guards --------------------------------------------------------------------------------------------------------------------------------
def test_the_guards_set_their_bits_and_return_the_references_unmodified():
    s = sc.mini_stab(2)
    a = cop_shift(sc.balanced(s), dx=0.0625)
    far = with_(a, placement=a["placement"] + 16.0)  # every CoP sixteen metres away in x and in y
    outs, state = run(s, [far, far, far])
    assert outs[0]["flags"][0] == 0
    for o in outs[1:]:
        assert o["flags"][0] == stb.COP | stb.LCOP | stb.RCOP | stb.ERR_COP and sc.bits(o["ref_out"]) == sc.bits(a["ref"])
    _, clean = run(s, [a, a, a])
    assert state.view(np.int32)[0, :10].tolist() == clean.view(np.int32)[0, :10].tolist() == [2, 1] * 5  # the filters advanced all the same
    # far in x alone is no error (the reference asks for both)
    place = a["placement"].copy()
    place[0, [s.lf_pos, s.rf_pos]] += 16.0
    assert not run(s, [with_(a, placement=place)] * 2)[0][1]["flags"][0] & stb.ERR_COP
    # the force guard sits inside the torso law: 800 N on a 5 kg robot, once both force filters are ready and a previous solution exists
    light = sc.mini_stab(2, mass=5.0)
    outs, state = run(light, [with_(a, x_prev=None), a, a])
    assert not outs[0]["flags"][0] & stb.ERR_FORCE and outs[0]["flags"][0] == 0
    for o in outs[1:]:
        assert o["flags"][0] == stb.COP | stb.LCOP | stb.RCOP | stb.ERR_FORCE and sc.bits(o["ref_out"]) == sc.bits(a["ref"])
    assert sc.states_equal(state, clean)
    # other instances of the batch are not affected
    two = {k: np.concatenate([far[k], a[k]]) for k in a}
    o = run(s, [two, two])[0][1]
    assert o["flags"][0] & stb.ERR_COP and o["flags"][1] == stb.COP | stb.LCOP | stb.RCOP | stb.COM | stb.LANKLE | stb.RANKLE | stb.FFDA
    assert o["ref_out"][1, 0] == 0.125 + 0.03125


# ---- the streams the GPU tests run -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 7])
def test_the_parity_streams_decide_clearly_and_reach_every_branch(window):
    for s in (sc.mini_stab(window), sc.tree_stab(window)):
        ticks = sc.streams(s, 31_000 + window)
        outs, states = sc.reference_run(s, ticks)  # (asserts)
        assert len(outs) == 3 * window + 5 and ticks[0]["x_prev"] is None and states[-1].shape == (sc.NMAX, 40 + 64 * window)
        # a stream cut anywhere and carried on gives the same bits; no state at all is a fresh one
        cut = window + 2
        state = np.zeros_like(states[0])
        for t in ticks[:cut]:
            stb.step(s, state, t)
        assert sc.bits(state) == sc.bits(states[cut - 1])
        first = stb.step(s, None, ticks[0])
        assert all(np.array_equal(first[k], outs[0][k], equal_nan=True) for k in first)


# ---- the library's surface ---------------------------------------------------------------------------------------------------------------------
NEW = {"wbcqp_stabilizer_state_bytes", "wbcqp_stabilize", "wbcqp_stabilize_host", "wbcqp_observe_acom", "wbcqp_observe_acom_host"}


def test_symbols_declared_exported_bound_and_null_handle(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(capi.EXPORTS)
    assert re.search(r"#define\s+WBCQP_MAX_STAB_WINDOW\s+64\b", hdr)
    for name in ("COP", "LCOP", "RCOP", "COM", "LANKLE", "RANKLE", "FFDA", "ERR_COP", "ERR_FORCE"):
        assert re.search(r"WBCQP_STAB_%s\s*=\s*%d\b" % (name, getattr(stb, name)), hdr), name
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in NEW:
        assert hasattr(raw, sym) and getattr(lib, sym).argtypes, sym
    for name in ("stabilize", "stabilize_host"):
        assert callable(getattr(capi.Handle, name))
    assert ctypes.sizeof(capi.CObservables) == 4 * ctypes.sizeof(ctypes.c_void_p)  # acom is an argument of its own: the struct keeps its size
    assert lib.wbcqp_observe_acom(None, 0, 1, None, None, None, None, None) == ERR_INVALID
    assert lib.wbcqp_observe_acom_host(None, 0, 1, None, None, None, None) == ERR_INVALID
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cs, cin, out = capi.c_stabilizer(sc.mini_stab(3)), capi.CStabInputs(p, p, p, p, p, 24, None, 0), capi.CStabOutputs(p, None, None)
    assert lib.wbcqp_stabilize(None, ctypes.byref(cs), 1, ctypes.byref(cin), None, ctypes.byref(out), None) == ERR_INVALID
    assert lib.wbcqp_stabilize_host(None, ctypes.byref(cs), 1, ctypes.byref(cin), None, ctypes.byref(out)) == ERR_INVALID


def test_state_bytes_of_valid_and_refused_stabilizers(built_lib):
    from inria_wbc_amd import capi
    for w in sc.WINDOWS:
        for s in (sc.mini_stab(w), sc.talos_stab(w), sc.tree_stab(w)):
            assert capi.stabilizer_state_bytes(s) == stb.state_bytes(w) == 40 + 64 * w
    bad = [dict(window=0), dict(window=65), dict(dt=0.0), dict(dt=-1e-3), dict(dt=np.nan), dict(dt=np.inf), dict(mass=0.0), dict(mass=np.nan),
           dict(com_gains=(0, 0, np.inf, 0, 0, 0)), dict(ankle_gains=(np.nan, 0, 0, 0, 0, 0)), dict(ffda_gains=(0, 0, np.nan)), dict(normal=(0, np.inf, 1)),
           dict(com_ref=-1), dict(lf_ref=-1), dict(rf_ref=-3), dict(torso_ref=-1), dict(lf_contact_ref=-2), dict(rf_force_col=-2), dict(lf_pos=-1), dict(rf_pos=-1),
           dict(nref=128), dict(com_ref=121), dict(torso_ref=106), dict(rf_contact_ref=106), dict(nref=-1),
           dict(lf_ref=0), dict(lf_contact_ref=57), dict(rf_ref=10)]  # (the last three: two blocks overlap)
    for kw in bad:
        assert capi.stabilizer_state_bytes(sc.mini_stab(**{"window": 3, **kw})) == 0, kw
    assert capi.stabilizer_state_bytes(None) == 0
    ok = [dict(lf_contact_ref=-1), dict(lf_force_col=-1, rf_force_col=-1), dict(com_gains=(0,) * 6), dict(normal=(0, 0, -1)), dict(nref=200, com_ref=191)]
    for kw in ok:
        assert capi.stabilizer_state_bytes(sc.mini_stab(3, **kw)) == 232, kw


def test_from_taskmap_finds_the_offsets_by_name():
    from inria_wbc_amd import structure
    m = mdl.talos_like()
    tm = mdl.build_taskmap(m, structure.talos_structure(), mdl.talos_stack())
    s = sc.talos_stab(5)
    blk = {b.name: b.ref for b in tm.blocks}
    assert (s.com_ref, s.lf_ref, s.rf_ref, s.torso_ref) == (blk["com"], blk["lf"], blk["rf"], blk["torso"]) and s.nref == tm.nref
    assert (s.lf_contact_ref, s.rf_contact_ref) == tuple(tm.contact_ref) and (s.lf_force_col, s.rf_force_col) == (m.nv, m.nv + 12)
    assert s.mass == m.inertia[:, 0].sum() and s.dt == tm.dt and (s.lf_pos, s.rf_pos) == (9, 21)
    sets = mdl.talos_contact_sets(m)
    name = next(k for k, (st, _) in sets.items() if st.nc == 1)
    st1, tm1 = sets[name]
    kept = [c.name for c in st1.contacts]
    s1 = stb.from_taskmap(m, tm1, mdl.talos_stack(), 5, sc.COM_GAINS, sc.ANKLE_GAINS, sc.FFDA_GAINS, contacts=kept)
    gone = "lf" if kept == ["contact_rfoot"] else "rf"
    assert getattr(s1, gone + "_contact_ref") == -1 and getattr(s1, gone + "_force_col") == -1 and s1.nref == tm.nref
    assert {s1.lf_contact_ref, s1.rf_contact_ref} == {-1, int(tm1.contact_ref[0])} and {s1.lf_force_col, s1.rf_force_col} == {-1, m.nv}
    with pytest.raises(KeyError):
        stb.from_taskmap(m, tm, mdl.talos_stack(), 5, sc.COM_GAINS, sc.ANKLE_GAINS, sc.FFDA_GAINS, names=dict(torso="chest"))


# ---- acom ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["talos", "tree"])
def test_observe_acom_against_the_oracle(name):
    from oracle import rbd
    from inria_wbc_amd import observe
    m = mdl.talos_like() if name == "talos" else mdl.random_tree(3, 24, True)
    qs, vs = [], []
    for k in range(6):
        rng = np.random.default_rng(52_000 + k)
        q = m.q0.copy()
        q[7:] += 0.3 * rng.standard_normal(m.na)
        q[0:3] += rng.standard_normal(3)
        q[3:7] += 0.3 * rng.standard_normal(4)
        q[3:7] /= np.linalg.norm(q[3:7])
        qs.append(q)
        vs.append(0.5 * rng.standard_normal(m.nv))
    q, v = np.stack(qs), np.stack(vs)
    got = observe.observe(m, q, v, [], acom=True)
    om = rbd.OracleModel(m)
    want = np.stack([rbd.rbd_terms(om, q[i], v[i])["acom"].copy() for i in range(6)])
    err = np.abs(got["acom"] - want).max() / max(1.0, np.abs(want).max())
    print("observe.py's acom against the oracle, %s: %.1e (largest entry %.2f)" % (m.name, err, np.abs(want).max()))
    assert err <= TOL_ROWS and np.abs(want).max() > 0.1
    assert "acom" not in observe.observe(m, q, v, []) and np.array_equal(observe.observe(m, q, v, [])["vcom"], got["vcom"])
