"""Reference programs on the host (no GPU): the numpy expansion of inria_wbc_amd.refprog against the streams it restates (model.WalkOnSpotPlan,
trajs.move_com_stream, trajs.cartesian_stream), bit for bit; the refusals of the device-free wbcqp_check_program; the C ABI's new declarations."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import capi, refprog, trajs
from inria_wbc_amd import model as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _walk(Tc=0.05, Tf=0.02, step=0.05):
    m = mdl.talos_like()
    sets = mdl.talos_contact_sets(m)
    return m, sets, mdl.WalkOnSpotPlan(m, {k: tm for k, (_, tm) in sets.items()}, Tc, Tf, step)


def test_walk_on_spot_program_expands_to_the_plan_bit_for_bit():
    m, sets, plan = _walk(0.4, 0.15, 0.05)  # intro 400, cycle 1400
    prog = refprog.walk_on_spot_program(plan)
    assert (prog.n_intro, prog.n_cycle) == (plan.phase_len[0], plan.cycle) == (400, 1400)
    start, n = 150, 3000
    offsets = np.array([0, 1, 149, 150, 151, 700, 2500, 3300, -40])  # before, at and after `start`; one that never starts in the window
    assert start + n > prog.length + offsets[5]  # the wrap is crossed
    ref, sch = refprog.expand(prog, plan.base, offsets, start, n)
    sch_want, ref_want = plan.plan(offsets, start, n)
    assert ref.dtype == np.float64 and sch.dtype == np.int32
    assert np.array_equal(sch, sch_want)
    assert np.array_equal(ref, ref_want), np.argwhere(ref != ref_want)[:5]
    assert set(np.unique(sch)) == {0, 1, 2}
    # the same window in two pieces is the same rows
    a, _ = refprog.expand(prog, plan.base, offsets, start, 1000)
    b, _ = refprog.expand(prog, plan.base, offsets, start + 1000, n - 1000)
    assert np.array_equal(np.concatenate([a, b]), ref)


def test_move_com_program_expands_to_the_squat_stream_bit_for_bit():
    m = mdl.talos_like()
    dt, dst, nref = 1e-3, 7, 40
    pos, vel, acc = trajs.move_com_stream(m.com(m.q0), [[0.0, 0.0, -0.2]], "001", dt, 2.0, loop=True, absolute=False)
    prog = refprog.move_com_program(nref, dst, m.com(m.q0), [[0.0, 0.0, -0.2]], "001", dt, 2.0, loop=True, absolute=False)
    assert (prog.n_intro, prog.n_cycle) == (0, 4000) == (0, len(pos))
    base = np.random.default_rng(0).standard_normal(nref)
    ref, sch = refprog.expand(prog, base, [0, -37, 4100], 0, 4200)
    assert sch is None
    want = np.concatenate([pos, vel, acc], axis=1)
    assert np.array_equal(ref[:4000, 0, dst:dst + 9], want)
    assert np.array_equal(ref[4000:, 0, dst:dst + 9], want[:200])  # the loop
    assert np.array_equal(ref[:, 1, dst:dst + 9], want[(np.arange(4200) + 37) % 4000])
    assert np.array_equal(ref[:4100, 2, dst:dst + 9], np.tile(want[0], (4100, 1)))  # not started: the first sample
    keep = np.r_[0:dst, dst + 9:nref]
    assert np.array_equal(ref[..., keep], np.broadcast_to(base[keep], ref[..., keep].shape))
    # absolute targets, no loop: the last sample is held
    pos, vel, acc = trajs.move_com_stream(m.com(m.q0), [[0.1, 0.0, 0.7], [0.0, 0.05, 0.8]], "101", dt, 0.3, loop=False, absolute=True)
    prog = refprog.move_com_program(nref, dst, m.com(m.q0), [[0.1, 0.0, 0.7], [0.0, 0.05, 0.8]], "101", dt, 0.3, loop=False, absolute=True)
    ref, _ = refprog.expand(prog, base, [0], 0, len(pos) + 5)
    want = np.concatenate([pos, vel, acc], axis=1)
    assert np.array_equal(ref[:len(pos), 0, dst:dst + 9], want) and np.array_equal(ref[len(pos):, 0, dst:dst + 9], np.tile(want[-1], (5, 1)))


def test_cartesian_program_expands_to_the_cartesian_stream_bit_for_bit():
    m = mdl.talos_like()
    Rf, pf = m.frame_placements(m.q0)
    f = m.frame("leg_left_6_joint")
    R0 = mdl._rot(2, 0.3) @ mdl._rot(0, -0.2) @ Rf[f]
    dt, dst, nref = 1e-3, (3, 50), 80
    args = dict(rel_pos=[0.05, -0.02, 0.1], dt=dt, duration=0.25, loop=True, rel_rpy=[0.3, -0.2, 0.5])
    R, p, vel, acc = trajs.cartesian_stream(R0, pf[f], **args)
    prog = refprog.cartesian_program(nref, dst, R0, pf[f], **args)
    assert prog.tracks[0].segments[0].angle > 0.1
    base = np.random.default_rng(1).standard_normal(nref)
    ref, _ = refprog.expand(prog, base, [0, 13], 0, len(p))
    want = np.concatenate([p, np.swapaxes(R, 1, 2).reshape(-1, 9), vel, acc], axis=1)
    for d in dst:
        assert np.array_equal(ref[:, 0, d:d + 24], want)
        assert np.array_equal(ref[13:, 1, d:d + 24], want[:len(p) - 13])
    keep = np.r_[0:3, 27:50, 74:80]
    assert np.array_equal(ref[..., keep], np.broadcast_to(base[keep], ref[..., keep].shape))
    # a relative track starts from every instance's own placement
    rel = refprog.cartesian_program(nref, 3, np.eye(3), np.zeros(3), relative=True, **args)
    bases = np.random.default_rng(2).standard_normal((2, nref))
    for i, ang in enumerate((0.4, -1.1)):
        bases[i, 6:15] = mdl._rot(1, ang).T.reshape(9)
    ref, _ = refprog.expand(rel, bases, [0, 0], 0, 100)
    R1, p1, v1, a1 = trajs.cartesian_stream(np.eye(3), np.zeros(3), **args)
    for i, ang in enumerate((0.4, -1.1)):
        Rb = mdl._rot(1, ang)
        assert np.allclose(ref[:, i, 3:6], bases[i, 3:6] + p1[:100], rtol=0, atol=1e-15)
        assert np.allclose(ref[:, i, 6:15].reshape(-1, 3, 3).transpose(0, 2, 1), Rb @ R1[:100], rtol=0, atol=1e-15)
        assert np.allclose(ref[:, i, 18:21], v1[:100, 3:] @ Rb.T, rtol=0, atol=1e-12)


def _refused(prog, batch, n_slots, *needles, offsets=None):
    with pytest.raises(capi.WbcqpError) as e:
        capi.check_program(prog, batch, n_slots, offsets)
    assert e.value.code == 1
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def test_check_program_refuses_what_the_header_lists(built_lib):
    m, sets, plan = _walk()
    good = refprog.walk_on_spot_program(plan)
    capi.check_program(good, 5, 3)
    capi.check_program(good, 5, 0)

    def variant(f):
        p = copy.deepcopy(good)
        f(p)
        return p

    hold = lambda n: [(np.zeros(3), np.zeros(3), 1.0, n)]  # noqa: E731
    many = variant(lambda p: [p.add_vec(200 + k, hold(p.length), dim=1) for k in range(14)])
    assert len(many.tracks) == 17
    _refused(many, 5, 3, "17 tracks")
    _refused(variant(lambda p: p.tracks[1].segments.pop()), 5, 3, "track 1", "180 ticks", "230")
    _refused(variant(lambda p: setattr(p.tracks[2].segments[3], "n_steps", 0)), 5, 3, "track 2", "segment 3", "n_steps")
    _refused(variant(lambda p: setattr(p.tracks[0].segments[1], "T", 0.0)), 5, 3, "track 0", "segment 1", "T <= 0")
    _refused(variant(lambda p: setattr(p.tracks[2], "dst", (good.nref - 8, -1))), 5, 3, "track 2", "leaves [0, nref")
    _refused(variant(lambda p: setattr(p.tracks[2], "dst", (p.tracks[0].dst[1] + 20, -1))), 5, 3, "track 2", "overlaps track 0")
    _refused(variant(lambda p: setattr(p.tracks[2], "dim", 2)), 5, 3, "track 2", "dim 2")
    _refused(variant(lambda p: setattr(p.tracks[0].segments[2], "axis", np.array([1.0, 0.1, 0.0]))), 5, 3, "track 0", "segment 2", "unit")

    def bad_set(p):
        p.set_of = p.set_of.copy()
        p.set_of[77] = 3
    _refused(variant(bad_set), 5, 3, "set_of[77] = 3")
    capi.check_program(variant(bad_set), 5, 4)
    empty = refprog.Program(10, 1e-3, 0, 0)
    _refused(empty, 1, 1, "empty timeline")


def test_new_symbols_are_declared_exported_and_bound(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    lib = ctypes.CDLL(built_lib)
    bound = {"wbcqp_check_program": capi.check_program, "wbcqp_reference_samples": capi.Handle.reference_samples,
             "wbcqp_rollout_program": capi.Handle.rollout_program, "wbcqp_rollout_mixed_program": capi.Handle.rollout_mixed_program}
    for sym, f in bound.items():
        assert sym in declared and sym in capi.EXPORTS and hasattr(lib, sym) and callable(f), sym
    assert lib.wbcqp_version() == 151
    for name in ("wbcqp_segment", "wbcqp_track", "wbcqp_program"):
        assert "} %s;" % name in hdr
    # the structs as the header lays them out (LP64): segment = int32 + pad, then 20 doubles; track = six int32, a pointer; program below
    assert ctypes.sizeof(capi.CSegment) == 8 + 8 * 20 == 168 and capi.CSegment.T.offset == 8 and capi.CSegment.angle.offset == 160
    assert ctypes.sizeof(capi.CTrack) == 32 and capi.CTrack.segments.offset == 24
    assert ctypes.sizeof(capi.CProgram) == 64
    assert [f for f, _ in capi.CProgram._fields_] == ["nref", "base_stride", "base", "offset", "n_intro", "n_cycle", "dt", "n_tracks", "tracks", "set_of"]
    assert (refprog.TRACK_VEC, refprog.TRACK_SE3, refprog.POSE_ONLY, refprog.RELATIVE, refprog.MAX_TRACKS) == (0, 1, 1, 2, 16)
    for text in ("WBCQP_TRACK_VEC = 0", "WBCQP_TRACK_SE3 = 1", "#define WBCQP_TRACK_POSE_ONLY 1", "#define WBCQP_TRACK_RELATIVE 2", "#define WBCQP_MAX_TRACKS 16"):
        assert text in hdr
