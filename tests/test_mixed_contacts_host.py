"""Host side of a fleet in mixed contact sets (no GPU): the contact-subset task maps share the full stack's reference layout and pass the
library's model check, and the walk-on-spot plan switches contact sets where walk_on_spot.cpp does, on floor(T / dt) phase boundaries."""
import ctypes

import numpy as np
import pytest

from inria_wbc_amd import capi, structure
from inria_wbc_amd import model as mdl


@pytest.mark.parametrize("robot", ["talos", "icub"])
def test_contact_subset_maps_share_the_full_layout_and_pass_the_model_check(robot):
    m = mdl.talos_like() if robot == "talos" else mdl.icub_like()
    sets = mdl.talos_contact_sets(m) if robot == "talos" else mdl.icub_contact_sets(m)
    full_st = structure.talos_structure() if robot == "talos" else structure.icub_structure()
    full = mdl.build_taskmap(m, full_st, mdl.talos_stack() if robot == "talos" else mdl.icub_stack())
    assert list(sets)[:2] == ["both", "no_l"] and len(sets) == (3 if robot == "talos" else 2)
    for name, (st, tm) in sets.items():
        assert tm.nref == full.nref
        assert [b.ref for b in tm.blocks] == [b.ref for b in full.blocks] and tm.posture_ref == full.posture_ref
        for c, f in enumerate(tm.contact_frame):  # a kept contact has the offset it has in the full map
            assert tm.contact_ref[c] == full.contact_ref[list(full.contact_frame).index(f)]
        assert tm.ncontact == st.nc == (2 if name == "both" else 1)
        assert capi.check_model(st, m, tm) > 0, name
    if robot == "talos":  # no_l keeps the right foot, no_r the left one -- on the same single-support shape
        assert sets["no_l"][1].contact_frame[0] == m.frame("leg_right_6_joint")
        assert sets["no_r"][1].contact_frame[0] == m.frame("leg_left_6_joint")
        assert sets["no_l"][0].n == sets["no_r"][0].n == 62


def test_contact_subset_map_refused_on_its_own_layout_is_not_the_shared_one():
    # the single-support stack built on its own has a shorter reference row: that is what a mix refuses (nref differs)
    m = mdl.talos_like()
    own = mdl.build_taskmap(m, structure.talos_structure(single_support=True), [n for n in mdl.talos_stack() if n["name"] != "contact_lfoot"])
    assert own.nref == mdl.talos_contact_sets(m)["no_l"][1].nref - 24


@pytest.mark.parametrize("T,dt", [(1.0, 1e-3), (0.2, 1e-3), (0.1, 1e-3), (0.03, 1e-3), (0.3, 1e-3)])
def test_walk_on_spot_plan_switches_on_floor_boundaries(T, dt):
    m = mdl.talos_like()
    maps = {k: tm for k, (_, tm) in mdl.talos_contact_sets(m, dt).items()}
    n = int(np.floor(T / dt))
    plan = mdl.WalkOnSpotPlan(m, maps, T, T, 0.03)
    assert plan.phase_len == [n] * 7 and plan.cycle == 6 * n
    assert plan.phase_names == ["INIT", "LIFT_UP_LF", "LIFT_DOWN_LF", "MOVE_COM_LEFT", "LIFT_UP_RF", "LIFT_DOWN_RF", "MOVE_COM_RIGHT"]
    both, no_l, no_r = (mdl.WalkOnSpotPlan.SETS.index(s) for s in ("both", "no_l", "no_r"))
    sch, ref = plan.plan([0], 0, n + 2 * 6 * n)
    s = sch[:, 0]
    # remove_contact on the first tick of LIFT_UP_xF, add_contact on the last tick of LIFT_DOWN_xF (walk_on_spot.cpp:165-184)
    want = np.full(s.size, both)
    for c in range(2):
        b = n + c * 6 * n
        want[b:b + 2 * n - 1] = no_l
        want[b + 3 * n:b + 5 * n - 1] = no_r
    assert np.array_equal(s, want)
    # staggered: instance i is instance 0 delayed by offsets[i]; before its start it stands on both feet on INIT's first sample
    offs = [0, 7, n + 3]
    sch2, ref2 = plan.plan(offs, 5, 3 * n)
    for i, o in enumerate(offs):
        for t in range(3 * n):
            k = 5 + t - o
            assert sch2[t, i] == (s[k] if k >= 0 else both)
            assert np.array_equal(ref2[t, i], ref[max(k, 0), 0])
    # the references: LIFT_DOWN_LF starts step_height up, the contact's reference is the foot's, the CoM is over the right foot after INIT
    lf = plan.lf_ref
    assert abs(ref[2 * n, 0, lf + 2] - ref[0, 0, lf + 2] - 0.03) < 1e-12
    assert np.array_equal(ref[:, 0, plan.cl_ref:plan.cl_ref + 12], ref[:, 0, lf:lf + 12])
    assert np.allclose(ref[n, 0, plan.com_ref:plan.com_ref + 2], plan.rf_low[:2])
    assert (ref[:, 0, plan.cl_ref + 12:plan.cl_ref + 24] == 0).all()


def test_mixed_entry_points_are_declared_and_bound():
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "wbcqp.h")).read()
    for sym in ("wbcqp_tick_mixed", "wbcqp_rollout_mixed"):
        assert sym + "(" in hdr and sym in capi.EXPORTS
    assert ctypes.sizeof(capi.CMix) == 4 + 4 + 8 + 8 + 8 + 8  # int32 n_slots (+ padding), slots, w, tlb, tub
