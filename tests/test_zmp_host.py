"""CPU tests of the ZMP force distributor (wbcqp_stabilize_zmp) and of a tick's force references (wbcqp_set_force_references): the transcription
(inria_wbc_amd/stabilizer.py: zmp_distribute, zmp_admittance, step(zmp=...)) on hand-worked power-of-two cases, its guards and their order, the streams
the GPU parity grid runs (every branch reached, every comparison clear), the library's surface, the task maps with force references, and the solver
inputs of the GPU tests through the oracle.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import model as mdl
from inria_wbc_amd import stabilizer as stb
from inria_wbc_amd import structure
from tests import force_ref_cases as fc
from tests import stabilizer_cases as sc
from tests import zmp_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
DT = 2.0 ** -7
PL, PR = (0.0, 0.125), (0.0, -0.125)
M = 64.0
HALF = -32.0 * 9.81  # ((-0.5) 64) 9.81: half the weight, as the law signs it
FULL = -64.0 * 9.81


def neg_zero(x):
    return x == 0.0 and math.copysign(1.0, x) < 0


# ---- distribute: hand-worked ------------------------------------------------------------------------------------------------------------------
def test_on_the_segment_the_weight_splits_by_the_projection():
    # u = (0, -1/4), e = (0, -1), dd = -1/8, proj = (0, 0): L = 1/4, a1 = a2 = 1/8, alpha = 1/2
    alpha, left, right, ok = stb.zmp_distribute(M, (0.03125, 0.0), PL, PR)
    assert ok and alpha == 0.5
    # tau0.x = (1/32) f_r + (1/32) f_l = f / 16 < 0: all of it on the right foot; tau0.y = (1/8) f_r - (1/8) f_l = 0
    assert left == [0.0, 0.0, HALF, 0.0, 0.0, 0.0] and right == [0.0, 0.0, HALF, 0.0, -HALF / 16, 0.0]
    assert neg_zero(left[4]) and not neg_zero(left[3])  # -tauL.x with tauL.x = +0: the sign is kept
    # a quarter of the way from the left foot: alpha = 1/4
    alpha, left, right, ok = stb.zmp_distribute(M, (0.0, 0.0625), PL, PR)
    assert ok and alpha == 0.25 and left[2] == (-0.75 * M) * 9.81 and right[2] == (-0.25 * M) * 9.81


def test_beyond_a_foot_that_foot_takes_everything():
    alpha, left, right, ok = stb.zmp_distribute(M, (0.0, 0.5), PL, PR)  # beyond the left foot: a1 = 3/8 < a2 = 5/8, residual 3/4
    assert ok and alpha == 0.0 and left[2] == FULL and neg_zero(right[2])
    assert left[3] == 0.375 * FULL and right[3] == 0.0  # tau0.y = -(PL.y - z.y) f_l = (3/8) f_l, all of it (1 - alpha) on the left
    alpha, left, right, ok = stb.zmp_distribute(M, (0.0, -0.5), PL, PR)
    assert ok and alpha == 1.0 and right[2] == FULL and neg_zero(left[2]) and right[3] == -0.375 * FULL  # tau0.y = -(PR.y - z.y) f_r


def test_exactly_on_a_foot():
    alpha, left, right, ok = stb.zmp_distribute(M, PL, PL, PR)  # proj = PL: a1 = 0, a2 = L, on the segment: alpha = 0 / L
    assert ok and alpha == 0.0 and left[2] == FULL and left[3] == 0.0
    alpha, left, right, ok = stb.zmp_distribute(M, PR, PL, PR)
    assert ok and alpha == 1.0 and right[2] == FULL


def test_one_foot_only():
    alpha, left, right, ok = stb.zmp_distribute(M, (0.03125, 0.0), PL, (7.0, 7.0), True, False)  # left only: alpha = 0, PR = (0, 0) whatever is passed
    assert ok and alpha == 0.0 and left[2] == FULL and neg_zero(right[2])
    # tau0 = -(PL - z) f_l = (f_l / 32, -f_l / 8): x < 0, so the RIGHT block carries it although that foot is in the air (as the reference)
    assert left == [0.0, 0.0, FULL, -FULL / 8, 0.0, 0.0] and right == [0.0, 0.0, 0.0, 0.0, -FULL / 32, 0.0] and neg_zero(left[4])
    alpha, left, right, ok = stb.zmp_distribute(M, (0.03125, 0.0), (7.0, 7.0), PR, False, True)
    # tau0 = -(PR - z) f_r = (f_r / 32, f_r / 8)
    assert ok and alpha == 1.0 and right == [0.0, 0.0, FULL, FULL / 8, -FULL / 32, 0.0] and left == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and neg_zero(left[2])
    with pytest.raises(ValueError):
        stb.zmp_distribute(M, (0.0, 0.0), PL, PR, False, False)


def test_the_sign_of_the_moment_about_x_chooses_the_foot():
    _, left, right, _ = stb.zmp_distribute(M, (0.03125, 0.0), PL, PR)  # tau0.x = f / 16 < 0: the right foot's
    assert right[4] == -HALF / 16 and neg_zero(left[4])
    _, left, right, _ = stb.zmp_distribute(M, (-0.03125, 0.0), PL, PR)  # tau0.x = -f / 16 >= 0: the left foot's
    assert left[4] == HALF / 16 and neg_zero(right[4])
    _, left, right, _ = stb.zmp_distribute(M, (0.0, 0.0), PL, PR)  # tau0.x = 0: not < 0, the left foot's
    assert neg_zero(left[4]) and neg_zero(right[4])


def test_coincident_feet_give_a_nan_alpha_and_no_error():
    alpha, left, right, ok = stb.zmp_distribute(M, (0.03125, 0.0), PL, PL)  # |0 - 0 - 0| < 1e-10: alpha = 0 / 0
    assert ok and math.isnan(alpha) and math.isnan(left[2]) and math.isnan(right[2])


def test_non_finite_inputs_reach_the_branch_that_should_not_exist():
    for z in ((math.nan, 0.0), (0.0, math.nan), (math.inf, 0.0)):
        alpha, _, _, ok = stb.zmp_distribute(M, z, PL, PR)
        assert not ok and math.isnan(alpha), z


def test_admittance_gains_select_the_model_or_the_measurement():
    zero, one = (0.0,) * 6, (1.0,) * 6
    zm, zs = (0.03125, 0.0), (0.0, 0.5)  # the model's ZMP on the segment (alpha 1/2), the measured one beyond the left foot (alpha 0)
    _, tl, tr, _ = stb.zmp_distribute(M, zm, PL, PR)
    _, sl, sr, _ = stb.zmp_distribute(M, zs, PL, PR)
    left, right, at, am, ok = stb.zmp_admittance(DT, zero, zero, M, zm, zs, PL, PR)
    assert ok and (at, am) == (0.5, 0.0) and left == tl and right == tr  # p = d = 0: the model's distribution
    left, right, _, _, _ = stb.zmp_admittance(DT, one, zero, M, zm, zs, PL, PR)
    assert np.array_equal(left, sl) and np.array_equal(right, sr)  # p = 1, d = 0: the measured one (t - (t - s) is exact here: s is 2 t or 0)
    # one entry by hand: t = f/2, s = f, e = -f/2; p = 1/2, d = 1/256, dt = 1/128: (t + f/4) + (f/512) 128 = f/2 + f/4 + f/4 = f
    left, _, _, _, _ = stb.zmp_admittance(DT, (0.5,) * 6, (2.0 ** -8,) * 6, M, zm, zs, PL, PR)
    assert left[2] == FULL


# ---- inside a tick ----------------------------------------------------------------------------------------------------------------------------
def run(s, z, ticks):
    state = np.zeros((ticks[0]["ref"].shape[0], stb.state_bytes(s.window)), np.uint8)
    return [stb.step(s, state, t, zmp=z) for t in ticks]


def test_the_law_runs_with_the_com_law_and_writes_both_blocks():
    s, z = zc.mini(2)
    inp = sc.balanced(s, 1)
    inp["ref"][:, 129:141] = 7.0
    outs = run(s, z, [inp, inp, inp])
    assert outs[0]["flags"][0] == 0 and sc.bits(outs[0]["ref_out"]) == sc.bits(inp["ref"]) and np.isnan(outs[0]["alpha"]).all()  # no valid CoP: passes through
    for o in outs[1:]:
        assert o["flags"][0] & stb.ZMP and o["flags"][0] & stb.COM and not o["flags"][0] & (stb.ERR_ZMP | stb.ERR_COP | stb.ERR_FORCE)
        assert np.array_equal(o["alpha"][0], (0.5, 0.5))
        # model and measurement agree (a robot in balance): fref = t.  Feet at x = 1/8 = the ZMP's x: no moment
        half = (-0.5 * 90.0) * 9.81
        assert np.array_equal(o["ref_out"][0, 129:135], (0.0, 0.0, half, 0.0, 0.0, 0.0)) and np.array_equal(o["ref_out"][0, 135:141], (0.0, 0.0, half, 0.0, 0.0, 0.0))
    # without the distributor the same tick leaves the blocks alone and every other entry equal
    state = np.zeros((1, stb.state_bytes(2)), np.uint8)
    plain = [stb.step(s, state, inp) for _ in range(3)][-1]
    keep = np.setdiff1d(np.arange(s.nref), np.arange(129, 141))
    assert sc.bits(plain["ref_out"][0, keep]) == sc.bits(outs[-1]["ref_out"][0, keep]) and (plain["ref_out"][0, 129:141] == 7.0).all()
    assert plain["flags"][0] == outs[-1]["flags"][0] & ~stb.ZMP and "alpha" not in plain


def test_offsets_of_minus_one_write_nothing_and_an_inactive_foot_still_gets_its_block():
    s, _ = zc.mini(1)
    inp = sc.balanced(s, 1)
    inp["ref"][:, 129:141] = 7.0
    o = stb.step(s, None, inp, zmp=stb.ZmpDistributor(zc.ZMP_P, zc.ZMP_D, -1, -1))
    assert o["flags"][0] & stb.ZMP and sc.bits(o["ref_out"]) == sc.bits(stb.step(s, None, inp)["ref_out"])
    s, z = zc.mini(1, right=False)  # the right contact is not active: alpha = 0, and the right block is written all the same (with -0 and zeros)
    o = stb.step(s, None, inp, zmp=z)
    assert o["alpha"][0, 0] == 0.0 and o["ref_out"][0, 131] == (-1.0 * 90.0) * 9.81 and (o["ref_out"][0, 135:141] == 0.0).all()
    with pytest.raises(AssertionError):
        stb.step(sc.mini_stab(1, nref=141, lf_contact_ref=-1, rf_contact_ref=-1), None, inp, zmp=z)


def test_a_nan_com_sets_err_zmp_and_leaves_the_references_alone():
    s, z = zc.mini(1)
    inp = sc.balanced(s, 2)
    inp["ref"][:, 129:141] = 7.0
    inp["com"][1, 0] = np.nan
    o = stb.step(s, None, inp, zmp=z)
    assert o["flags"][0] & stb.ZMP and o["flags"][1] == stb.COP | stb.LCOP | stb.RCOP | stb.ERR_ZMP
    assert sc.bits(o["ref_out"][1]) == sc.bits(inp["ref"][1]) and np.isnan(o["alpha"][1]).all() and not np.isnan(o["cop"][1]).any()


def test_the_three_guards_in_the_references_order():
    s, z = zc.mini(1)
    base = sc.balanced(s, 1)
    far = {k: (v.copy() if v is not None else None) for k, v in base.items()}
    far["placement"][:, s.lf_pos:s.lf_pos + 2] += 16.0
    far["placement"][:, s.rf_pos:s.rf_pos + 2] += 16.0
    heavy = {k: (v.copy() if v is not None else None) for k, v in base.items()}
    heavy["wrench"][:, [2, 8]] = 100.0 * s.mass

    def flags(inp, nan_com=False):
        inp = {k: (v.copy() if v is not None else None) for k, v in inp.items()}
        if nan_com:
            inp["com"][0, 1] = np.nan
        state = np.zeros((1, stb.state_bytes(1)), np.uint8)
        o = stb.step(s, state, inp, zmp=z)
        assert sc.bits(o["ref_out"]) == sc.bits(inp["ref"]) and state.any()  # the row is ref's, the filters have advanced
        return int(o["flags"][0]) & (stb.ERR_COP | stb.ERR_ZMP | stb.ERR_FORCE | stb.ZMP | stb.COM)

    assert flags(far) == stb.ERR_COP and flags(far, nan_com=True) == stb.ERR_COP  # far CoP first
    assert flags(base, nan_com=True) == stb.ERR_ZMP and flags(heavy, nan_com=True) == stb.ERR_ZMP  # then the distributor's, before the force guard
    assert flags(heavy) == stb.ERR_FORCE  # the force guard last: no law's bit, ZMP's included


# ---- the streams of the GPU grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", zc.WINDOWS)
@pytest.mark.parametrize("shape", list(zc.SHAPES))
def test_the_parity_streams_reach_every_branch_and_decide_every_comparison_clearly(shape, window):
    s, z = zc.SHAPES[shape](window)
    ticks = zc.streams(s, z, zc.seed_of(shape, window))
    assert len(ticks) == 3 * window + 5
    outs, states = zc.reference_run(s, z, ticks)  # (asserts: branches, margins, pass-through)
    # the stabiliser's own results are what they are without the distributor, wherever ERR_ZMP does not end the tick
    state = np.zeros((sc.NMAX, stb.state_bytes(window)), np.uint8)
    keep = np.setdiff1d(np.arange(s.nref), np.concatenate([np.arange(o, o + 6) for o in (z.lf_force_ref, z.rf_force_ref)]))
    for t, inp in enumerate(ticks):
        plain = stb.step(s, state, inp)
        fine = (outs[t]["flags"] & stb.ERR_ZMP) == 0
        assert np.array_equal(plain["flags"][fine], outs[t]["flags"][fine] & ~stb.ZMP)
        assert np.array_equal(plain["ref_out"][fine][:, keep], outs[t]["ref_out"][fine][:, keep], equal_nan=True)
        assert sc.bits(state) == sc.bits(states[t])


# ---- the library's surface ----------------------------------------------------------------------------------------------------------------------
NEW = {"wbcqp_set_force_references", "wbcqp_stabilize_zmp", "wbcqp_stabilize_zmp_host"}


def test_symbols_declared_exported_bound_and_null_handle(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(capi.EXPORTS)
    assert re.search(r"WBCQP_STAB_ZMP\s*=\s*512\b", hdr) and re.search(r"WBCQP_STAB_ERR_ZMP\s*=\s*1024\b", hdr) and (stb.ZMP, stb.ERR_ZMP) == (512, 1024)
    assert "Not here: the ZMP force distributor" not in hdr and "wbcqp_zmp_distributor" in hdr
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in NEW:
        assert hasattr(raw, sym) and getattr(lib, sym).argtypes, sym
    for name in ("set_force_references", "stabilize_zmp", "stabilize_zmp_host"):
        assert callable(getattr(capi.Handle, name))
    assert ctypes.sizeof(capi.CZmpDistributor) == 12 * 8 + 8
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    s, z = zc.mini(3)
    cs, cz = capi.c_stabilizer(s), capi.c_zmp_distributor(z)
    cin, out = capi.CStabInputs(p, p, p, p, p, 24, None, 0), capi.CStabOutputs(p, None, None)
    assert lib.wbcqp_stabilize_zmp(None, ctypes.byref(cs), ctypes.byref(cz), 1, ctypes.byref(cin), None, ctypes.byref(out), None, None) == ERR_INVALID
    assert lib.wbcqp_stabilize_zmp_host(None, ctypes.byref(cs), ctypes.byref(cz), 1, ctypes.byref(cin), None, ctypes.byref(out), None) == ERR_INVALID
    assert lib.wbcqp_set_force_references(None, 0, None, None) == ERR_INVALID
    # the state is the stabiliser's: the distributor adds nothing to it
    assert capi.stabilizer_state_bytes(s) == stb.state_bytes(3) == 40 + 64 * 3


# ---- task maps with force references ---------------------------------------------------------------------------------------------------------------
def test_build_taskmap_with_force_references():
    m = mdl.talos_like()
    st, stack = structure.talos_structure(), mdl.talos_stack()
    plain, with_ = mdl.build_taskmap(m, st, stack), mdl.build_taskmap(m, st, stack, force_refs=True)
    assert plain.contact_fref is None and plain.nref == 305 and mdl.build_taskmap(m, st, stack, force_refs=False).nref == 305
    assert with_.nref == plain.nref + 6 * with_.ncontact and list(with_.contact_fref) == [305, 311]
    assert np.array_equal(with_.contact_ref, plain.contact_ref) and [b.ref for b in with_.blocks] == [b.ref for b in plain.blocks]
    assert with_.posture_ref == plain.posture_ref
    for sets_of, mk in ((mdl.talos_contact_sets, mdl.talos_like), (mdl.icub_contact_sets, mdl.icub_like)):
        mm = mk()
        old, new = sets_of(mm), sets_of(mm, force_refs=True)
        nref = {tm.nref for _, tm in new.values()}
        full = new["both"][1]
        assert len(nref) == 1 and full.nref == old["both"][1].nref + 12 and list(full.contact_fref) == [full.nref - 12, full.nref - 6]
        names = [n["name"] for n in (mdl.talos_stack() if mk is mdl.talos_like else mdl.icub_stack()) if n["type"] == "contact"]
        for key, (_, tm) in new.items():
            assert tm.contact_fref.size == tm.ncontact and np.array_equal(tm.contact_fref_all, full.contact_fref)  # one offset per contact in every set
            assert np.array_equal(tm.contact_ref, old[key][1].contact_ref) and old[key][1].contact_fref is None
            for c, o in zip(tm.contact_ref, tm.contact_fref):  # the block of the contact whose motion reference sits at c
                assert o == full.contact_fref[list(full.contact_ref).index(c)]
        z = stb.zmp_from_taskmap(new["no_l"][1], mdl.talos_stack() if mk is mdl.talos_like else mdl.icub_stack(), zc.ZMP_P, zc.ZMP_D)
        assert (z.lf_force_ref, z.rf_force_ref) == (full.contact_fref[names.index("contact_lfoot")], full.contact_fref[names.index("contact_rfoot")])


def test_the_latch_moves_a_robot_once_and_for_good():
    latch = stb.ZmpLatch(4)
    assert list(latch.which()) == [0, 0, 0, 0]
    latch.update(np.array([0, stb.ZMP | stb.COM, stb.ERR_ZMP, stb.COM], np.int32))
    assert list(latch.which(2, 5)) == [2, 5, 2, 2]
    latch.update(np.array([stb.ZMP, 0, 0, 0], np.int32))  # robot 1's law did not run this tick: it stays
    assert list(latch.which()) == [1, 1, 0, 0] and list(latch.which(np.array([0, 1, 2, 0]), np.array([3, 4, 5, 3]))) == [3, 4, 2, 0]


def test_the_talos_files_constants():
    f = stb.STAB_FILES["talos"]
    assert f["double_support"]["zmp_w"] == (1.0, 1.0, 1.0, 2.0, 2.0, 2.0) and f["single_support"]["zmp_w"] == (1.0, 1.0, 0.01, 2.0, 2.0, 2.0)
    for kind in ("single_support", "double_support"):
        assert f[kind]["zmp_p"] == (0.0, 0.0, 2.0, 10.0, 10.0, 0.0) and f[kind]["zmp_d"] == (0.0, 0.0, 0.0005, 0.0001, 0.002, 0.0)
    assert "use_zmp: false" in stb.stab_file_text(f["double_support"]) and "zmp_w" not in stb.stab_file_text(f["double_support"])  # the files are written as before


# ---- the solver inputs of the GPU tests, through the oracle -----------------------------------------------------------------------------------------
def test_the_oracle_solves_every_solver_input_of_the_gpu_tests(built_lib):
    case = fc.solve_case()
    assert (case["oracle"]["status"] == 0).all() and case["b1_force"].shape == (fc.SOLVE_BATCH, 12) and (np.abs(case["b1_force"][:, [2, 8]]) > 100.0).all()
    loop = fc.closed_loop_reference()
    for t, tick in enumerate(loop["ticks"]):
        assert (tick["status"] == 0).all(), (t, tick["status"])
    assert loop["latched_at"] == fc.LOOP_LATCH_AT
