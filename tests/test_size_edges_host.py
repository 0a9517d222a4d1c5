"""The size-edge cases (tests/size_edges.py) on the CPU: what the host's layout arithmetic answers for every stack of the tables (wbcqp_layout_of needs
no device), and that the reference does on each batch what the batch is there for -- drops at every position at n = 16, a full step onto a vertex at
n <= 2, row 255 of a 256-row stack picked and active, rows past the 256th of the dense seam picked, neq = n.  The kernels themselves:
tests/test_gpu_size_edges.py."""
import numpy as np
import pytest

from inria_wbc_amd import capi
from tests import size_edges as se

KEYS = ("lds_bytes", "waves_per_cu", "wave_per_qp")


def _drops(tot):
    return tot["partial_drop"] + tot["dual_drop"]


def test_the_one_wave_kernels_staging_division_is_exact():
    assert se.small_div_is_exact()


@pytest.mark.parametrize("case", se.SMALL_CASES, ids=[c.id for c in se.SMALL_CASES])
def test_small_stacks_run_one_wave_per_qp_and_the_reference_takes_their_branches(built_lib, oracle_mod, case):
    st = case.stack()
    L = capi.layout_of(st)
    assert st.n == st.nv == case.nv and st.n_dense == sum(case.dense) and st.n_sel == (case.nv if case.posture else 0)
    assert st.nin2 == (2 * case.nv if case.bounds else 0) and st.neq == 0
    assert {k: L[k] for k in KEYS} == dict(lds_bytes=case.lds_bytes, waves_per_cu=case.waves_per_cu, wave_per_qp=1), (case.id, L)
    st, inputs, ref = se.reference(case, oracle_mod)
    assert len(ref["status"]) == se.SMALL_BATCH and (ref["status"] == 0).mean() >= 0.9, case.id
    assert se.skipped_seeds(case, oracle_mod) == case.skipped, (case.id, se.skipped_seeds(case, oracle_mod))
    logs, cs, tot = se.censuses(case, oracle_mod)
    print(case.id, "max iterations", int(ref["iters"].max()), {k: tot.get(k) for k in ("full_add", "vertex", "partial_drop", "dual_drop", "drop_first", "drop_interior", "drop_last")})
    if "vertex" in case.needs:
        assert tot["vertex"] >= 1, (case.id, tot)
    if "drop" in case.needs:
        assert _drops(tot) >= 1, (case.id, tot)
    if "drop_positions" in case.needs:
        assert min(tot["drop_first"], tot["drop_interior"], tot["drop_last"]) >= 1, (case.id, tot)
    if "adds_only" in case.needs:
        assert _drops(tot) == 0 and tot["full_add"] >= se.SMALL_BATCH, (case.id, tot)
    if not case.bounds:
        assert st.nin2 == 0 and (ref["iters"] == 1).all()


def test_the_small_table_holds_the_sizes_it_is_there_for():
    sts = {c.id: c.stack() for c in se.SMALL_CASES}
    assert sorted({st.n for st in sts.values()}) == [1, 2, 3, 4, 6, 7, 8, 9, 16]
    full = sts["n16_full"]
    assert (full.r1, full.nin2, full.n_dense * full.nv, full.n_tasks) == (32, 32, 256, 5)  # every array of namespace sm filled exactly
    assert sts["n1_posture_only"].n_dense == 0 and sts["n2_two_rows"].n_sel == 0 and sts["n16_sixteen_tasks"].n_tasks == 16
    assert sts["n16_no_bounds"].nin2 == 0 and sts["n16_rows_only"].n_sel == 0


@pytest.mark.parametrize("case", se.COMPACT_CASES, ids=[c.id for c in se.COMPACT_CASES])
def test_the_compact_envelopes_limits_get_the_recorded_layout_and_the_reference_drops(built_lib, oracle_mod, case):
    st = case.stack()
    if case.layout == "refused":
        with pytest.raises(capi.WbcqpError) as e:
            capi.layout_of(st)
        assert e.value.code == se.UNSUPPORTED and case.error in str(e.value), (case.id, str(e.value))
        return
    L = capi.layout_of(st)
    assert {k: L[k] for k in KEYS} == dict(lds_bytes=case.lds_bytes, waves_per_cu=case.waves_per_cu, wave_per_qp=0), (case.id, L)
    assert (L["dense_h"], L["specialised"]) == (0, 0)
    assert se.in_compact_envelope(st) == (case.layout == "compact"), case.id
    assert 6 * st.nc < st.nv  # (more contact rows than velocities: redundant equalities in synth)
    st, inputs, ref = se.reference(case, oracle_mod)
    assert len(ref["status"]) == se.COMPACT_BATCH and (ref["status"] == 0).mean() >= 0.9, case.id
    assert se.skipped_seeds(case, oracle_mod) == case.skipped, (case.id, se.skipped_seeds(case, oracle_mod))
    logs, cs, tot = se.censuses(case, oracle_mod)
    print(case.id, "n", st.n, "neq", st.neq, "nu", st.nu, "nin2", st.nin2, "max iterations", int(ref["iters"].max()), "drops", _drops(tot))
    if case.act:
        assert _drops(tot) >= 10 and ref["iters"].max() >= 20, (case.id, _drops(tot), int(ref["iters"].max()))
    else:
        assert _drops(tot) >= 1, case.id


def test_the_compact_table_reaches_each_limit():
    by = {c.id: c for c in se.COMPACT_CASES}
    sts = {c.id: c.stack() for c in se.COMPACT_CASES}
    assert sts["nin2_256"].nin2 == 256 and sts["nin2_260"].nin2 == 260 and sts[se.ROW_255_CASE].nin2 == 256
    assert sts["nu8"].nu == 8 and sts["nu8_nv48"].nu == 8 and sts["nu9"].nu == 9 and sts["nu9"].neq == 21
    free = sts["nu0_free64"]
    assert free.nu == 0 and free.n - free.neq == 64 and (sts["free65"].nv, sts["free65"].n) == (53, 65)
    for k in ("flight", "flight_act"):
        assert (sts[k].nu, sts[k].neq, sts[k].k, sts[k].nc) == (6, 6, 0, 0)
    assert (sts["one_contact_nu0"].nu, sts["one_contact_nu0"].neq) == (0, 6) and (sts["fixed52"].nv, sts["fixed52"].nin2, sts["fixed52"].neq) == (52, 208, 0)
    assert (sts["fixed40"].nv, sts["fixed40"].neq, sts["fixed40"].nv + 23) == (40, 0, 63)
    assert [c.layout for c in by.values()].count("compact") == 7 and [c.layout for c in by.values()].count("refused") == 3


def test_row_255_is_picked_and_active_in_the_reference(oracle_mod):
    case = next(c for c in se.COMPACT_CASES if c.id == se.ROW_255_CASE)
    st, inputs, ref = se.reference(case, oracle_mod)
    logs, cs, tot = se.censuses(case, oracle_mod)
    rows = se.rows_seen(logs, oracle_mod)
    assert rows.max() == 255 and (rows >= 250).sum() >= 2, rows[-8:]
    word7 = ref["active_mask"][:, 7]
    assert ((word7 >> 31) & 1).sum() >= 1 and (word7 != 0).sum() >= 2  # bit 31 of mask word 7 at a solution


def test_reclassified_qps_part_from_the_oracle_at_a_near_tie(oracle_mod):
    """A class-A QP filed as not class A (size_edges.RECLASSIFIED) shows the near tie it is filed for: the numpy model of the compact loop leaves the
    oracle's path at a pick whose two candidates' s differ by less than solver_branches.NEAR_TIE relative, and the oracle takes the other one."""
    from tests import solver_branches as sb
    cases = {c.id: c for c in se.SMALL_CASES + se.COMPACT_CASES}
    for (cid, seed), why in se.RECLASSIFIED.items():
        case = cases[cid]
        st, inputs, ref = se.reference(case, oracle_mod)
        i = se.seeds_of(case, oracle_mod).index(seed)
        one = {k: v[i:i + 1] for k, v in inputs.items()}
        assert sb.classify(st, one, seed, oracle_mod)[0] == "A" and not se.class_a(case, oracle_mod)[i], (cid, seed)
        tie = sb.parting_pick(st, one, oracle_mod)
        print(cid, seed, tie)
        assert tie["parted"] and tie["rel"] < sb.NEAR_TIE and tie["oracle_row"] == tie["other"], (cid, seed, tie, why)
    assert len(se.RECLASSIFIED) <= 2


@pytest.mark.parametrize("size", se.DENSE_SIZES, ids=["n%d_neq%d_nin%d" % s for s in se.DENSE_SIZES])
def test_dense_sizes_meet_their_conditions_in_the_reference(oracle_mod, size):
    n, neq, nin = size
    seeds, replaced = se.dense_seeds(size, oracle_mod)
    assert seeds == se.dense_table_seeds(size) and replaced == se.DENSE_REPLACED.get(size), (size, seeds, replaced)
    outs = [oracle_mod.eiquadprog_log(*se.dense_qp(n, neq, nin, s)) for s in seeds]
    assert all(o["status"] == 0 for o in outs), size
    ev = np.concatenate([o["events"] for o in outs])
    print(size, "iterations", [o["iters"] for o in outs], "iq", [o["iq"] for o in outs])
    if nin >= 257:
        picked = ev[ev[:, 0] == oracle_mod.EV_PICK, 1]
        assert np.isin(ev[:, 0], (oracle_mod.EV_PARTIAL_DROP, oracle_mod.EV_DUAL_DROP)).sum() >= 1 and (picked >= 256).sum() >= 1, size
    if neq == n:
        assert all(o["iq"] == n for o in outs)


def test_the_dense_seams_lds_arithmetic_ends_at_n_99():
    N = se.DENSE_N_MAX
    for neq in (0, 22, 40, N):
        assert se.dense_lds_bytes(N, min(neq, N)) <= 160 * 1024 < se.dense_lds_bytes(N + 1, neq), neq
    assert all(se.dense_lds_bytes(n, neq) <= 160 * 1024 for n, neq, _ in se.DENSE_SIZES)


@pytest.mark.parametrize("name,st,code,text", se.refused_stacks(), ids=[r[0] for r in se.refused_stacks()])
def test_refused_stacks_get_the_documented_code_from_the_host_arithmetic(built_lib, name, st, code, text):
    with pytest.raises(capi.WbcqpError) as e:
        capi.layout_of(st)
    assert e.value.code == code and text in str(e.value), (name, e.value.code, str(e.value))
