"""CPU tests of the torque monitor (wbcqp_detect_torque_collisions): the numpy transcription of the reference's filters and detector
(inria_wbc_amd/torque_monitor.py) on hand-worked cases, the shift-register form of the consecutive rule against the ring of signs, the thresholds
reader on the reference's settings file, and the library's surface (symbols declared, exported, bound, refusing a NULL handle; state_bytes).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from inria_wbc_amd import torque_monitor as tmon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1  # WBCQP_ERR_INVALID (include/wbcqp.h)
FIXTURE = os.path.join(ROOT, "tests", "golden", "talos_collision_thresholds.yaml")


def col(*x):
    return np.array(x, dtype=np.float64)


# ---- the filters ---------------------------------------------------------------------------------------------------------------------------
def test_the_window_grows_and_then_slides():
    f = tmon.MovingAverageFilter(1, 3)
    assert not f.data_ready()
    got = [float(f.filter(col(x))[0]) for x in (1.0, 2.0, 6.0, 10.0, 2.0)]
    # 1 | 1 2 | 1 2 6 | 2 6 10 | 6 10 2
    assert got == [1.0, 1.5, 3.0, 6.0, 6.0] and f.data_ready()
    # a sum oldest first and one division, not a mean of rounded parts
    g = tmon.MovingAverageFilter(1, 3)
    for x in (1e16, 1.0, -1e16):
        last = float(g.filter(col(x))[0])
    assert last == ((1e16 + 1.0) + -1e16) / 3.0 == 0.0
    # a window of one is the sample itself; two variables are filtered side by side
    one = tmon.MovingAverageFilter(2, 1)
    assert [one.filter(col(a, -a)).tolist() for a in (3.0, 5.0)] == [[3.0, -3.0], [5.0, -5.0]]


def test_the_median_with_even_and_odd_counts():
    f = tmon.MedianFilter(1, 4)
    got = [float(f.filter(col(x))[0]) for x in (5.0, 1.0, 9.0, 3.0, 7.0, 7.0)]
    # 5 | 1 5 -> 3 | 1 5 9 -> 5 | 1 3 5 9 -> 4 | (1 9 3 7) 1 3 7 9 -> 5 | (9 3 7 7) 3 7 7 9 -> 7
    assert got == [5.0, 3.0, 5.0, 4.0, 5.0, 7.0]
    g = tmon.MedianFilter(1, 3)
    assert [float(g.filter(col(x))[0]) for x in (2.0, 8.0, 4.0, 6.0)] == [2.0, 5.0, 4.0, 6.0]


# ---- the detector --------------------------------------------------------------------------------------------------------------------------
def run(det, discrepancies):
    """check() per step with sensors = 0 and target = the wanted discrepancy; the joint's validity after each step."""
    return [bool(det.check(col(d), col(0.0))) for d in discrepancies]


@pytest.mark.parametrize("max_invalid", [1, 2, 5])
def test_a_joint_latches_on_exactly_the_kth_same_signed_invalid_step(max_invalid):
    K = max_invalid + 1
    for sign in (1.0, -1.0):
        det = tmon.TorqueCollisionDetection([1.0])
        det.set_max_consecutive_invalid(max_invalid)
        ok = run(det, [0.5] + [2.0 * sign] * (K + 2))
        assert ok == [True] * K + [False] * 3, (sign, ok)  # the (K-1)-th invalid step is still valid, the K-th is not
        assert det.get_invalid_ids() == [0]


def test_alternating_signs_never_latch_and_one_valid_step_restarts_the_count():
    det = tmon.TorqueCollisionDetection([1.0])
    det.set_max_consecutive_invalid(2)
    assert run(det, [2.0, -2.0] * 10) == [True] * 20
    det = tmon.TorqueCollisionDetection([1.0])
    det.set_max_consecutive_invalid(2)
    #                  1    2    ok   1    2    3     4    ok   1
    ok = run(det, [2.0, 2.0, 0.1, 2.0, 2.0, 2.0, 2.0, 0.9, 2.0])
    assert ok == [True, True, True, True, True, False, False, True, True]
    # the bound is strict: |d| == threshold is invalid
    det = tmon.TorqueCollisionDetection([1.0])
    assert run(det, [1.0, np.nextafter(1.0, 0.0)]) == [False, True]


def test_k_equal_one_is_the_raw_validity():
    rng = np.random.default_rng(5)
    d = rng.standard_normal((200, 3)) * 2.0
    det = tmon.TorqueCollisionDetection([1.0, 2.0, 0.5])
    det.set_max_consecutive_invalid(0)
    for t in range(d.shape[0]):
        det.check(d[t], np.zeros(3))
        assert np.array_equal(det.get_validity().astype(bool), np.abs(d[t]) < col(1.0, 2.0, 0.5))


def test_an_offset_shifts_the_discrepancy_and_a_filter_is_applied_first():
    det = tmon.TorqueCollisionDetection([1.0, 1.0])
    det.set_filter(tmon.MovingAverageFilter(2, 2))
    det.set_offset(col(0.25, -4.0))
    assert not det.check(col(3.0, 3.0), col(2.0, 6.0))  # filtered 2, 6 (+ offset: 2.25, 2) -> d 0.75, 1.0: the second is invalid (K = 1, strict bound)
    assert det.get_filtered_sensors().tolist() == [2.25, 2.0] and det.get_discrepancy().tolist() == [0.75, 1.0]
    assert det.get_invalid_ids() == [1]
    det.remove_offset()
    det.check(col(3.0, 3.0), col(4.0, 2.0))  # window (2, 4), (6, 2) -> 3, 4
    assert det.get_filtered_sensors().tolist() == [3.0, 4.0] and det.get_discrepancy().tolist() == [0.0, -1.0]


def test_reset_equals_a_new_object():
    rng = np.random.default_rng(6)
    mon = tmon.Monitor(joint=[0, 1, 2], threshold=[1.0, 0.5, 2.0], filter=tmon.FILTER_MEDIAN, window=4, max_invalid=2)
    model, sensor = rng.standard_normal((40, 1, 3)) * 2, rng.standard_normal((40, 1, 3))
    used = mon.detector()
    for t in range(17):  # (17 is no multiple of K = 3: the ring of signs restarts at column 1 either way)
        used.check(model[t, 0], sensor[t, 0])
    used.reset()
    a, b = tmon.detect(mon, model, sensor, state=used), tmon.detect(mon, model, sensor)
    for k in ("detected", "invalid", "discrepancy", "filtered", "first_tick", "n_detected"):
        assert np.array_equal(a[k], b[k]), k
    assert 0 < b["n_detected"][0] < 40


def test_detect_carries_its_state_and_reports_the_first_tick():
    mon = tmon.Monitor(joint=[2, 0], threshold=[1.0, 1.0], filter=tmon.FILTER_NONE, max_invalid=1)
    model = np.zeros((6, 2, 3))
    model[2:, 1, 2] = 5.0  # instance 1, monitored joint 0 (column 2) from tick 2: invalid from tick 3
    whole = tmon.detect(mon, model, np.zeros((6, 2, 2)))
    assert whole["first_tick"].tolist() == [-1, 3] and whole["n_detected"].tolist() == [0, 3]
    assert whole["invalid"][:, 1].tolist() == [0, 0, 0, 1, 1, 1] and whole["detected"][:, 0].tolist() == [0] * 6
    first = tmon.detect(mon, model[:3], np.zeros((3, 2, 2)))
    second = tmon.detect(mon, model[3:], np.zeros((3, 2, 2)), state=first["state"])
    assert np.array_equal(np.concatenate([first["invalid"], second["invalid"]]), whole["invalid"])
    assert second["first_tick"].tolist() == [-1, 0]  # (of THIS call)


@pytest.mark.parametrize("max_invalid", [0, 1, 5, 31])
def test_the_shift_registers_equal_the_ring_of_signs(max_invalid):
    rng = np.random.default_rng(100 + max_invalid)
    T, n = 600, 8
    # runs of one sign of random length, interrupted by valid steps, sign changes, zeros and NaNs
    d = np.zeros((T, n))
    for j in range(n):
        t = 0
        while t < T:
            length = int(rng.integers(1, 2 * max_invalid + 4))
            d[t:t + length, j] = rng.choice([-3.0, 3.0, 0.2, -0.2]) * rng.uniform(0.5, 1.5)
            t += length
    d[rng.random((T, n)) < 0.01] = 0.0
    d[rng.random((T, n)) < 0.005] = np.nan
    thr = np.full(n, 1.0)
    thr[0] = -1.0  # everything is raw-invalid, a zero has no sign
    det = tmon.TorqueCollisionDetection(thr)
    det.set_max_consecutive_invalid(max_invalid)
    ring = np.zeros((T, n), dtype=bool)
    for t in range(T):
        det.check(d[t], np.zeros(n))
        ring[t] = ~det.get_validity().astype(bool)
    regs = tmon.shift_register_invalid(d, thr, max_invalid)
    assert np.array_equal(ring, regs)
    assert ring.any() and not ring.all() and ring.sum() > 20 and (~ring).sum() > 20  # both outcomes


# ---- the settings ---------------------------------------------------------------------------------------------------------------------------
def test_the_thresholds_reader_on_the_references_file():
    thr = tmon.read_thresholds(FIXTURE)
    assert thr.shape == (22,) and len(tmon.TALOS_JOINTS) == 22 and len(tmon.TALOS_THRESHOLDS) == 22
    assert (thr[:12] == 1e10).all() and (thr[12:] == 1.0).all()
    # a file that names two joints and one unknown key leaves the other defaults
    assert np.array_equal(tmon.read_thresholds(os.devnull), np.asarray(tmon.TALOS_THRESHOLDS))
    assert tmon.TALOS_THRESHOLDS[3] == 4.4e5 and tmon.TALOS_THRESHOLDS[12] == 10.0 and tmon.TALOS_JOINTS[17] == "arm_left_4_joint"


# ---- the library's surface ------------------------------------------------------------------------------------------------------------------
NEW = {"wbcqp_torque_monitor_state_bytes", "wbcqp_detect_torque_collisions", "wbcqp_detect_torque_collisions_host"}


def test_symbols_declared_exported_bound_and_null_handle(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(capi.EXPORTS)
    for name, value in (("MAX_MONITORED", 64), ("MAX_FILTER_WINDOW", 64), ("MAX_INVALID", 31), ("VERSION", 151)):
        assert re.search(r"#define\s+WBCQP_%s\s+%d\b" % (name, value), hdr), name
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in NEW:
        assert hasattr(raw, sym), sym
        assert getattr(lib, sym).argtypes, sym
    for name in ("detect_torque_collisions", "detect_torque_collisions_host"):
        assert callable(getattr(capi.Handle, name))
    # a NULL handle is refused before anything else is looked at
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mb = capi.TorqueMonitorBuffers(tmon.Monitor(joint=[0], threshold=[1.0]))
    out = capi.CTorqueChecks()
    assert lib.wbcqp_detect_torque_collisions(None, ctypes.byref(mb.c), 1, 1, p, 1, p, None, ctypes.byref(out), None) == ERR_INVALID
    assert lib.wbcqp_detect_torque_collisions_host(None, ctypes.byref(mb.c), 1, 1, p, 1, p, None, ctypes.byref(out)) == ERR_INVALID


def test_state_bytes_of_valid_and_invalid_monitors(built_lib):
    from inria_wbc_amd import capi
    lib = capi.load_library()
    ok = dict(joint=[3, 1, 3], threshold=[1.0, -2.0, np.inf], offset=None, filter=tmon.FILTER_MEAN, window=30, max_invalid=5)
    mon = lambda **kw: tmon.Monitor(**dict(ok, **kw))  # noqa: E731
    for m in (mon(), mon(filter=tmon.FILTER_MEDIAN, window=64), mon(filter=tmon.FILTER_NONE, window=0), mon(window=1, max_invalid=31, offset=[0.0, 1.0, -1.0]),
              mon(joint=list(range(64)), threshold=[1.0] * 64, max_invalid=0)):
        assert capi.torque_monitor_state_bytes(m) == m.state_bytes() > 0
    assert capi.torque_monitor_state_bytes(mon()) == 8 + 8 * 3 + 8 * 30 * 3
    assert capi.torque_monitor_state_bytes(mon(filter=tmon.FILTER_NONE)) == 8 + 8 * 3
    bad = [mon(joint=[], threshold=[]), mon(joint=list(range(65)), threshold=[1.0] * 65), mon(filter=3), mon(filter=-1), mon(window=0), mon(window=65),
           mon(max_invalid=-1), mon(max_invalid=32), mon(joint=[0, -1, 2]), mon(threshold=[1.0, np.nan, 1.0]), mon(offset=[0.0, np.inf, 0.0]),
           mon(offset=[np.nan, 0.0, 0.0])]
    for m in bad:
        assert capi.torque_monitor_state_bytes(m) == 0, m
    assert lib.wbcqp_torque_monitor_state_bytes(None) == 0
    c = capi.TorqueMonitorBuffers(mon()).c
    c.joint = None
    assert lib.wbcqp_torque_monitor_state_bytes(ctypes.byref(c)) == 0
    c = capi.TorqueMonitorBuffers(mon()).c
    c.threshold = None
    assert lib.wbcqp_torque_monitor_state_bytes(ctypes.byref(c)) == 0
