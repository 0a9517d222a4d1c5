"""Talos' torque-collision safety through the C++ facade (inria_wbc_amd/csrc/host): TalosPosTracker with collision_detection.activated, the
reference's talos_pos_tracker.cpp:62-158 for every instance of a batch (wbcqp_detect_torque_collisions_host behind update())."""
import os
import re
import subprocess

import numpy as np
import pytest

from inria_wbc_amd import torque_monitor as tmon
from tests import model_queries as mq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = os.path.join(ROOT, "tests", "golden", "talos_collision_thresholds.yaml")


@pytest.fixture(scope="module")
def host_build(built_lib):
    return mq.host_build()


@pytest.mark.gpu
def test_one_pushed_arm_among_eight_robots(host_build, tmp_path):
    """Eight Talos instances run humanoid::move_com (the squat) for 60 ticks with collision_detection on (filter_size 5, max_invalid 2, the
    reference's thresholds file).  The sensors are the controller's own sliced tau(), except that instance 5's arm_left_4_joint reads 3 N m more from
    tick 20.  collision_detected() is 1 for that instance alone, from the tick the transcription of the reference's detector names on the same two
    streams; clear_collision_detection() frees it and it latches again; the other instances' commands are bit-equal to a controller without the
    detection; a missing or mis-sized joints_torque is refused in the reference's words; activated: false stays a plain tick.  The 60 ticks follow
    one warm-up tick and a clear (the program's header says why: tau() is zero before the first solve)."""
    B, K, bad, t_push, t_clear = 8, 60, 5, 20, 40
    streams = str(tmp_path / "streams.txt")
    r = subprocess.run([host_build["torque_collision_facade_test"], os.path.join(ROOT, "configs/talos/pos_tracker_model.yaml"),
                        os.path.join(ROOT, "configs/talos/squat.yaml"), THRESHOLDS, str(K), str(B), streams], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln and not ln.startswith(("tick", "mis-sized")))
    assert lines["instances"] == str(B) and lines["joints"] == "22" and lines["ids name their joints"] == "1"
    thr = tmon.read_thresholds(THRESHOLDS)
    assert np.array_equal(np.array(lines["thresholds"].split(), dtype=np.float64), thr)
    ids = [int(x) for x in lines["ids"].split()]
    assert len(set(ids)) == 22 and min(ids) >= 6  # (behind the floating base's six)
    arm4 = tmon.TALOS_JOINTS.index("arm_left_4_joint")
    assert lines["pushed"] == "instance %d joint %d by 3 from tick %d, cleared at tick %d" % (bad, arm4, t_push, t_clear)
    assert float(lines["max |tau| monitored"]) > 1.0  # (the legs carry the robot)
    # the refusals, in the reference's words; one row of 22 numbers serves every instance
    assert "torque collision detection requires torque sensor data" in lines["missing"]
    sized = [ln for ln in r.stdout.splitlines() if ln.startswith("mis-sized: ")]
    assert len(sized) == 2 and all("torque sensor data has a wrong size. call torque_sensor_joints() for needed values" in ln for ln in sized)
    assert lines["one row for all"] == "(not refused)"
    assert lines["cleared"] == "1 flags up before, 0 after"
    assert lines["command rows of the other instances that differ"] == "0"

    # the reference's detector on the two streams the program wrote: a fresh one from tick 0 and from the tick of the clear
    rows = {"m": [], "s": []}
    for ln in open(streams):
        rows[ln[0]].append([float(x) for x in ln.split()[1:]])
    model, sensor = (np.array(rows[k]).reshape(K, B, 22) for k in "ms")
    assert np.array_equal(sensor[:t_push], model[:t_push]) and np.abs(model[0]).max() > 1.0  # (the counted ticks follow a warm-up tick)
    diff = sensor - model
    assert np.abs(diff[t_push:, bad, arm4] - 3.0).max() < 1e-12 and np.count_nonzero(np.abs(diff) > 1e-12) == K - t_push
    mon = tmon.Monitor(joint=np.arange(22), threshold=thr, filter=tmon.FILTER_MEAN, window=5, max_invalid=2)
    ref = [tmon.detect(mon, model[:t_clear], sensor[:t_clear]), tmon.detect(mon, model[t_clear:], sensor[t_clear:])]
    want = np.concatenate([ref[0]["detected"], ref[1]["detected"]])
    want_bits = np.concatenate([ref[0]["invalid"], ref[1]["invalid"]])
    ticks = [re.match(r"tick (\d+) detected:((?: \d)+) invalid of %d:((?: \d+)*)$" % bad, ln) for ln in r.stdout.splitlines() if ln.startswith("tick ")]
    assert len(ticks) == K and all(ticks)
    got = np.array([[int(x) for x in m.group(2).split()] for m in ticks])
    assert np.array_equal(got, want)
    for t, m in enumerate(ticks):
        assert sum(1 << int(j) for j in m.group(3).split()) == int(want_bits[t, bad]), t
    # that instance alone, on that joint alone; the mean of five samples crosses 1 N m with the second pushed sample, two more ticks latch
    assert not got[:, [i for i in range(B) if i != bad]].any()
    first, again = int(ref[0]["first_tick"][bad]), t_clear + int(ref[1]["first_tick"][bad])
    assert first == t_push + 1 + 2 and got[first:t_clear, bad].all() and not got[:first, bad].any()
    assert again == t_clear + 2 and not got[t_clear:again, bad].any() and got[again:, bad].all()  # (a fresh window holds pushed samples only)
    assert int(want_bits[-1, bad]) == 1 << arm4
