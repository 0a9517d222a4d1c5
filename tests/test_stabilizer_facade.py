"""The stabiliser through the C++ facade (inria_wbc_amd/csrc/host): HumanoidPosTracker with stabilizer.activated, the reference's
humanoid_pos_tracker.cpp:41-302 for every instance of a batch (wbcqp_observe_acom_host and wbcqp_stabilize_host behind update())."""
import os
import subprocess

import numpy as np
import pytest

from inria_wbc_amd import model as mdl
from inria_wbc_amd import observe, structure
from inria_wbc_amd import stabilizer as stb
from tests import model_queries as mq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "talos")


@pytest.fixture(scope="module")
def host_build(built_lib):
    return mq.host_build()


def test_emitted_stabilizer_files_hold_the_packages_constants(built_lib):
    """tools/emit_configs.py (run by the build) writes the three stabiliser files and a CONTROLLER tree that switches the stabiliser on, for Talos
    and iCub, with use_zmp off."""
    for robot in ("talos", "icub"):
        d = os.path.join(ROOT, "configs", robot)
        for kind, cfg in stb.STAB_FILES[robot].items():
            text = open(os.path.join(d, "stab_%s.yaml" % kind)).read()
            assert "use_zmp: false" in text and "filter_size: %d\n" % cfg["window"] in text
            for key, name in (("com", "com_gains"), ("ankle", "ankle_gains"), ("ffda", "ffda_gains")):
                line = next(ln for ln in text.splitlines() if ln.startswith(key + ":"))
                assert [float(x) for x in line.split("[")[1].rstrip("]").split(",")] == list(cfg[name]), (robot, kind, key)
        tree = open(os.path.join(d, "pos_tracker_stab.yaml")).read()
        assert "name: humanoid-pos-tracker" in tree and "activated: true" in tree
        for key, kind in (("params_ss", "single_support"), ("params_ds", "double_support"), ("params_fixed_base", "fixed_base")):
            assert "%s: stab_%s.yaml" % (key, kind) in tree
    assert stb.STAB_FILES["talos"]["double_support"]["ankle_gains"][0] == 0.25 and stb.STAB_FILES["icub"]["double_support"]["ankle_gains"] == (0.0,) * 6


@pytest.mark.gpu
def test_four_robots_squat_on_stabilised_references(host_build, tmp_path):
    """Four Talos instances run humanoid::move_com (the squat) for 40 ticks in DOUBLE_SUPPORT with the reference's gains (window 7) and sensors that
    differ per instance and tick.  The transcription of the reference, run on what the program dumped -- the sensors, the previous solution's foot
    forces, the stored references, and com / acom / ankle positions from observe.py at the state the PREVIOUS tick started from -- gives the program's
    flags and cop() and the references the tick read (to 1e-9: observe.py against the device is 1e-10, the laws divide by dt^2 after gains of 3e-8).
    With the state the tick itself starts from it does not: the lag is there.  The stored references equal an unstabilised controller's in every bit;
    the required sensors are asked for in the reference's words; three numbers serve all instances; an absurd ground force on one instance raises the
    reference's message with the instance, before the solve."""
    B, K = 4, 40
    dump = str(tmp_path / "dump.txt")
    r = subprocess.run([host_build["stabilizer_facade_test"], os.path.join(CFG, "pos_tracker_stab.yaml"), os.path.join(CFG, "squat.yaml"), str(K), str(B), dump],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    m, st = mdl.talos_like(), structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    assert lines["instances"] == str(B) and lines["nref"] == str(tm.nref)
    for key, words in (("lf_force", "the stabilizer needs the LF force"), ("rf_force", "the stabilizer needs the RF force"),
                       ("lf_torque", "the stabilizer needs the LF torque"), ("rf_torque", "the stabilizer needs the RF torque"),
                       ("imu_vel", "the stabilizer imu needs angular velocity")):
        assert words in lines["missing " + key], key
    assert "lf_force" in lines["mis-sized"] and lines["mis-sized"] != "(not refused)"
    assert lines["ticks where the stored references differ from the unstabilised controller's"] == "0"
    assert int(lines["instances whose commands differ from the unstabilised controller's"]) == B  # the stabiliser does something
    assert lines["three numbers for all"] == "(not refused)" and lines["instances with instance 0's flags"] == str(B)
    assert "ground force is more than 10*M*g" in lines["absurd force"] and "[instance 2]" in lines["absurd force"]
    assert lines["error bits"] == "0 0 1 0" and lines["ticks solved meanwhile"].startswith("0 ")

    rows = {k: [] for k in "qvwxsrf"}
    for ln in open(dump):
        rows[ln[0]].append([float(x) for x in ln.split()[1:]])
    arr = {k: np.array(v).reshape(K, B, -1) for k, v in rows.items() if k != "x"}
    assert arr["q"].shape[2] == m.nq and arr["r"].shape[2] == tm.nref
    g = stb.STAB_FILES["talos"]["double_support"]
    s = stb.from_taskmap(m, tm, mdl.talos_stack(), g["window"], g["com_gains"], g["ankle_gains"], g["ffda_gains"])
    s.lf_force_col, s.rf_force_col = 0, 12  # the facade hands the two feet's forces over side by side
    ankles = observe.frame_ids(m, ["leg_left_6_joint", "leg_right_6_joint"])

    def transcribe(lag):
        state = np.zeros((B, stb.state_bytes(s.window)), np.uint8)
        out = []
        for t in range(K):
            # lag: the state dumped for tick t is the one tick t - 1 started from; without it: the one tick t starts from (dumped for tick t + 1)
            src = t if lag else min(t + 1, K - 1)
            o = observe.observe(m, arr["q"][src], arr["v"][src], ankles, acom=True)
            x = np.array(rows["x"][t * B:(t + 1) * B])
            out.append(stb.step(s, state, dict(ref=arr["s"][t], wrench=arr["w"][t], com=o["com"], acom=o["acom"], placement=o["placement"].reshape(B, -1),
                                               x_prev=x if x.size else None)))
        return out

    want = transcribe(True)
    assert not rows["x"][0] and len(rows["x"][B]) == 24  # no previous solution on the first tick
    flags = arr["f"][:, :, 0].astype(np.int64)
    for t in range(K):
        assert np.array_equal(flags[t], want[t]["flags"]), t
        valid = want[t]["cop"][:, 0]  # (both feet carry weight throughout: the combined CoP is the valid one once the window is full)
        assert np.allclose(arr["f"][t, :, 1:], valid, rtol=0, atol=1e-9, equal_nan=True), t
        assert np.abs(arr["r"][t] - want[t]["ref_out"]).max() <= 1e-9 * max(1.0, np.abs(want[t]["ref_out"]).max()), t
    full = stb.COP | stb.LCOP | stb.RCOP | stb.COM | stb.LANKLE | stb.RANKLE | stb.FFDA
    assert (flags[:s.window - 1] == 0).all() and (flags[s.window - 1:] == full).all()
    assert np.isnan(arr["f"][0, :, 1:]).all() and np.array_equal(arr["r"][0], arr["s"][0])  # nothing is valid yet: the references pass unchanged
    moved = np.abs(arr["r"][-1] - arr["s"][-1])
    # every law moved something on every instance (by how much is the transcription's business, above: a CoM gain of 1e-3 on a CoP a few cm off)
    assert (moved[:, s.com_ref] > 0).all() and (moved[:, s.lf_ref + 3:s.lf_ref + 12].max(axis=1) > 0).all()
    assert (moved[:, s.torso_ref + 3:s.torso_ref + 12].max(axis=1) > 0).all()
    # the contact takes the foot task's velocity and acceleration
    assert np.array_equal(arr["r"][-1][:, s.lf_contact_ref + 12:s.lf_contact_ref + 24], arr["r"][-1][:, s.lf_ref + 12:s.lf_ref + 24])
    # the lag is there: observing the state a tick starts from gives other references than the program's
    wrong = transcribe(False)
    span = range(K - 10, K - 1)
    with_lag = max(np.abs(arr["r"][t] - want[t]["ref_out"]).max() for t in span)
    without_lag = max(np.abs(arr["r"][t] - wrong[t]["ref_out"]).max() for t in span)
    print("references against the transcription: %.1e with the lag, %.1e without" % (with_lag, without_lag))
    assert without_lag > 100 * max(with_lag, 1e-13)


@pytest.mark.gpu
def test_use_zmp_in_the_active_file_and_missing_params_are_refused(host_build, tmp_path):
    """use_zmp: true is refused where the file becomes ACTIVE (here: on set_behavior_type(DOUBLE_SUPPORT)), with a message that says to set use_zmp:
    false; in a file that is not active it is accepted.  activated: true without the params_* keys stays refused."""
    for f in os.listdir(CFG):
        if os.path.isfile(os.path.join(CFG, f)) and not f.startswith("stab_"):
            os.symlink(os.path.join(CFG, f), str(tmp_path / f))
    files = stb.STAB_FILES["talos"]

    def run(zmp_in, tree=None):
        for kind, cfg in files.items():
            (tmp_path / ("stab_%s.yaml" % kind)).write_text(stb.stab_file_text(cfg, use_zmp=(kind == zmp_in)))
        path = str(tmp_path / "pos_tracker_stab.yaml")
        if tree is not None:
            path = str(tmp_path / "other.yaml")
            open(path, "w").write(tree)
        return subprocess.run([host_build["stabilizer_facade_test"], path, os.path.join(CFG, "squat.yaml"), "0", "2", str(tmp_path / "d.txt")],
                              capture_output=True, text=True, timeout=120)

    r = run("double_support")
    assert r.returncode == 1 and "use_zmp" in r.stderr and "set use_zmp: false" in r.stderr and "DOUBLE_SUPPORT" in r.stderr, r.stdout + r.stderr
    r = run("single_support")  # not the active file
    assert r.returncode == 0 and "constructed" in r.stdout, r.stdout + r.stderr
    r = run("fixed_base")  # active from the constructor on
    assert r.returncode == 1 and "set use_zmp: false" in r.stderr and "FIXED_BASE" in r.stderr
    tree = open(os.path.join(CFG, "pos_tracker_stab.yaml")).read().split("    params_ss")[0]
    r = run(None, tree)
    assert r.returncode == 1 and "stabilizer" in r.stderr and "not part of this build" in r.stderr and "params_fixed_base" in r.stderr
