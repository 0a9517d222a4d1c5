"""The reference's self-collision check through the C++ facade (inria_wbc_amd/csrc/host): CONTROLLER.check_model_collisions / collision_path,
Controller::is_model_colliding, collision_index and the latch that stops a colliding instance's commands (wbcqp_check_collisions_host behind
ModelSource), and its refusal on a source without a model."""
import os
import subprocess

import numpy as np
import pytest

from tests import model_queries as mq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "talos_collisions.yaml")


@pytest.fixture(scope="module")
def host_build(built_lib):
    return mq.host_build()


@pytest.mark.gpu
def test_one_of_eight_robots_collides_and_stops_sending(host_build, tmp_path):
    """Eight Talos instances squat for 6 ticks; instance 5 starts with its shoulders rolled inwards by 0.5 rad, an arm 4 cm inside a leg's spheres.  Its
    q() / dq() / ddq() / tau() stand still from the tick after the hit while q_solver() goes on as it does without the check; the other seven
    are bit-equal to a controller without the check; collision_index names the pair the numpy statement names; a step back refreshes the answer."""
    from inria_wbc_amd import collision, model as mdl
    B, k, out = 8, 5, str(tmp_path / "col.bin")
    r = subprocess.run([host_build["collision_facade_test"], os.path.join(ROOT, "configs/talos/pos_tracker_model.yaml"),
                        os.path.join(ROOT, "configs/talos/squat.yaml"), FIXTURE, "6", str(B), str(k), "0.5", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["instances"] == str(B)
    assert lines["hit seen after tick"] == "1", r.stdout
    for key in ("others never collide", "commands frozen from the tick after the hit", "solver state keeps advancing",
                "solver state equals the run without the check", "other instances bit-equal to the run without the check",
                "without the check q() is q_solver() and nothing collides", "send_cmd is 0 for k alone", "step back to the start frees everybody",
                "step back with another instance driven names it alone"):
        assert lines[key] == "1", (key, r.stdout)
    # trips to the device, counted in the problem source: the latch's check after each of the 6 ticks (is_model_colliding and collision_index
    # after it: kept) and one after each of the two steps back; a controller without the check makes none
    assert lines["device calls"] == "observe 0, check_collisions 8, mass_matrix 0, jacobians 0, hessians 0", r.stdout
    assert lines["device calls without the check"] == "observe 0, check_collisions 0, mass_matrix 0, jacobians 0, hessians 0", r.stdout
    # the final state and flags against the numpy statement; the names against pair_names
    m = mdl.talos_like()
    t = collision.sphere_table(m, FIXTURE)
    a = np.fromfile(out, dtype=np.float64)
    assert a.size == B * m.nq + B
    q, flags = a[:B * m.nq].reshape(B, m.nq), a[B * m.nq:].astype(np.int32)
    want = collision.check(m, t, q)
    assert np.array_equal(flags, want["colliding"]) and flags.tolist() == [int(i == k) for i in range(B)]
    (ma, ia), (mb, ib) = collision.pair_names(t, want["first_pair"][k])
    assert lines["collision_index"] == "%s %d %s %d" % (ma, ia, mb, ib), r.stdout
    assert lines["collision_index of a free instance"] == "[] -1"
    q1 = np.stack([m.q0] * 2)
    q1[1, 7 + m.joint_names.index("arm_left_2_joint") - 1] -= 0.5
    q1[1, 7 + m.joint_names.index("arm_right_2_joint") - 1] += 0.5
    w1 = collision.check(m, t, q1)
    assert w1["colliding"].tolist() == [0, 1]
    (ma, ia), (mb, ib) = collision.pair_names(t, w1["first_pair"][1])
    assert lines["collision_index after that step back"] == "%s %d %s %d" % (ma, ia, mb, ib)


@pytest.mark.gpu
def test_a_source_without_a_model_is_refused(host_build, tmp_path):
    r = mq.run_file_source(host_build["collision_facade_test"], tmp_path, FIXTURE)
    assert r.returncode == 0 and "refused: 1" in r.stdout and "check_model_collisions" in r.stdout, r.stdout + r.stderr
