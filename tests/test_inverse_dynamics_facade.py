"""The model-side torques through the C++ facade (inria_wbc_amd/csrc/host): Controller::rnea_double_support on a model-driven controller
(wbcqp_inverse_dynamics_host behind ModelSource), and its refusals."""
import os
import subprocess

import pytest

from tests import model_queries as mq
from tests.test_inverse_dynamics_host import AUDIT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_build(built_lib):
    return mq.host_build()


@pytest.mark.gpu
def test_rnea_double_support_after_move_com(host_build):
    """20 ticks of humanoid::move_com (the squat) on 8 Talos instances, a step back to the state the last tick started from, and the QP's own
    contact wrenches as the foot sensors: rnea_double_support is zero on the base rows and tau() on the actuated rows at the audit bar
    (tests/test_inverse_dynamics_host.py); add_foot_mass equals the same correction made in the program from RobotWrapper::framePosition and
    applied at the sole frames, to 1e-10; a missing sensor key is refused in the reference's words."""
    B = 8
    r = subprocess.run([host_build["inverse_dynamics_facade_test"], os.path.join(ROOT, "configs/talos/pos_tracker_model.yaml"),
                        os.path.join(ROOT, "configs/talos/squat.yaml"), "20", str(B)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["instances"] == str(B)
    assert float(lines["max |contact wrench|"]) > 100.0 and float(lines["max |tau|"]) > 1.0  # (the feet carry the robot)
    assert float(lines["max |rnea_double_support| on the base rows"]) <= AUDIT_TOL
    assert float(lines["max |rnea_double_support - tau()| on the actuated rows"]) <= AUDIT_TOL
    assert float(lines["max |base rows| without the wrenches"]) > 100.0
    assert float(lines["max |add_foot_mass - the correction by hand at the sole frames|"]) <= 1e-10
    assert float(lines["max |add_foot_mass - without|"]) > 1e-3
    assert lines["missing key refused"] == "1 unknown frame refused: 1", r.stdout


@pytest.mark.gpu
def test_file_source_refuses(host_build, tmp_path):
    r = mq.run_file_source(host_build["inverse_dynamics_facade_test"], tmp_path)
    assert r.returncode == 0 and "refused: 2 of 2" in r.stdout, r.stdout + r.stderr
