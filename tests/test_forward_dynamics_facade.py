"""M(q), forward dynamics and the stable-PD commands through the C++ facade (inria_wbc_amd/csrc/host): Controller::inertia_matrix,
Controller::forward_dynamics and robots::compute_spd on a model-driven controller (wbcqp_mass_matrix_host, wbcqp_forward_dynamics_host,
wbcqp_spd_commands_host behind ModelSource), and their refusal on a FileSource."""
import os
import subprocess

import numpy as np
import pytest

from tests import model_queries as mq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_build(built_lib):
    return mq.host_build()


@pytest.mark.gpu
def test_inertia_matrix_and_compute_spd_after_move_com(host_build, tmp_path):
    """20 ticks of humanoid::move_com (the squat) on 4 Talos instances: inertia_matrix() and compute_spd equal Handle.mass_matrix_host and
    Handle.spd_commands_host on the state the program wrote, bit for bit (the same library call on the same model), with the reference's float
    gains; forward_dynamics(tau()) likewise."""
    from inria_wbc_amd import capi, forward_dynamics as fd
    B, out = 4, str(tmp_path / "fdyn.bin")
    r = subprocess.run([host_build["forward_dynamics_facade_test"], os.path.join(ROOT, "configs/talos/pos_tracker_model.yaml"),
                        os.path.join(ROOT, "configs/talos/squat.yaml"), "20", str(B), out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["instances"] == str(B)
    assert lines["kept"] == "1 refreshed after qp_step_back: 1", r.stdout
    # trips to the device, counted in the problem source: inertia_matrix() asked three times at one state (1) and once after the step back (1)
    assert lines["device calls"] == "observe 0, check_collisions 0, mass_matrix 2, jacobians 0, hessians 0", r.stdout
    assert float(lines["max |M - M'|"]) == 0.0 and float(lines["min M(j, j)"]) > 0.0
    assert float(lines["max |commands| on the base rows"]) == 0.0 and float(lines["max |commands| on the actuated rows"]) > 1.0
    assert lines["commands for nv-wide targets equal"] == "1"
    assert float(lines["max |compute_velocities(target, target)|"]) == 0.0
    assert lines["forward dynamics failed instances"] == "0"
    m, st, tm = mq.talos_case()
    a = np.fromfile(out, dtype=np.float64)
    sizes = [B * m.nq, B * m.nv, B * m.nv * m.nv, B * m.na, B * m.nv, B * m.nv, B * m.nv]
    assert a.size == sum(sizes)
    q, dq, M, target, cmd, tau, acc = np.split(a, np.cumsum(sizes)[:-1])
    q, dq, target, tau = q.reshape(B, m.nq), dq.reshape(B, m.nv), target.reshape(B, m.na), tau.reshape(B, m.nv)
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        assert np.array_equal(h.mass_matrix_host(0, q).reshape(-1), M)
        kp, kd = fd.spd_gains(0.001)
        assert np.array_equal(h.spd_commands_host(0, (0.001, float(kp), float(kd)), q, dq, target)["commands"].reshape(-1), cmd)
        want, info = h.forward_dynamics_host(0, q, dq, tau)
        assert (info == 0).all() and np.array_equal(want.reshape(-1), acc)
    finally:
        h.close()


@pytest.mark.gpu
def test_file_source_refuses(host_build, tmp_path):
    r = mq.run_file_source(host_build["forward_dynamics_facade_test"], tmp_path)
    assert r.returncode == 0 and "refused: 3 of 3" in r.stdout, r.stdout + r.stderr
