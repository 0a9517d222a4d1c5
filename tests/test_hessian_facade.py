"""The kinematic Hessians and the Jacobians' time variation through the C++ facade (inria_wbc_amd/csrc/host): Controller::hessian and
Controller::jacobian_time_variation on a model-driven controller (wbcqp_set_jacobian_frames, wbcqp_kinematic_hessians_host behind ModelSource),
and their refusal on a FileSource."""
import os
import subprocess

import numpy as np
import pytest

from tests import model_queries as mq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = ("leg_left_6_joint", "gripper_right_joint")


@pytest.fixture(scope="module")
def host_build(built_lib):
    return mq.host_build()


@pytest.mark.gpu
def test_hessians_after_move_com(host_build, tmp_path):
    """20 ticks of humanoid::move_com (the squat) on 2 Talos instances: hessian(frame) and jacobian_time_variation(frame) in the three
    conventions equal Handle.kinematic_hessians_host on the state the program wrote, bit for bit (the same library call on the same model)."""
    from inria_wbc_amd import capi, observe
    B, out = 2, str(tmp_path / "hes.bin")
    r = subprocess.run([host_build["hessian_facade_test"], os.path.join(ROOT, "configs/talos/pos_tracker_model.yaml"),
                        os.path.join(ROOT, "configs/talos/squat.yaml"), "20", str(B), out, *FRAMES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["instances"] == str(B)
    assert lines["world is the default"] == "1" and lines["refreshed after qp_step_back"] == "1", r.stdout
    assert lines["a second frame leaves the first"] == "1" and lines["an unknown frame is refused"] == "1"
    # trips to the device, counted in the problem source.  Hessians: H of the first frame in three conventions (3; WORLD again: kept), dJ in
    # three (3), the second frame's H and dJ in LOCAL (2; it joins and drops every kept J, H and dJ), the first frame's H and dJ in WORLD again
    # (2; LOCAL's H came with the second), the unknown frame's refused call (1; it drops everything again) and H in WORLD after it (1), H and dJ
    # in WORLD after the step back (2).  Jacobians: the first frame in LOCAL before the second frame joins and after (2)
    assert lines["device calls"] == "observe 0, check_collisions 0, mass_matrix 0, jacobians 2, hessians 14", r.stdout
    assert float(lines["max |H v - dJ|"]) <= 1e-10 * max(1.0, float(lines["max |dJ|"])) and float(lines["max |dJ|"]) > 0.0
    m, st, tm = mq.talos_case()
    nv = m.nv
    a = np.fromfile(out, dtype=np.float64)
    sizes = [B * m.nq, B * nv] + 4 * [B * 6 * nv * nv] + 4 * [B * 6 * nv]
    assert a.size == sum(sizes)
    q, v, Hw, Hl, Ha, H2, Dw, Dl, Da, D2 = np.split(a, np.cumsum(sizes)[:-1])
    q, v = q.reshape(B, m.nq), v.reshape(B, nv)
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_jacobian_frames(0, observe.frame_ids(m, FRAMES))
        for rf, H1, D1 in ((capi.RF_WORLD, Hw, Dw), (capi.RF_LOCAL, Hl, Dl), (capi.RF_LOCAL_WORLD_ALIGNED, Ha, Da)):
            want = h.kinematic_hessians_host(0, q, v, rf)
            assert np.array_equal(want["H"][:, 0].reshape(-1), H1) and np.array_equal(want["dJ"][:, 0].reshape(-1), D1), rf
            if rf == capi.RF_LOCAL:
                assert np.array_equal(want["H"][:, 1].reshape(-1), H2) and np.array_equal(want["dJ"][:, 1].reshape(-1), D2)
        assert np.abs(Hw).max() > 0.1 and not np.array_equal(Hw, Hl) and not np.array_equal(Hl, Ha) and np.abs(v).max() > 0
    finally:
        h.close()


@pytest.mark.gpu
def test_file_source_refuses(host_build, tmp_path):
    """A source without a model refuses in the words jacobian uses."""
    r = mq.run_file_source(host_build["hessian_facade_test"], tmp_path)
    assert r.returncode == 0 and "refused: 4 of 4" in r.stdout, r.stdout + r.stderr
    assert "this problem source has no model: jacobian needs a model-driven source (CONTROLLER.model)" in r.stdout
