"""Frame Jacobians, the CoM Jacobian and the centroidal momentum matrix through the C++ facade (inria_wbc_amd/csrc/host): Controller::jacobian,
Controller::jacobian_com and Controller::momentum_matrix on a model-driven controller (wbcqp_set_jacobian_frames, wbcqp_jacobians_host behind
ModelSource), and their refusal on a FileSource."""
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
def test_jacobians_after_move_com(host_build, tmp_path):
    """20 ticks of humanoid::move_com (the squat) on 2 Talos instances: jacobian(frame) in the three conventions, jacobian_com() and
    momentum_matrix() equal Handle.jacobians_host on the state the program wrote, bit for bit (the same library call on the same model)."""
    from inria_wbc_amd import capi, observe
    B, out = 2, str(tmp_path / "jac.bin")
    r = subprocess.run([host_build["jacobian_facade_test"], os.path.join(ROOT, "configs/talos/pos_tracker_model.yaml"),
                        os.path.join(ROOT, "configs/talos/squat.yaml"), "20", str(B), out, *FRAMES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(": ", 1) for ln in r.stdout.splitlines() if ": " in ln)
    assert lines["instances"] == str(B)
    assert lines["world is the default"] == "1"
    assert lines["kept"] == "1 refreshed after qp_step_back: 1", r.stdout
    assert lines["a second frame leaves the first"] == "1" and lines["an unknown frame is refused"] == "1"
    # trips to the device, counted in the problem source: the first frame in three conventions (3; WORLD again, Jcom and Ag twice: kept), the
    # second frame in LOCAL (1; it drops every kept J), the first in WORLD again (1; LOCAL came with the second), the unknown frame's refused
    # call (1; it drops every kept J and Jcom) and WORLD after it (1), WORLD after the step back (1; Ag comes with it)
    assert lines["device calls"] == "observe 0, check_collisions 0, mass_matrix 0, jacobians 8, hessians 0", r.stdout
    assert float(lines["max |angular rows, aligned - world|"]) == 0.0
    m, st, tm = mq.talos_case()
    mass = float(m.inertia[:, 0].sum())
    lo, hi = (float(x) for x in lines["Ag / Jcom between"].split())
    assert abs(lo - mass) <= 1e-6 * mass and abs(hi - mass) <= 1e-6 * mass  # (printed with six digits)
    a = np.fromfile(out, dtype=np.float64)
    sizes = [B * m.nq] + 4 * [B * 6 * m.nv] + [B * 3 * m.nv, B * 6 * m.nv]
    assert a.size == sum(sizes)
    q, Jw, Jl, Ja, J2, Jcom, Ag = np.split(a, np.cumsum(sizes)[:-1])
    q = q.reshape(B, m.nq)
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_jacobian_frames(0, observe.frame_ids(m, FRAMES))
        for rf, first in ((capi.RF_WORLD, Jw), (capi.RF_LOCAL, Jl), (capi.RF_LOCAL_WORLD_ALIGNED, Ja)):
            want = h.jacobians_host(0, q, None, rf)
            assert np.array_equal(want["J"][:, 0].reshape(-1), first), rf
            assert np.array_equal(want["Jcom"].reshape(-1), Jcom) and np.array_equal(want["Ag"].reshape(-1), Ag), rf
            if rf == capi.RF_LOCAL:
                assert np.array_equal(want["J"][:, 1].reshape(-1), J2)
        assert np.abs(Jw).max() > 0.1 and not np.array_equal(Jw, Jl) and not np.array_equal(Jl, Ja)
    finally:
        h.close()


@pytest.mark.gpu
def test_file_source_refuses(host_build, tmp_path):
    """A source without a model refuses in the words of its siblings (inertia_matrix, forward_dynamics, rnea_double_support)."""
    r = mq.run_file_source(host_build["jacobian_facade_test"], tmp_path)
    assert r.returncode == 0 and "refused: 4 of 4" in r.stdout, r.stdout + r.stderr
    assert "this problem source has no model: jacobian needs a model-driven source (CONTROLLER.model)" in r.stdout
