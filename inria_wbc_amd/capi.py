"""ctypes binding of the C ABI in include/wbcqp.h (libwbcqp.so).

This is plumbing: every call goes to the HIP library. There is no Python or CPU implementation of
the solve behind it -- if the library is missing or no gfx950 device is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Dict, Optional, Sequence

import numpy as np

from .structure import Structure

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwbcqp.so")

WBCQP_OK = 0
ERR_NAMES = {0: "OK", 1: "INVALID", 2: "HIP", 3: "UNSUPPORTED", 4: "NO_DEVICE", 5: "RCCL"}
F64, F32 = 0, 1
K_STAMPS = 32  # phase stamps per QP of the -DWBCQP_STAMPS diagnostic build (kStamps, csrc/wbcqp_prims.hpp)
FIELDS = ("M", "h", "A", "b1", "Ac", "bc", "blb", "bub", "tlb", "tub", "w", "Acop")
OUT_FIELDS = ("x", "tau", "status", "iters", "objective", "n_active", "active_mask")  # wbcqp_outputs (active_mask: uint32 [batch, 8], in/out)

# every symbol include/wbcqp.h declares
EXPORTS = ("wbcqp_version", "wbcqp_last_error", "wbcqp_create", "wbcqp_destroy", "wbcqp_set_structure",
           "wbcqp_layout_of", "wbcqp_solve_batch", "wbcqp_solve_batch_host", "wbcqp_solve_ragged",
           "wbcqp_allgather_tau", "wbcqp_integrate", "wbcqp_integrate_host", "wbcqp_set_model", "wbcqp_check_model", "wbcqp_problem_data",
           "wbcqp_problem_data_host", "wbcqp_tick", "wbcqp_tick_host", "wbcqp_tick_graph_create", "wbcqp_tick_graph_launch", "wbcqp_tick_graph_destroy",
           "wbcqp_sync", "wbcqp_launch_order", "wbcqp_solve_dense", "wbcqp_solve_dense_host", "wbcqp_rollout",
           "wbcqp_tick_mixed", "wbcqp_rollout_mixed", "wbcqp_task_costs", "wbcqp_rollout_traced", "wbcqp_rollout_mixed_traced",
           "wbcqp_check_program", "wbcqp_reference_samples", "wbcqp_rollout_program", "wbcqp_rollout_mixed_program",
           "wbcqp_set_observed_frames", "wbcqp_observe", "wbcqp_observe_host", "wbcqp_observe_acom", "wbcqp_observe_acom_host",
           "wbcqp_set_collision_spheres", "wbcqp_check_collisions", "wbcqp_check_collisions_host",
           "wbcqp_set_wrench_frames", "wbcqp_inverse_dynamics", "wbcqp_inverse_dynamics_host",
           "wbcqp_mass_matrix", "wbcqp_mass_matrix_host", "wbcqp_forward_dynamics", "wbcqp_forward_dynamics_host",
           "wbcqp_spd_commands", "wbcqp_spd_commands_host",
           "wbcqp_set_jacobian_frames", "wbcqp_jacobians", "wbcqp_jacobians_host",
           "wbcqp_kinematic_hessians", "wbcqp_kinematic_hessians_host",
           "wbcqp_inverse_dynamics_derivatives", "wbcqp_inverse_dynamics_derivatives_host",
           "wbcqp_torque_monitor_state_bytes", "wbcqp_detect_torque_collisions", "wbcqp_detect_torque_collisions_host",
           "wbcqp_stabilizer_state_bytes", "wbcqp_stabilize", "wbcqp_stabilize_host",
           "wbcqp_set_force_references", "wbcqp_stabilize_zmp", "wbcqp_stabilize_zmp_host")
OBSERVABLES = ("com", "vcom", "placement", "velocity")  # what wbcqp_observe writes (wbcqp_observables); per instance 3, 3, n_frames x 12, n_frames x 6
# (a fifth output, acom [3], comes from wbcqp_observe_acom: asked for by name -- observe(acom=...), observe_host(acom=True))
STAB_INPUTS = ("ref", "wrench", "com", "acom", "placement", "x_prev")  # the arrays of wbcqp_stab_inputs
STAB_OUTPUTS = ("ref_out", "flags", "cop")  # what wbcqp_stabilize writes (wbcqp_stab_outputs)
TORQUE_CHECKS = ("detected", "invalid", "discrepancy", "filtered", "first_tick", "n_detected")  # what wbcqp_detect_torque_collisions writes (wbcqp_torque_checks)
JACOBIAN_OUTPUTS = ("J", "Jcom", "Ag", "drift", "dAgv")  # what wbcqp_jacobians writes (wbcqp_jacobian_outputs); per instance n_frames x 6 x nv, 3 x nv, 6 x nv, n_frames x 6, 6
# what wbcqp_kinematic_hessians writes (wbcqp_hessian_outputs; per instance n_frames x 6 x nv x nv, n_frames x 6 x nv).  The names and the struct
# are defined beside the numpy statement of the call and imported here: the one binding struct that lives outside this module.
# tests/test_capi_binding.py fixes the number of structures THIS module defines (31) and checks their layouts, and existing tests stay as they
# are; CHessianOutputs' layout is checked against the header in tests/test_hessians_host.py with the same function.
from .hessians import OUTPUTS as HESSIAN_OUTPUTS, CHessianOutputs  # noqa: E402
# what wbcqp_inverse_dynamics_derivatives writes (wbcqp_id_derivative_outputs; per instance nv x nv each): defined beside the call's numpy statement
# for the same reason; the layout is checked against the header in tests/test_id_derivatives_host.py.
from .id_derivatives import OUTPUTS as ID_DERIVATIVE_OUTPUTS, CIdDerivativeOutputs  # noqa: E402
RF_WORLD, RF_LOCAL, RF_LOCAL_WORLD_ALIGNED = 0, 1, 2  # wbcqp_reference_frame: pinocchio's values
COLLISIONS = ("colliding", "first_pair", "n_pairs", "clearance", "centres")  # what wbcqp_check_collisions writes (wbcqp_collisions)
TRACE_FIELDS = ("q", "v", "x", "tau", "status", "iters", "objective", "cost")  # what a roll-out can keep per recorded tick (wbcqp_trace)
ROW_FIELDS = ("M", "h", "A", "b1", "Ac", "bc", "blb", "bub", "Acop")  # what wbcqp_problem_data writes (Acop: stacks with a cop task)

c_i32_p = C.POINTER(C.c_int32)
c_f64_p = C.POINTER(C.c_double)


class WbcqpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("wbcqp error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


class CStructure(C.Structure):
    _fields_ = [
        ("nv", C.c_int32), ("na", C.c_int32), ("nc", C.c_int32),
        ("n_dense", C.c_int32), ("n_tasks", C.c_int32), ("dense_row_task", c_i32_p),
        ("n_sel", C.c_int32), ("sel_col", c_i32_p), ("sel_task", c_i32_p),
        ("forcereg_mat", c_f64_p), ("forcereg_task", c_i32_p),
        ("force_gen", c_f64_p), ("fric_mat", c_f64_p), ("fric_lb", c_f64_p), ("fric_ub", c_f64_p),
        ("n_bound", C.c_int32), ("bound_col", c_i32_p), ("act_bounds", C.c_int32),
        ("n_ineq_blocks", C.c_int32), ("ineq_kind", c_i32_p), ("ineq_arg", c_i32_p),
        ("hessian_reg", C.c_double), ("max_iter", C.c_int32),
        ("n_acteq", C.c_int32), ("acteq_joint", c_i32_p), ("acteq_scale", c_f64_p), ("acteq_task", C.c_int32), ("cop_task", C.c_int32),
    ]


class CLayout(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n", "neq", "nin", "nin2", "r1", "len_M", "len_h", "len_A", "len_b1", "len_Ac",
                                         "len_bc", "len_blb", "len_bub", "len_tlb", "len_tub", "len_w", "lds_bytes",
                                         "waves_per_cu")] + [("algorithmic_bytes", C.c_int64), ("wave_per_qp", C.c_int32), ("dense_h", C.c_int32), ("len_Acop", C.c_int32), ("specialised", C.c_int32)]


class CInputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in FIELDS]


class COutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in OUT_FIELDS]


class CDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_int32)]


class CDenseInputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("H", "g", "CE", "ce0", "CI", "ci0")]


class CDenseOutput(C.Structure):
    _fields_ = [("batch", C.c_int32), ("n", C.c_int32), ("x", C.POINTER(C.c_double)), ("status", C.POINTER(C.c_int32)),
                ("iters", C.POINTER(C.c_int32)), ("objective", C.POINTER(C.c_double)), ("n_active", C.POINTER(C.c_int32))]


class CGroup(C.Structure):
    _fields_ = [("slot", C.c_int32), ("batch", C.c_int32), ("inp", CInputs), ("out", COutputs)]


class CModel(C.Structure):
    _fields_ = [("nbody", C.c_int32), ("floating_base", C.c_int32), ("parent", c_i32_p), ("jtype", c_i32_p), ("placement", c_f64_p),
                ("inertia", c_f64_p), ("gravity", C.c_double * 3), ("nframe", C.c_int32), ("frame_body", c_i32_p),
                ("frame_placement", c_f64_p), ("q_lb", c_f64_p), ("q_ub", c_f64_p), ("dq_max", c_f64_p)]


class CTask(C.Structure):
    _fields_ = [("kind", C.c_int32), ("frame", C.c_int32), ("mask", C.c_int32), ("kp", C.c_double), ("kd", C.c_double), ("ref", C.c_int32),
                ("n_avoided", C.c_int32), ("avoided_frame", c_i32_p), ("avoided_r0", c_f64_p), ("radius", C.c_double),
                ("margin", C.c_double), ("m", C.c_double)]


class CTaskMap(C.Structure):
    _fields_ = [("n_task", C.c_int32), ("task", C.POINTER(CTask)), ("posture_kp", C.c_double), ("posture_kd", C.c_double),
                ("posture_ref", C.c_int32), ("n_contact", C.c_int32), ("contact_frame", c_i32_p), ("contact_kp", c_f64_p),
                ("contact_kd", c_f64_p), ("contact_ref", c_i32_p), ("bounds", C.c_int32), ("dt", C.c_double), ("nref", C.c_int32)]


class CState(C.Structure):
    _fields_ = [("q", C.c_void_p), ("v", C.c_void_p), ("ref", C.c_void_p), ("momentum", C.c_void_p)]


class CRolloutIO(C.Structure):
    _fields_ = [("state", CState), ("tlb", C.c_void_p), ("tub", C.c_void_p), ("w", C.c_void_p), ("out", COutputs), ("q_next", C.c_void_p),
                ("v_next", C.c_void_p), ("q_solver", C.c_void_p), ("dt", C.c_double), ("iters_sum", C.c_void_p), ("ticks_ok", C.c_void_p)]


class CTickIO(C.Structure):
    pass  # fields set below (needs CInputs / COutputs)


CTickIO._fields_ = [("state", CState), ("rows", CInputs), ("out", COutputs), ("q_next", C.c_void_p), ("v_next", C.c_void_p),
                    ("q_solver", C.c_void_p), ("dt", C.c_double)]

class CMix(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("slots", c_i32_p), ("w", C.POINTER(C.c_void_p)), ("tlb", C.c_void_p), ("tub", C.c_void_p)]


class CMixedIO(C.Structure):
    _fields_ = [("state", CState), ("out", COutputs), ("q_next", C.c_void_p), ("v_next", C.c_void_p), ("q_solver", C.c_void_p), ("dt", C.c_double)]


class CTrace(C.Structure):
    _fields_ = [("stride", C.c_int32)] + [(k, C.c_void_p) for k in TRACE_FIELDS]


class CSegment(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("T", C.c_double), ("x0", C.c_double * 3), ("xf", C.c_double * 3), ("R0", C.c_double * 9),
                ("axis", C.c_double * 3), ("angle", C.c_double)]


class CTrack(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dim", C.c_int32), ("flags", C.c_int32), ("dst", C.c_int32 * 2), ("n_segments", C.c_int32),
                ("segments", C.POINTER(CSegment))]


class CProgram(C.Structure):
    _fields_ = [("nref", C.c_int32), ("base_stride", C.c_int32), ("base", C.c_void_p), ("offset", c_i32_p), ("n_intro", C.c_int32),
                ("n_cycle", C.c_int32), ("dt", C.c_double), ("n_tracks", C.c_int32), ("tracks", C.POINTER(CTrack)), ("set_of", c_i32_p)]


class CObservables(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in OBSERVABLES]


class CJacobianOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in JACOBIAN_OUTPUTS]


class CSpd(C.Structure):
    _fields_ = [("dt", C.c_double), ("kp", C.c_double), ("kd", C.c_double)]


class CSphereModel(C.Structure):
    _fields_ = [("n_spheres", C.c_int32), ("body", c_i32_p), ("member", c_i32_p), ("centre", c_f64_p), ("diameter", C.POINTER(C.c_float))]


class CCollisions(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in COLLISIONS]


class CTorqueMonitor(C.Structure):
    _fields_ = [("n_joints", C.c_int32), ("joint", c_i32_p), ("threshold", c_f64_p), ("offset", c_f64_p), ("filter", C.c_int32), ("window", C.c_int32),
                ("max_invalid", C.c_int32)]


class CTorqueChecks(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in TORQUE_CHECKS]


class TorqueMonitorBuffers:
    """Host-side wbcqp_torque_monitor from a torque_monitor.Monitor (anything with its attributes); keeps the arrays alive."""

    def __init__(self, monitor):
        self.joint = np.ascontiguousarray(monitor.joint, dtype=np.int32).reshape(-1)
        self.threshold = np.ascontiguousarray(monitor.threshold, dtype=np.float64).reshape(-1)
        self.offset = None if monitor.offset is None else np.ascontiguousarray(monitor.offset, dtype=np.float64).reshape(-1)
        assert self.threshold.size == self.joint.size and (self.offset is None or self.offset.size == self.joint.size)
        self.c = CTorqueMonitor(int(self.joint.size), self.joint.ctypes.data_as(c_i32_p), self.threshold.ctypes.data_as(c_f64_p),
                                self.offset.ctypes.data_as(c_f64_p) if self.offset is not None else None, int(monitor.filter), int(monitor.window),
                                int(monitor.max_invalid))


class CStabilizer(C.Structure):
    _fields_ = [("window", C.c_int32), ("dt", C.c_double), ("mass", C.c_double), ("com_gains", C.c_double * 6), ("ankle_gains", C.c_double * 6),
                ("ffda_gains", C.c_double * 3), ("nref", C.c_int32), ("com_ref", C.c_int32), ("lf_ref", C.c_int32), ("rf_ref", C.c_int32),
                ("torso_ref", C.c_int32), ("lf_contact_ref", C.c_int32), ("rf_contact_ref", C.c_int32), ("lf_force_col", C.c_int32),
                ("rf_force_col", C.c_int32), ("normal", C.c_double * 3), ("lf_pos", C.c_int32), ("rf_pos", C.c_int32)]


class CStabInputs(C.Structure):
    _fields_ = [("ref", C.c_void_p), ("wrench", C.c_void_p), ("com", C.c_void_p), ("acom", C.c_void_p), ("placement", C.c_void_p), ("ldp", C.c_int32),
                ("x_prev", C.c_void_p), ("ldx", C.c_int32)]


class CStabOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in STAB_OUTPUTS]


class CZmpDistributor(C.Structure):
    _fields_ = [("p", C.c_double * 6), ("d", C.c_double * 6), ("lf_force_ref", C.c_int32), ("rf_force_ref", C.c_int32)]


def c_zmp_distributor(zmp) -> CZmpDistributor:
    """wbcqp_zmp_distributor from a stabilizer.ZmpDistributor (anything with its attributes)."""
    vec = lambda a: (C.c_double * 6)(*[float(x) for x in np.asarray(a, dtype=np.float64).reshape(6)])  # noqa: E731
    return CZmpDistributor(vec(zmp.p), vec(zmp.d), int(zmp.lf_force_ref), int(zmp.rf_force_ref))


def c_stabilizer(stab) -> CStabilizer:
    """wbcqp_stabilizer from a stabilizer.Stabilizer (anything with its attributes)."""
    vec = lambda a, n: (C.c_double * n)(*[float(x) for x in np.asarray(a, dtype=np.float64).reshape(n)])  # noqa: E731
    return CStabilizer(int(stab.window), float(stab.dt), float(stab.mass), vec(stab.com_gains, 6), vec(stab.ankle_gains, 6), vec(stab.ffda_gains, 3),
                       int(stab.nref), int(stab.com_ref), int(stab.lf_ref), int(stab.rf_ref), int(stab.torso_ref), int(stab.lf_contact_ref),
                       int(stab.rf_contact_ref), int(stab.lf_force_col), int(stab.rf_force_col), vec(stab.normal, 3), int(stab.lf_pos), int(stab.rf_pos))


def stabilizer_state_bytes(stab) -> int:
    """wbcqp_stabilizer_state_bytes: bytes of one instance's filters, 0 for a stabiliser the library refuses (None: a NULL one).  Host code: no GPU
    needed."""
    return int(load_library().wbcqp_stabilizer_state_bytes(C.byref(c_stabilizer(stab)) if stab is not None else None))


def torque_monitor_state_bytes(monitor) -> int:
    """wbcqp_torque_monitor_state_bytes: bytes of one instance's detector state, 0 for a monitor the library refuses.  Host code: no GPU needed."""
    return int(load_library().wbcqp_torque_monitor_state_bytes(C.byref(TorqueMonitorBuffers(monitor).c)))


def _sig(*argtypes, restype=C.c_int):
    return restype, list(argtypes)


_vp, _int, _p = C.c_void_p, C.c_int, C.POINTER
# How every symbol of EXPORTS is declared: name -> (restype, argtypes), after the prototypes of include/wbcqp.h (tests/test_capi_binding.py holds the
# two against each other).  A handle, a stream and an array of the handle's dtype are c_void_p.
SIGNATURES = {
    "wbcqp_version": _sig(),
    "wbcqp_last_error": _sig(_vp, restype=C.c_char_p),
    "wbcqp_create": _sig(_p(CDesc), _p(_vp)),
    "wbcqp_destroy": _sig(_vp),
    "wbcqp_set_structure": _sig(_vp, _int, _p(CStructure)),
    "wbcqp_layout_of": _sig(_p(CStructure), _p(CLayout)),
    "wbcqp_solve_batch": _sig(_vp, _int, _int, _p(CInputs), _p(COutputs), _vp),
    "wbcqp_solve_ragged": _sig(_vp, _int, _p(CGroup), _vp),
    "wbcqp_solve_dense": _sig(_vp, _int, _int, _int, _int, _int, _p(CDenseInputs), _p(COutputs), _vp),
    "wbcqp_solve_dense_host": _sig(_vp, _int, _int, _int, _int, _int, _p(CDenseInputs), _p(_p(CDenseOutput))),
    "wbcqp_allgather_tau": _sig(_vp, _vp, _vp, _vp, C.c_size_t, _vp),
    "wbcqp_sync": _sig(_vp, _vp),
    "wbcqp_launch_order": _sig(_vp, c_i32_p, C.c_int32, c_i32_p),
    "wbcqp_integrate": _sig(_vp, _int, _int, _int, C.c_double, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp),
    "wbcqp_set_model": _sig(_vp, _int, _p(CModel), _p(CTaskMap)),
    "wbcqp_check_model": _sig(_p(CStructure), _p(CModel), _p(CTaskMap), c_i32_p),
    "wbcqp_set_force_references": _sig(_vp, _int, c_i32_p, c_f64_p),
    "wbcqp_problem_data": _sig(_vp, _int, _int, _p(CState), _p(CInputs), _vp),
    "wbcqp_tick": _sig(_vp, _int, _int, _p(CTickIO), _vp),
    "wbcqp_tick_graph_create": _sig(_vp, _int, _int, _p(CTickIO), _p(_vp)),
    "wbcqp_tick_graph_launch": _sig(_vp, _vp, _vp),
    "wbcqp_tick_graph_destroy": _sig(_vp, _vp),
    "wbcqp_rollout": _sig(_vp, _int, _int, _int, _p(CRolloutIO), _vp),
    "wbcqp_tick_mixed": _sig(_vp, _p(CMix), _int, c_i32_p, _p(CMixedIO), _vp),
    "wbcqp_rollout_mixed": _sig(_vp, _p(CMix), _int, _int, c_i32_p, _p(CRolloutIO), _vp),
    "wbcqp_task_costs": _sig(_vp, _int, _int, _p(CInputs), _vp, _vp, _vp, _vp),
    "wbcqp_rollout_traced": _sig(_vp, _int, _int, _int, _p(CRolloutIO), _p(CTrace), _vp),
    "wbcqp_rollout_mixed_traced": _sig(_vp, _p(CMix), _int, _int, c_i32_p, _p(CRolloutIO), _p(CTrace), _vp),
    "wbcqp_check_program": _sig(_p(CProgram), _int, _int),
    "wbcqp_reference_samples": _sig(_vp, _p(CProgram), _int, _int, _int, _vp, _vp),
    "wbcqp_rollout_program": _sig(_vp, _int, _int, _int, _int, _p(CRolloutIO), _p(CProgram), _p(CTrace), _vp),
    "wbcqp_rollout_mixed_program": _sig(_vp, _p(CMix), _int, _int, _int, _p(CRolloutIO), _p(CProgram), _p(CTrace), _vp),
    "wbcqp_set_observed_frames": _sig(_vp, _int, _int, c_i32_p),
    "wbcqp_observe": _sig(_vp, _int, _int, _vp, _vp, _p(CObservables), _vp),
    "wbcqp_observe_acom": _sig(_vp, _int, _int, _vp, _vp, _p(CObservables), _vp, _vp),
    "wbcqp_set_collision_spheres": _sig(_vp, _int, _p(CSphereModel)),
    "wbcqp_check_collisions": _sig(_vp, _int, _int, _vp, _p(CCollisions), _vp),
    "wbcqp_set_wrench_frames": _sig(_vp, _int, _int, c_i32_p),
    "wbcqp_inverse_dynamics": _sig(_vp, _int, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp),
    "wbcqp_mass_matrix": _sig(_vp, _int, _int, _vp, _vp, _vp),
    "wbcqp_forward_dynamics": _sig(_vp, _int, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp),
    "wbcqp_spd_commands": _sig(_vp, _int, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp),
    "wbcqp_set_jacobian_frames": _sig(_vp, _int, _int, c_i32_p),
    "wbcqp_jacobians": _sig(_vp, _int, _int, _vp, _vp, _int, _p(CJacobianOutputs), _vp),
    "wbcqp_kinematic_hessians": _sig(_vp, _int, _int, _vp, _vp, _int, _p(CHessianOutputs), _vp),
    "wbcqp_inverse_dynamics_derivatives": _sig(_vp, _int, _int, _vp, _vp, _vp, _int, _vp, _p(CIdDerivativeOutputs), _vp),
    "wbcqp_torque_monitor_state_bytes": _sig(_p(CTorqueMonitor), restype=C.c_int64),
    "wbcqp_detect_torque_collisions": _sig(_vp, _p(CTorqueMonitor), _int, _int, _vp, _int, _vp, _vp, _p(CTorqueChecks), _vp),
    "wbcqp_stabilizer_state_bytes": _sig(_p(CStabilizer), restype=C.c_int64),
    "wbcqp_stabilize": _sig(_vp, _p(CStabilizer), _int, _p(CStabInputs), _vp, _p(CStabOutputs), _vp),
    "wbcqp_stabilize_zmp": _sig(_vp, _p(CStabilizer), _p(CZmpDistributor), _int, _p(CStabInputs), _vp, _p(CStabOutputs), _vp, _vp),
}
# the _host forms that are the device signature without the stream
for _name in ("wbcqp_solve_batch", "wbcqp_integrate", "wbcqp_problem_data", "wbcqp_tick", "wbcqp_observe", "wbcqp_observe_acom",
              "wbcqp_check_collisions", "wbcqp_inverse_dynamics", "wbcqp_mass_matrix", "wbcqp_forward_dynamics", "wbcqp_spd_commands",
              "wbcqp_jacobians", "wbcqp_kinematic_hessians", "wbcqp_inverse_dynamics_derivatives", "wbcqp_detect_torque_collisions", "wbcqp_stabilize", "wbcqp_stabilize_zmp"):
    SIGNATURES[_name + "_host"] = (SIGNATURES[_name][0], SIGNATURES[_name][1][:-1])


def declare(lib):
    """Gives every export of a CDLL of the library (any build of it) its restype and argtypes from SIGNATURES; returns the CDLL."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def stamp_buffer_setter(lib):
    """wbcqp_debug_set_stamp_buffer(handle, device buffer of K_STAMPS int64 per QP) of a -DWBCQP_STAMPS build, declared: a diagnostic that is not in
    the header, so not in EXPORTS.  None on a library without the symbol."""
    fn = getattr(lib, "wbcqp_debug_set_stamp_buffer", None)
    if fn is not None:
        fn.restype, fn.argtypes = C.c_int, [_vp, _vp]
    return fn


def dev_ptr(t):
    """Device tensor (anything with numel() and data_ptr()), EMPTY IS ABSENT: None or no elements -> NULL."""
    return t.data_ptr() if t is not None and t.numel() else None


def dev_ptr_given(t):
    """Device tensor, EMPTY IS GIVEN: only None -> NULL (the library says what is wrong with an empty tensor); an int is a device address."""
    return t if t is None or isinstance(t, int) else t.data_ptr()


def host_ptr(a):
    """Host (numpy) array: None -> NULL."""
    return a.ctypes.data if a is not None else None


def _check_state(state):
    assert state is None or (state.dtype == np.uint8 and state.flags["C_CONTIGUOUS"]), "state: a contiguous uint8 array [B, state_bytes]"


def host_outputs(spec, names, null_empty: bool = False):
    """The outputs of a _host call.  spec: name -> (shape, dtype) in the field order of the C struct that takes them; names: the ones asked for.
    Returns (name -> zero-filled array for `names`, the pointers in spec order: NULL for a name not asked for and, with null_empty, for an array
    without elements)."""
    res = {k: np.zeros(*spec[k]) for k in names}
    return res, [res[k].ctypes.data if k in res and (res[k].size or not null_empty) else None for k in spec]


def c_inputs(ptrs) -> CInputs:
    """wbcqp_inputs from name -> pointer; a field the mapping lacks is NULL."""
    return CInputs(*[ptrs.get(k) for k in FIELDS])


def _check(lib, rc: int, handle=None):
    if rc != WBCQP_OK:
        raise WbcqpError(rc, (lib.wbcqp_last_error(handle) or b"").decode())


_lib = None


def load_library(path: Optional[str] = None):
    """Loads libwbcqp.so -- after torch, when torch is installed: the library links libamdhip64.so.7, and a process in which it comes FIRST gets
    /opt/rocm's HIP runtime while a later `import torch` brings torch's bundled one.  Two runtimes on one GPU work, but the first one then answers
    hipOccupancyMaxActiveBlocksPerMultiprocessor with 1 for every solve kernel (measured, tools/occ_state_probe.py --torch-after; the library overrules
    such an answer and says so on stderr).  This module moves tensors that torch allocated, so torch's runtime is the one to share."""
    global _lib
    if _lib is not None:
        return _lib
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401  (before the CDLL below: one HIP runtime per process)
        except ImportError:
            pass
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s is missing: build it with `python -m inria_wbc_amd.build` (hipcc, gfx950). "
            "There is no fallback implementation." % path)
    _lib = declare(C.CDLL(path, mode=C.RTLD_GLOBAL))
    return _lib


class ProgramBuffers:
    """Host-side wbcqp_program built from a `refprog.Program` (anything with its attributes), the per-instance start ticks and the base rows (a device
    tensor [B, nref] or [nref] / [1, nref], or None for the device-free check); keeps the arrays alive."""

    def __init__(self, prog, offsets, base=None):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        self.base = base
        tracks = (CTrack * max(1, len(prog.tracks)))()
        self._segs = []
        for k, t in enumerate(prog.tracks):
            segs = (CSegment * max(1, len(t.segments)))()
            for j, g in enumerate(t.segments):
                segs[j].n_steps, segs[j].T, segs[j].angle = int(g.n_steps), float(g.T), float(g.angle)
                segs[j].x0[:], segs[j].xf[:] = [float(x) for x in g.x0], [float(x) for x in g.xf]
                segs[j].R0[:] = [float(x) for x in np.asarray(g.R0).reshape(9)]
                segs[j].axis[:] = [float(x) for x in g.axis]
            self._segs.append(segs)
            tracks[k].kind, tracks[k].dim, tracks[k].flags, tracks[k].n_segments = int(t.kind), int(t.dim), int(t.flags), len(t.segments)
            tracks[k].dst[:] = [int(t.dst[0]), int(t.dst[1])]
            tracks[k].segments = C.cast(segs, C.POINTER(CSegment))
        self._tracks = tracks
        self.set_of = None if prog.set_of is None else np.ascontiguousarray(prog.set_of, dtype=np.int32)
        p = CProgram()
        p.nref, p.n_intro, p.n_cycle, p.dt, p.n_tracks = int(prog.nref), int(prog.n_intro), int(prog.n_cycle), float(prog.dt), len(prog.tracks)
        p.base = base.data_ptr() if base is not None else None
        p.base_stride = 1 if base is not None and base.dim() == 2 and base.shape[0] > 1 else 0
        p.offset = self.offsets.ctypes.data_as(c_i32_p)
        p.tracks = C.cast(tracks, C.POINTER(CTrack))
        p.set_of = self.set_of.ctypes.data_as(c_i32_p) if self.set_of is not None else None
        self.c = p


def check_program(prog, batch: int, n_slots: int = 0, offsets=None) -> None:
    """wbcqp_check_program: validates a reference program on the host -- no GPU needed.  Raises WbcqpError with the library's message otherwise."""
    lib = load_library()
    pb = ProgramBuffers(prog, np.zeros(batch, np.int32) if offsets is None else offsets)
    _check(lib, lib.wbcqp_check_program(C.byref(pb.c), int(batch), int(n_slots)))


class _KeptArrays:
    """The arrays a host-side C struct points into, kept alive with it; an empty one is passed as one zero (never a NULL)."""

    def __init__(self):
        self._keep = []

    def _kept(self, a, dtype, ctype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.size == 0:
            a = np.zeros(1, dtype=dtype)
        self._keep.append(a)
        return a.ctypes.data_as(ctype)

    def ip(self, a):
        return self._kept(a, np.int32, c_i32_p)

    def dp(self, a):
        return self._kept(a, np.float64, c_f64_p)


class ModelBuffers(_KeptArrays):
    """Host-side wbcqp_model + wbcqp_taskmap built from a `model.Model` and a `model.TaskMap`; keeps the arrays alive."""

    def __init__(self, model, tm):
        super().__init__()
        ip, dp = self.ip, self.dp
        m = CModel()
        m.nbody, m.floating_base = model.nbody, int(model.floating_base)
        m.parent, m.jtype = ip(model.parent), ip(model.jtype)
        m.placement, m.inertia = dp(model.placement), dp(model.inertia)
        m.gravity[:] = model.gravity
        m.nframe = model.nframe
        m.frame_body, m.frame_placement = ip(model.frame_body), dp(model.frame_placement)
        m.q_lb, m.q_ub, m.dq_max = dp(model.q_lb), dp(model.q_ub), dp(model.dq_max)
        tasks = (CTask * max(1, len(tm.blocks)))()
        for i, b in enumerate(tm.blocks):
            t = tasks[i]
            t.kind, t.frame, t.mask, t.kp, t.kd, t.ref = b.kind, b.frame, b.mask, b.kp, b.kd, b.ref
            t.n_avoided = len(b.avoided)
            t.avoided_frame = ip([f for f, _ in b.avoided])
            t.avoided_r0 = dp([r for _, r in b.avoided])
            t.radius, t.margin, t.m = b.radius, b.margin, b.m
        self._tasks = tasks
        k = CTaskMap()
        k.n_task = len(tm.blocks)
        k.task = C.cast(tasks, C.POINTER(CTask))
        k.posture_kp, k.posture_kd, k.posture_ref = tm.posture_kp, tm.posture_kd, tm.posture_ref
        k.n_contact = tm.ncontact
        k.contact_frame, k.contact_kp, k.contact_kd, k.contact_ref = ip(tm.contact_frame), dp(tm.contact_kp), dp(tm.contact_kd), ip(tm.contact_ref)
        k.bounds, k.dt, k.nref = int(tm.n_bound > 0), tm.dt, tm.nref
        self.model, self.taskmap = m, k


class StructureBuffers(_KeptArrays):
    """Host-side wbcqp_structure built from a `Structure`; keeps the numpy arrays alive."""

    def __init__(self, st: Structure):
        super().__init__()
        ip, dp = self.ip, self.dp
        B, lb, ub = st.friction()
        s = CStructure()
        s.nv, s.na, s.nc = st.nv, st.na, st.nc
        s.n_dense, s.n_tasks = st.n_dense, st.n_tasks
        s.dense_row_task = ip(st.dense_row_task)
        s.n_sel = st.n_sel
        s.sel_col = ip(st.sel_col)
        s.sel_task = ip(st.sel_task)
        s.forcereg_mat = dp(st.forcereg_mat())
        s.forcereg_task = ip(st.forcereg_task)
        s.force_gen = dp(st.force_gen())
        s.fric_mat, s.fric_lb, s.fric_ub = dp(B), dp(lb), dp(ub)
        s.n_bound = st.n_bound
        s.bound_col = ip(st.bound_col)
        s.act_bounds = int(st.act_bounds)
        s.n_ineq_blocks = len(st.ineq_blocks)
        s.ineq_kind = ip([k for k, _ in st.ineq_blocks])
        s.ineq_arg = ip([a for _, a in st.ineq_blocks])
        s.hessian_reg = st.hessian_reg
        s.max_iter = st.max_iter
        s.n_acteq = st.n_acteq
        s.acteq_joint = ip(st.acteq_joint)
        s.acteq_scale = dp(st.acteq_scale)
        s.acteq_task = int(st.acteq_task)
        s.cop_task = int(st.cop_task)
        self.c = s


def layout_of(st: Structure) -> Dict[str, int]:
    """wbcqp_layout_of: sizes, per-QP array lengths and LDS footprint (pure host; no GPU needed)."""
    lib = load_library()
    sb = StructureBuffers(st)
    L = CLayout()
    _check(lib, lib.wbcqp_layout_of(C.byref(sb.c), C.byref(L)))
    return {k: getattr(L, k) for k, _ in CLayout._fields_}


def check_model(st: Structure, model, tm) -> int:
    """wbcqp_check_model: validates (structure, tree, task bindings) on the host -- no GPU needed -- and returns the LDS bytes one
    instance of the rows kernel needs.  Raises WbcqpError with the library's message otherwise."""
    lib = load_library()
    sb, mb = StructureBuffers(st), ModelBuffers(model, tm)
    lds = C.c_int32(0)
    _check(lib, lib.wbcqp_check_model(C.byref(sb.c), C.byref(mb.model), C.byref(mb.taskmap), C.byref(lds)))
    return int(lds.value)


FLAG_INDEX_ORDER = 1  # wbcqp_desc.flags: launch in index order (default: longest-first, see include/wbcqp.h)
FLAG_NO_PACKING = 4   # wbcqp_desc.flags: plain longest-first order for the queue (default: bin-packed order for small launches)
FLAG_QUEUE = 8        # wbcqp_desc.flags: the queue also when several workgroups share a CU (default there: hardware dispatch)
FLAG_FULL_LDS = 16    # wbcqp_desc.flags: keep the one-QP-per-CU LDS layout (default: compact layout, two QPs per CU, where eligible)
FLAG_WARM_START = 64  # wbcqp_desc.flags: OPT-IN pick priority for the rows of outputs["active_mask"] (not eiquadprog's rule; include/wbcqp.h)
FLAG_WORKGROUP_PER_QP = 32  # wbcqp_desc.flags: four waves per QP also for n <= 16 (default there: one wavefront per QP, wbcqp_small.hpp)
FLAG_GENERIC_KERNEL = 128  # wbcqp_desc.flags: the generic compact kernel also for the shipped stacks (default: their own instantiations)
FLAG_HW_DISPATCH = 2  # wbcqp_desc.flags: one workgroup per QP through the hardware dispatcher (default: resident workgroups + queue)


def flag_refresh(n: int) -> int:
    """wbcqp_desc.flags: renew the launch order every n-th launch (WBCQP_FLAG_REFRESH; 0 = default 4)"""
    return (n & 0xff) << 8


class Handle:
    """wbcqp_handle bound to one HIP device."""

    def __init__(self, device: int = 0, dtype: int = F64, flags: int = 0):
        self.lib = load_library()
        self.dtype = dtype
        self.np_dtype = np.float64 if dtype == F64 else np.float32
        self.device = device
        self._h = C.c_void_p()
        self._structs: Dict[int, Structure] = {}
        self._lengths: Dict[int, Dict[str, int]] = {}  # slot -> Structure.field_lengths() of what set_structure uploaded
        # slot -> the structure's companions the library cannot be asked for: "model" (model, task map), the numbers of "observed" frames, "spheres", "wrench" frames
        self._companions: Dict[int, dict] = {}
        desc = CDesc(device, dtype, flags)
        _check(self.lib, self.lib.wbcqp_create(C.byref(desc), C.byref(self._h)))

    def _check(self, rc: int):
        if rc != WBCQP_OK:
            _check(self.lib, rc, self._h)

    def close(self):
        if self._h:
            self.lib.wbcqp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_structure(self, slot: int, st: Structure):
        sb = StructureBuffers(st)
        self._check(self.lib.wbcqp_set_structure(self._h, slot, C.byref(sb.c)))
        self._structs[slot], self._lengths[slot] = st, st.field_lengths()
        self._companions_of(slot, reset=True)

    def _companions_of(self, slot: int, reset: bool = False) -> dict:
        """The slot's record; reset: a fresh one (the library drops the model, the selections of frames and the sphere table with the structure or the model)."""
        if reset or slot not in self._companions:
            self._companions[slot] = {"model": None, "observed": 0, "spheres": 0, "wrench": 0, "jacobian": 0}
        return self._companions[slot]

    def _host(self, *arrays):
        """Host arrays as the library reads them: contiguous, of the handle's dtype; None stays None."""
        return [None if a is None else np.ascontiguousarray(a, dtype=self.np_dtype) for a in arrays]

    def _nv(self, slot: int) -> int:
        """nv of the slot's model: what the _host forms of the model queries size their outputs by."""
        return self._companions_of(slot)["model"][0].nv

    # ---- device-pointer path (torch tensors are only carriers of device memory) ----
    def _rows(self, slot: int, batch: int, rows, names=FIELDS) -> CInputs:
        """wbcqp_inputs from device tensors: those of `names` that are given and that the slot's structure has; each checked against its length."""
        L = self._lengths[slot]
        ptrs = {}
        for k in names:
            t = rows.get(k)
            if L[k] and t is not None:
                assert t.is_cuda and t.is_contiguous() and t.numel() == batch * L[k], (k, tuple(t.shape), batch, L[k])
                ptrs[k] = t.data_ptr()
        return c_inputs(ptrs)

    def _pack(self, slot: int, batch: int, inputs, outputs):
        return self._rows(slot, batch, inputs), self._outs(outputs)

    def solve_batch(self, slot: int, batch: int, inputs: Dict[str, "object"], outputs: Dict[str, "object"], stream: int = 0):
        cin, cout = self._pack(slot, batch, inputs, outputs)
        self._check(self.lib.wbcqp_solve_batch(self._h, slot, batch, C.byref(cin), C.byref(cout), C.c_void_p(stream)))

    def solve_ragged(self, groups: Sequence[tuple], stream: int = 0):
        """groups: sequence of (slot, batch, inputs, outputs) with device tensors."""
        arr = (CGroup * len(groups))()
        for i, (slot, batch, inputs, outputs) in enumerate(groups):
            cin, cout = self._pack(slot, batch, inputs, outputs)
            arr[i].slot, arr[i].batch, arr[i].inp, arr[i].out = slot, batch, cin, cout
        self._check(self.lib.wbcqp_solve_ragged(self._h, len(groups), arr, C.c_void_p(stream)))

    def integrate(self, batch: int, nv: int, floating_base: bool, dt: float, q, dq, x, ldx: int, status, q_next, v_next,
                  q_solver=None, stream: int = 0):
        """State integration after the path (controller.cpp:250-272) on device tensors (anything with .data_ptr())."""
        ptr = dev_ptr_given
        self._check(self.lib.wbcqp_integrate(self._h, batch, nv, 1 if floating_base else 0, float(dt), ptr(q), ptr(dq), ptr(x), ldx,
                                             ptr(status), ptr(q_next), ptr(v_next), ptr(q_solver), C.c_void_p(stream)))

    def set_model(self, slot: int, model, tm):
        """Binds a kinematic tree and its task bindings to a slot that holds the matching structure (wbcqp_set_model)."""
        mb = ModelBuffers(model, tm)
        self._check(self.lib.wbcqp_set_model(self._h, slot, C.byref(mb.model), C.byref(mb.taskmap)))
        self._companions_of(slot, reset=True)["model"] = (model, tm)

    def set_force_references(self, slot: int, force_ref: Optional[Sequence[int]], weight):
        """wbcqp_set_force_references: force_ref [nc] offsets of the contacts' 6-number force references in a reference row (TaskMap.contact_fref;
        -1: none), weight [nc, 6] the w_f the slot's forcereg_mat was made with.  After set_model, dropped with the model."""
        fr = None if force_ref is None else np.ascontiguousarray(force_ref, dtype=np.int32).reshape(-1)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        self._check(self.lib.wbcqp_set_force_references(self._h, slot, fr.ctypes.data_as(c_i32_p) if fr is not None else None,
                                                        w.ctypes.data_as(c_f64_p) if w is not None else None))

    def _select_frames(self, slot: int, frames: Sequence[int], setter, what: str):
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        self._check(setter(self._h, slot, int(fr.size), fr.ctypes.data_as(c_i32_p)))
        self._companions_of(slot)[what] = int(fr.size)

    def set_observed_frames(self, slot: int, frames: Sequence[int]):
        """Which frames of the slot's model wbcqp_observe reports: indices into the model's frame table (observe.frame_ids turns names into
        them), repeats allowed, at most 64 (wbcqp_set_observed_frames)."""
        self._select_frames(slot, frames, self.lib.wbcqp_set_observed_frames, "observed")

    def observe(self, slot: int, batch: int, q, v=None, com=None, vcom=None, placement=None, velocity=None, stream: int = 0, acom=None):
        """CoM and frame poses of `batch` states on device tensors (wbcqp_observe): q [batch, nq], v [batch, nv] (None when neither vcom, acom nor
        velocity is asked for); outputs, each optional: com / vcom / acom [batch, 3], placement [batch, n_frames, 12], velocity [batch, n_frames, 6]."""
        out = CObservables(dev_ptr(com), dev_ptr(vcom), dev_ptr(placement), dev_ptr(velocity))
        if acom is not None:  # (wbcqp_observe_acom: the same launch with one more output)
            self._check(self.lib.wbcqp_observe_acom(self._h, slot, int(batch), dev_ptr(q), dev_ptr(v), C.byref(out), dev_ptr(acom), C.c_void_p(stream)))
            return
        self._check(self.lib.wbcqp_observe(self._h, slot, int(batch), dev_ptr(q), dev_ptr(v), C.byref(out), C.c_void_p(stream)))

    def observe_host(self, slot: int, q: np.ndarray, v: Optional[np.ndarray] = None, acom: bool = False) -> Dict[str, np.ndarray]:
        """wbcqp_observe_host: dict(com [B, 3], placement [B, n_frames, 12]) and, when v is given, vcom [B, 3] and velocity [B, n_frames, 6]
        (placement / velocity only when frames are selected); acom=True (needs v) adds acom [B, 3].  The library cannot be asked how many frames a slot observes, so the outputs are
        sized from what THIS Handle's set_observed_frames last selected on the slot: a selection made any other way (the raw library, another
        wrapper of the same handle) is not seen here -- such callers size their own buffers and use observe()."""
        q, v = self._host(q, v)
        B, f = q.shape[0], self.np_dtype
        nf = self._companions_of(slot)["observed"]
        names = ["com", "placement"] if nf else ["com"]
        if v is not None:
            names += ["vcom", "velocity"] if nf else ["vcom"]
        res, ptrs = host_outputs({"com": ((B, 3), f), "vcom": ((B, 3), f), "placement": ((B, nf, 12), f), "velocity": ((B, nf, 6), f)}, names)
        out = CObservables(*ptrs)
        if acom:
            res["acom"] = np.zeros((B, 3), f)
            self._check(self.lib.wbcqp_observe_acom_host(self._h, slot, B, q.ctypes.data, host_ptr(v), C.byref(out), res["acom"].ctypes.data))
            return res
        self._check(self.lib.wbcqp_observe_host(self._h, slot, B, q.ctypes.data, host_ptr(v), C.byref(out)))
        return res

    def set_wrench_frames(self, slot: int, frames: Sequence[int]):
        """Where the wrenches of inverse_dynamics act: indices into the model's frame table (observe.frame_ids turns names into them), repeats
        allowed, at most 8 (wbcqp_set_wrench_frames)."""
        self._select_frames(slot, frames, self.lib.wbcqp_set_wrench_frames, "wrench")

    def inverse_dynamics(self, slot: int, batch: int, q, tau, v=None, a=None, lda: int = 0, wrench=None, stream: int = 0):
        """tau = M(q) a + nle(q, v) - sum_k J_k' w_k of `batch` states on device tensors (wbcqp_inverse_dynamics): q [batch, nq], tau [batch, nv];
        v [batch, nv] or None (zero); a or None (zero): row i starts lda elements after row i - 1 (lda = 0: a.shape[-1]), so a tick's x serves;
        wrench [batch, n_frames, 6] or None: linear, angular in the own axes of the frames of set_wrench_frames."""
        if a is not None and lda == 0:
            lda = int(a.shape[-1])
        ptr = dev_ptr_given
        self._check(self.lib.wbcqp_inverse_dynamics(self._h, slot, int(batch), ptr(q), ptr(v), ptr(a), int(lda), ptr(wrench), ptr(tau),
                                                    C.c_void_p(stream)))

    def inverse_dynamics_host(self, slot: int, q: np.ndarray, v: Optional[np.ndarray] = None, a: Optional[np.ndarray] = None,
                              wrench: Optional[np.ndarray] = None) -> np.ndarray:
        """wbcqp_inverse_dynamics_host: tau [B, nv].  a [B, lda] with lda >= nv: its first nv columns are the accelerations (a tick's x as it is)."""
        q, v, a, wrench = self._host(q, v, a, wrench)
        B = q.shape[0]
        tau = np.zeros((B, self._nv(slot)), self.np_dtype)
        dat = host_ptr
        self._check(self.lib.wbcqp_inverse_dynamics_host(self._h, slot, B, q.ctypes.data, dat(v), dat(a), int(a.shape[-1]) if a is not None else 0,
                                                         dat(wrench), tau.ctypes.data))
        return tau

    def inverse_dynamics_derivatives(self, slot: int, batch: int, q, v=None, a=None, lda: int = 0, wrench=None, dtau_dq=None, dtau_dv=None,
                                     stream: int = 0):
        """dtau/dq and dtau/dv of the inverse dynamics of `batch` states on device tensors (wbcqp_inverse_dynamics_derivatives); the inputs are
        inverse_dynamics': q [batch, nq]; v [batch, nv] or None (zero); a or None (zero): row i starts lda elements after row i - 1 (lda = 0:
        a.shape[-1]); wrench [batch, n_frames, 6] or None.  Outputs, each optional: dtau_dq, dtau_dv [batch, nv, nv] ([b, i, j] = d tau_i / d q_j,
        d tau_i / d v_j; dtau_dv needs v)."""
        if a is not None and lda == 0:
            lda = int(a.shape[-1])
        ptr = dev_ptr_given
        out = CIdDerivativeOutputs(ptr(dtau_dq), ptr(dtau_dv))
        self._check(self.lib.wbcqp_inverse_dynamics_derivatives(self._h, slot, int(batch), ptr(q), ptr(v), ptr(a), int(lda), ptr(wrench),
                                                                C.byref(out), C.c_void_p(stream)))

    def inverse_dynamics_derivatives_host(self, slot: int, q: np.ndarray, v: Optional[np.ndarray] = None, a: Optional[np.ndarray] = None,
                                          wrench: Optional[np.ndarray] = None, which: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
        """wbcqp_inverse_dynamics_derivatives_host: a dict of the outputs named in `which` (of ID_DERIVATIVE_OUTPUTS), each [B, nv, nv].  which
        None: dtau_dq and, with v, dtau_dv.  a [B, lda] with lda >= nv: its first nv columns are the accelerations."""
        q, v, a, wrench = self._host(q, v, a, wrench)
        B, nv, f = q.shape[0], self._nv(slot), self.np_dtype
        if which is None:
            which = ["dtau_dq"] + (["dtau_dv"] if v is not None else [])
        res, ptrs = host_outputs({k: ((B, nv, nv), f) for k in ID_DERIVATIVE_OUTPUTS}, which)
        out = CIdDerivativeOutputs(*ptrs)
        dat = host_ptr
        self._check(self.lib.wbcqp_inverse_dynamics_derivatives_host(self._h, slot, B, q.ctypes.data, dat(v), dat(a),
                                                                     int(a.shape[-1]) if a is not None else 0, dat(wrench), C.byref(out)))
        return res

    def mass_matrix(self, slot: int, batch: int, q, M, stream: int = 0):
        """M(q) of `batch` states on device tensors (wbcqp_mass_matrix): q [batch, nq], M [batch, nv, nv], both triangles."""
        self._check(self.lib.wbcqp_mass_matrix(self._h, slot, int(batch), dev_ptr_given(q), dev_ptr_given(M), C.c_void_p(stream)))

    def mass_matrix_host(self, slot: int, q: np.ndarray) -> np.ndarray:
        """wbcqp_mass_matrix_host: M [B, nv, nv]."""
        q = np.ascontiguousarray(q, dtype=self.np_dtype)
        B, nv = q.shape[0], self._nv(slot)
        M = np.zeros((B, nv, nv), self.np_dtype)
        self._check(self.lib.wbcqp_mass_matrix_host(self._h, slot, B, q.ctypes.data, M.ctypes.data))
        return M

    @staticmethod
    def _damping(damping):
        """(the array to keep alive, its pointer) of a HOST damping [nv], or (None, None)."""
        if damping is None:
            return None, None
        d = np.ascontiguousarray(damping, dtype=np.float64).reshape(-1)
        return d, d.ctypes.data

    def forward_dynamics(self, slot: int, batch: int, q, a, v=None, tau=None, ldt: int = 0, wrench=None, damping=None, info=None, stream: int = 0):
        """(M(q) + diag(damping)) a = tau - nle(q, v) + sum_k J_k' w_k of `batch` states on device tensors (wbcqp_forward_dynamics): q [batch, nq],
        a [batch, nv]; v [batch, nv] or None (zero); tau or None (zero): ALL nv entries per row, row i ldt elements after row i - 1 (ldt = 0:
        tau.shape[-1]); wrench [batch, n_frames, 6] or None, as for inverse_dynamics; damping: a HOST array [nv] or None; info: int32 [batch] or None."""
        if tau is not None and ldt == 0:
            ldt = int(tau.shape[-1])
        keep, dptr = self._damping(damping)  # (keep: holds the converted array alive until the call has copied it)
        ptr = dev_ptr_given
        self._check(self.lib.wbcqp_forward_dynamics(self._h, slot, int(batch), ptr(q), ptr(v), ptr(tau), int(ldt), ptr(wrench), dptr, ptr(a), ptr(info),
                                                    C.c_void_p(stream)))

    def forward_dynamics_host(self, slot: int, q: np.ndarray, v: Optional[np.ndarray] = None, tau: Optional[np.ndarray] = None,
                              wrench: Optional[np.ndarray] = None, damping=None):
        """wbcqp_forward_dynamics_host: (a [B, nv], info [B]).  tau [B, ldt] with ldt >= nv: its first nv columns are the torques."""
        q, v, tau, wrench = self._host(q, v, tau, wrench)
        B, nv = q.shape[0], self._nv(slot)
        a, info = np.zeros((B, nv), self.np_dtype), np.zeros(B, np.int32)
        dat = host_ptr
        keep, dptr = self._damping(damping)  # (keep: holds the converted array alive until the call has copied it)
        self._check(self.lib.wbcqp_forward_dynamics_host(self._h, slot, B, q.ctypes.data, dat(v), dat(tau), int(tau.shape[-1]) if tau is not None else 0,
                                                         dat(wrench), dptr, a.ctypes.data, info.ctypes.data))
        return a, info

    def spd_commands(self, slot: int, batch: int, law, q, target, commands, v=None, ldtarget: int = 0, wrench=None, qddot=None, info=None,
                     stream: int = 0):
        """The reference's compute_spd on device tensors (wbcqp_spd_commands).  law: (dt, kp, kd) -- forward_dynamics.spd_gains(dt) gives the
        reference's gains; q [batch, nq]; target: na entries per row, ldtarget apart (0: target.shape[-1]); commands [batch, nv]; qddot
        [batch, nv] or None; wrench as for inverse_dynamics (the reference's constraint forces)."""
        if ldtarget == 0:
            ldtarget = int(target.shape[-1])
        c = CSpd(*[float(x) for x in law])
        ptr = dev_ptr_given
        self._check(self.lib.wbcqp_spd_commands(self._h, slot, int(batch), C.byref(c), ptr(q), ptr(v), ptr(target), int(ldtarget), ptr(wrench),
                                                ptr(commands), ptr(qddot), ptr(info), C.c_void_p(stream)))

    def spd_commands_host(self, slot: int, law, q: np.ndarray, v: Optional[np.ndarray], target: np.ndarray, wrench: Optional[np.ndarray] = None):
        """wbcqp_spd_commands_host: dict(commands [B, nv], qddot [B, nv], info [B]).  target [B, ldtarget] with ldtarget >= na."""
        q, v, target, wrench = self._host(q, v, target, wrench)
        B, nv = q.shape[0], self._nv(slot)
        spec = {"commands": ((B, nv), self.np_dtype), "qddot": ((B, nv), self.np_dtype), "info": ((B,), np.int32)}  # (the call's last three arguments)
        res, ptrs = host_outputs(spec, spec)
        dat = host_ptr
        c = CSpd(*[float(x) for x in law])
        self._check(self.lib.wbcqp_spd_commands_host(self._h, slot, B, C.byref(c), q.ctypes.data, dat(v), dat(target), int(target.shape[-1]), dat(wrench),
                                                     *ptrs))
        return res

    def set_jacobian_frames(self, slot: int, frames: Sequence[int]):
        """Which frames of the slot's model jacobians reports in J and drift: indices into the model's frame table (observe.frame_ids turns names
        into them), repeats allowed, at most 64 (wbcqp_set_jacobian_frames).  A selection of its own, beside the observed and the wrench frames."""
        self._select_frames(slot, frames, self.lib.wbcqp_set_jacobian_frames, "jacobian")

    def jacobians(self, slot: int, batch: int, q, v=None, reference_frame: int = RF_LOCAL, J=None, Jcom=None, Ag=None, drift=None, dAgv=None,
                  stream: int = 0):
        """Frame Jacobians, the CoM Jacobian and the centroidal momentum matrix of `batch` states on device tensors (wbcqp_jacobians): q [batch, nq],
        v [batch, nv] (None when neither drift nor dAgv is asked for); outputs, each optional: J [batch, n_frames, 6, nv], Jcom [batch, 3, nv],
        Ag [batch, 6, nv], drift [batch, n_frames, 6], dAgv [batch, 6]."""
        out = CJacobianOutputs(*[dev_ptr_given(t) for t in (J, Jcom, Ag, drift, dAgv)])
        self._check(self.lib.wbcqp_jacobians(self._h, slot, int(batch), dev_ptr_given(q), dev_ptr_given(v), int(reference_frame), C.byref(out),
                                             C.c_void_p(stream)))

    def jacobians_host(self, slot: int, q: np.ndarray, v: Optional[np.ndarray] = None, reference_frame: int = RF_LOCAL,
                       which: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
        """wbcqp_jacobians_host: a dict of the outputs named in `which` (of JACOBIAN_OUTPUTS).  which None: everything the arguments admit -- Jcom
        and Ag; J when frames are selected; with v, dAgv and (frames selected, not RF_WORLD) drift.  J and drift are sized from what THIS Handle's
        set_jacobian_frames last selected on the slot (see observe_host)."""
        q, v = self._host(q, v)
        B, nv, nf, f = q.shape[0], self._nv(slot), self._companions_of(slot)["jacobian"], self.np_dtype
        if which is None:
            which = ["Jcom", "Ag"] + (["J"] if nf else []) + (["dAgv"] if v is not None else []) + (
                ["drift"] if v is not None and nf and reference_frame != RF_WORLD else [])
        res, ptrs = host_outputs({"J": ((B, nf, 6, nv), f), "Jcom": ((B, 3, nv), f), "Ag": ((B, 6, nv), f), "drift": ((B, nf, 6), f), "dAgv": ((B, 6), f)},
                                 which)
        out = CJacobianOutputs(*ptrs)
        self._check(self.lib.wbcqp_jacobians_host(self._h, slot, B, q.ctypes.data, host_ptr(v), int(reference_frame), C.byref(out)))
        return res

    def kinematic_hessians(self, slot: int, batch: int, q, v=None, reference_frame: int = RF_LOCAL, H=None, dJ=None, stream: int = 0):
        """The kinematic Hessians and the Jacobians' time variation of `batch` states on device tensors (wbcqp_kinematic_hessians), for the frames of
        set_jacobian_frames: q [batch, nq], v [batch, nv] (None when dJ is not asked for); outputs, each optional: H [batch, n_frames, 6, nv, nv]
        (H[b, f, r, j, k] = d J[b, f, r, j] / d q_k), dJ [batch, n_frames, 6, nv]."""
        out = CHessianOutputs(*[dev_ptr_given(t) for t in (H, dJ)])
        self._check(self.lib.wbcqp_kinematic_hessians(self._h, slot, int(batch), dev_ptr_given(q), dev_ptr_given(v), int(reference_frame),
                                                      C.byref(out), C.c_void_p(stream)))

    def kinematic_hessians_host(self, slot: int, q: np.ndarray, v: Optional[np.ndarray] = None, reference_frame: int = RF_LOCAL,
                                which: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
        """wbcqp_kinematic_hessians_host: a dict of the outputs named in `which` (of HESSIAN_OUTPUTS).  which None: H and, with v, dJ.  Sized from
        what THIS Handle's set_jacobian_frames last selected on the slot (see observe_host)."""
        q, v = self._host(q, v)
        B, nv, nf, f = q.shape[0], self._nv(slot), self._companions_of(slot)["jacobian"], self.np_dtype
        if which is None:
            which = ["H"] + (["dJ"] if v is not None else [])
        res, ptrs = host_outputs({"H": ((B, nf, 6, nv, nv), f), "dJ": ((B, nf, 6, nv), f)}, which)
        out = CHessianOutputs(*ptrs)
        self._check(self.lib.wbcqp_kinematic_hessians_host(self._h, slot, B, q.ctypes.data, host_ptr(v), int(reference_frame), C.byref(out)))
        return res

    def detect_torque_collisions(self, monitor, batch: int, n_ticks: int, tau_model, ldt: int, tau_sensor, state=None, detected=None, invalid=None,
                                 discrepancy=None, filtered=None, first_tick=None, n_detected=None, stream: int = 0):
        """External collisions from joint torques on device tensors (wbcqp_detect_torque_collisions).  monitor: a torque_monitor.Monitor;
        tau_model: row (t, i) starts (t * batch + i) * ldt elements after its data pointer (or an int: a device address, e.g. the output of
        inverse_dynamics moved by six elements); tau_sensor [n_ticks, batch, n_joints]; state: uint8 / float64 tensor of batch * state_bytes bytes,
        in and out, or None; outputs, each optional: detected [n_ticks, batch] int32, invalid [n_ticks, batch] int64 (bit j: joint j),
        discrepancy / filtered [n_ticks, batch, n_joints] (the handle's dtype), first_tick / n_detected [batch] int32."""
        mb = TorqueMonitorBuffers(monitor)
        ptr = dev_ptr_given
        out = CTorqueChecks(ptr(detected), ptr(invalid), ptr(discrepancy), ptr(filtered), ptr(first_tick), ptr(n_detected))
        self._check(self.lib.wbcqp_detect_torque_collisions(self._h, C.byref(mb.c), int(batch), int(n_ticks), ptr(tau_model), int(ldt), ptr(tau_sensor),
                                                            ptr(state), C.byref(out), C.c_void_p(stream)))

    def detect_torque_collisions_host(self, monitor, tau_model: np.ndarray, tau_sensor: np.ndarray, state: Optional[np.ndarray] = None,
                                      outputs: Sequence[str] = TORQUE_CHECKS) -> Dict[str, np.ndarray]:
        """wbcqp_detect_torque_collisions_host: tau_model [T, B, ldt], tau_sensor [T, B, n_joints]; state: a contiguous uint8 array
        [B, state_bytes], updated in place, or None.  Returns the outputs named in `outputs` as numpy arrays (invalid as uint64)."""
        tau_model, tau_sensor = self._host(tau_model, tau_sensor)
        T, B, n = tau_sensor.shape
        assert tau_model.shape[:2] == (T, B), (tau_model.shape, tau_sensor.shape)
        _check_state(state)
        res, ptrs = host_outputs({"detected": ((T, B), np.int32), "invalid": ((T, B), np.uint64), "discrepancy": ((T, B, n), self.np_dtype),
                                  "filtered": ((T, B, n), self.np_dtype), "first_tick": ((B,), np.int32), "n_detected": ((B,), np.int32)}, outputs)
        mb = TorqueMonitorBuffers(monitor)
        out = CTorqueChecks(*ptrs)
        self._check(self.lib.wbcqp_detect_torque_collisions_host(self._h, C.byref(mb.c), B, T, tau_model.ctypes.data, int(tau_model.shape[2]),
                                                                 tau_sensor.ctypes.data, host_ptr(state), C.byref(out)))
        return res

    @staticmethod
    def _stab_io(stab, ref, wrench, com, acom, placement, ldp, x_prev, ldx, ref_out, flags, cop):
        """(wbcqp_stabilizer, wbcqp_stab_inputs, wbcqp_stab_outputs) of stabilize and stabilize_zmp, from device tensors or device addresses."""
        ptr = dev_ptr_given
        width = lambda t, ld: int(ld) if ld or t is None or isinstance(t, int) else int(t.numel() // max(int(t.shape[0]), 1))  # noqa: E731
        cin = CStabInputs(ptr(ref), ptr(wrench), ptr(com), ptr(acom), ptr(placement), width(placement, ldp), ptr(x_prev), width(x_prev, ldx))
        return c_stabilizer(stab), cin, CStabOutputs(ptr(ref_out), ptr(flags), ptr(cop))

    def stabilize(self, stab, batch: int, ref, wrench, com, acom, placement, ldp: int = 0, x_prev=None, ldx: int = 0, state=None, ref_out=None,
                  flags=None, cop=None, stream: int = 0):
        """One tick of the stabiliser on device tensors (wbcqp_stabilize).  stab: a stabilizer.Stabilizer; ref [batch, nref], wrench [batch, 12],
        com / acom [batch, 3]; placement: row i starts i * ldp elements after its data pointer (ldp = 0: its row length), as observe() writes it;
        x_prev: the previous tick's x, rows ldx apart (0: its row length), or None; state: uint8 / float64 tensor of batch * state_bytes bytes, in
        and out, or None; outputs, each optional: ref_out [batch, nref] (may be ref), flags [batch] int32, cop [batch, 3, 2]."""
        cs, cin, out = self._stab_io(stab, ref, wrench, com, acom, placement, ldp, x_prev, ldx, ref_out, flags, cop)
        self._check(self.lib.wbcqp_stabilize(self._h, C.byref(cs), int(batch), C.byref(cin), dev_ptr_given(state), C.byref(out), C.c_void_p(stream)))

    def stabilize_zmp(self, stab, zmp, batch: int, ref, wrench, com, acom, placement, ldp: int = 0, x_prev=None, ldx: int = 0, state=None,
                      ref_out=None, flags=None, cop=None, alpha=None, stream: int = 0):
        """stabilize with the ZMP force distributor (wbcqp_stabilize_zmp).  zmp: a stabilizer.ZmpDistributor, or None (then this IS stabilize);
        alpha [batch, 2]: one more optional output."""
        cs, cin, out = self._stab_io(stab, ref, wrench, com, acom, placement, ldp, x_prev, ldx, ref_out, flags, cop)
        cz = C.byref(c_zmp_distributor(zmp)) if zmp is not None else None
        self._check(self.lib.wbcqp_stabilize_zmp(self._h, C.byref(cs), cz, int(batch), C.byref(cin), dev_ptr_given(state), C.byref(out),
                                                 dev_ptr_given(alpha), C.c_void_p(stream)))

    def _stabilize_host(self, export, distributor: tuple, stab, inputs, state, names, outputs):
        """The body of stabilize_host and stabilize_zmp_host.  export: the symbol itself; distributor: the arguments it takes between the stabiliser
        and the batch (none, or the wbcqp_zmp_distributor); names: the outputs it has."""
        a = dict(zip(STAB_INPUTS, self._host(*[inputs.get(k) for k in STAB_INPUTS])))
        B = a["ref"].shape[0]
        a = {k: (t.reshape(B, -1) if t is not None else None) for k, t in a.items()}
        _check_state(state)
        dat = host_ptr
        cin = CStabInputs(dat(a["ref"]), dat(a["wrench"]), dat(a["com"]), dat(a["acom"]), dat(a["placement"]), int(a["placement"].shape[1]),
                          dat(a["x_prev"]), int(a["x_prev"].shape[1]) if a["x_prev"] is not None else 0)
        shape = {"ref_out": ((B, int(stab.nref)), self.np_dtype), "flags": ((B,), np.int32), "cop": ((B, 3, 2), self.np_dtype),
                 "alpha": ((B, 2), self.np_dtype)}
        res, ptrs = host_outputs({k: shape[k] for k in names}, outputs)
        cs, out = c_stabilizer(stab), CStabOutputs(*ptrs[:3])
        self._check(export(self._h, C.byref(cs), *distributor, B, C.byref(cin), host_ptr(state), C.byref(out), *ptrs[3:]))
        return res

    def stabilize_zmp_host(self, stab, zmp, inputs: Dict[str, np.ndarray], state: Optional[np.ndarray] = None,
                           outputs: Sequence[str] = STAB_OUTPUTS + ("alpha",)) -> Dict[str, np.ndarray]:
        """wbcqp_stabilize_zmp_host: stabilize_host with the distributor (zmp None: stabilize_host's bits); `alpha` [B, 2] is one more output."""
        cz = C.byref(c_zmp_distributor(zmp)) if zmp is not None else None
        return self._stabilize_host(self.lib.wbcqp_stabilize_zmp_host, (cz,), stab, inputs, state, STAB_OUTPUTS + ("alpha",), outputs)

    def stabilize_host(self, stab, inputs: Dict[str, np.ndarray], state: Optional[np.ndarray] = None,
                       outputs: Sequence[str] = STAB_OUTPUTS) -> Dict[str, np.ndarray]:
        """wbcqp_stabilize_host: inputs as stabilizer.step takes them (ref [B, nref], wrench [B, 12], com, acom [B, 3], placement [B, ldp], x_prev
        [B, ldx] or absent); state: a contiguous uint8 array [B, state_bytes], updated in place, or None.  Returns the outputs named in `outputs`."""
        return self._stabilize_host(self.lib.wbcqp_stabilize_host, (), stab, inputs, state, STAB_OUTPUTS, outputs)

    def set_collision_spheres(self, slot: int, table):
        """The slot's sphere model (wbcqp_set_collision_spheres): a collision.SphereTable (collision.sphere_table builds one from the reference's
        collision file), or None / an empty table to drop it."""
        n = 0 if table is None else int(table.n_spheres)
        if n == 0:
            sm = CSphereModel(0, None, None, None, None)
        else:
            keep = (np.ascontiguousarray(table.body, dtype=np.int32), np.ascontiguousarray(table.member, dtype=np.int32),
                    np.ascontiguousarray(table.centre, dtype=np.float64), np.ascontiguousarray(table.diameter, dtype=np.float32))
            sm = CSphereModel(n, keep[0].ctypes.data_as(c_i32_p), keep[1].ctypes.data_as(c_i32_p), keep[2].ctypes.data_as(c_f64_p),
                              keep[3].ctypes.data_as(C.POINTER(C.c_float)))
        self._check(self.lib.wbcqp_set_collision_spheres(self._h, slot, C.byref(sm)))
        self._companions_of(slot)["spheres"] = n

    def check_collisions(self, slot: int, batch: int, q, colliding=None, first_pair=None, n_pairs=None, clearance=None, centres=None, stream: int = 0):
        """Self-collision of `batch` states on device tensors (wbcqp_check_collisions): q [batch, nq]; outputs, each optional: colliding [batch],
        first_pair [batch, 2], n_pairs [batch] (int32), clearance [batch], centres [batch, n_spheres, 3] (the handle's dtype)."""
        out = CCollisions(dev_ptr(colliding), dev_ptr(first_pair), dev_ptr(n_pairs), dev_ptr(clearance), dev_ptr(centres))
        self._check(self.lib.wbcqp_check_collisions(self._h, slot, int(batch), dev_ptr(q), C.byref(out), C.c_void_p(stream)))

    def check_collisions_host(self, slot: int, q: np.ndarray) -> Dict[str, np.ndarray]:
        """wbcqp_check_collisions_host: the five outputs as numpy arrays.  Like observe_host, `centres` is sized from what THIS Handle's
        set_collision_spheres last uploaded on the slot."""
        q = np.ascontiguousarray(q, dtype=self.np_dtype)
        B = q.shape[0]
        ns = self._companions_of(slot)["spheres"]
        res, ptrs = host_outputs({"colliding": ((B,), np.int32), "first_pair": ((B, 2), np.int32), "n_pairs": ((B,), np.int32),
                                  "clearance": ((B,), self.np_dtype), "centres": ((B, ns, 3), self.np_dtype)}, COLLISIONS, null_empty=True)
        out = CCollisions(*ptrs)
        self._check(self.lib.wbcqp_check_collisions_host(self._h, slot, B, q.ctypes.data, C.byref(out)))
        return res

    def problem_data(self, slot: int, batch: int, state: Dict[str, "object"], rows: Dict[str, "object"], stream: int = 0):
        """q, v, ref -> M, h, A, b1, Ac, bc, blb, bub on device tensors (wbcqp_problem_data)."""
        cs, cin = self._state(state), self._rows(slot, batch, rows, ROW_FIELDS)
        self._check(self.lib.wbcqp_problem_data(self._h, slot, batch, C.byref(cs), C.byref(cin), C.c_void_p(stream)))

    def _host_rows(self, slot: int, batch: int):
        """(name -> zero-filled [batch, L[name]] array, name -> its pointer) for the rows a _host call writes (ROW_FIELDS); a row the slot's
        structure does not have is an array without columns and a NULL."""
        L = self._lengths[slot]
        rows, ptrs = host_outputs({k: ((batch, L[k]), self.np_dtype) for k in ROW_FIELDS}, ROW_FIELDS, null_empty=True)
        return rows, dict(zip(ROW_FIELDS, ptrs))

    def problem_data_host(self, slot: int, q: np.ndarray, v: np.ndarray, ref: np.ndarray) -> Dict[str, np.ndarray]:
        q, v, ref = self._host(q, v, ref)
        batch = q.shape[0]
        res, ptrs = self._host_rows(slot, batch)
        mom = np.zeros((batch, 6), self.np_dtype)
        cs = CState(q.ctypes.data, v.ctypes.data, ref.ctypes.data, mom.ctypes.data)
        cin = c_inputs(ptrs)
        self._check(self.lib.wbcqp_problem_data_host(self._h, slot, batch, C.byref(cs), C.byref(cin)))
        res["momentum"] = mom  # centroidal momentum Ag v: linear, then angular about the CoM (controller.cpp:245 keeps the last three)
        return res

    def _tick_io(self, slot: int, batch: int, state, rows, out, q_next, v_next, dt: float, q_solver=None) -> CTickIO:
        cin, cout = self._pack(slot, batch, rows, out)
        io = CTickIO()
        io.state = self._state(state, need_ref=True)
        io.rows, io.out = cin, cout
        io.q_next, io.v_next, io.q_solver, io.dt = q_next.data_ptr(), v_next.data_ptr(), dev_ptr(q_solver), float(dt)
        return io

    def tick(self, slot: int, batch: int, state, rows, out, q_next, v_next, dt: float, q_solver=None, stream: int = 0):
        """rows -> QP -> integration for one control tick (wbcqp_tick), device tensors."""
        io = self._tick_io(slot, batch, state, rows, out, q_next, v_next, dt, q_solver)
        self._check(self.lib.wbcqp_tick(self._h, slot, batch, C.byref(io), C.c_void_p(stream)))

    def rollout(self, slot: int, batch: int, n_ticks: int, state, limits, out, q_next, v_next, dt: float, q_solver=None, iters_sum=None,
                ticks_ok=None, stream: int = 0):
        """n_ticks control ticks of every instance in one launch, no batch barrier (wbcqp_rollout).  state: q [B, nq], v [B, nv],
        ref [n_ticks, B, nref] (+ optional momentum [B, 6]); limits: tlb, tub, w; out: x, tau, status, iters of the LAST tick."""
        assert state["ref"].is_contiguous() and state["ref"].shape[0] == n_ticks and state["ref"].shape[1] == batch
        limits["w"]  # (a call without weights is refused here, not in the library)
        self.rollout_traced(slot, batch, n_ticks, state, limits, out, q_next, v_next, dt, None, 1, q_solver, iters_sum, ticks_ok, stream)

    def _mix(self, slots: Sequence[int], w: Sequence, tlb=None, tub=None):
        """wbcqp_mix: slots (one per contact set of one robot model), w[k] = device tensor [B, n_tasks of slots[k]] by instance (or None)."""
        slots_arr = np.ascontiguousarray(slots, dtype=np.int32)
        w_arr = (C.c_void_p * max(len(slots_arr), 1))(*[dev_ptr(t) for t in w])
        mix = CMix(len(slots_arr), slots_arr.ctypes.data_as(c_i32_p), C.cast(w_arr, C.POINTER(C.c_void_p)), dev_ptr(tlb), dev_ptr(tub))
        return mix, (slots_arr, w_arr)  # (the second item keeps the arrays alive for the call)

    @staticmethod
    def _outs(out, names=OUT_FIELDS) -> COutputs:
        """wbcqp_outputs from device tensors; names: the leading fields to take.  One that is missing or not taken is NULL."""
        return COutputs(*[dev_ptr(out.get(k)) for k in names])

    def _state(self, state, need_ref: bool = False) -> CState:
        """wbcqp_state from device tensors q, v (ref, momentum [batch, 6]: an output); need_ref: a state without ref is refused here."""
        return CState(state["q"].data_ptr(), state["v"].data_ptr(), state["ref"].data_ptr() if need_ref else dev_ptr(state.get("ref")),
                      dev_ptr(state.get("momentum")))

    def _rollout_io(self, state, out, q_next, v_next, dt: float, q_solver, iters_sum, ticks_ok, need_ref: bool = False, limits=None) -> CRolloutIO:
        """limits: (slot, dict of tlb, tub, w) for a roll-out of one slot; a mixed one carries them in its wbcqp_mix."""
        io = CRolloutIO()
        if limits is not None:
            slot, lim = limits
            if self._structs[slot].act_bounds:
                io.tlb, io.tub = dev_ptr(lim.get("tlb")), dev_ptr(lim.get("tub"))
            io.w = dev_ptr(lim.get("w"))
        io.state = self._state(state, need_ref)
        io.out = self._outs(out)
        io.q_next, io.v_next, io.q_solver, io.dt = q_next.data_ptr(), v_next.data_ptr(), dev_ptr(q_solver), float(dt)
        io.iters_sum, io.ticks_ok = dev_ptr(iters_sum), dev_ptr(ticks_ok)
        return io

    def tick_mixed(self, slots: Sequence[int], which, state, w: Sequence, out, q_next, v_next, dt: float, tlb=None, tub=None, q_solver=None,
                   stream: int = 0):
        """One tick of B instances of one robot model, instance i in the contact set of slots[which[i]] (wbcqp_tick_mixed).  which: host
        int array [B]; state: q, v, ref [B, nref] (+ momentum [B, 6]) by instance; w[k]: [B, n_tasks of slots[k]] by instance; tlb / tub
        [B, na]; out: x [B, ldx = max n], tau, status, iters (objective, n_active, active_mask) by instance."""
        which = np.ascontiguousarray(which, dtype=np.int32)
        mix, keep = self._mix(slots, w, tlb, tub)
        io = CMixedIO()
        io.state, io.out = self._state(state), self._outs(out)
        io.q_next, io.v_next, io.q_solver, io.dt = q_next.data_ptr(), v_next.data_ptr(), dev_ptr(q_solver), float(dt)
        self._check(self.lib.wbcqp_tick_mixed(self._h, C.byref(mix), int(which.size), which.ctypes.data_as(c_i32_p), C.byref(io),
                                              C.c_void_p(stream)))
        del keep

    def rollout_mixed(self, slots: Sequence[int], schedule, state, w: Sequence, out, q_next, v_next, dt: float, tlb=None, tub=None,
                      q_solver=None, iters_sum=None, ticks_ok=None, stream: int = 0):
        """K ticks of a fleet in mixed contact sets, enqueued up front (wbcqp_rollout_mixed).  schedule: host int array [K, B] of indices
        into slots; state: q [B, nq], v [B, nv], ref [K, B, nref] (+ momentum [B, 6] of the last tick's state); out: the last tick's."""
        self.rollout_mixed_traced(slots, schedule, state, w, out, q_next, v_next, dt, None, 1, tlb, tub, q_solver, iters_sum, ticks_ok, stream)

    def task_costs(self, slot: int, batch: int, rows: Dict[str, "object"], x, tau, cost, stream: int = 0):
        """Per-task costs ||A_t x - b_t|| of a solved record (wbcqp_task_costs), device tensors: rows (A, b1, Acop read) as given to
        solve_batch, x [B, n], tau [B, na] (may be None without a torque task), cost [B, n_tasks] written."""
        cin = c_inputs({k: dev_ptr(rows.get(k)) for k in ("A", "b1", "Acop")})
        self._check(self.lib.wbcqp_task_costs(self._h, slot, batch, C.byref(cin), dev_ptr(x), dev_ptr(tau), dev_ptr(cost),
                                              C.c_void_p(stream)))

    @staticmethod
    def _trace(trace, stride: int):
        """wbcqp_trace from a dict of device tensors (any of TRACE_FIELDS; a missing one is not recorded), or None: no trace."""
        if trace is None:
            return None
        ct = CTrace()
        ct.stride = int(stride)
        for k in TRACE_FIELDS:
            setattr(ct, k, dev_ptr(trace.get(k)))
        return C.byref(ct)

    def rollout_traced(self, slot: int, batch: int, n_ticks: int, state, limits, out, q_next, v_next, dt: float, trace=None, stride: int = 1,
                       q_solver=None, iters_sum=None, ticks_ok=None, stream: int = 0):
        """rollout() that also keeps every stride-th tick's results (wbcqp_rollout_traced).  trace: dict of device tensors, q [n_rec, B, nq],
        v [n_rec, B, nv], x [n_rec, B, n], tau [n_rec, B, na], status / iters [n_rec, B] int32, objective [n_rec, B], cost [n_rec, B, n_tasks]
        (n_rec = n_ticks // stride); a field left out is not recorded; trace=None is rollout()."""
        io = self._rollout_io(state, out, q_next, v_next, dt, q_solver, iters_sum, ticks_ok, need_ref=True, limits=(slot, limits))
        self._check(self.lib.wbcqp_rollout_traced(self._h, slot, batch, n_ticks, C.byref(io), self._trace(trace, stride), C.c_void_p(stream)))

    def rollout_mixed_traced(self, slots: Sequence[int], schedule, state, w: Sequence, out, q_next, v_next, dt: float, trace=None, stride: int = 1,
                             tlb=None, tub=None, q_solver=None, iters_sum=None, ticks_ok=None, stream: int = 0):
        """rollout_mixed() that also keeps every stride-th tick's results (wbcqp_rollout_mixed_traced); trace as for rollout_traced, with
        x [n_rec, B, max n] and cost [n_rec, B, max n_tasks] over the slots (zero past an instance's own slot's n / n_tasks)."""
        schedule = np.ascontiguousarray(schedule, dtype=np.int32)
        K, B = schedule.shape
        mix, keep = self._mix(slots, w, tlb, tub)
        io = self._rollout_io(state, out, q_next, v_next, dt, q_solver, iters_sum, ticks_ok)
        self._check(self.lib.wbcqp_rollout_mixed_traced(self._h, C.byref(mix), int(B), int(K), schedule.ctypes.data_as(c_i32_p), C.byref(io),
                                                        self._trace(trace, stride), C.c_void_p(stream)))
        del keep

    def reference_samples(self, prog, base, offsets, tick0: int, n_ticks: int, out, stream: int = 0):
        """The references of call ticks [0, n_ticks) of a call at tick0, written to the device tensor out [n_ticks, B, nref] by refgen_kernel
        (wbcqp_reference_samples).  prog: a refprog.Program; base: device tensor [B, nref] or [nref]; offsets: host ints [B]."""
        pb = ProgramBuffers(prog, offsets, base)
        B = pb.offsets.size
        assert out.is_contiguous() and out.numel() == n_ticks * B * prog.nref, (tuple(out.shape), n_ticks, B, prog.nref)
        self._check(self.lib.wbcqp_reference_samples(self._h, C.byref(pb.c), B, int(tick0), int(n_ticks), dev_ptr(out), C.c_void_p(stream)))
        return out

    def rollout_program(self, slot: int, batch: int, tick0: int, n_ticks: int, prog, base, offsets, state, limits, out, q_next, v_next, dt: float,
                        trace=None, stride: int = 1, q_solver=None, iters_sum=None, ticks_ok=None, stream: int = 0):
        """rollout_traced() with the references generated on the device from a reference program (wbcqp_rollout_program): state needs q and v
        only; call tick t plays behaviour tick tick0 + t - offsets[i] of instance i."""
        pb = ProgramBuffers(prog, offsets, base)
        assert pb.offsets.size == batch, (pb.offsets.size, batch)
        io = self._rollout_io(dict(state, ref=None), out, q_next, v_next, dt, q_solver, iters_sum, ticks_ok, limits=(slot, limits))
        self._check(self.lib.wbcqp_rollout_program(self._h, slot, batch, int(tick0), n_ticks, C.byref(io), C.byref(pb.c), self._trace(trace, stride),
                                                   C.c_void_p(stream)))

    def rollout_mixed_program(self, slots: Sequence[int], batch: int, tick0: int, n_ticks: int, prog, base, offsets, state, w: Sequence, out, q_next,
                              v_next, dt: float, trace=None, stride: int = 1, tlb=None, tub=None, q_solver=None, iters_sum=None, ticks_ok=None,
                              stream: int = 0):
        """rollout_mixed_traced() by program (wbcqp_rollout_mixed_program): the library makes the schedule from prog.set_of, offsets and tick0."""
        pb = ProgramBuffers(prog, offsets, base)
        assert pb.offsets.size == batch, (pb.offsets.size, batch)
        mix, keep = self._mix(slots, w, tlb, tub)
        io = self._rollout_io(dict(state, ref=None), out, q_next, v_next, dt, q_solver, iters_sum, ticks_ok)
        self._check(self.lib.wbcqp_rollout_mixed_program(self._h, C.byref(mix), batch, int(tick0), n_ticks, C.byref(io), C.byref(pb.c),
                                                         self._trace(trace, stride), C.c_void_p(stream)))
        del keep

    def _host_outs(self, st: Structure, batch: int):
        """(name -> array, wbcqp_outputs of their pointers) for a _host solve: zeros, status -99; the caller cuts tau to [:, :na] after the call."""
        f = self.np_dtype
        out, ptrs = host_outputs({"x": ((batch, st.n), f), "tau": ((batch, max(st.na, 1)), f), "status": ((batch,), np.int32),
                                  "iters": ((batch,), np.int32), "objective": ((batch,), f), "n_active": ((batch,), np.int32),
                                  "active_mask": ((batch, 8), np.uint32)}, OUT_FIELDS)  # (active_mask in/out: zeros = no warm-start hint)
        out["status"][:] = -99
        return out, COutputs(*ptrs)

    def tick_host(self, slot: int, q: np.ndarray, v: np.ndarray, ref: np.ndarray, tlb, tub, w, dt: float, want_rows: bool = False):
        """One whole tick with host arrays (wbcqp_tick_host): returns dict(x, tau, status, iters, objective, n_active, active_mask, q_next, v_next,
        q_solver, momentum[, rows])."""
        st = self._structs[slot]
        q, v, ref, w = self._host(q, v, ref, w)
        B = q.shape[0]
        rows, ptrs = self._host_rows(slot, B) if want_rows else ({}, {})
        if self._lengths[slot]["tlb"]:
            tlb, tub = self._host(tlb, tub)
            ptrs.update(tlb=tlb.ctypes.data, tub=tub.ctypes.data)
        ptrs["w"] = w.ctypes.data
        io = CTickIO()
        out, io.out = self._host_outs(st, B)
        out.update(q_next=np.zeros_like(q), v_next=np.zeros_like(v), q_solver=np.zeros_like(v), momentum=np.zeros((B, 6), self.np_dtype))
        io.state = CState(q.ctypes.data, v.ctypes.data, ref.ctypes.data, out["momentum"].ctypes.data)
        io.rows = c_inputs(ptrs)
        io.q_next, io.v_next, io.q_solver, io.dt = out["q_next"].ctypes.data, out["v_next"].ctypes.data, out["q_solver"].ctypes.data, float(dt)
        self._check(self.lib.wbcqp_tick_host(self._h, slot, B, C.byref(io)))
        out["tau"] = out["tau"][:, :st.na]
        if want_rows:
            out["rows"] = rows
        return out

    def tick_graph(self, slot: int, batch: int, state, rows, out, q_next, v_next, dt: float, q_solver=None) -> int:
        """Captures the tick into a HIP graph bound to these buffers; returns the graph handle for tick_graph_launch."""
        io = self._tick_io(slot, batch, state, rows, out, q_next, v_next, dt, q_solver)
        g = C.c_void_p()
        self._check(self.lib.wbcqp_tick_graph_create(self._h, slot, batch, C.byref(io), C.byref(g)))
        return g.value

    def tick_graph_launch(self, graph: int, stream: int = 0):
        self._check(self.lib.wbcqp_tick_graph_launch(self._h, C.c_void_p(graph), C.c_void_p(stream)))

    def tick_graph_destroy(self, graph: int):
        self.lib.wbcqp_tick_graph_destroy(self._h, C.c_void_p(graph))

    def launch_order(self):
        """(order, packed): the launch order the next solve of the last launch's shape will use; order is None before any"""
        buf = np.zeros(1 << 16, dtype=np.int32)
        packed = C.c_int32(0)
        n = self.lib.wbcqp_launch_order(self._h, buf.ctypes.data_as(c_i32_p), buf.size, C.byref(packed))
        if n < 0:
            self._check(n)
        return (buf[:n].copy() if n else None), bool(packed.value)

    def sync(self, stream: int = 0):
        self._check(self.lib.wbcqp_sync(self._h, C.c_void_p(stream)))

    # ---- host-pointer path ----
    def solve_batch_host(self, slot: int, inputs: Dict[str, np.ndarray], hint=None) -> Dict[str, np.ndarray]:
        """wbcqp_solve_batch_host.  hint: [batch, 8] words (any 32-bit integer type) that fill outputs.active_mask before the call -- under
        FLAG_WARM_START the library reads them as the pick hint (include/wbcqp.h); None: zeros, no hint."""
        st, L = self._structs[slot], self._lengths[slot]
        batch = int(np.asarray(inputs["h"]).reshape(-1, st.nv).shape[0])
        keep = {k: np.ascontiguousarray(inputs[k], dtype=self.np_dtype).reshape(batch, L[k]) for k in FIELDS if L[k]}
        cin = c_inputs({k: a.ctypes.data for k, a in keep.items()})
        out, cout = self._host_outs(st, batch)
        if hint is not None:
            out["active_mask"][:] = np.ascontiguousarray(hint).view(np.uint32).reshape(batch, 8)
        self._check(self.lib.wbcqp_solve_batch_host(self._h, slot, batch, C.byref(cin), C.byref(cout)))
        out["tau"] = out["tau"][:, :st.na]
        return out

    def solve_dense_host(self, H, g, CE, ce0, CI, ci0, max_iter: int = 0):
        """The narrow seam (wbcqp_solve_dense_host): dense QPs in eiquadprog's convention, [B, ...] double arrays.  The
        returned arrays are COPIES of the handle-owned HQPOutput (which is valid until the next call)."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        H, g = f(H), f(g)
        if H.ndim == 2:
            H, g = H[None], g[None]
        B, n = g.shape
        CE = f(CE).reshape(B, -1, n) if CE is not None and np.size(CE) else np.zeros((B, 0, n))
        CI = f(CI).reshape(B, -1, n) if CI is not None and np.size(CI) else np.zeros((B, 0, n))
        neq, nin = CE.shape[1], CI.shape[1]
        ce0 = f(ce0).reshape(B, neq) if neq else np.zeros((B, 0))
        ci0 = f(ci0).reshape(B, nin) if nin else np.zeros((B, 0))
        din = CDenseInputs(*[host_ptr(a if a.size else None) for a in (H, g, CE, ce0, CI, ci0)])
        res = C.POINTER(CDenseOutput)()
        self._check(self.lib.wbcqp_solve_dense_host(self._h, B, n, neq, nin, int(max_iter), C.byref(din), C.byref(res)))
        o = res.contents
        return dict(x=np.ctypeslib.as_array(o.x, shape=(B, n)).copy(), status=np.ctypeslib.as_array(o.status, shape=(B,)).copy(),
                    iters=np.ctypeslib.as_array(o.iters, shape=(B,)).copy(), objective=np.ctypeslib.as_array(o.objective, shape=(B,)).copy(),
                    n_active=np.ctypeslib.as_array(o.n_active, shape=(B,)).copy())

    def solve_dense(self, n: int, neq: int, nin: int, inputs: Dict[str, "object"], outputs: Dict[str, "object"], max_iter: int = 0,
                    stream: int = 0):
        """Device-pointer form of the narrow seam (wbcqp_solve_dense): inputs H, g, CE, ce0, CI, ci0 and outputs x, status, iters
        (objective, n_active optional) are device tensors of the handle's dtype, [batch, ...]."""
        batch = inputs["g"].shape[0]
        din = CDenseInputs(*[dev_ptr(inputs.get(k)) for k in ("H", "g", "CE", "ce0", "CI", "ci0")])
        cout = self._outs(outputs, OUT_FIELDS[:-1])  # (an active_mask among the outputs is not passed on)
        self._check(self.lib.wbcqp_solve_dense(self._h, int(batch), int(n), int(neq), int(nin), int(max_iter), C.byref(din), C.byref(cout),
                                               C.c_void_p(stream)))

    def allgather_tau(self, comm: int, send_ptr: int, recv_ptr: int, count: int, stream: int = 0):
        self._check(self.lib.wbcqp_allgather_tau(self._h, C.c_void_p(comm), C.c_void_p(send_ptr), C.c_void_p(recv_ptr),
                                                 count, C.c_void_p(stream)))
