#!/usr/bin/env python3
"""What it costs to know a fleet's torques: wbcqp_inverse_dynamics (q, v, a and two foot wrenches in, tau out) on B Talos-like robots.

    python tools/inverse_dynamics_bench.py --mode kernels [--batch 8192] [--reps 50]
        launches rnea_kernel, observe_kernel and the rows kernel (wbcqp_problem_data) on the same states, `reps` times each per batch and
        nothing else: the program to put behind `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/inverse_dynamics_bench.py --mode
        kernels`; the three kernels' times then come from that ONE trace (python tools/rocpd_kernel_stats.py <dir>/.../*_results.db --match ...).
        The expectation to confirm or refute: rnea_kernel's time at B = 8192 lies below terms_kernel's.  Prints the algorithmic
        bytes per instance, (nq + 2 nv + 6 n_frames + nv) x 8 B.
    python tools/inverse_dynamics_bench.py --mode trace [--batch 1024] [--ticks 2000] [--stride 10]
        the audit of a traced roll-out: its states and solutions ([n_rec][B][nq], [.][nv], x [.][n], resident in HBM) through inverse dynamics
        (a) on the device in one call over n_rec x B rows with a = x (lda = n), timed by device events, against (b) copying them down and
        running the numpy statement (inria_wbc_amd/dynamics.py) on a sample of the rows, scaled to all of them.  An APPROXIMATION, as
        tools/observe_bench.py says of itself: the states are synthetic (256 drawn by sample_states, tiled; x and the wrenches random -- the
        cost does not depend on how they came about), the host side is numpy on --sample states extrapolated to all (`host_ms_extrapolated`).
Writes profiles/rnea/inverse_dynamics_bench_<mode>.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WRENCH_FRAMES = ["leg_left_6_joint", "leg_right_6_joint"]
OBSERVED = ["leg_left_6_joint", "leg_right_6_joint", "gripper_left_joint", "gripper_right_joint", "base_link", "torso_2_link", "head_2_joint", "arm_left_4_joint"]
HBM_PEAK = 8.0e12  # bytes / s, the data sheet's figure


def _setup():
    from inria_wbc_amd import capi, observe, structure
    from inria_wbc_amd import model as mdl
    m = mdl.talos_like()
    st = structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)
    frames = observe.frame_ids(m, WRENCH_FRAMES)
    h.set_wrench_frames(0, frames)
    h.set_observed_frames(0, observe.frame_ids(m, OBSERVED))
    return h, m, st, tm, frames


def _states(m, tm, st, n, dev, torch, distinct=256):
    """n rows: `distinct` different ones, tiled.  q, v, ref as sample_states draws them; x [n, st.n] (dv first) and wrench [n, 2, 6] random."""
    from inria_wbc_amd import model as mdl
    k = min(n, distinct)
    s = mdl.sample_states(m, tm, k, 9_200_000, q_noise=0.05, v_noise=0.2)
    rng = np.random.default_rng(9_200_001)
    s["x"] = rng.standard_normal((k, st.n))
    s["wrench"] = 100.0 * rng.standard_normal((k, len(WRENCH_FRAMES) * 6))
    rep = -(-n // k)
    return {key: torch.from_numpy(np.ascontiguousarray(np.tile(a, (rep, 1))[:n])).to(dev) for key, a in s.items()}


def kernels(batches, reps):
    import torch
    from inria_wbc_amd import capi, dynamics
    dev = torch.device("cuda", 0)
    h, m, st, tm, frames = _setup()
    sp = torch.cuda.current_stream().cuda_stream
    L = st.field_lengths()
    res = dict(mode="kernels", wrench_frames=WRENCH_FRAMES, reps=reps, rnea_bytes_per_instance=dynamics.algorithmic_bytes(m, len(frames)),
               observe_bytes_per_instance=8 * (m.nq + m.nv + 6 + 18 * len(OBSERVED)), terms_bytes_per_instance=tm.algorithmic_bytes(m, st),
               hbm_peak_bytes_per_s=HBM_PEAK, batches={})
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    for B in batches:
        s = _states(m, tm, st, B, dev, torch)
        tau = f(B, m.nv)
        obs = dict(com=f(B, 3), vcom=f(B, 3), placement=f(B, len(OBSERVED), 12), velocity=f(B, len(OBSERVED), 6))
        rows = {k: f(B, max(L[k], 1)) for k in capi.ROW_FIELDS}
        ev = {}
        for what, call in (("rnea", lambda: h.inverse_dynamics(0, B, s["q"], tau, v=s["v"], a=s["x"], lda=st.n, wrench=s["wrench"], stream=sp)),
                           ("observe", lambda: h.observe(0, B, s["q"], s["v"], stream=sp, **obs)),
                           ("terms", lambda: h.problem_data(0, B, s, rows, stream=sp))):
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            e1.synchronize()
            ev[what + "_us_per_launch_back_to_back"] = 1e3 * e0.elapsed_time(e1) / reps  # (launches in a row: includes the gaps; the trace has the kernel)
        res["batches"][str(B)] = ev
    h.close()
    return res


def trace(batch, ticks, stride, sample):
    import torch
    from inria_wbc_amd import dynamics
    dev = torch.device("cuda", 0)
    h, m, st, tm, frames = _setup()
    sp = torch.cuda.current_stream().cuda_stream
    n_rec = ticks // stride
    n = n_rec * batch
    s = _states(m, tm, st, n, dev, torch)  # [n_rec x B][.]: the layout of wbcqp_trace.q / .v / .x
    tau = torch.zeros(n, m.nv, dtype=torch.float64, device=dev)
    call = lambda: h.inverse_dynamics(0, n, s["q"], tau, v=s["v"], a=s["x"], lda=st.n, wrench=s["wrench"], stream=sp)  # noqa: E731
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    call()
    tau_h = tau.cpu().numpy()
    dev_and_down_ms = 1e3 * (time.perf_counter() - t0)
    # the other way round: everything down, the tree walked on the host, one state at a time
    t0 = time.perf_counter()
    qh, vh, xh, wh = (s[k].cpu().numpy() for k in ("q", "v", "x", "wrench"))
    copy_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = dynamics.inverse_dynamics(m, qh[:sample], vh[:sample], xh[:sample], frames, wh[:sample])
    numpy_ms_per_state = 1e3 * (time.perf_counter() - t0) / sample
    err = float(np.abs(tau_h[:sample] - want).max() / max(1.0, np.abs(want).max()))
    h.close()
    return dict(mode="trace", batch=batch, ticks=ticks, stride=stride, n_rec=n_rec, states=n, wrench_frames=WRENCH_FRAMES,
                device_ms_median=float(np.median(dev_ms)), device_ms_min=float(np.min(dev_ms)), device_and_results_down_ms=dev_and_down_ms,
                states_down_ms=copy_ms, numpy_ms_per_state=numpy_ms_per_state, numpy_states_timed=sample,
                host_ms_extrapolated=copy_ms + numpy_ms_per_state * n, max_rel_difference_on_the_sample=err,
                note="host_ms_extrapolated = the copy down + numpy's time per state on `numpy_states_timed` states x all states (one core)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "trace"), required=True)
    ap.add_argument("--batch", type=int, nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = kernels(a.batch or [8192], a.reps) if a.mode == "kernels" else trace((a.batch or [1024])[0], a.ticks, a.stride, a.sample)
    path = a.out or os.path.join(ROOT, "profiles", "rnea", "inverse_dynamics_bench_%s.json" % a.mode)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
