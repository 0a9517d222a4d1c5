#!/usr/bin/env python3
"""What it costs to know where a fleet is: wbcqp_observe (CoM, its velocity, 8 frames' placements and velocities) on B Talos-like robots.

    python tools/observe_bench.py --mode kernels [--batch 1024 8192] [--reps 50]
        launches observe_kernel and the rows kernel (wbcqp_problem_data) on the same states, `reps` times each per batch and nothing else:
        the program to put behind `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/observe_bench.py --mode kernels`; the two
        kernels' times then come from that ONE trace (python tools/rocpd_kernel_stats.py <dir>/.../*_results.db --match ...).  Prints the
        algorithmic bytes per instance, (nq + nv + 6 + 18 n_frames) x 8 B, so that the share of the HBM roofline follows from the trace.
    python tools/observe_bench.py --mode roofline --batch 8192 --kernel-us <observe_kernel's mean time in that trace>
        the share of the HBM roofline: algorithmic bytes x batch over the data sheet's 8 TB/s, over the traced kernel time (no GPU needed).
    python tools/observe_bench.py --mode trace [--batch 1024] [--ticks 2000] [--stride 10]
        a traced roll-out's states ([n_rec][B][nq], [n_rec][B][nv], resident in HBM) observed (a) on the device in one call over
        n_rec x B rows, timed by device events, against (b) copying q and v down and running the numpy statement (inria_wbc_amd/observe.py)
        on a sample of the rows, scaled to all of them.  An APPROXIMATION of "a traced roll-out against the host": the states are synthetic
        (256 drawn by sample_states, tiled -- the observables' cost does not depend on how the states came about), the host side is numpy on
        --sample states extrapolated to all (`host_ms_extrapolated`), and the C++ RobotWrapper is not timed.
Writes profiles/observe/observe_bench_<mode>.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = ["leg_left_6_joint", "leg_right_6_joint", "gripper_left_joint", "gripper_right_joint", "base_link", "torso_2_link", "head_2_joint", "arm_left_4_joint"]
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
    frames = observe.frame_ids(m, FRAMES)
    h.set_observed_frames(0, frames)
    return h, m, st, tm, frames


def _states(m, tm, n, dev, torch, distinct=256):
    """n states: `distinct` different ones, tiled (drawing a million states on the host would take longer than everything measured)."""
    from inria_wbc_amd import model as mdl
    s = mdl.sample_states(m, tm, min(n, distinct), 9_100_000, q_noise=0.05, v_noise=0.2)
    rep = -(-n // s["q"].shape[0])
    return {k: torch.from_numpy(np.ascontiguousarray(np.tile(a, (rep, 1))[:n])).to(dev) for k, a in s.items()}


def _outs(n, nf, dev, torch):
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    return dict(com=f(n, 3), vcom=f(n, 3), placement=f(n, nf, 12), velocity=f(n, nf, 6))


def kernels(batches, reps):
    import torch
    from inria_wbc_amd import capi
    dev = torch.device("cuda", 0)
    h, m, st, tm, frames = _setup()
    sp = torch.cuda.current_stream().cuda_stream
    L = st.field_lengths()
    res = dict(mode="kernels", frames=FRAMES, reps=reps, observe_bytes_per_instance=8 * (m.nq + m.nv + 6 + 18 * len(frames)),
               terms_bytes_per_instance=tm.algorithmic_bytes(m, st), hbm_peak_bytes_per_s=HBM_PEAK, batches={})
    for B in batches:
        s = _states(m, tm, B, dev, torch)
        out = _outs(B, len(frames), dev, torch)
        rows = {k: torch.zeros(B, max(L[k], 1), dtype=torch.float64, device=dev) for k in capi.ROW_FIELDS}
        ev = {}
        for what, call in (("observe", lambda: h.observe(0, B, s["q"], s["v"], stream=sp, **out)), ("terms", lambda: h.problem_data(0, B, s, rows, stream=sp))):
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


def roofline(batch, kernel_us, n_frames=len(FRAMES)):
    """Share of the HBM roofline of one observe_kernel launch on Talos-like robots: the least time the bytes could take over the time they took."""
    from inria_wbc_amd import model as mdl
    m = mdl.talos_like()
    per = 8 * (m.nq + m.nv + 6 + 18 * n_frames)
    least_us = 1e6 * per * batch / HBM_PEAK
    return dict(mode="roofline", batch=batch, n_frames=n_frames, bytes_per_instance=per, bytes=per * batch, hbm_peak_bytes_per_s=HBM_PEAK,
                least_us=least_us, kernel_us=kernel_us, share_of_hbm_roofline=least_us / kernel_us, achieved_bytes_per_s=per * batch / (1e-6 * kernel_us))


def trace(batch, ticks, stride, sample):
    import torch
    from inria_wbc_amd import observe
    dev = torch.device("cuda", 0)
    h, m, st, tm, frames = _setup()
    sp = torch.cuda.current_stream().cuda_stream
    n_rec = ticks // stride
    n = n_rec * batch
    s = _states(m, tm, n, dev, torch)  # [n_rec x B][nq], [n_rec x B][nv]: the layout of wbcqp_trace.q / .v
    out = _outs(n, len(frames), dev, torch)
    for _ in range(3):
        h.observe(0, n, s["q"], s["v"], stream=sp, **out)
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.observe(0, n, s["q"], s["v"], stream=sp, **out)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    # the same with the results brought to the host (what a logger pays)
    t0 = time.perf_counter()
    h.observe(0, n, s["q"], s["v"], stream=sp, **out)
    host_out = {k: v.cpu() for k, v in out.items()}
    dev_and_down_ms = 1e3 * (time.perf_counter() - t0)
    # the other way round: the states down, the tree walked on the host, one state at a time
    t0 = time.perf_counter()
    qh, vh = s["q"].cpu().numpy(), s["v"].cpu().numpy()
    copy_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = observe.observe(m, qh[:sample], vh[:sample], frames)
    numpy_ms_per_state = 1e3 * (time.perf_counter() - t0) / sample
    err = {k: float(np.abs(host_out[k].numpy()[:sample] - want[k]).max()) for k in want}
    h.close()
    return dict(mode="trace", batch=batch, ticks=ticks, stride=stride, n_rec=n_rec, states=n, frames=FRAMES, device_ms_median=float(np.median(dev_ms)),
                device_ms_min=float(np.min(dev_ms)), device_and_results_down_ms=dev_and_down_ms, states_down_ms=copy_ms, numpy_ms_per_state=numpy_ms_per_state,
                numpy_states_timed=sample, host_ms_extrapolated=copy_ms + numpy_ms_per_state * n, max_abs_difference_on_the_sample=err,
                note="host_ms_extrapolated = the copy down + numpy's time per state on `numpy_states_timed` states x all states (one core)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "trace", "roofline"), required=True)
    ap.add_argument("--batch", type=int, nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--kernel-us", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "roofline":
        print(json.dumps(roofline((a.batch or [8192])[0], a.kernel_us)))
        sys.exit(0)
    r = kernels(a.batch or [1024, 8192], a.reps) if a.mode == "kernels" else trace((a.batch or [1024])[0], a.ticks, a.stride, a.sample)
    path = a.out or os.path.join(ROOT, "profiles", "observe", "observe_bench_%s.json" % a.mode)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
