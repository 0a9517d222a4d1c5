#!/usr/bin/env python3
"""What it costs to watch a fleet's joint torques for collisions: wbcqp_detect_torque_collisions (the reference's 22 Talos joints, a moving
average over 30 samples, max_invalid 5) on B robots over a stream of ticks.

    python tools/torque_monitor_bench.py --mode kernels [--batch 1024] [--ticks 2000] [--reps 10]
        launches torque_monitor_kernel `reps` times per (filter, batch) on [ticks][B][na] arrays and nothing else: the program to put behind
        `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/torque_monitor_bench.py --mode kernels`; the kernel's time comes from that
        trace (python tools/rocpd_kernel_stats.py <dir>/.../*_results.db --match torque_monitor).  The figure to confirm or refute (DESIGN
        4.17): about 300 cycles per tick with the mean filter, 0.25 ms for 2000 ticks of 1024 robots.  Prints the bytes a launch moves.
    python tools/torque_monitor_bench.py --mode trace [--batch 1024] [--ticks 2000]
        a trace's tau ([ticks][B][na], stride 1, resident in HBM) monitored (a) on the device in one call with every output, timed by device
        events, against (b) copying tau down and running the transcription of the reference's detector (inria_wbc_amd/torque_monitor.py) on
        --sample instances, scaled to all of them.  An APPROXIMATION, as tools/observe_bench.py says of itself: the torques are synthetic (a
        smooth stream per joint plus noise, a push on every 16th robot from the middle of the stream -- the cost does not depend on how they
        came about), and the host side is extrapolated from a sample (`host_ms_extrapolated`).
Writes profiles/torque_monitor/torque_monitor_bench_<mode>.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NA = 44  # Talos' actuated joints: a trace's tau is [ticks][B][44]


def _monitor(filt):
    from inria_wbc_amd import model as mdl
    from inria_wbc_amd import torque_monitor as tmon
    names = mdl.talos_like().joint_names[1:]
    return tmon.Monitor(joint=[names.index(j) for j in tmon.TALOS_JOINTS], threshold=tmon.TALOS_THRESHOLDS, filter=filt, window=30, max_invalid=5)


def _streams(ticks, B, mon, torch, dev):
    """model [ticks][B][NA] and sensors [ticks][B][22] on the device: the sensors are the model's monitored columns plus noise, and every 16th
    robot's arm_left_4_joint reads 15 N m more from the middle of the stream on."""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    t = torch.arange(ticks, dtype=torch.float64, device=dev)[:, None, None]
    model = 20.0 * torch.randn(1, B, NA, generator=g, dtype=torch.float64, device=dev) + 3.0 * torch.sin(2e-3 * t)
    sensors = model[:, :, torch.as_tensor(list(mon.joint), device=dev)] + 0.05 * torch.randn(ticks, B, mon.n_joints, generator=g, dtype=torch.float64, device=dev)
    sensors[ticks // 2:, ::16, 17] += 15.0
    return model.contiguous(), sensors.contiguous()


def _outputs(ticks, B, n, torch, dev):
    return dict(detected=torch.zeros(ticks, B, dtype=torch.int32, device=dev), invalid=torch.zeros(ticks, B, dtype=torch.int64, device=dev),
                discrepancy=torch.zeros(ticks, B, n, dtype=torch.float64, device=dev), filtered=torch.zeros(ticks, B, n, dtype=torch.float64, device=dev),
                first_tick=torch.zeros(B, dtype=torch.int32, device=dev), n_detected=torch.zeros(B, dtype=torch.int32, device=dev))


def _timed(call, torch, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def kernels(batches, ticks, reps):
    import torch
    from inria_wbc_amd import capi
    from inria_wbc_amd import torque_monitor as tmon
    dev = torch.device("cuda", 0)
    h = capi.Handle(0, capi.F64)
    sp = torch.cuda.current_stream().cuda_stream
    res = dict(mode="kernels", ticks=ticks, reps=reps, batches={})
    for B in batches:
        per = {}
        for name, filt in (("none", tmon.FILTER_NONE), ("mean", tmon.FILTER_MEAN), ("median", tmon.FILTER_MEDIAN)):
            mon = _monitor(filt)
            model, sensors = _streams(ticks, B, mon, torch, dev)
            flags = {k: v for k, v in _outputs(ticks, B, mon.n_joints, torch, dev).items() if k in ("detected", "invalid", "first_tick", "n_detected")}
            ms = _timed(lambda: h.detect_torque_collisions(mon, B, ticks, model, NA, sensors, stream=sp, **flags), torch, reps)
            per[name] = dict(ms_median_by_events=float(np.median(ms)), ms_min_by_events=float(np.min(ms)),
                             bytes_read=int(ticks * B * mon.n_joints * 16), bytes_written=int(ticks * B * 12 + B * 8),
                             robots_detected=int((flags["first_tick"] >= 0).sum().item()))
        res["batches"][str(B)] = per
    h.close()
    return res


def trace(B, ticks, sample):
    import torch
    from inria_wbc_amd import capi
    from inria_wbc_amd import torque_monitor as tmon
    dev = torch.device("cuda", 0)
    h = capi.Handle(0, capi.F64)
    sp = torch.cuda.current_stream().cuda_stream
    mon = _monitor(tmon.FILTER_MEAN)
    model, sensors = _streams(ticks, B, mon, torch, dev)
    out = _outputs(ticks, B, mon.n_joints, torch, dev)
    dev_ms = _timed(lambda: h.detect_torque_collisions(mon, B, ticks, model, NA, sensors, stream=sp, **out), torch, 10)
    t0 = time.perf_counter()
    h.detect_torque_collisions(mon, B, ticks, model, NA, sensors, stream=sp, detected=out["detected"], invalid=out["invalid"],
                               first_tick=out["first_tick"], n_detected=out["n_detected"])
    got = {k: out[k].cpu().numpy() for k in ("detected", "invalid", "first_tick", "n_detected")}
    dev_and_flags_down_ms = 1e3 * (time.perf_counter() - t0)
    # the other way round: the torques down, the reference's detector on the host
    t0 = time.perf_counter()
    mh, sh = model.cpu().numpy(), sensors.cpu().numpy()
    copy_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = tmon.detect(mon, mh[:, :sample], sh[:, :sample])
    host_ms_per_robot = 1e3 * (time.perf_counter() - t0) / sample
    same = all(np.array_equal(got[k][..., :sample].view(want[k].dtype), want[k]) for k in got)
    h.close()
    return dict(mode="trace", batch=B, ticks=ticks, stride=1, joints=mon.n_joints, window=mon.window, max_invalid=mon.max_invalid,
                device_ms_median=float(np.median(dev_ms)), device_ms_min=float(np.min(dev_ms)), device_and_flags_down_ms=dev_and_flags_down_ms,
                torques_down_ms=copy_ms, transcription_ms_per_robot=host_ms_per_robot, robots_timed_on_the_host=sample,
                host_ms_extrapolated=copy_ms + host_ms_per_robot * B, flags_equal_on_the_sample=bool(same),
                robots_detected=int((got["first_tick"] >= 0).sum()),
                note="host_ms_extrapolated = the copy down + the transcription's time per robot on `robots_timed_on_the_host` robots x all robots "
                     "(numpy, one core, all sampled robots in step)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "trace"), required=True)
    ap.add_argument("--batch", type=int, nargs="+", default=None)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = kernels(a.batch or [64, 1024], a.ticks, a.reps) if a.mode == "kernels" else trace((a.batch or [1024])[0], a.ticks, a.sample)
    path = a.out or os.path.join(ROOT, "profiles", "torque_monitor", "torque_monitor_bench_%s.json" % a.mode)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
