#!/usr/bin/env python3
"""What it costs to know where a fleet's frames move: wbcqp_jacobians on B Talos-like robots (default 1024) with 2 and with 8 selected frames.

    python tools/jacobians_bench.py [--batch 1024] [--reps 200] [--rounds 5] [--no-gpu | --render] [--out DIR]

Device: per call kind, `rounds` windows of `reps` launches in a row between two events after a warm-up of the same shape; microseconds per
launch (back to back: includes the launch gaps), the median window and the spread of the windows.  Beside it the algorithmic bytes of the call
(jacobians.algorithmic_bytes: q, and v where a drift term is asked for, in; the outputs out -- about 23 KB per Talos robot with 8 frames) and
what share of the 8 TB/s HBM peak that traffic over the measured time is.  The kernel is a store stream: that share is the figure to read.
Kernel resources: read from the built library's code object (tools/kernel_regs.py).  Reported, not gated: no timing bar is set.
--no-gpu: everything but the timings (they are written as "not measured").
Writes profiles/jacobians/jacobians_bench.json and profiles/jacobians/INDEX.md; the accuracy section of INDEX.md is the text of
profiles/jacobians/accuracy.md (the figures tests/test_gpu_jacobians.py prints), kept beside it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = ["leg_left_6_joint", "leg_right_6_joint", "gripper_left_joint", "gripper_right_joint", "base_link", "head_2_joint", "arm_left_4_joint",
          "arm_right_4_joint"]
HBM_PEAK = 8.0e12  # bytes per second (MI355X)
OUT = os.path.join(ROOT, "profiles", "jacobians")
CALLS = (("J", ("J",), True), ("J", ("J",), False), ("Jcom + Ag", ("Jcom", "Ag"), True), ("every output", ("J", "Jcom", "Ag", "drift", "dAgv"), True))


def resources():
    from tools import kernel_regs
    lib = os.path.join(ROOT, "inria_wbc_amd", "lib", "libwbcqp.so")
    return [dict(kernel=n.split("(")[0].replace("void wbcqp::", ""), vgprs=v, agprs=a, scratch=s, lds=g) for v, a, s, g, n in kernel_regs.kernels(lib)
            if "jacobian_kernel" in n]


def bench(B, reps, rounds, gpu):
    from inria_wbc_amd import jacobians as jac
    from inria_wbc_amd import model as mdl
    from inria_wbc_amd import observe, structure
    m = mdl.talos_like()
    res = dict(batch=B, reps=reps, rounds=rounds, model=m.name, nv=m.nv, frames=FRAMES, hbm_peak_bytes_per_s=HBM_PEAK, kernel=resources(), calls=[])
    for nf in (2, 8):
        for what, which, local in CALLS:
            which = tuple(k for k in which)
            res["calls"].append(dict(call=what, n_frames=nf, outputs=list(which), reference_frame="LOCAL" if local else "WORLD",
                                     bytes_per_instance=jac.algorithmic_bytes(m, nf, which), us_per_launch=None, us_windows=None, share_of_hbm_peak=None))
    if not gpu:
        return res
    import torch
    from inria_wbc_amd import capi
    dev = torch.device("cuda", 0)
    st = structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)
    k = min(B, 256)
    s = mdl.sample_states(m, tm, k, 9_400_000, q_noise=0.05, v_noise=0.2)
    rep = -(-B // k)
    q, v = (torch.from_numpy(np.ascontiguousarray(np.tile(s[key], (rep, 1))[:B])).to(dev) for key in ("q", "v"))
    sp = torch.cuda.current_stream().cuda_stream
    shape = lambda key, nf: {"J": (B, nf, 6, m.nv), "Jcom": (B, 3, m.nv), "Ag": (B, 6, m.nv), "drift": (B, nf, 6), "dAgv": (B, 6)}[key]  # noqa: E731
    for c in res["calls"]:
        nf = c["n_frames"]
        h.set_jacobian_frames(0, observe.frame_ids(m, FRAMES[:nf]))
        out = {key: torch.zeros(*shape(key, nf), dtype=torch.float64, device=dev) for key in c["outputs"]}
        rf = capi.RF_LOCAL if c["reference_frame"] == "LOCAL" else capi.RF_WORLD
        need_v = "drift" in out or "dAgv" in out
        call = lambda: h.jacobians(0, B, q, v if need_v else None, rf, stream=sp, **out)  # noqa: E731
        for _ in range(reps):  # the warm-up: the shape that is timed
            call()
        torch.cuda.synchronize()
        windows = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            e1.synchronize()
            windows.append(1e3 * e0.elapsed_time(e1) / reps)
        assert all(bool(torch.isfinite(t).all().item()) for t in out.values())
        c["us_windows"] = windows
        c["us_per_launch"] = statistics.median(windows)
        c["share_of_hbm_peak"] = c["bytes_per_instance"] * B / (c["us_per_launch"] * 1e-6) / HBM_PEAK
    h.close()
    return res


def index_md(res):
    B = res["batch"]
    lines = ["# profiles/jacobians — `wbcqp_jacobians`", "",
             "**Kernel resources** (the built library's code object, `python tools/kernel_regs.py`; cross-compiled for gfx950):", "",
             "| kernel | VGPRs | AGPRs | scratch B/lane | LDS B/workgroup |", "| --- | --- | --- | --- | --- |"]
    lines += ["| `%(kernel)s` | %(vgprs)d | %(agprs)d | %(scratch)d | %(lds)d |" % k for k in res["kernel"]]
    lines += ["", "No LDS and no barrier: a wave keeps everything in registers and lane j stores column j as it is formed. "
              "`build.check_resources` refuses `jacobian_kernel` with any AGPR, scratch or spill.", "",
              "**Timings** (`python tools/jacobians_bench.py`, `jacobians_bench.json`: %d Talos-like instances, F64, %d windows of %d launches in a row "
              "between two events after a warm-up of the same shape; microseconds per launch including the launch gaps, median window and the "
              "windows' range; bytes: `jacobians.algorithmic_bytes`; share of peak: those bytes over the median time against 8 TB/s of HBM -- "
              "a whole-call rate, not the kernel's alone):" % (B, res["rounds"], res["reps"]), "",
              "| call | frames | bytes per instance | bytes per launch | µs per launch (range) | share of the HBM peak |", "| --- | --- | --- | --- | --- | --- |"]
    for c in res["calls"]:
        if c["us_per_launch"] is None:
            t, share = "not measured", "not measured"
        else:
            t = "%.1f (%.1f .. %.1f)" % (c["us_per_launch"], min(c["us_windows"]), max(c["us_windows"]))
            share = "%.1f %%" % (100.0 * c["share_of_hbm_peak"])
        lines.append("| %s, %s | %d | %d | %d | %s | %s |" % (c["call"], c["reference_frame"], c["n_frames"], c["bytes_per_instance"], c["bytes_per_instance"] * B, t, share))
    lines += ["", "Reported, not gated: nothing exists at the parent commit to compare against and the issue sets no timing bar. Not measured: the "
              "kernel alone in a `rocprofv3 --kernel-trace` run (the figures above include the gaps between launches), other batch sizes, an F32 handle.", ""]
    acc = os.path.join(OUT, "accuracy.md")
    lines += ["**Accuracy** (relative to max(1, the reference array's largest entry); the bar everywhere is 1e-10)", ""]
    lines += [open(acc).read().rstrip()] if os.path.exists(acc) else ["not measured"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--render", action="store_true", help="write INDEX.md again from the jacobians_bench.json in --out; nothing is run")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.render:
        with open(os.path.join(args.out, "jacobians_bench.json")) as fh:
            r = json.load(fh)
    else:
        r = bench(args.batch, args.reps, args.rounds, not args.no_gpu)
        with open(os.path.join(args.out, "jacobians_bench.json"), "w") as fh:
            json.dump(r, fh, indent=1)
    with open(os.path.join(args.out, "INDEX.md"), "w") as fh:
        fh.write(index_md(r))
    print(json.dumps(r))
