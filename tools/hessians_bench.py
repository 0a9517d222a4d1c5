#!/usr/bin/env python3
"""What it costs to know how a fleet's Jacobians change: wbcqp_kinematic_hessians on B Talos-like robots (default 1024) with 2 and with 8
selected frames, the calls dJ, H and both.

    python tools/hessians_bench.py [--batch 1024] [--reps 200] [--rounds 5] [--no-gpu | --render] [--out DIR]

Device: per call kind, `rounds` windows of `reps` launches in a row between two events after a warm-up of the same shape; microseconds per
launch (back to back: includes the launch gaps), the median window and the spread of the windows.  Beside it the algorithmic bytes of the call
(hessians.algorithmic_bytes: q, and v where dJ is asked for, in; the outputs out -- 120 KB per frame and Talos robot for H) and what share of the
8 TB/s HBM peak that traffic over the measured time is, a whole-call rate.  The kernel is a store stream: that share is the figure to read.
The two store shapes of H (one k per lane; two consecutive k per lane in one store of twice the width) are two instantiations of the kernel,
timed side by side on two handles: a handle created with WBCQP_HESSIAN_STORE=wide in the environment launches the wide one, "narrow" is a
handle of the library left to itself.  All calls and shapes of one number of frames take their windows in turn inside one loop, so the rows of
a block can be compared with each other; a launch stores up to a GB and the card's clocks move with the load, so a row is NOT comparable with
a run in which it was measured alone.  Kernel resources: read from the built library's code object (tools/kernel_regs.py).  Reported, not gated: no timing bar is set.
--no-gpu: everything but the timings (they are written as "not measured").
Writes profiles/hessians/hessians_bench.json and profiles/hessians/INDEX.md; the accuracy section of INDEX.md is the text of
profiles/hessians/accuracy.md (the figures tests/test_hessians_host.py and tests/test_gpu_hessians.py print), kept beside it."""
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
OUT = os.path.join(ROOT, "profiles", "hessians")
CALLS = (("dJ", ("dJ",)), ("H", ("H",)), ("H + dJ", ("H", "dJ")))
SHAPES = ("narrow", "wide")  # WBCQP_HESSIAN_STORE
ENV = "WBCQP_HESSIAN_STORE"


def resources():
    from tools import kernel_regs
    lib = os.path.join(ROOT, "inria_wbc_amd", "lib", "libwbcqp.so")
    return [dict(kernel=n.split("(")[0].replace("void wbcqp::", ""), vgprs=v, agprs=a, scratch=s, lds=g) for v, a, s, g, n in kernel_regs.kernels(lib)
            if "hessian_kernel" in n]


def bench(B, reps, rounds, gpu):
    from inria_wbc_amd import hessians as hs
    from inria_wbc_amd import model as mdl
    from inria_wbc_amd import observe, structure
    m = mdl.talos_like()
    res = dict(batch=B, reps=reps, rounds=rounds, model=m.name, nv=m.nv, frames=FRAMES, hbm_peak_bytes_per_s=HBM_PEAK, kernel=resources(), calls=[])
    for nf in (2, 8):
        for what, which in CALLS:
            res["calls"].append(dict(call=what, n_frames=nf, outputs=list(which), reference_frame="LOCAL",
                                     bytes_per_instance=hs.algorithmic_bytes(m, nf, which), shapes={}))
    if not gpu:
        return res
    import torch
    from inria_wbc_amd import capi
    dev = torch.device("cuda", 0)
    st = structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    before = os.environ.get(ENV)
    handles = {}
    try:
        for sh in SHAPES:  # (the library reads the variable once, when a handle is created)
            os.environ.pop(ENV, None) if sh == "narrow" else os.environ.__setitem__(ENV, sh)
            handles[sh] = capi.Handle(0, capi.F64)
    finally:
        os.environ.pop(ENV, None) if before is None else os.environ.__setitem__(ENV, before)
    handles["default"] = handles["narrow"]
    for h in handles.values():
        h.set_structure(0, st)
        h.set_model(0, m, tm)
    k = min(B, 256)
    s = mdl.sample_states(m, tm, k, 9_500_000, q_noise=0.05, v_noise=0.2)
    rep = -(-B // k)
    q, v = (torch.from_numpy(np.ascontiguousarray(np.tile(s[key], (rep, 1))[:B])).to(dev) for key in ("q", "v"))
    sp = torch.cuda.current_stream().cuda_stream
    shape = lambda key, nf: {"H": (B, nf, 6, m.nv, m.nv), "dJ": (B, nf, 6, m.nv)}[key]  # noqa: E731
    try:
        for nf in (2, 8):
            # every (call, store shape) of this number of frames takes its windows in turn inside one loop: a GB of stores per launch moves the
            # card's clocks within seconds, and whatever drifts over the run drifts under all of them alike
            mine = [c for c in res["calls"] if c["n_frames"] == nf]
            for h in handles.values():
                h.set_jacobian_frames(0, observe.frame_ids(m, FRAMES[:nf]))
            out = {key: torch.zeros(*shape(key, nf), dtype=torch.float64, device=dev) for key in ("H", "dJ")}
            variants = [(c, sh) for c in mine for sh in (SHAPES if "H" in c["outputs"] else ("default",))]  # (dJ's stores have one shape)

            def call(c, sh):
                handles[sh].kinematic_hessians(0, B, q, v if "dJ" in c["outputs"] else None, capi.RF_LOCAL, stream=sp, **{key: out[key] for key in c["outputs"]})

            windows = {(c["call"], sh): [] for c, sh in variants}
            for c, sh in variants:  # the warm-up: the shapes that are timed
                for _ in range(reps):
                    call(c, sh)
            torch.cuda.synchronize()
            for _ in range(rounds):
                for c, sh in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        call(c, sh)
                    e1.record()
                    e1.synchronize()
                    windows[(c["call"], sh)].append(1e3 * e0.elapsed_time(e1) / reps)
            assert all(bool(torch.isfinite(t).all().item()) for t in out.values())
            for c, sh in variants:
                w = windows[(c["call"], sh)]
                med = statistics.median(w)
                c["shapes"][sh] = dict(us_windows=w, us_per_launch=med, share_of_hbm_peak=c["bytes_per_instance"] * B / (med * 1e-6) / HBM_PEAK)
            del out
    finally:
        for sh in SHAPES:
            handles[sh].close()
    return res


def index_md(res):
    B = res["batch"]
    lines = ["# profiles/hessians — `wbcqp_kinematic_hessians`", "",
             "**Kernel resources** (the built library's code object, `python tools/kernel_regs.py`; cross-compiled for gfx950):", "",
             "| kernel | VGPRs | AGPRs | scratch B/lane | LDS B/workgroup |", "| --- | --- | --- | --- | --- |"]
    lines += ["| `%(kernel)s` | %(vgprs)d | %(agprs)d | %(scratch)d | %(lds)d |" % k for k in res["kernel"]]
    lines += ["", "No LDS and no barrier: a wave keeps everything in registers; column j of a frame is broadcast from its lane into scalar registers "
              "and a row `H[f][r][j][0 .. nv)` is one contiguous store across the wave. `build.check_resources` refuses `hessian_kernel` with any "
              "AGPR, scratch or spill. `<TI, false>` is the narrow store shape, what every call gets; `<TI, true>` the wide one. `jacobian_kernel` is "
              "untouched: 122 VGPRs, 0 AGPRs, 0 scratch as before.", "",
             "**Timings** (`python tools/hessians_bench.py`, `hessians_bench.json`: %d Talos-like instances (nv = %d), F64, LOCAL, %d windows of %d "
             "launches in a row between two events after a warm-up of the same shape; microseconds per launch including the launch gaps, median "
             "window and the windows' range; bytes: `hessians.algorithmic_bytes`; share of peak: those bytes over the median time against 8 TB/s of "
             "HBM -- a whole-call rate, not the kernel's alone). All rows of one number of frames take their windows in turn inside one loop. H's two store shapes: "
             "*narrow* is one k per lane (8-byte stores in F64), *wide* two consecutive k per lane (16-byte stores), each on a handle of its own:" % (B, res["nv"], res["rounds"], res["reps"]),
             "", "| call | frames | store shape | bytes per instance | bytes per launch | µs per launch (range) | share of the HBM peak |",
             "| --- | --- | --- | --- | --- | --- | --- |"]
    for c in res["calls"]:
        rows = c["shapes"] or {"-": None}
        for sh, r in rows.items():
            if r is None:
                t, share = "not measured", "not measured"
            else:
                t = "%.1f (%.1f .. %.1f)" % (r["us_per_launch"], min(r["us_windows"]), max(r["us_windows"]))
                share = "%.1f %%" % (100.0 * r["share_of_hbm_peak"])
            lines.append("| %s | %d | %s | %d | %d | %s | %s |" % (c["call"], c["n_frames"], sh, c["bytes_per_instance"], c["bytes_per_instance"] * B, t, share))
    note = os.path.join(OUT, "store_shapes.md")
    lines += ["", "**The store shape kept**", ""]
    lines += [open(note).read().rstrip()] if os.path.exists(note) else ["not measured"]
    lines += ["", "Reported, not gated: nothing exists at the parent commit to compare against and the issue sets no timing bar. Not measured: the "
              "kernel alone in a `rocprofv3 --kernel-trace` run (the figures above include the gaps between launches), other batch sizes, the "
              "other two conventions, an F32 handle.", ""]
    acc = os.path.join(OUT, "accuracy.md")
    lines += ["**Accuracy**", ""]
    lines += [open(acc).read().rstrip()] if os.path.exists(acc) else ["not measured"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--render", action="store_true", help="write INDEX.md again from the hessians_bench.json in --out; nothing is run")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.render:
        with open(os.path.join(args.out, "hessians_bench.json")) as fh:
            r = json.load(fh)
    else:
        r = bench(args.batch, args.reps, args.rounds, not args.no_gpu)
        with open(os.path.join(args.out, "hessians_bench.json"), "w") as fh:
            json.dump(r, fh, indent=1)
    with open(os.path.join(args.out, "INDEX.md"), "w") as fh:
        fh.write(index_md(r))
    print(json.dumps(r))
