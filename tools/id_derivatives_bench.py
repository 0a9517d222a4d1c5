#!/usr/bin/env python3
"""What the linearisation of a fleet's inverse dynamics costs: wbcqp_inverse_dynamics_derivatives on B Talos-like robots (default 1024) with two
foot wrenches -- both outputs, dtau_dq alone, dtau_dv alone.

    python tools/id_derivatives_bench.py [--batch 1024] [--reps 200] [--rounds 5] [--no-gpu | --render] [--out DIR]

Device: per call, `rounds` windows of `reps` launches in a row between two events after a warm-up of the same shape; microseconds per launch
(back to back: includes the launch gaps), the median window and the windows' range.  In the same loop, so that the rows can be compared:
wbcqp_inverse_dynamics (rnea_kernel alone) on the same states, wbcqp_mass_matrix and wbcqp_forward_dynamics (fdyn_kernel; the latter behind
rnea_kernel), and what the call replaces -- central differences of wbcqp_inverse_dynamics: 4 nv launches (2 nv for each matrix) on perturbed
copies of the state, timed as 4 nv launches in a row and reported as one row.  Beside each the algorithmic bytes of the call and what share of the
8 TB/s HBM peak that traffic over the measured time is, a whole-call rate.  Kernel resources: read from the built library's code object
(tools/kernel_regs.py).  Reported, not gated: no timing bar is set.  --no-gpu: everything but the timings ("not measured").
Writes id_derivatives_bench.json and INDEX.md into --out (default profiles/idderiv); the accuracy section of INDEX.md is the text of accuracy.md
beside it (the figures tests/test_id_derivatives_host.py and tests/test_gpu_id_derivatives.py print)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = ["leg_left_6_joint", "leg_right_6_joint"]
HBM_PEAK = 8.0e12  # bytes per second (MI355X)
OUT = os.path.join(ROOT, "profiles", "idderiv")
CALLS = (("dtau_dq + dtau_dv", ("dtau_dq", "dtau_dv")), ("dtau_dq", ("dtau_dq",)), ("dtau_dv", ("dtau_dv",)))


def resources():
    from tools import kernel_regs
    lib = os.path.join(ROOT, "inria_wbc_amd", "lib", "libwbcqp.so")
    return [dict(kernel=n.split("(")[0].replace("void wbcqp::", ""), vgprs=v, agprs=a, scratch=s, lds=g) for v, a, s, g, n in kernel_regs.kernels(lib)
            if "id_derivatives_kernel" in n or "rnea_kernel" in n or "fdyn_kernel" in n]


def bench(B, reps, rounds, gpu):
    from inria_wbc_amd import dynamics, forward_dynamics
    from inria_wbc_amd import id_derivatives as idd
    from inria_wbc_amd import model as mdl
    from inria_wbc_amd import observe, structure
    m = mdl.talos_like()
    nv = m.nv
    res = dict(batch=B, reps=reps, rounds=rounds, model=m.name, nv=nv, frames=FRAMES, hbm_peak_bytes_per_s=HBM_PEAK, kernel=resources(), calls=[])
    for what, which in CALLS:
        res["calls"].append(dict(call="wbcqp_inverse_dynamics_derivatives: " + what, launches=1, bytes_per_instance=idd.algorithmic_bytes(m, 2, which)))
    res["calls"].append(dict(call="wbcqp_inverse_dynamics (rnea_kernel alone)", launches=1, bytes_per_instance=dynamics.algorithmic_bytes(m, 2)))
    res["calls"].append(dict(call="wbcqp_mass_matrix (fdyn_kernel, phase 1)", launches=1,
                             bytes_per_instance=forward_dynamics.algorithmic_bytes(m, "mass_matrix")))
    res["calls"].append(dict(call="wbcqp_forward_dynamics (rnea_kernel + fdyn_kernel)", launches=2,
                             bytes_per_instance=forward_dynamics.algorithmic_bytes(m, "forward_dynamics", 2)))
    res["calls"].append(dict(call="what the call replaces: %d launches of wbcqp_inverse_dynamics on perturbed states" % (4 * nv), launches=4 * nv,
                             bytes_per_instance=4 * nv * dynamics.algorithmic_bytes(m, 2)))
    if not gpu:
        return res
    import torch
    from inria_wbc_amd import capi
    dev = torch.device("cuda", 0)
    st = structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        h.set_wrench_frames(0, observe.frame_ids(m, FRAMES))
        k = min(B, 256)
        s = mdl.sample_states(m, tm, k, 9_600_000, q_noise=0.05, v_noise=0.2)
        rep = -(-B // k)
        rng = np.random.default_rng(9_600_001)
        up = lambda t: torch.from_numpy(np.ascontiguousarray(np.tile(t, (rep,) + (1,) * (t.ndim - 1))[:B])).to(dev)  # noqa: E731
        q, v, a, w = up(s["q"]), up(s["v"]), up(rng.standard_normal((k, nv))), up(300.0 * rng.standard_normal((k, 2, 6)))
        out = {key: torch.zeros(B, nv, nv, dtype=torch.float64, device=dev) for key in ("dtau_dq", "dtau_dv", "M")}
        tau, acc = (torch.zeros(B, nv, dtype=torch.float64, device=dev) for _ in range(2))
        info = torch.zeros(B, dtype=torch.int32, device=dev)
        sp = torch.cuda.current_stream().cuda_stream

        def rnea():
            h.inverse_dynamics(0, B, q, tau, v=v, a=a, wrench=w, stream=sp)

        def replaced():
            for _ in range(4 * nv):
                rnea()

        fns = [lambda which=which: h.inverse_dynamics_derivatives(0, B, q, v=v, a=a, wrench=w, stream=sp, **{key: out[key] for key in which})
               for _, which in CALLS]
        fns += [rnea, lambda: h.mass_matrix(0, B, q, out["M"], stream=sp),
                lambda: h.forward_dynamics(0, B, q, acc, v=v, tau=a, wrench=w, info=info, stream=sp), replaced]
        windows = [[] for _ in fns]
        for f, c in zip(fns, res["calls"]):  # the warm-up: the shapes that are timed
            for _ in range(max(1, reps // c["launches"])):
                f()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for i, (f, c) in enumerate(zip(fns, res["calls"])):
                n = max(1, reps // c["launches"])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    f()
                e1.record()
                e1.synchronize()
                windows[i].append(1e3 * e0.elapsed_time(e1) / n)
        assert all(bool(torch.isfinite(t).all().item()) for t in list(out.values()) + [tau, acc])
        for c, wnd in zip(res["calls"], windows):
            med = statistics.median(wnd)
            c.update(us_windows=wnd, us_per_call=med, share_of_hbm_peak=c["bytes_per_instance"] * B / (med * 1e-6) / HBM_PEAK)
    finally:
        h.close()
    return res


def index_md(res, out_dir):
    B = res["batch"]
    lines = ["# profiles/idderiv — `wbcqp_inverse_dynamics_derivatives`", "",
             "**Kernel resources** (the built library's code object, `python tools/kernel_regs.py`; cross-compiled for gfx950):", "",
             "| kernel | VGPRs | AGPRs | scratch B/lane | LDS B/workgroup |", "| --- | --- | --- | --- | --- |"]
    lines += ["| `%(kernel)s` | %(vgprs)d | %(agprs)d | %(scratch)d | %(lds)d |" % k for k in res["kernel"]]
    lines += ["", "`id_derivatives_kernel` uses no LDS and no barrier: a wave keeps everything in registers, the 28 composite numbers of a body are "
              "folded leaf to root over `readlane` broadcasts, row i's `S_i`, `P_i`, `E_i` are broadcast into scalar registers and a row of either "
              "matrix is one contiguous store across the wave. The row loop did not need to be split from the sweeps by an LDS image. "
              "`build.check_resources` refuses the kernel with any AGPR, scratch or spill. `rnea_kernel` and `fdyn_kernel` are untouched "
              "(`device_asm_vs_parent.txt`: only the two new instantiations differ from the parent commit).", "",
             "**Timings** (`python tools/id_derivatives_bench.py`, `id_derivatives_bench.json`: %d Talos-like instances (nv = %d), F64, two foot "
             "wrenches, %d windows of about %d launches in a row between two events after a warm-up of the same shape; microseconds per call "
             "including the launch gaps, median window and the windows' range; bytes: the modules' `algorithmic_bytes`; share of peak: those bytes "
             "over the median time against 8 TB/s of HBM, a whole-call rate). All rows take their windows in turn inside one loop:" %
             (B, res["nv"], res["rounds"], res["reps"]), "",
             "| call | launches | bytes per instance | µs per call (range) | share of the HBM peak |", "| --- | --- | --- | --- | --- |"]
    for c in res["calls"]:
        if "us_per_call" in c:
            t = "%.1f (%.1f .. %.1f)" % (c["us_per_call"], min(c["us_windows"]), max(c["us_windows"]))
            share = "%.1f %%" % (100.0 * c["share_of_hbm_peak"])
        else:
            t = share = "not measured"
        lines.append("| %s | %d | %d | %s | %s |" % (c["call"], c["launches"], c["bytes_per_instance"], t, share))
    lines += ["", "The stores are 2 nv^2 8 B = 40 KB per Talos robot, 41 MB per 1024. Reported, not gated: nothing exists at the parent commit to "
              "compare against and no timing bar is set. Not measured: the kernel alone in a `rocprofv3 --kernel-trace` run (the figures above "
              "include the gaps between launches), other batch sizes, an F32 handle.", ""]
    acc = os.path.join(out_dir, "accuracy.md")
    lines += ["**Accuracy**", ""]
    lines += [open(acc).read().rstrip()] if os.path.exists(acc) else ["not measured"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--render", action="store_true", help="write INDEX.md again from the id_derivatives_bench.json in --out; nothing is run")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.render:
        with open(os.path.join(args.out, "id_derivatives_bench.json")) as fh:
            r = json.load(fh)
    else:
        r = bench(args.batch, args.reps, args.rounds, not args.no_gpu)
        with open(os.path.join(args.out, "id_derivatives_bench.json"), "w") as fh:
            json.dump(r, fh, indent=1)
    with open(os.path.join(args.out, "INDEX.md"), "w") as fh:
        fh.write(index_md(r, args.out))
    print(json.dumps(r))
