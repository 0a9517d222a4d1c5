#!/usr/bin/env python3
"""What it costs to know which accelerations a fleet's torques produce: wbcqp_mass_matrix, wbcqp_forward_dynamics and wbcqp_spd_commands on B
Talos-like robots (default 1024), set beside wbcqp_inverse_dynamics (rnea_kernel alone) and beside the CPU route.

    python tools/forward_dynamics_bench.py [--batch 1024] [--reps 50] [--cpu-states 64]

Device: `reps` calls in a row between two events per call kind, microseconds per call (back to back: includes the launch gaps; a forward-dynamics
and an SPD call are TWO kernels, rnea_kernel then fdyn_kernel).  CPU route: the oracle's rbd_terms (M, nle, Jl) plus np.linalg.solve per state,
one core, timed on --cpu-states states and scaled to the batch (`cpu_us_extrapolated`).  Kernel resources: from the build's
-Rpass-analysis=kernel-resource-usage remarks (tools/kernel_resources.py prints them for every kernel).  Reported, not gated: nothing exists
at the parent commit to compare against.  Writes profiles/fdyn/forward_dynamics_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WRENCH_FRAMES = ["leg_left_6_joint", "leg_right_6_joint"]
DT = 0.001


def bench(B, reps, cpu_states):
    import torch
    from inria_wbc_amd import capi, observe, structure
    from inria_wbc_amd import forward_dynamics as fd
    from inria_wbc_amd import model as mdl
    from oracle import rbd
    dev = torch.device("cuda", 0)
    m = mdl.talos_like()
    st = structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)
    frames = observe.frame_ids(m, WRENCH_FRAMES)
    h.set_wrench_frames(0, frames)
    k = min(B, 256)
    s = mdl.sample_states(m, tm, k, 9_300_000, q_noise=0.05, v_noise=0.2)
    rng = np.random.default_rng(9_300_001)
    host = dict(q=s["q"], v=s["v"], tau=np.concatenate([np.zeros((k, m.nv - m.na)), rng.uniform(-1.0, 1.0, (k, m.na)) * m.tau_max], axis=1),
                wrench=100.0 * rng.standard_normal((k, len(frames), 6)), target=s["q"][:, m.nq - m.na:] + 0.01 * rng.standard_normal((k, m.na)))
    rep = -(-B // k)
    d = {key: torch.from_numpy(np.ascontiguousarray(np.tile(a, (rep,) + (1,) * (a.ndim - 1))[:B])).to(dev) for key, a in host.items()}
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    M, a, cmd, qdd, tau_id, info = f(B, m.nv, m.nv), f(B, m.nv), f(B, m.nv), f(B, m.nv), f(B, m.nv), torch.zeros(B, dtype=torch.int32, device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    kp, kd = (float(g) for g in fd.spd_gains(DT))
    calls = (("inverse_dynamics", lambda: h.inverse_dynamics(0, B, d["q"], tau_id, v=d["v"], wrench=d["wrench"], stream=sp)),
             ("mass_matrix", lambda: h.mass_matrix(0, B, d["q"], M, stream=sp)),
             ("forward_dynamics", lambda: h.forward_dynamics(0, B, d["q"], a, v=d["v"], tau=d["tau"], wrench=d["wrench"], info=info, stream=sp)),
             ("spd_commands", lambda: h.spd_commands(0, B, (DT, kp, kd), d["q"], d["target"], cmd, v=d["v"], wrench=d["wrench"], qddot=qdd, info=info,
                                                     stream=sp)))
    res = dict(batch=B, reps=reps, model=m.name, nv=m.nv, wrench_frames=WRENCH_FRAMES, lds_bytes_per_workgroup=4 * m.nv * (m.nv | 1) * 8,
               bytes_per_instance={c: fd.algorithmic_bytes(m, c, len(frames)) for c in ("mass_matrix", "forward_dynamics", "spd_commands")}, us_per_call={})
    for what, call in calls:
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        res["us_per_call"][what] = 1e3 * e0.elapsed_time(e1) / reps
    assert int(info.abs().max().item()) == 0
    # the CPU route on one core: the oracle's terms and a dense solve, state by state
    om = rbd.OracleModel(m)
    n = min(cpu_states, k)
    t0 = time.perf_counter()
    acpu = np.zeros((n, m.nv))
    for i in range(n):
        t = rbd.rbd_terms(om, host["q"][i], host["v"][i])
        b = host["tau"][i] - t["nle"]
        for j, fr in enumerate(frames):
            b += t["Jl"][fr].T @ host["wrench"][i, j]
        acpu[i] = np.linalg.solve(t["M"], b)
    per_state = 1e6 * (time.perf_counter() - t0) / n
    got = a.cpu().numpy()[:n]
    res.update(cpu_us_per_state=per_state, cpu_states_timed=n, cpu_us_extrapolated=per_state * B,
               max_rel_difference_of_a_on_the_cpu_states=float(np.abs(got - acpu).max() / max(1.0, np.abs(acpu).max())),
               note="cpu_us_extrapolated = rbd_terms + np.linalg.solve per state on one core x batch; a differs by cond(M) x rounding, see tests")
    h.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cpu-states", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    r = bench(args.batch, args.reps, args.cpu_states)
    path = args.out or os.path.join(ROOT, "profiles", "fdyn", "forward_dynamics_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(r, fh, indent=1)
    print(json.dumps(r))
