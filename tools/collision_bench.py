#!/usr/bin/env python3
"""What the sphere check costs: wbcqp_check_collisions with the reference's Talos table (tests/golden/talos_collisions.yaml, 112 spheres in 5 members
on the Talos-like model) on B robots, beside wbcqp_observe and the rows kernel on the same states.

    python tools/collision_bench.py [--batch 1024 8192] [--reps 50]
        launches collide_kernel, observe_kernel and the rows kernel (wbcqp_problem_data) `reps` times each per batch and nothing else: the program
        to put behind `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/collision_bench.py`; the three kernels' times then
        come from that ONE trace (python tools/rocpd_kernel_stats.py <dir>/.../*_results.db --match collide_kernel observe_kernel terms_kernel).
        Without a profiler it prints each call's time per launch back to back (device events: includes the gaps between launches).
The check's algorithmic traffic is nq doubles in and 16 B out per robot (colliding, first_pair, n_pairs): it is bound by LDS reads and issue, not by
HBM.  (A trace needs no mode of its own here: checking a traced roll-out's q array is the same launch with batch = n_rec x batch.)
Writes profiles/collision/collision_bench_kernels.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FRAMES = ["leg_left_6_joint", "leg_right_6_joint", "gripper_left_joint", "gripper_right_joint", "base_link", "torso_2_link", "head_2_joint", "arm_left_4_joint"]
FIXTURE = os.path.join(ROOT, "tests", "golden", "talos_collisions.yaml")


def _states(m, tm, n, dev, torch, distinct=256):
    """n states: `distinct` different ones, tiled."""
    from inria_wbc_amd import model as mdl
    s = mdl.sample_states(m, tm, min(n, distinct), 9_100_000, q_noise=0.05, v_noise=0.2)
    rep = -(-n // s["q"].shape[0])
    return {k: torch.from_numpy(np.ascontiguousarray(np.tile(a, (rep, 1))[:n])).to(dev) for k, a in s.items()}


def kernels(batches, reps):
    import torch
    from inria_wbc_amd import capi, collision, observe, structure
    from inria_wbc_amd import model as mdl
    dev = torch.device("cuda", 0)
    m, st = mdl.talos_like(), structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)
    frames = observe.frame_ids(m, FRAMES)
    h.set_observed_frames(0, frames)
    table = collision.sphere_table(m, FIXTURE)
    h.set_collision_spheres(0, table)
    sp = torch.cuda.current_stream().cuda_stream
    L = st.field_lengths()
    res = dict(n_spheres=table.n_spheres, members=table.member_names, reps=reps, collide_bytes_per_instance=8 * m.nq + 16, batches={})
    for B in batches:
        s = _states(m, tm, B, dev, torch)
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
        out = dict(com=f(B, 3), vcom=f(B, 3), placement=f(B, len(frames), 12), velocity=f(B, len(frames), 6))
        rows = {k: torch.zeros(B, max(L[k], 1), dtype=torch.float64, device=dev) for k in capi.ROW_FIELDS}
        flags = dict(colliding=torch.zeros(B, dtype=torch.int32, device=dev), first_pair=torch.zeros(B, 2, dtype=torch.int32, device=dev),
                     n_pairs=torch.zeros(B, dtype=torch.int32, device=dev))
        ev = {}
        for what, call in (("collide", lambda: h.check_collisions(0, B, s["q"], stream=sp, **flags)),
                           ("observe", lambda: h.observe(0, B, s["q"], s["v"], stream=sp, **out)), ("terms", lambda: h.problem_data(0, B, s, rows, stream=sp))):
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            e1.synchronize()
            ev[what + "_us_per_launch_back_to_back"] = 1e3 * e0.elapsed_time(e1) / reps
        ev["colliding"] = int(flags["colliding"].sum().item())
        res["batches"][str(B)] = ev
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    res = kernels(a.batch, a.reps)
    os.makedirs(os.path.join(ROOT, "profiles", "collision"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "collision", "collision_bench_kernels.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
