#!/usr/bin/env python3
"""What generating a roll-out's references on the device costs and saves: the fleet of tools/fleet_walk_bench.py (B Talos-like robots walking on the
spot, staggered offsets, the same warm-up) over the same ticks three ways, alternated, `--repeats` times each from the same state:
  (a) program   ONE wbcqp_rollout_mixed_program call for all the ticks (refgen_kernel makes the rows, the library the schedule)
  (b) uploaded  wbcqp_rollout_mixed in chunks of --chunk ticks, references planned on the host and uploaded BEFORE the timed region (the yardstick:
                the device path as it was)
  (c) planned   as (b) with the host plan and the copy inside the timed region (what a caller pays without programs)
(a) is repeated for every chunk length of --sweep (WBCQP_REFPROG_CHUNK, a handle each).  Then the squat: wbcqp_rollout_program against wbcqp_rollout
on pre-uploaded references.  Times are wall-clock around a device synchronisation (the host's share is the point of (c)).  The generator's own share
comes from a kernel trace of this program: rocprofv3 --kernel-trace --stats -- python tools/refprog_bench.py --only a

    python tools/refprog_bench.py [--batch 1024] [--ticks 1400] [--chunk 100] [--repeats 3] [--sweep 8,32,128] [--only abcs] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from inria_wbc_amd import capi, refprog, structure  # noqa: E402
from inria_wbc_amd import model as mdl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=0, help="timed ticks per run (0: one pass of the timeline, intro + cycle)")
    ap.add_argument("--chunk", type=int, default=100, help="ticks per wbcqp_rollout_mixed call of (b) and (c)")
    ap.add_argument("--warmup", type=int, default=1300)
    ap.add_argument("--phase", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sweep", default="8,32,128")
    ap.add_argument("--only", default="abcs")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    B = args.batch
    m = mdl.talos_like()
    sets = mdl.talos_contact_sets(m)
    names = list(sets)
    slots = list(range(len(names)))
    plan = mdl.WalkOnSpotPlan(m, {k: tm for k, (_, tm) in sets.items()}, args.phase, args.phase, 0.05)
    prog = refprog.walk_on_spot_program(plan)
    K = args.ticks or prog.length
    offsets = (np.arange(B) * plan.cycle) // B
    full = sets["both"][1]
    dt = full.dt
    s = mdl.sample_states(m, full, B, 1, q_noise=0.0, v_noise=0.0, ref_noise=0.0)
    w = []
    for st, _ in sets.values():
        wk = st.default_weights.copy()
        if "momentum" in st.task_names:
            wk[st.task_names.index("momentum")] = 0.0
        w.append(torch.from_numpy(np.tile(wk, (B, 1))).to(dev))
    tlb = torch.from_numpy(np.tile(-m.tau_max, (B, 1))).to(dev)
    tub = torch.from_numpy(np.tile(m.tau_max, (B, 1))).to(dev)
    ldx = max(st.n for st, _ in sets.values())
    stream = torch.cuda.current_stream().cuda_stream
    base = torch.from_numpy(plan.base).to(dev)
    out = dict(x=torch.zeros(B, ldx, dtype=torch.float64, device=dev), tau=torch.zeros(B, m.na, dtype=torch.float64, device=dev),
               status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev))
    qn, vn = torch.zeros(B, m.nq, dtype=torch.float64, device=dev), torch.zeros(B, m.nv, dtype=torch.float64, device=dev)
    tok = torch.zeros(B, dtype=torch.int32, device=dev)

    def fleet_handle(chunk=None):
        if chunk is None:
            os.environ.pop("WBCQP_REFPROG_CHUNK", None)
        else:
            os.environ["WBCQP_REFPROG_CHUNK"] = str(chunk)
        h = capi.Handle(0, capi.F64)
        for sl, nm in zip(slots, names):
            h.set_structure(sl, sets[nm][0])
            h.set_model(sl, m, sets[nm][1])
        return h

    def by_program(h, q, v, k0, n):
        h.rollout_mixed_program(slots, B, k0, n, prog, base, offsets, dict(q=q, v=v), w, out, qn, vn, dt, tlb=tlb, tub=tub, ticks_ok=tok, stream=stream)

    def by_array(h, q, v, sch, ref_d):
        h.rollout_mixed(slots, sch, dict(q=q, v=v, ref=ref_d), w, out, qn, vn, dt, tlb=tlb, tub=tub, ticks_ok=tok, stream=stream)

    h = fleet_handle()
    # warm-up: the fleet walks into its gait, by program (one call)
    q0, v0 = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)
    by_program(h, q0, v0, 0, args.warmup)
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == args.warmup).all(), "a QP failed during the warm-up"
    q0, v0 = qn.clone(), vn.clone()
    k_start = args.warmup
    chunks = [(k0, min(args.chunk, k_start + K - k0)) for k0 in range(k_start, k_start + K, args.chunk)]
    res = {"a": [], "b": [], "c": [], "c_plan_s": []}
    finals = {}

    def run_a(hh):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        by_program(hh, q0, v0, k_start, K)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        assert (tok.cpu().numpy() == K).all()
        return sec

    def run_chunks(timed_plan):
        q, v = q0, v0
        pre = None if timed_plan else [(sch, torch.from_numpy(ref).to(dev)) for sch, ref in (plan.plan(offsets, k0, n) for k0, n in chunks)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan_s = 0.0
        for i, (k0, n) in enumerate(chunks):
            if timed_plan:
                tp = time.perf_counter()
                sch, ref = plan.plan(offsets, k0, n)
                plan_s += time.perf_counter() - tp
                ref_d = torch.from_numpy(ref).to(dev)
            else:
                sch, ref_d = pre[i]
            by_array(h, q, v, sch, ref_d)
            if timed_plan:
                torch.cuda.synchronize()  # (the page of `ref` is reused by the next plan)
            q, v = qn.clone(), vn.clone()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, plan_s

    for r in range(args.repeats):
        if "a" in args.only:
            res["a"].append(run_a(h))
            finals["a"] = qn.clone()
        if "b" in args.only:
            res["b"].append(run_chunks(False)[0])
            finals["b"] = qn.clone()
        if "c" in args.only:
            sec, plan_s = run_chunks(True)
            res["c"].append(sec)
            res["c_plan_s"].append(plan_s)
    rep = {"batch": B, "ticks": K, "array_chunk": args.chunk, "repeats": args.repeats, "phase_s": args.phase, "default_refprog_chunk": 32}
    us = lambda xs: [x / K * 1e6 for x in xs]  # noqa: E731
    for k, label in (("a", "a_program_one_call"), ("b", "b_array_preuploaded"), ("c", "c_array_plan_and_copy_timed")):
        if res[k]:
            rep[label] = {"us_per_tick_median": float(np.median(us(res[k]))), "us_per_tick": us(res[k])}
    if res["c"]:
        rep["c_array_plan_and_copy_timed"]["host_plan_us_per_tick"] = us(res["c_plan_s"])
    if res["b"]:
        rep["b_spread_us_per_tick"] = float(max(us(res["b"])) - min(us(res["b"])))
    if "a" in finals and "b" in finals:  # the device's polynomial is not numpy's to the last bit: the two walks agree to rounding, not bit for bit
        rep["a_vs_b_max_abs_q_difference"] = float((finals["a"] - finals["b"]).abs().max().item())
    h.close()
    if "a" in args.only and args.sweep:
        rep["chunk_sweep_us_per_tick"] = {}
        for c in [int(x) for x in args.sweep.split(",")]:
            hh = fleet_handle(c)
            run_a(hh)  # (the handle's first call allocates)
            rep["chunk_sweep_us_per_tick"][str(c)] = us([run_a(hh) for _ in range(args.repeats)])
            hh.close()
        os.environ.pop("WBCQP_REFPROG_CHUNK", None)
    if "s" in args.only:  # the squat: one slot, 1024 instances 37 i ticks into the stream
        st = structure.talos_structure()
        tm = mdl.build_taskmap(m, st, mdl.talos_stack())
        ss = mdl.sample_states(m, tm, B, 93_000, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
        com = next(b for b in tm.blocks if b.kind == mdl.T_COM)
        sq = refprog.move_com_program(tm.nref, com.ref, m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0)
        so = -37 * np.arange(B)
        Ks = 200
        hs = capi.Handle(0, capi.F64)
        hs.set_structure(0, st)
        hs.set_model(0, m, tm)
        sb = torch.from_numpy(ss["ref"]).to(dev)
        state = dict(q=torch.from_numpy(ss["q"]).to(dev), v=torch.from_numpy(ss["v"]).to(dev))
        lim = dict(tlb=tlb, tub=tub, w=torch.from_numpy(np.tile(st.default_weights, (B, 1))).to(dev))
        o2 = dict(x=torch.zeros(B, st.n, dtype=torch.float64, device=dev), tau=out["tau"], status=out["status"], iters=out["iters"])
        ref_d = hs.reference_samples(sq, sb, so, 0, Ks, torch.zeros(Ks, B, tm.nref, dtype=torch.float64, device=dev), stream=stream)
        t = {"program": [], "array": []}
        for r in range(args.repeats + 3):  # (the library's first roll-outs of a shape try one and two sub-batches and allocate: not kept)
            for form in ("program", "array"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if form == "program":
                    hs.rollout_program(0, B, 0, Ks, sq, sb, so, state, lim, o2, qn, vn, tm.dt, stream=stream)
                else:
                    hs.rollout(0, B, Ks, dict(state, ref=ref_d), lim, o2, qn, vn, tm.dt, stream=stream)
                torch.cuda.synchronize()
                if r >= 3:
                    t[form].append((time.perf_counter() - t0) / Ks * 1e6)
        hs.close()
        rep["squat_us_per_tick"] = t
    print(json.dumps(rep))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
