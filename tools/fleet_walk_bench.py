#!/usr/bin/env python3
"""A fleet of B Talos-like robots walking on the spot with uniformly staggered phase offsets (humanoid::walk-on-spot, 200-tick phases):
at any tick about a third of the fleet stands on one foot, and which instances do changes at every lift-off and touchdown.

Three ways to drive it, each timed by device events over the same chunks of ticks after a warm-up that walks every instance into its gait:
  (a) mixed    wbcqp_rollout_mixed: the chunk's K ticks enqueued in one call (rows per contact set, ONE solve launch, scatter + integrate)
  (b) host     per tick, a torch gather of each contact set's instances, one wbcqp_tick per set, a scatter back (what a caller does today)
  (c) lockstep wbcqp_rollout on the double-support slot only: every instance in the same contact set (the ceiling: one specialised launch)
(a) and (b) compute the same states bit for bit (checked at the end of every chunk); (c) is another workload of the same size.

    python tools/fleet_walk_bench.py [--batch 1024] [--chunk 100] [--chunks 3] [--only a|b|c] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from inria_wbc_amd import capi  # noqa: E402
from inria_wbc_amd import model as mdl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1300, help="ticks walked before timing (every instance past its start offset)")
    ap.add_argument("--phase", type=float, default=0.2, help="traj_com_duration = traj_foot_duration [s]")
    ap.add_argument("--only", default="abc")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    B, K = args.batch, args.chunk
    m = mdl.talos_like()
    sets = mdl.talos_contact_sets(m)
    names = list(sets)
    h = capi.Handle(0, capi.F64)
    slots = list(range(len(names)))
    for sl, nm in zip(slots, names):
        h.set_structure(sl, sets[nm][0])
        h.set_model(sl, m, sets[nm][1])
    plan = mdl.WalkOnSpotPlan(m, {k: tm for k, (_, tm) in sets.items()}, args.phase, args.phase, 0.05)
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
    q, v = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)

    def new_out(n_cols):
        return dict(x=torch.zeros(B, n_cols, dtype=torch.float64, device=dev), tau=torch.zeros(B, m.na, dtype=torch.float64, device=dev),
                    status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev))

    out = new_out(ldx)
    qn, vn = torch.zeros_like(q), torch.zeros_like(v)
    isum, tok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    # warm-up: walk the fleet into its gait with (a)
    t0 = time.time()
    for k0 in range(0, args.warmup, K):
        sch, ref = plan.plan(offsets, k0, min(K, args.warmup - k0))
        h.rollout_mixed(slots, sch, dict(q=q, v=v, ref=torch.from_numpy(ref).to(dev)), w, out, qn, vn, dt, tlb=tlb, tub=tub, iters_sum=isum,
                        ticks_ok=tok, stream=stream)
        torch.cuda.synchronize()
        assert (tok.cpu().numpy() == sch.shape[0]).all(), "a QP failed during the warm-up"
        q, qn = qn.clone(), q
        v, vn = vn.clone(), v
    print("warm-up: %d ticks in %.1f s" % (args.warmup, time.time() - t0), file=sys.stderr)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {k: [] for k in "abc"}
    share = []
    # (b)'s buffers: one per contact set, sized for the whole batch (a set's instances are a prefix of them)
    Lf = {nm: sets[nm][0].field_lengths() for nm in names}
    rows_b = {nm: {f: torch.zeros(B * max(Lf[nm][f], 1), dtype=torch.float64, device=dev) for f in capi.ROW_FIELDS} for nm in names}
    same = True
    for c in range(args.chunks):
        k0 = args.warmup + c * K
        sch, ref = plan.plan(offsets, k0, K)
        share.append(float((sch != names.index("both")).mean()))
        ref_d = torch.from_numpy(ref).to(dev)
        qa = qb = None
        if "a" in args.only:  # (a) one call
            torch.cuda.synchronize()
            e0.record()
            h.rollout_mixed(slots, sch, dict(q=q, v=v, ref=ref_d), w, out, qn, vn, dt, tlb=tlb, tub=tub, iters_sum=isum, ticks_ok=tok, stream=stream)
            e1.record()
            torch.cuda.synchronize()
            res["a"].append(e0.elapsed_time(e1) * 1e-3)
            assert (tok.cpu().numpy() == K).all()
            qa, va = qn.clone(), vn.clone()
        if "b" in args.only:  # (b) from the host: gather, one wbcqp_tick per contact set, scatter
            idx = [[torch.from_numpy(np.nonzero(sch[t] == k)[0]).to(dev) for k in range(len(names))] for t in range(K)]
            cq, cv = q.clone(), v.clone()
            torch.cuda.synchronize()
            e0.record()
            for t in range(K):
                nq_, nv_ = torch.empty_like(cq), torch.empty_like(cv)
                for k, nm in enumerate(names):
                    ii = idx[t][k]
                    nb = int(ii.numel())
                    if nb == 0:
                        continue
                    st = sets[nm][0]
                    rows = {f: rows_b[nm][f][:nb * max(Lf[nm][f], 1)] for f in capi.ROW_FIELDS}
                    rows["w"] = w[k].index_select(0, ii)
                    rows["tlb"], rows["tub"] = tlb.index_select(0, ii), tub.index_select(0, ii)
                    o = dict(x=torch.empty(nb, st.n, dtype=torch.float64, device=dev), tau=torch.empty(nb, m.na, dtype=torch.float64, device=dev),
                             status=torch.empty(nb, dtype=torch.int32, device=dev), iters=torch.empty(nb, dtype=torch.int32, device=dev))
                    sq, sv = torch.empty(nb, m.nq, dtype=torch.float64, device=dev), torch.empty(nb, m.nv, dtype=torch.float64, device=dev)
                    sub = dict(q=cq.index_select(0, ii), v=cv.index_select(0, ii), ref=ref_d[t].index_select(0, ii))
                    h.tick(slots[k], nb, sub, rows, o, sq, sv, dt, stream=stream)
                    nq_.index_copy_(0, ii, sq)
                    nv_.index_copy_(0, ii, sv)
                cq, cv = nq_, nv_
            e1.record()
            torch.cuda.synchronize()
            res["b"].append(e0.elapsed_time(e1) * 1e-3)
            qb = cq
            if qa is not None:
                same = same and bool(torch.equal(qa, qb))
        if "c" in args.only:  # (c) lockstep: the double-support slot for everyone, one wbcqp_rollout
            outc = new_out(sets["both"][0].n)
            qc, vc = torch.zeros_like(q), torch.zeros_like(v)
            lim = dict(tlb=tlb, tub=tub, w=w[names.index("both")])
            torch.cuda.synchronize()
            e0.record()
            h.rollout(slots[names.index("both")], B, K, dict(q=q, v=v, ref=ref_d), lim, outc, qc, vc, dt, stream=stream)
            e1.record()
            torch.cuda.synchronize()
            res["c"].append(e0.elapsed_time(e1) * 1e-3)
        if qa is not None:
            q, v = qa, va
        elif qb is not None:
            q, v = qb, cv
    h.close()
    rep = {"batch": B, "ticks_per_chunk": K, "chunks": args.chunks, "phase_s": args.phase, "one_foot_share": float(np.mean(share)),
           "a_and_b_bitwise_equal": same if ("a" in args.only and "b" in args.only) else None}
    for k, label in (("a", "rollout_mixed"), ("b", "host_split_ticks"), ("c", "lockstep_rollout")):
        if res[k]:
            sec = float(np.median(res[k]))
            rep[label] = {"ticks_per_s": K / sec, "qp_per_s": B * K / sec, "us_per_tick": sec / K * 1e6, "samples_s": res[k]}
    if res["a"] and res["b"]:
        rep["a_over_b"] = rep["host_split_ticks"]["us_per_tick"] / rep["rollout_mixed"]["us_per_tick"]
    if res["a"] and res["c"]:
        rep["a_over_c"] = rep["lockstep_rollout"]["us_per_tick"] / rep["rollout_mixed"]["us_per_tick"]
    print(json.dumps(rep))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
