#!/usr/bin/env python3
"""What a per-tick trace costs a roll-out: wbcqp_rollout against wbcqp_rollout_traced with every field recorded at stride 1 and at
stride 10, on the Talos squat stream (B Talos-like robots, K ticks, instance i one tick ahead of instance i - 1 on the reference).  The
three forms alternate in one process, each timed by a pair of device events; the median per form is reported, with the standalone
wbcqp_task_costs launch on a solved record.  Writes profiles/trace/rollout_trace_bench.json.
python tools/rollout_trace_bench.py [--batch 1024] [--ticks 200] [--reps 7]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(batch=1024, ticks=200, reps=7):
    import torch
    from inria_wbc_amd import capi, structure, trajs
    from inria_wbc_amd import model as mdl
    m = mdl.talos_like()
    st = structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    B, K = batch, ticks
    dev = torch.device("cuda", 0)
    s = mdl.sample_states(m, tm, B, 9_000_000, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    com_blk = next(b for b in tm.blocks if b.kind == mdl.T_COM)
    pos, vel, acc = trajs.move_com_stream(m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0, loop=True, absolute=False)
    tab = np.concatenate([pos, vel, acc], axis=1)
    refs = np.repeat(s["ref"][None], K, axis=0).copy()
    refs[:, :, com_blk.ref:com_blk.ref + 9] = tab[(np.arange(K)[:, None] + np.arange(B)[None, :]) % len(tab)]
    f64 = dict(dtype=torch.float64, device=dev)
    lim = dict(tlb=torch.from_numpy(np.tile(-m.tau_max, (B, 1))).to(dev), tub=torch.from_numpy(np.tile(m.tau_max, (B, 1))).to(dev),
               w=torch.from_numpy(np.tile(st.default_weights, (B, 1))).to(dev))
    state = dict(q=torch.from_numpy(s["q"]).to(dev), v=torch.from_numpy(s["v"]).to(dev), ref=torch.from_numpy(np.ascontiguousarray(refs)).to(dev))
    out = dict(x=torch.zeros(B, st.n, **f64), tau=torch.zeros(B, st.na, **f64), status=torch.zeros(B, dtype=torch.int32, device=dev),
               iters=torch.zeros(B, dtype=torch.int32, device=dev), objective=torch.zeros(B, **f64))
    qn, vn = torch.zeros(B, m.nq, **f64), torch.zeros(B, m.nv, **f64)
    isum, tok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)

    def trace(stride):
        n = K // stride
        return dict(q=torch.zeros(n, B, m.nq, **f64), v=torch.zeros(n, B, m.nv, **f64), x=torch.zeros(n, B, st.n, **f64),
                    tau=torch.zeros(n, B, st.na, **f64), status=torch.zeros(n, B, dtype=torch.int32, device=dev),
                    iters=torch.zeros(n, B, dtype=torch.int32, device=dev), objective=torch.zeros(n, B, **f64), cost=torch.zeros(n, B, st.n_tasks, **f64))

    forms = {"untraced": None, "stride1": (trace(1), 1), "stride10": (trace(10), 10)}
    sp = torch.cuda.current_stream().cuda_stream
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)

    def one(form):
        if forms[form] is None:
            h.rollout(0, B, K, state, lim, out, qn, vn, tm.dt, iters_sum=isum, ticks_ok=tok, stream=sp)
        else:
            tr, stride = forms[form]
            h.rollout_traced(0, B, K, state, lim, out, qn, vn, tm.dt, trace=tr, stride=stride, iters_sum=isum, ticks_ok=tok, stream=sp)

    for _ in range(2):  # the roll-out's allocations and its measured choice of sub-batches settle
        for f in forms:
            one(f)
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one(f)
            e1.record()
            e1.synchronize()
            ms[f].append(e0.elapsed_time(e1))
    # the standalone cost launch on the last tick's record (the roll-out's record is internal: a wbcqp_tick fills one)
    L = st.field_lengths()
    rows = {k: torch.zeros(B, max(L[k], 1), **f64) for k in capi.ROW_FIELDS}
    rows.update(lim)
    h.tick(0, B, dict(q=qn, v=vn, ref=state["ref"][K - 1]), rows, out, torch.zeros_like(qn), torch.zeros_like(vn), tm.dt, stream=sp)
    cost = torch.zeros(B, st.n_tasks, **f64)
    for _ in range(3):
        h.task_costs(0, B, rows, out["x"], out["tau"], cost, stream=sp)
    torch.cuda.synchronize()
    cms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.task_costs(0, B, rows, out["x"], out["tau"], cost, stream=sp)
        e1.record()
        e1.synchronize()
        cms.append(e0.elapsed_time(e1))
    h.close()
    med = {f: float(np.median(v)) for f, v in ms.items()}
    rec_bytes = 8 * B * (L["A"] + L["b1"] + st.n + st.na + st.n_tasks)
    return dict(batch=B, ticks=K, reps=reps, ms=ms, median_ms=med, us_per_tick={f: 1e3 * v / K for f, v in med.items()},
                ratio_stride1=med["stride1"] / med["untraced"], ratio_stride10=med["stride10"] / med["untraced"],
                task_costs_us_median=1e3 * float(np.median(cms)), task_costs_us_min=1e3 * float(np.min(cms)),
                task_costs_bytes=rec_bytes, note="task_costs timed by events around one launch: includes the launch's fixed cost")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace", "rollout_trace_bench.json"))
    a = ap.parse_args()
    r = run(a.batch, a.ticks, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps({k: v for k, v in r.items() if k != "ms"}))
