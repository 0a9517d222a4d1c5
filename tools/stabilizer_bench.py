#!/usr/bin/env python3
"""What the stabiliser costs a fleet: B Talos-like robots (default 1024), a device-only chain per tick

    observe (com, acom, the two ankle frames of the state the tick starts from)  ->  stabilise  ->  tick with ref_out

against the plain tick on the same states, and the stabiliser's kernel alone.  Timed by device events:
    stabilize_ms          one wbcqp_stabilize launch on resident arrays (median and minimum over --reps)
    tick_ms               K ticks without the stabiliser, per tick
    stabilised_tick_ms    K ticks of the chain, per tick
An APPROXIMATION, as tools/observe_bench.py says of itself: the sensors are synthetic (each foot carries about half the weight, with noise and a
slow sideways sway, so every law applies once the window has filled), and the chain observes the state a tick STARTS from, where the facade of
the reference lags by one tick -- the cost is the same.  The stabiliser uses the reference's Talos double-support gains and window (7).
Writes profiles/stabilizer/stabilizer_bench.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _per_tick_ms(fn, torch, K, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / K)
    return ms


def run(B, K, reps):
    import torch
    from inria_wbc_amd import capi, observe, structure
    from inria_wbc_amd import model as mdl
    from inria_wbc_amd import stabilizer as stb
    dev = torch.device("cuda", 0)
    m, st = mdl.talos_like(), structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    g = stb.TALOS_GAINS
    stab = stb.from_taskmap(m, tm, mdl.talos_stack(), g["window"], g["com_gains"], g["ankle_gains"], g["ffda_gains"])
    s = mdl.sample_states(m, tm, B, 9_100_000, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    L = st.field_lengths()
    rows = {k: torch.zeros(B, max(L[k], 1), **f64) for k in capi.ROW_FIELDS}
    rows.update(tlb=up(np.tile(-m.tau_max, (B, 1))), tub=up(np.tile(m.tau_max, (B, 1))), w=up(np.tile(st.default_weights, (B, 1))))
    out = dict(x=torch.zeros(B, st.n, **f64), tau=torch.zeros(B, st.na, **f64), status=torch.zeros(B, dtype=torch.int32, device=dev),
               iters=torch.zeros(B, dtype=torch.int32, device=dev))
    q0, v0, ref = up(s["q"]), up(s["v"]), up(s["ref"])
    # sensors of K ticks: about half the weight on each foot, noise, a slow sway in the ankle torques
    rng = np.random.default_rng(11)
    weight = stab.mass * 9.81
    wrench = np.zeros((K, B, 12))
    wrench[..., [2, 8]] = weight / 2 + 20.0 * rng.standard_normal((K, B, 2))
    wrench[..., [0, 1, 6, 7]] = 5.0 * rng.standard_normal((K, B, 4))
    wrench[..., [3, 4, 9, 10]] = 3.0 * np.sin(0.02 * np.arange(K))[:, None, None] + 0.5 * rng.standard_normal((K, B, 4))
    wrench = up(wrench)
    com, acom, place = torch.zeros(B, 3, **f64), torch.zeros(B, 3, **f64), torch.zeros(B, 2, 12, **f64)
    ref_out, flags = torch.zeros_like(ref), torch.zeros(B, dtype=torch.int32, device=dev)
    state = torch.zeros(B, stb.state_bytes(stab.window), dtype=torch.uint8, device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)
    h.set_observed_frames(0, observe.frame_ids(m, ["leg_left_6_joint", "leg_right_6_joint"]))

    def chain(stabilised):
        q, v = q0.clone(), v0.clone()
        qn, vn = torch.zeros_like(q), torch.zeros_like(v)
        if stabilised:
            state.zero_()
        for t in range(K):
            if stabilised:
                h.observe(0, B, q, v, com=com, placement=place, acom=acom, stream=sp)
                h.stabilize(stab, B, ref, wrench[t], com, acom, place, ldp=24, x_prev=out["x"] if t else None, ldx=st.n, state=state, ref_out=ref_out,
                            flags=flags, stream=sp)
            h.tick(0, B, dict(q=q, v=v, ref=ref_out if stabilised else ref), rows, out, qn, vn, tm.dt, stream=sp)
            q, qn = qn, q
            v, vn = vn, v

    plain = _per_tick_ms(lambda: chain(False), torch, K, reps)
    stabd = _per_tick_ms(lambda: chain(True), torch, K, reps)
    applied = {name: int(((flags & bit) != 0).sum().item()) for name, bit in (("com", stb.COM), ("left ankle", stb.LANKLE), ("right ankle", stb.RANKLE),
                                                                              ("torso", stb.FFDA), ("error", stb.ERR_COP | stb.ERR_FORCE))}
    ok = int((out["status"] == 0).sum().item())
    # the kernel alone, on the arrays the last tick left (the state keeps advancing: a launch's cost does not depend on what the window holds)
    alone = _per_tick_ms(lambda: h.stabilize(stab, B, ref, wrench[K - 1], com, acom, place, ldp=24, x_prev=out["x"], ldx=st.n, state=state, ref_out=ref_out,
                                             flags=flags, stream=sp), torch, 1, max(reps, 20))
    h.close()
    moved = B * (2 * stab.nref + 12 + 6 + 6 + 24 + 2 * stb.state_bytes(stab.window) // 8 + 1) * 8
    return dict(batch=B, ticks=K, reps=reps, window=stab.window, nref=stab.nref, stabilize_ms_median=float(np.median(alone)), stabilize_ms_min=float(np.min(alone)),
                stabilize_bytes_moved=int(moved), tick_ms_median=float(np.median(plain)), tick_ms_min=float(np.min(plain)),
                stabilised_tick_ms_median=float(np.median(stabd)), stabilised_tick_ms_min=float(np.min(stabd)),
                laws_applied_on_the_last_tick=applied, solved_on_the_last_tick=ok,
                note="stabilised tick = observe (com, acom, two frames) + stabilise + tick; one launch of each per tick, timed over the whole chain by device events")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.batch, a.ticks, a.reps)
    path = a.out or os.path.join(ROOT, "profiles", "stabilizer", "stabilizer_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
