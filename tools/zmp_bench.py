#!/usr/bin/env python3
"""What the ZMP force distributor costs a fleet: B Talos-like robots (default 1024) in double support, synthetic foot wrenches, per tick

    observe_acom  ->  stabilize_zmp  ->  latch (flags to the host)  ->  tick_mixed over {default weights, zmp_w}

beside the same loop with zmp = NULL (every robot stays in the default slot), the two stabiliser instantiations alone, and the rows kernel on a slot
with and without force references.  Timed by device events:
    stabilize_ms / stabilize_zmp_ms     one launch of stabilize_kernel<., false> / <., true> on resident arrays
    rows_ms / rows_fref_ms              one wbcqp_problem_data on a slot without / with wbcqp_set_force_references
    loop_ms / loop_zmp_ms               K ticks of the loop, per tick (the latch's copy of the flags is in both)
--tree PATH imports the package of another checkout with its own built library (the parent commit's, for the rows kernel's figure on the same box in
the same session; then only rows_ms is measured, through calls that checkout has too).  An APPROXIMATION in the sense of tools/stabilizer_bench.py: synthetic sensors, and the
chain observes the state a tick starts from.  Writes profiles/stabilizer/zmp_bench.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ms(fn, torch, K, reps):
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
    return dict(median=float(np.median(ms)), min=float(np.min(ms)))


def rows_only(B, reps, tree):
    """One wbcqp_problem_data on B Talos states, with the package found on sys.path (this tree's, or --tree's)."""
    import torch
    from inria_wbc_amd import capi, structure
    from inria_wbc_amd import model as mdl
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    m, st = mdl.talos_like(), structure.talos_structure()
    tm = mdl.build_taskmap(m, st, mdl.talos_stack())
    s = mdl.sample_states(m, tm, B, 9_200_000, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    L = st.field_lengths()
    rows = {k: torch.zeros(B, max(L[k], 1), dtype=torch.float64, device=dev) for k in capi.ROW_FIELDS}
    state = dict(q=up(s["q"]), v=up(s["v"]), ref=up(s["ref"]))
    h = capi.Handle(0, capi.F64)
    h.set_structure(0, st)
    h.set_model(0, m, tm)
    sp = torch.cuda.current_stream().cuda_stream
    r = _ms(lambda: [h.problem_data(0, B, state, rows, stream=sp) for _ in range(20)], torch, 20, max(reps, 50))  # (20 launches back to back per interval)
    h.close()
    return dict(batch=B, nref=int(tm.nref), package=os.path.dirname(capi.__file__), rows_ms=r)


def run(B, K, reps):
    import dataclasses
    import torch
    from inria_wbc_amd import capi, observe
    from inria_wbc_amd import model as mdl
    from inria_wbc_amd import stabilizer as stb
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    m = mdl.talos_like()
    g = stb.STAB_FILES["talos"]["double_support"]
    st_d, tm = mdl.talos_contact_sets(m, force_refs=True)["both"]
    st_z = dataclasses.replace(st_d, contacts=[dataclasses.replace(c, force_reg_weights=g["zmp_w"]) for c in st_d.contacts])
    stack = mdl.talos_stack()
    s = mdl.sample_states(m, tm, B, 9_200_000, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    q0, v0, ref = up(s["q"]), up(s["v"]), up(s["ref"])
    sp = torch.cuda.current_stream().cuda_stream
    L = st_d.field_lengths()
    rows = {k: torch.zeros(B, max(L[k], 1), **f64) for k in capi.ROW_FIELDS}
    h = capi.Handle(0, capi.F64)
    for slot, st in enumerate((st_d, st_z)):
        h.set_structure(slot, st)
        h.set_model(slot, m, tm)
    res = dict(batch=B, ticks=K, reps=reps, nref=int(tm.nref))
    res["rows_ms"] = _ms(lambda: h.problem_data(0, B, dict(q=q0, v=v0, ref=ref), rows, stream=sp), torch, 1, max(reps, 50))
    w_of = lambda st: np.array([c.force_reg_weights for c in st.contacts], dtype=np.float64)  # noqa: E731
    h.set_force_references(1, tm.contact_fref, w_of(st_z))
    res["rows_fref_ms"] = _ms(lambda: h.problem_data(1, B, dict(q=q0, v=v0, ref=ref), rows, stream=sp), torch, 1, max(reps, 50))
    h.set_force_references(0, tm.contact_fref, w_of(st_d))
    h.set_observed_frames(0, observe.frame_ids(m, ["leg_left_6_joint", "leg_right_6_joint"]))
    stab = stb.from_taskmap(m, tm, stack, g["window"], g["com_gains"], g["ankle_gains"], g["ffda_gains"])
    zmp = stb.zmp_from_taskmap(tm, stack, g["zmp_p"], g["zmp_d"])
    rng = np.random.default_rng(12)
    weight = stab.mass * 9.81
    wrench = np.zeros((K, B, 12))
    wrench[..., [2, 8]] = weight / 2 + 20.0 * rng.standard_normal((K, B, 2))
    wrench[..., [0, 1, 6, 7]] = 5.0 * rng.standard_normal((K, B, 4))
    wrench[..., [3, 4, 9, 10]] = 3.0 * np.sin(0.02 * np.arange(K))[:, None, None] + 0.5 * rng.standard_normal((K, B, 4))
    wrench = up(wrench)
    com, acom, place = torch.zeros(B, 3, **f64), torch.zeros(B, 3, **f64), torch.zeros(B, 2, 12, **f64)
    ref_out, flags, alpha = torch.zeros_like(ref), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, 2, **f64)
    state = torch.zeros(B, stb.state_bytes(stab.window), dtype=torch.uint8, device=dev)
    out = dict(x=torch.zeros(B, st_d.n, **f64), tau=torch.zeros(B, st_d.na, **f64), status=torch.zeros(B, dtype=torch.int32, device=dev),
               iters=torch.zeros(B, dtype=torch.int32, device=dev))
    w = [up(np.tile(st.default_weights, (B, 1))) for st in (st_d, st_z)]
    tlb, tub = up(np.tile(-m.tau_max, (B, 1))), up(np.tile(m.tau_max, (B, 1)))
    latched = {}

    def loop(z):
        q, v = q0.clone(), v0.clone()
        qn, vn = torch.zeros_like(q), torch.zeros_like(v)
        state.zero_()
        latch = stb.ZmpLatch(B)
        for t in range(K):
            h.observe(0, B, q, v, com=com, placement=place, acom=acom, stream=sp)
            h.stabilize_zmp(stab, z, B, ref, wrench[t], com, acom, place, ldp=24, x_prev=out["x"] if t else None, ldx=st_d.n, state=state, ref_out=ref_out,
                            flags=flags, alpha=alpha if z is not None else None, stream=sp)
            latch.update(flags.cpu().numpy())
            h.tick_mixed([0, 1], latch.which(), dict(q=q, v=v, ref=ref_out), w, out, qn, vn, tm.dt, tlb=tlb, tub=tub, stream=sp)
            q, qn = qn, q
            v, vn = vn, v
        latched[z is not None] = int(latch.latched.sum())

    res["loop_ms"] = _ms(lambda: loop(None), torch, K, reps)
    res["loop_zmp_ms"] = _ms(lambda: loop(zmp), torch, K, reps)
    res["latched_after_the_loop"] = dict(without=latched[False], with_zmp=latched[True])
    res["solved_on_the_last_tick"] = int((out["status"] == 0).sum().item())
    res["zmp_ran_on_the_last_tick"] = int(((flags & stb.ZMP) != 0).sum().item())
    one = lambda z: h.stabilize_zmp(stab, z, B, ref, wrench[K - 1], com, acom, place, ldp=24, x_prev=out["x"], ldx=st_d.n, state=state, ref_out=ref_out,  # noqa: E731
                                    flags=flags, alpha=alpha if z is not None else None, stream=sp)
    res["stabilize_ms"] = _ms(lambda: one(None), torch, 1, max(reps, 50))
    res["stabilize_zmp_ms"] = _ms(lambda: one(zmp), torch, 1, max(reps, 50))
    h.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows-only", action="store_true", help="time wbcqp_problem_data alone, on the plain Talos map (no force references)")
    ap.add_argument("--tree", default=None, help="with --rows-only: import inria_wbc_amd from this checkout instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    r = rows_only(a.batch, a.reps, a.tree) if a.rows_only or a.tree else run(a.batch, a.ticks, a.reps)
    path = a.out or os.path.join(ROOT, "profiles", "stabilizer", "zmp_bench_rows.json" if a.rows_only or a.tree else "zmp_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))
