"""What the tests of a tick's force references share (tests/test_zmp_host.py, test_gpu_force_refs.py, test_gpu_zmp_closed_loop.py): structures whose
contacts carry other force-regularisation weights, the patch of an oracle record's b1, the one solve-parity input and the closed loop's CPU side
(transcription, oracle rows with patched b1, oracle solve, integration), each computed once.  A plain module."""
import dataclasses
import functools

import numpy as np

from inria_wbc_amd import model as mdl
from inria_wbc_amd import observe as obs
from inria_wbc_amd import stabilizer as stb
from inria_wbc_amd import structure

TALOS_DS = stb.STAB_FILES["talos"]["double_support"]
ZMP_W = TALOS_DS["zmp_w"]
SOLVE_BATCH, SOLVE_SEED = 5, 52_000
LOOP_B, LOOP_WINDOW, LOOP_TICKS = 5, 2, 12
LOOP_LATCH_AT = [1, 2, 3, 4, -1]  # robot i's feet are loaded from tick i on: its CoP is valid, and the law runs, one tick later (window 2); robot 4: never
ANKLES = ("leg_left_6_joint", "leg_right_6_joint")


def with_weights(st, w):
    """`st` with every contact's force-regularisation weights replaced by w (forcereg_mat = diag(w) T)."""
    return dataclasses.replace(st, contacts=[dataclasses.replace(c, force_reg_weights=tuple(float(x) for x in w)) for c in st.contacts])


def weights_of(st):
    return np.array([c.force_reg_weights for c in st.contacts], dtype=np.float64).reshape(st.nc, 6)


def force_rows(st):
    """Indices into b1 of the force-regularisation entries [nc, 6]."""
    return (st.n_dense + st.n_sel + np.arange(6 * st.nc)).reshape(st.nc, 6)


def patch_b1(st, fref, rows, ref):
    """An oracle record with the force entries of b1 set to the float64 product w_f * f_ref (fref [nc]: offsets in ref, -1: none)."""
    rows = dict(rows, b1=np.array(rows["b1"], dtype=np.float64, copy=True))
    w = weights_of(st)
    for c in range(st.nc):
        if fref[c] >= 0:
            rows["b1"][:, force_rows(st)[c]] = w[c][None, :] * np.asarray(ref, dtype=np.float64)[:, fref[c]:fref[c] + 6]
    return rows


def law_sized_references(m, tm, ref, seed):
    """Force references of the size the law produces, into the blocks of ref: the admittance of Talos' file for a model ZMP near the middle of the feet
    and a measured one a centimetre or two away."""
    rng = np.random.default_rng(seed)
    mass = float(m.inertia[:, 0].sum())
    cl, cr = (int(x) for x in tm.contact_ref[:2])
    for i in range(ref.shape[0]):
        PL, PR = ref[i, cl:cl + 2], ref[i, cr:cr + 2]
        mid = 0.5 * (PL + PR)
        left, right, _, _, ok = stb.zmp_admittance(tm.dt, TALOS_DS["zmp_p"], TALOS_DS["zmp_d"], mass, mid + rng.normal(0.0, 0.01, 2), mid + rng.normal(0.0, 0.02, 2), PL, PR)
        assert ok
        ref[i, tm.contact_fref[0]:tm.contact_fref[0] + 6], ref[i, tm.contact_fref[1]:tm.contact_fref[1] + 6] = left, right
    return ref


@functools.lru_cache(maxsize=None)
def solve_case():
    """Talos in double support with zmp_w weights, SOLVE_BATCH states, force references of the law's size; the oracle's rows with b1 patched and its solve."""
    from oracle import oracle as orc
    from oracle import rbd
    m = mdl.talos_like()
    st = with_weights(structure.talos_structure(), ZMP_W)
    tm = mdl.build_taskmap(m, st, mdl.talos_stack(), force_refs=True)
    s = mdl.sample_states(m, tm, SOLVE_BATCH, SOLVE_SEED, q_noise=0.01, v_noise=0.05, ref_noise=0.005)
    law_sized_references(m, tm, s["ref"], SOLVE_SEED)
    B = SOLVE_BATCH
    lim = dict(tlb=np.tile(-m.tau_max, (B, 1)), tub=np.tile(m.tau_max, (B, 1)), w=np.tile(st.default_weights, (B, 1)))
    rows = patch_b1(st, tm.contact_fref, rbd.task_rows(m, tm, st, s["q"], s["v"], s["ref"]), s["ref"])
    b1_force = rows["b1"][:, force_rows(st).reshape(-1)]
    return dict(m=m, st=st, tm=tm, states=s, lim=lim, rows=rows, b1_force=b1_force, oracle=orc.tick_batch(st, dict(rows, **lim)))


def loop_setup():
    """The closed loop's ingredients: Talos-like robots in double support, two slots of one contact set (default weights, zmp_w), the stabiliser and
    distributor of Talos' double-support file at window 2, the base reference row and the synthetic foot wrenches [T, B, 12]."""
    m = mdl.talos_like()
    st_d, tm = mdl.talos_contact_sets(m, force_refs=True)["both"]
    st_z = with_weights(st_d, ZMP_W)
    stack = mdl.talos_stack()
    stab = stb.from_taskmap(m, tm, stack, LOOP_WINDOW, TALOS_DS["com_gains"], TALOS_DS["ankle_gains"], TALOS_DS["ffda_gains"])
    z = stb.zmp_from_taskmap(tm, stack, TALOS_DS["zmp_p"], TALOS_DS["zmp_d"])
    B, T = LOOP_B, LOOP_TICKS
    s = mdl.sample_states(m, tm, B, 53_000, q_noise=0.002, v_noise=0.01, ref_noise=0.0)
    half = 0.5 * stab.mass * 9.81
    wrench = np.zeros((T, B, 12))
    wrench[:, :, [2, 8]] = 10.0  # a foot that carries nothing: below FMIN, no CoP, no force sample
    for i in range(4):
        for t in range(i, T):
            wrench[t, i] = (2.0, -1.0, half + 5.0 * i, 1.0 + i, -2.0 - 0.25 * t, 0.125, -1.0, 2.0, half - 5.0 * i, -1.5, 2.5 + i, 0.25)
    return dict(m=m, sts=(st_d, st_z), tm=tm, stab=stab, zmp=z, states=s, wrench=wrench, frames=obs.frame_ids(m, list(ANKLES)),
                tlb=np.tile(-m.tau_max, (B, 1)), tub=np.tile(m.tau_max, (B, 1)), w=[np.tile(st.default_weights, (B, 1)) for st in (st_d, st_z)])


@functools.lru_cache(maxsize=None)
def closed_loop_reference():
    """The loop on the CPU: per tick observe -> step(zmp) -> latch -> per slot (oracle rows, b1 patched, oracle solve, integration)."""
    from oracle import oracle as orc
    from oracle import rbd
    L = loop_setup()
    m, tm, stab, z = L["m"], L["tm"], L["stab"], L["zmp"]
    B = LOOP_B
    q, v, ref = L["states"]["q"].copy(), L["states"]["v"].copy(), L["states"]["ref"]
    state = np.zeros((B, stb.state_bytes(stab.window)), np.uint8)
    latch, x_prev, ticks = stb.ZmpLatch(B), None, []
    latched_at = [-1] * B
    for t in range(LOOP_TICKS):
        o = obs.observe(m, q, v, L["frames"], acom=True)
        so = stb.step(stab, state, dict(ref=ref, wrench=L["wrench"][t], com=o["com"], acom=o["acom"], placement=o["placement"].reshape(B, -1), x_prev=x_prev), zmp=z)
        before = latch.latched.copy()
        which = latch.update(so["flags"]).astype(np.int32)
        for i in np.nonzero(latch.latched & ~before)[0]:
            latched_at[i] = t
        x, tau = np.zeros((B, L["sts"][0].n)), np.zeros((B, m.na))
        status, iters = np.zeros(B, np.int32), np.zeros(B, np.int32)
        nq_, nv_ = q.copy(), v.copy()
        for k, st in enumerate(L["sts"]):
            idx = np.nonzero(which == k)[0]
            if idx.size == 0:
                continue
            rows = patch_b1(st, tm.contact_fref, rbd.task_rows(m, tm, st, q[idx], v[idx], so["ref_out"][idx]), so["ref_out"][idx])
            oo = orc.tick_batch(st, dict(rows, tlb=L["tlb"][idx], tub=L["tub"][idx], w=L["w"][k][idx]))
            nxt = orc.integrate(True, tm.dt, q[idx], v[idx], oo["x"][:, :st.nv])
            ok = oo["status"] == 0
            nq_[idx[ok]], nv_[idx[ok]] = nxt["q_next"][ok], nxt["v_next"][ok]
            x[idx], tau[idx], status[idx], iters[idx] = oo["x"], oo["tau"], oo["status"], oo["iters"]
        ticks.append(dict(flags=so["flags"].copy(), which=which, ref_out=so["ref_out"], alpha=so["alpha"], x=x, tau=tau, status=status, iters=iters, q=nq_.copy(), v=nv_.copy()))
        q, v, x_prev = nq_, nv_, x
    return dict(setup=L, ticks=ticks, latched_at=latched_at)
