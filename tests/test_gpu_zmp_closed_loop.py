"""A fleet in closed loop with the ZMP force distributor: five Talos-like robots in double support, window 2, twelve ticks; each tick
observe_acom -> stabilize_zmp -> latch -> tick_mixed over two slots of one contact set (default force-regularisation weights, zmp_w), all on the device.
Synthetic foot wrenches load the robots' feet from different ticks on, so their CoPs become valid, the law runs and they move to the zmp_w slot at
different ticks; one robot's feet never carry anything and it stays in the default slot.  Yardstick: the same loop on the CPU (tests/force_ref_cases.py:
transcription, oracle rows with b1 patched by the product w_f * f_ref, oracle solve, integration), tick by tick under assert_parity's bars."""
import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import stabilizer as stb
from tests import force_ref_cases as fc
from tests.test_gpu_stabilize import ROT_BAR
from tests.util import assert_parity, device_outputs, host_outputs

pytestmark = pytest.mark.gpu


def test_robots_latch_at_their_own_ticks_and_the_loop_follows_the_cpu_loop():
    import torch
    dev = torch.device("cuda", 0)
    want = fc.closed_loop_reference()
    L = want["setup"]
    m, tm, stab, z, (st_d, st_z) = L["m"], L["tm"], L["stab"], L["zmp"], L["sts"]
    B, T = fc.LOOP_B, fc.LOOP_TICKS
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    h = capi.Handle(0, capi.F64)
    try:
        for slot, st in enumerate((st_d, st_z)):
            h.set_structure(slot, st)
            h.set_model(slot, m, tm)
            h.set_force_references(slot, tm.contact_fref, fc.weights_of(st))
        h.set_observed_frames(0, L["frames"])
        q, v, ref = up(L["states"]["q"]), up(L["states"]["v"]), up(L["states"]["ref"])
        assert (L["states"]["ref"][:, tm.contact_fref[0]:] == 0).all()  # the base row holds zeros in the force blocks: what "put the references back" restores
        wrench, w, tlb, tub = up(L["wrench"]), [up(a) for a in L["w"]], up(L["tlb"]), up(L["tub"])
        com, acom, place = (torch.zeros(B, n, dtype=torch.float64, device=dev) for n in (3, 3, 24))
        ref_out, flags = torch.zeros_like(ref), torch.zeros(B, dtype=torch.int32, device=dev)
        alpha = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        state = torch.zeros(B, stb.state_bytes(stab.window), dtype=torch.uint8, device=dev)
        latch, x_prev, latched_at = stb.ZmpLatch(B), None, [-1] * B
        stream = torch.cuda.current_stream().cuda_stream
        rot = stb.rotation_entries(stab)
        plain = np.setdiff1d(np.arange(stab.nref), rot)
        for t in range(T):
            h.observe(0, B, q, v, com=com, placement=place, acom=acom, stream=stream)
            h.stabilize_zmp(stab, z, B, ref, wrench[t], com, acom, place, x_prev=x_prev, state=state, ref_out=ref_out, flags=flags, alpha=alpha, stream=stream)
            before = latch.latched.copy()
            which = latch.update(flags.cpu().numpy()).astype(np.int32)  # (the copy waits for the stream)
            for i in np.nonzero(latch.latched & ~before)[0]:
                latched_at[i] = t
            out = device_outputs(B, st_d, dev)
            qn, vn = torch.zeros_like(q), torch.zeros_like(v)
            h.tick_mixed([0, 1], which, dict(q=q, v=v, ref=ref_out), w, out, qn, vn, tm.dt, tlb=tlb, tub=tub, stream=stream)
            torch.cuda.synchronize()
            c = want["ticks"][t]
            assert np.array_equal(flags.cpu().numpy(), c["flags"]) and np.array_equal(which, c["which"]), (t, flags.cpu().numpy(), c["flags"])
            # the stabilised row: the two loops' states differ by the solver's rounding (bounded below), so the row is compared under the same bar
            r = ref_out.cpu().numpy()
            scale = np.maximum(1.0, np.abs(c["ref_out"]))
            assert (np.abs(r - c["ref_out"]) / scale).max() <= 1e-8, (t, float((np.abs(r - c["ref_out"]) / scale).max()))
            assert np.array_equal(np.isnan(alpha.cpu().numpy()), np.isnan(c["alpha"])) and np.nanmax(np.abs(alpha.cpu().numpy() - c["alpha"]), initial=0.0) <= 1e-8
            got = host_outputs(out, st_d)
            assert (got["status"] == 0).all(), (t, got["status"])
            for k, st in enumerate((st_d, st_z)):
                idx = np.nonzero(which == k)[0]
                if idx.size:
                    assert_parity(st, {f: got[f][idx] for f in ("x", "tau", "status", "iters")}, {f: c[f][idx] for f in ("x", "tau", "status", "iters")},
                                  what="closed loop with the ZMP distributor, tick %d slot %d" % (t, k), active=False)  # (active sets: the loops' states differ in the last bits)
            assert np.abs(qn.cpu().numpy() - c["q"]).max() <= 1e-8 and np.abs(vn.cpu().numpy() - c["v"]).max() <= 1e-6, (t, np.abs(qn.cpu().numpy() - c["q"]).max(), np.abs(vn.cpu().numpy() - c["v"]).max())
            q, v, x_prev = qn, vn, out["x"]
        assert latched_at == fc.LOOP_LATCH_AT == want["latched_at"], latched_at
        assert len({a for a in latched_at if a >= 0}) == 4 and not latch.latched[4]  # four different ticks; the robot whose CoP never becomes valid stays
        # once latched, for good: the last tick's slots
        assert list(which) == [1, 1, 1, 1, 0]
        fl = want["ticks"][-1]["flags"]
        assert (fl[:4] & stb.ZMP).all() and fl[4] == 0 and ROT_BAR < 1e-8
    finally:
        h.close()
