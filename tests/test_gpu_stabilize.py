"""GPU tests of the stabiliser (wbcqp_stabilize, stabilize_kernel) against the transcription of the reference's CoP estimator, filters and admittance
laws, inria_wbc_amd/stabilizer.py, and of wbcqp_observe_acom against observe.py.

Parity: windows (1, 2, 7, 64) x batches (1, 3, 5, 67) on the Talos map's reference rows and on the smallest shape, a stream of 3 window + 5 ticks, one
call per tick with the state carried on the device.  The transcription runs once per (shape, window) on the largest batch -- an instance's results depend
on its own rows alone, so a smaller batch is its first instances -- and asserts on the CPU that the streams decide every comparison clearly and reach
every branch (tests/stabilizer_cases.py).  F64: flags, the state at every tick, the CoPs (NaN where not valid) and every element of ref_out that is not
a rotation entry are the transcription's bit for bit; the rotation entries (through atan2 / sin / cos, where the device's libm and the host's differ by
a few ulp of values <= pi) lie within ROT_BAR."""
import ctypes as C

import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import model as mdl
from inria_wbc_amd import observe as obs
from inria_wbc_amd import stabilizer as stb
from tests import model_queries as mq
from tests import stabilizer_cases as sc

pytestmark = pytest.mark.gpu

BATCHES = mq.BATCHES  # 1, 3, 5, 67
# Largest |device - transcription| over the rotation entries of the whole parity grid, measured on an MI355X: see profiles/stabilizer/INDEX.md.
# The bar is four times that, and never above 1e-13 (beyond which something other than rounding is wrong).
ROT_MEASURED = 8.9e-16
ROT_BAR = min(4 * ROT_MEASURED, 1e-13)
SHAPES = {"talos": sc.talos_stab, "tree": sc.tree_stab, "mini": sc.mini_stab}
_REFERENCE = {}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def handle(built_lib):
    yield from mq.open_handle()


def reference(shape, window):
    """(stabiliser, inputs per tick, the transcription's outputs per tick, its state after each tick), computed once per (shape, window)."""
    key = (shape, window)
    if key not in _REFERENCE:
        s = SHAPES[shape](window)
        ticks = sc.streams(s, 31_000 + window)
        _REFERENCE[key] = (s, ticks) + sc.reference_run(s, ticks)
    return _REFERENCE[key]


def upload(ticks, lo, hi, td=None):
    """The stream's inputs for instances lo .. hi - 1 as device tensors [T, B, .] (x_prev: tick 0's row is unused)."""
    torch, dev = _torch()
    td = td or torch.float64
    x0 = np.zeros_like(ticks[1]["x_prev"])
    stack = lambda k: np.stack([(t[k] if t[k] is not None else x0)[lo:hi] for t in ticks])  # noqa: E731
    return {k: torch.from_numpy(stack(k)).to(dev).to(td).contiguous() for k in capi.STAB_INPUTS}


def run_stream(h, s, d, t0, t1, state=None, in_place=False):
    """Ticks t0 .. t1 - 1 of the uploaded stream d, one call per tick, the state (a device uint8 tensor [B, bytes], or None: zeros) carried on the device.
    -> dict(ref_out [T, B, nref], flags [T, B], cop [T, B, 3, 2], state [T, B, bytes]) as numpy arrays, and the state tensor."""
    torch, dev = _torch()
    T, B = t1 - t0, d["ref"].shape[1]
    td = d["ref"].dtype
    if state is None:
        state = torch.zeros(B, stb.state_bytes(s.window), dtype=torch.uint8, device=dev)
    out = dict(ref_out=torch.full((T, B, s.nref), float("nan"), dtype=td, device=dev), flags=torch.full((T, B), mq.UNSET, dtype=torch.int32, device=dev),
               cop=torch.zeros(T, B, 3, 2, dtype=td, device=dev), state=torch.zeros((T,) + tuple(state.shape), dtype=torch.uint8, device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    for k, t in enumerate(range(t0, t1)):
        ref_out = out["ref_out"][k]
        if in_place:
            ref_out.copy_(d["ref"][t])
        h.stabilize(s, B, ref_out if in_place else d["ref"][t], d["wrench"][t], d["com"][t], d["acom"][t], d["placement"][t],
                    x_prev=d["x_prev"][t] if t > 0 else None, state=state, ref_out=ref_out, flags=out["flags"][k], cop=out["cop"][k], stream=stream)
        out["state"][k].copy_(state)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, state


def same(a, b, what=""):
    """Two results of run_stream agree in every bit (NaNs of the CoP in the same places)."""
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=(k == "cop")), (what, k)


# ---- parity with the transcription ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", sc.WINDOWS)
@pytest.mark.parametrize("shape", ["talos", "tree"])
def test_parity_with_the_transcription(handle, shape, window):
    s, ticks, outs, states = reference(shape, window)
    T = len(ticks)
    want = dict(ref_out=np.stack([o["ref_out"] for o in outs]), flags=np.stack([o["flags"] for o in outs]), cop=np.stack([o["cop"] for o in outs]),
                state=np.stack(states))
    rot = stb.rotation_entries(s)
    plain = np.setdiff1d(np.arange(s.nref), rot)
    worst = 0.0
    for B in BATCHES[::-1]:
        got, _ = run_stream(handle, s, upload(ticks, 0, B), 0, T)
        assert np.array_equal(got["flags"], want["flags"][:, :B]), (shape, window, B)
        for t in range(T):
            assert sc.states_equal(got["state"][t], want["state"][t][:B]), (shape, window, B, t)
        assert np.array_equal(got["cop"], want["cop"][:, :B], equal_nan=True), (shape, window, B)
        assert sc.bits(got["ref_out"][:, :, plain]) == sc.bits(want["ref_out"][:, :B][:, :, plain]), (shape, window, B)
        diff = float(np.abs(got["ref_out"][:, :, rot] - want["ref_out"][:, :B][:, :, rot]).max())
        worst = max(worst, diff)
        assert diff <= ROT_BAR, (shape, window, B, diff)
    print("stabilize parity, %s window %d: rotation entries differ by at most %.2e (bar %.1e)" % (shape, window, worst, ROT_BAR))


# ---- a stream is a stream however it is cut ---------------------------------------------------------------------------------------------------
def test_a_stream_cut_into_two_handles_gives_the_bits_of_one_run(handle):
    torch, dev = _torch()
    s, ticks, _, _ = reference("mini", 7)
    T, B = len(ticks), 5
    d = upload(ticks, 3, 3 + B)  # (instances past the three fixed roles)
    whole, _ = run_stream(handle, s, d, 0, T)
    other = capi.Handle(0, capi.F64)
    try:
        for cut in range(1, T):  # at every tick
            first, state = run_stream(handle, s, d, 0, cut)
            carried = torch.from_numpy(state.cpu().numpy().copy()).to(dev)  # through the host
            second, _ = run_stream(other, s, d, cut, T, state=carried)
            same({k: np.concatenate([first[k], second[k]]) for k in whole}, whole, cut)
    finally:
        other.close()
    # no state at all is a fresh one: the first tick's outputs, nothing kept
    stream = torch.cuda.current_stream().cuda_stream
    ref_out, flags = torch.zeros(B, s.nref, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    cop = torch.zeros(B, 3, 2, dtype=torch.float64, device=dev)
    handle.stabilize(s, B, d["ref"][0], d["wrench"][0], d["com"][0], d["acom"][0], d["placement"][0], ref_out=ref_out, flags=flags, cop=cop, stream=stream)
    torch.cuda.synchronize()
    same(dict(ref_out=ref_out.cpu().numpy(), flags=flags.cpu().numpy(), cop=cop.cpu().numpy()), {k: whole[k][0] for k in ("ref_out", "flags", "cop")})


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    s, ticks, _, states = reference("talos", 7)
    t = 10  # mid-stream: every filter holds samples, the transcription's state of the tick before is the input (parity: it is the device's)
    d = upload(ticks, 0, sc.NMAX)

    def run(lo, hi):
        part = {k: v[:, lo:hi].contiguous() for k, v in d.items()}
        got, _ = run_stream(handle, s, part, t, t + 1, state=torch.from_numpy(states[t - 1][lo:hi].copy()).to(dev))
        return dict(ref_out=got["ref_out"][0], flags=got["flags"][0], cop=got["cop"][0].view(np.int64), state=got["state"][0])  # (NaNs as their bits)

    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(run, sc.NMAX)
    assert a["flags"].any() and np.isnan(a["cop"].view(np.float64)).any()


def test_outputs_are_written_whole_and_nothing_behind_them(handle):
    torch, dev = _torch()
    s = sc.mini_stab(1)
    B = 5
    inp = sc.balanced(s, B)
    inp["wrench"][:, 4] = -25.0 * np.arange(B)  # each instance's CoP somewhere else
    d = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    nst = B * stb.state_bytes(1) // 8
    bufs = dict(ref_out=mq.guarded(B * s.nref, torch.float64, dev, torch), flags=mq.guarded(B, torch.int32, dev, torch), cop=mq.guarded(B * 6, torch.float64, dev, torch),
                state=mq.guarded(nst, torch.float64, dev, torch))
    bufs["state"][1].zero_()
    handle.stabilize(s, B, d["ref"], d["wrench"], d["com"], d["acom"], d["placement"], x_prev=d["x_prev"], state=bufs["state"][1], ref_out=bufs["ref_out"][1],
                     flags=bufs["flags"][1], cop=bufs["cop"][1], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {k: mq.read_guarded(w, p.numel(), k) for k, (w, p) in bufs.items()}
    st = np.zeros((B, stb.state_bytes(1)), np.uint8)
    want = stb.step(s, st, inp)
    rot = stb.rotation_entries(s)
    plain = np.setdiff1d(np.arange(s.nref), rot)
    assert np.array_equal(got["flags"], want["flags"]) and (want["flags"] == 127).all() and np.array_equal(got["cop"].reshape(B, 3, 2), want["cop"])
    assert sc.bits(got["ref_out"].reshape(B, -1)[:, plain]) == sc.bits(want["ref_out"][:, plain]) and sc.bits(got["state"]) == sc.bits(st)
    assert np.abs(got["ref_out"].reshape(B, -1)[:, rot] - want["ref_out"][:, rot]).max() <= ROT_BAR
    # the balanced instance comes back as it went in, identity rotations included
    assert sc.bits(got["ref_out"].reshape(B, -1)[0]) == sc.bits(inp["ref"][0])


def test_in_place_equals_out_of_place_and_the_host_twin_has_the_same_bits(handle):
    s, ticks, _, _ = reference("talos", 2)
    T, B = len(ticks), 5
    d = upload(ticks, 0, B)
    apart, _ = run_stream(handle, s, d, 0, T)
    same(run_stream(handle, s, d, 0, T, in_place=True)[0], apart, "in place")
    state = np.zeros((B, stb.state_bytes(2)), np.uint8)
    for t, inp in enumerate(ticks):
        got = handle.stabilize_host(s, {k: (v[:B] if v is not None else None) for k, v in inp.items()}, state)
        same(dict(got, state=state), {k: apart[k][t] for k in apart}, ("host", t))
    # the host twin without a state, and asked for one output only
    only = handle.stabilize_host(s, {k: (v[:B] if v is not None else None) for k, v in ticks[0].items()}, None, outputs=("flags",))
    assert set(only) == {"flags"} and np.array_equal(only["flags"], apart["flags"][0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
class _Struct:
    """A host struct handed to both entry points as a pointer (what tests/model_queries.py asks of an argument: .ctypes.data / .data_ptr())."""

    def __init__(self, c, cls):
        p = C.pointer(c) if c is not None else C.POINTER(cls)()
        self.ctypes = type("ctypes", (), {"data": p})
        self.data_ptr = lambda: p
        self._keep = c


def test_refusals_match_between_the_entry_points_and_launch_nothing(handle):
    s = sc.mini_stab(3)
    B = 2
    inp = {k: mq.both(v) for k, v in sc.balanced(s, B).items()}
    out = dict(ref_out=mq.prefilled_both(B * s.nref), flags=mq.prefilled_both(B, int32=True), cop=mq.prefilled_both(B * 6))
    state = mq.prefilled_both(B * stb.state_bytes(3) // 8)
    O = mq.Out(capi.CStabOutputs, **out)
    ldp, ldx = 24, 30

    def I(ldp_=ldp, ldx_=ldx, **drop):
        m = dict(inp, ldp=ldp_, ldx=ldx_)
        m.update(drop)
        return mq.Out(capi.CStabInputs, **m)

    def S(**kw):
        return _Struct(capi.c_stabilizer(sc.mini_stab(**{"window": 3, **kw})), capi.CStabilizer)

    bad_stab = [dict(window=0), dict(window=65), dict(dt=0.0), dict(dt=-1.0), dict(dt=np.nan), dict(dt=np.inf), dict(mass=0.0), dict(mass=-2.0), dict(mass=np.inf),
                dict(com_gains=(0, np.nan, 0, 0, 0, 0)), dict(ankle_gains=(0, 0, 0, 0, 0, np.inf)), dict(ffda_gains=(np.nan, 0, 0)), dict(normal=(np.nan, 0, 1)),
                dict(com_ref=-1), dict(lf_ref=-1), dict(rf_ref=-1), dict(torso_ref=-1), dict(lf_pos=-1), dict(rf_pos=-1), dict(lf_contact_ref=-2),
                dict(lf_force_col=-2), dict(nref=128), dict(com_ref=121), dict(lf_ref=106), dict(rf_contact_ref=106), dict(rf_ref=20)]
    cases = [(S(**kw), B, I(), state, O) for kw in bad_stab]
    cases += [(_Struct(None, capi.CStabilizer), B, I(), state, O), (S(), B, None, state, O), (S(), -1, I(), state, O)]
    cases += [(S(), B, I(**{k: None}), state, O) for k in ("ref", "wrench", "com", "acom", "placement")]
    cases += [(S(), B, I(ldp_=23), state, O), (S(lf_pos=22), B, I(), state, O), (S(), B, I(ldx_=29), state, O), (S(rf_force_col=19), B, I(), state, O)]
    mq.host_refusals_match(handle, "stabilize", cases, list(out.values()) + [state])
    # accepted with nothing to do: batch == 0 (nothing is looked at beyond the checks); every output NULL and no state
    none = mq.Out(capi.CStabOutputs)
    mq.host_batch_zero(handle, "stabilize", [(S(), 0, I(), state, O), (S(), B, I(), None, none), (S(), B, I(), None, None)], list(out.values()) + [state])
    for args in [(S(), 0, I(), state, O), (S(), B, I(), None, none), (S(), B, I(), None, None)]:
        mq.raw(handle, "stabilize", 0, *args)
    mq._all_unwritten(list(out.values()) + [state], "a call with nothing to do wrote something")
    # accepted: a short ldx without x_prev; an inactive contact with a column of -1
    mq.raw(handle, "stabilize", 1, S(), B, I(ldx_=0, x_prev=None), None, mq.Out(capi.CStabOutputs, flags=out["flags"]))
    mq.raw(handle, "stabilize", 1, S(lf_force_col=-1, rf_force_col=-1), B, I(ldx_=0), None, mq.Out(capi.CStabOutputs, flags=out["flags"]))
    assert not mq.unwritten(out["flags"][1]).any()


# ---- a float handle ---------------------------------------------------------------------------------------------------------------------------
def test_a_float_handle_reads_float_computes_in_double_writes_float():
    torch, _ = _torch()
    s = sc.mini_stab(2)
    ticks = sc.streams(s, 33_000)
    B, T = 8, len(ticks)
    as_float = [{k: (v[:B].astype(np.float32).astype(np.float64) if v is not None else None) for k, v in t.items()} for t in ticks]
    state, margins, want = np.zeros((B, stb.state_bytes(2)), np.uint8), [], []
    for t in as_float:  # the transcription on what a float handle reads
        want.append(stb.step(s, state, t, margins))
    stb.clear_margin(margins, 1e-9)  # (the handle computes in double on exactly these inputs: its decisions are the transcription's)
    h32 = capi.Handle(0, capi.F32)
    try:
        got, st = run_stream(h32, s, upload(as_float, 0, B, torch.float32), 0, T)
    finally:
        h32.close()
    assert got["ref_out"].dtype == np.float32 and got["cop"].dtype == np.float32
    assert np.array_equal(got["flags"], np.stack([w["flags"] for w in want])) and sc.states_equal(got["state"][-1], state)
    for k in ("ref_out", "cop"):
        w = np.stack([x[k] for x in want])
        ulp = float(np.spacing(np.float32(np.nanmax(np.abs(w)))))
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        assert np.nanmax(np.abs(got[k].astype(np.float64) - w.astype(np.float32).astype(np.float64))) <= ulp, (k, ulp)


# ---- nothing else moves -----------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(handle):
    m, st, tm = mq.talos_case()
    s = stb.from_taskmap(m, tm, mdl.talos_stack(), 4, sc.COM_GAINS, sc.ANKLE_GAINS, sc.FFDA_GAINS)
    ankles = obs.frame_ids(m, ["leg_left_6_joint", "leg_right_6_joint"])

    def query(states, tick):
        o = handle.observe_host(3, states["q"], states["v"], acom=True)
        B = states["q"].shape[0]
        wrench = np.tile([3.0, -2.0, 420.0, 1.0, 5.0, 0.5, -4.0, 1.0, 380.0, -2.0, 3.0, 0.1], (B, 1))
        inp = dict(ref=states["ref"], wrench=wrench, com=o["com"], acom=o["acom"], placement=o["placement"].reshape(B, -1), x_prev=tick["x"])
        state = np.zeros((B, stb.state_bytes(4)), np.uint8)
        for _ in range(5):
            got = handle.stabilize_host(s, inp, state)
        assert (got["flags"] == 127).all() and not np.array_equal(got["ref_out"], states["ref"])

    mq.nothing_else_moves(handle, (m, st, tm), 79_000, query, observed=ankles)


# ---- acom -------------------------------------------------------------------------------------------------------------------------------------
def test_observe_acom_against_the_numpy_statement_and_the_other_outputs_keep_their_bits(handle):
    torch, dev = _torch()
    for name, case in (("talos", mq.talos_case), ("tree", mq.tree_case("stab_", 6, 24, True)), ("chain", mq.tree_case("stabc_", 8, 9, False, "chain"))):
        m, st, tm = case()
        handle.set_structure(3, st)
        handle.set_model(3, m, tm)
        handle.set_observed_frames(3, [0, 1])
        B = 67
        s = mdl.sample_states(m, tm, B, 81_000, q_noise=0.2, v_noise=0.5)
        want = obs.observe(m, s["q"], s["v"], [0, 1], acom=True)
        q, v = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["v"]).to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        n = dict(com=B * 3, vcom=B * 3, placement=B * 24, velocity=B * 12, acom=B * 3)

        def launch(which, batch=B):
            bufs = {k: mq.guarded(n[k] * batch // B, torch.float64, dev, torch) for k in which}
            handle.observe(3, batch, q[:batch].contiguous(), v[:batch].contiguous(), stream=stream, **{k: p for k, (_, p) in bufs.items()})
            torch.cuda.synchronize()
            return {k: mq.read_guarded(w, p.numel(), k) for k, (w, p) in bufs.items()}

        without, with_acom, alone = launch(capi.OBSERVABLES), launch(capi.OBSERVABLES + ("acom",)), launch(("acom",))
        for k in capi.OBSERVABLES:
            assert np.array_equal(without[k], with_acom[k]), (name, k)
        assert np.array_equal(alone["acom"], with_acom["acom"]) and np.array_equal(launch(("acom",), 5)["acom"], alone["acom"][:15])
        err = np.abs(with_acom["acom"].reshape(B, 3) - want["acom"]).max() / max(1.0, np.abs(want["acom"]).max())
        print("acom on the device against observe.py, %s: %.1e (largest entry %.2f)" % (name, err, np.abs(want["acom"]).max()))
        assert err <= 1e-10 and np.abs(want["acom"]).max() > 0.01
        host = handle.observe_host(3, s["q"], s["v"], acom=True)
        assert np.array_equal(host["acom"].reshape(-1), alone["acom"]) and "acom" not in handle.observe_host(3, s["q"], s["v"])
        buf = torch.full((B * 3,), float("nan"), dtype=torch.float64, device=dev)
        msg = mq.refused(handle, lambda: handle.observe(3, B, q, None, acom=buf, stream=stream))
        assert "acom" in msg and mq.unwritten(buf.cpu().numpy()).all()
