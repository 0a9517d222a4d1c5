"""GPU tests of the stabiliser with the ZMP force distributor (wbcqp_stabilize_zmp, the second instantiation of stabilize_kernel) against the
transcription, inria_wbc_amd/stabilizer.py step(zmp=...).

Parity: shapes talos and mini (both feet) and mini with one foot only, windows (1, 7) x batches (1, 5, 67), the streams of tests/zmp_cases.py
(3 window + 5 ticks, one call per tick, the state carried on the device).  The transcription runs once per (shape, window) and asserts on the CPU that
every branch is reached and every comparison is decided clearly.  F64: flags, the state at every tick, the CoPs, alpha, the two force-reference blocks
and every other entry of ref_out that is not a rotation entry are the transcription's bit for bit (a NaN is a NaN: its sign and payload are the
processor's); the rotation entries lie within test_gpu_stabilize's ROT_BAR."""
import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import stabilizer as stb
from tests import model_queries as mq
from tests import stabilizer_cases as sc
from tests import zmp_cases as zc
from tests.test_gpu_stabilize import ROT_BAR, _Struct, upload

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def handle(built_lib):
    yield from mq.open_handle()


def reference(shape, window):
    key = (shape, window)
    if key not in _REFERENCE:
        s, z = zc.SHAPES[shape](window)
        ticks = zc.streams(s, z, zc.seed_of(shape, window))
        _REFERENCE[key] = (s, z, ticks) + zc.reference_run(s, z, ticks)
    return _REFERENCE[key]


def run_stream(h, s, z, d, t0, t1, state=None, in_place=False, plain=False):
    """Ticks t0 .. t1 - 1 of the uploaded stream, one call per tick, the state carried on the device.  plain: through wbcqp_stabilize (no alpha)."""
    torch, dev = _torch()
    T, B = t1 - t0, d["ref"].shape[1]
    td = d["ref"].dtype
    if state is None:
        state = torch.zeros(B, stb.state_bytes(s.window), dtype=torch.uint8, device=dev)
    out = dict(ref_out=torch.full((T, B, s.nref), float("nan"), dtype=td, device=dev), flags=torch.full((T, B), mq.UNSET, dtype=torch.int32, device=dev),
               cop=torch.zeros(T, B, 3, 2, dtype=td, device=dev), alpha=torch.zeros(T, B, 2, dtype=td, device=dev),
               state=torch.zeros((T,) + tuple(state.shape), dtype=torch.uint8, device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    for k, t in enumerate(range(t0, t1)):
        ref_out = out["ref_out"][k]
        if in_place:
            ref_out.copy_(d["ref"][t])
        args = (B, ref_out if in_place else d["ref"][t], d["wrench"][t], d["com"][t], d["acom"][t], d["placement"][t])
        kw = dict(x_prev=d["x_prev"][t] if t > 0 else None, state=state, ref_out=ref_out, flags=out["flags"][k], cop=out["cop"][k], stream=stream)
        if plain:
            h.stabilize(s, *args, **kw)
        else:
            h.stabilize_zmp(s, z, *args, alpha=out["alpha"][k], **kw)
        out["state"][k].copy_(state)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not (plain and k == "alpha")}, state


def nan_blind_bits(a):
    """The bytes of a float array with every NaN made the same NaN."""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def same(a, b, what=""):
    for k in a:
        if k == "state":
            assert all(sc.states_equal(x, y) for x, y in zip(a[k], b[k])), (what, k)
        elif k == "flags":
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert nan_blind_bits(a[k]) == nan_blind_bits(b[k]), (what, k)


# ---- parity with the transcription ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", zc.WINDOWS)
@pytest.mark.parametrize("shape", list(zc.SHAPES))
def test_parity_with_the_transcription(handle, shape, window):
    s, z, ticks, outs, states = reference(shape, window)
    T = len(ticks)
    want = {k: np.stack([o[k] for o in outs]) for k in ("ref_out", "flags", "cop", "alpha")}
    want["state"] = np.stack(states)
    rot = stb.rotation_entries(s)
    plain = np.setdiff1d(np.arange(s.nref), rot)
    blocks = np.concatenate([np.arange(o, o + 6) for o in (z.lf_force_ref, z.rf_force_ref)])
    assert np.isin(blocks, plain).all()
    worst = 0.0
    for B in zc.BATCHES[::-1]:
        got, _ = run_stream(handle, s, z, upload(ticks, 0, B), 0, T)
        assert np.array_equal(got["flags"], want["flags"][:, :B]), (shape, window, B)
        for t in range(T):
            assert sc.states_equal(got["state"][t], want["state"][t][:B]), (shape, window, B, t)
        assert np.array_equal(got["cop"], want["cop"][:, :B], equal_nan=True), (shape, window, B)
        assert nan_blind_bits(got["alpha"]) == nan_blind_bits(want["alpha"][:, :B]), (shape, window, B)
        assert nan_blind_bits(got["ref_out"][:, :, blocks]) == nan_blind_bits(want["ref_out"][:, :B][:, :, blocks]), (shape, window, B, "force references")
        assert nan_blind_bits(got["ref_out"][:, :, plain]) == nan_blind_bits(want["ref_out"][:, :B][:, :, plain]), (shape, window, B)
        diff = float(np.nanmax(np.abs(got["ref_out"][:, :, rot] - want["ref_out"][:, :B][:, :, rot])))
        assert np.array_equal(np.isnan(got["ref_out"][:, :, rot]), np.isnan(want["ref_out"][:, :B][:, :, rot]))
        worst = max(worst, diff)
        assert diff <= ROT_BAR, (shape, window, B, diff)
    print("stabilize_zmp parity, %s window %d: force references bit for bit; rotation entries differ by at most %.2e (bar %.1e)" % (shape, window, worst, ROT_BAR))


# ---- bit identities ----------------------------------------------------------------------------------------------------------------------------
def test_no_distributor_is_wbcqp_stabilize_and_offsets_of_minus_one_add_the_flag_only(handle):
    s, z, ticks, outs, _ = reference("talos", 7)
    T, B = len(ticks), 5
    d = upload(ticks, 3, 3 + B)
    base, _ = run_stream(handle, s, z, d, 0, T, plain=True)
    none, _ = run_stream(handle, s, None, d, 0, T)  # zmp = NULL
    assert (none.pop("alpha") == 0).all()  # (the buffer's fill: without a distributor nothing writes alpha)
    same(none, base, "zmp NULL")
    off = stb.ZmpDistributor(z.p, z.d, -1, -1)
    got, _ = run_stream(handle, s, off, d, 0, T)
    ran = (got["flags"] & stb.ZMP) != 0
    want_ran = np.stack([o["flags"][3:3 + B] for o in outs]) & stb.ZMP != 0
    assert ran.any() and np.array_equal(ran, want_ran)
    clean = (np.stack([o["flags"][3:3 + B] for o in outs]) & stb.ERR_ZMP) == 0  # (instance 4's NaN com ends its tick with ERR_ZMP: wbcqp_stabilize knows no such guard)
    assert np.array_equal((got["flags"] & ~stb.ZMP)[clean], base["flags"][clean])
    assert nan_blind_bits(got["ref_out"][clean]) == nan_blind_bits(base["ref_out"][clean]) and np.array_equal(got["cop"], base["cop"], equal_nan=True)
    assert all(sc.states_equal(x, y) for x, y in zip(got["state"], base["state"]))
    assert not np.isnan(got["alpha"][ran]).any() and np.isnan(got["alpha"][~ran]).all()


def test_in_place_equals_out_of_place_and_the_host_twin_has_the_same_bits(handle):
    s, z, ticks, _, _ = reference("talos", 1)
    T, B = len(ticks), 5
    d = upload(ticks, 0, B)
    apart, _ = run_stream(handle, s, z, d, 0, T)
    same(run_stream(handle, s, z, d, 0, T, in_place=True)[0], apart, "in place")
    state = np.zeros((B, stb.state_bytes(1)), np.uint8)
    for t, inp in enumerate(ticks):
        got = handle.stabilize_zmp_host(s, z, {k: (v[:B] if v is not None else None) for k, v in inp.items()}, state)
        same(dict(got, state=state[None]), {k: (apart[k][t] if k != "state" else apart[k][t][None]) for k in apart}, ("host", t))
    only = handle.stabilize_zmp_host(s, z, {k: (v[:B] if v is not None else None) for k, v in ticks[0].items()}, None, outputs=("alpha",))
    assert set(only) == {"alpha"} and nan_blind_bits(only["alpha"]) == nan_blind_bits(apart["alpha"][0])
    plain = handle.stabilize_zmp_host(s, None, {k: (v[:B] if v is not None else None) for k, v in ticks[0].items()}, None, outputs=capi.STAB_OUTPUTS)
    want = handle.stabilize_host(s, {k: (v[:B] if v is not None else None) for k, v in ticks[0].items()}, None)
    same(plain, want, "host twin without a distributor")


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    torch, dev = _torch()
    s, z, ticks, _, states = reference("talos", 7)
    t = 10
    d = upload(ticks, 0, sc.NMAX)

    def run(lo, hi):
        part = {k: v[:, lo:hi].contiguous() for k, v in d.items()}
        got, _ = run_stream(handle, s, z, part, t, t + 1, state=torch.from_numpy(states[t - 1][lo:hi].copy()).to(dev))
        return dict(ref_out=got["ref_out"][0].view(np.int64), flags=got["flags"][0], cop=got["cop"][0].view(np.int64), alpha=got["alpha"][0].view(np.int64),
                    state=got["state"][0])  # (floats as their bits: NaNs included)

    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(run, sc.NMAX)
    assert (a["flags"] & stb.ZMP).any() and np.isnan(a["alpha"].view(np.float64)).any()


def test_outputs_are_written_whole_and_nothing_behind_them(handle):
    torch, dev = _torch()
    s, z = zc.mini(1)
    B = 5
    inp = sc.balanced(s, B)
    inp["wrench"][:, 4] = -25.0 * np.arange(B)  # each instance's CoP somewhere else
    inp["ref"][:, 129:141] = 7.0
    d = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    nst = B * stb.state_bytes(1) // 8
    bufs = dict(ref_out=mq.guarded(B * s.nref, torch.float64, dev, torch), flags=mq.guarded(B, torch.int32, dev, torch), cop=mq.guarded(B * 6, torch.float64, dev, torch),
                alpha=mq.guarded(B * 2, torch.float64, dev, torch), state=mq.guarded(nst, torch.float64, dev, torch))
    bufs["state"][1].zero_()
    handle.stabilize_zmp(s, z, B, d["ref"], d["wrench"], d["com"], d["acom"], d["placement"], x_prev=d["x_prev"], state=bufs["state"][1], ref_out=bufs["ref_out"][1],
                         flags=bufs["flags"][1], cop=bufs["cop"][1], alpha=bufs["alpha"][1], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {k: mq.read_guarded(w, p.numel(), k) for k, (w, p) in bufs.items()}
    st = np.zeros((B, stb.state_bytes(1)), np.uint8)
    want = stb.step(s, st, inp, zmp=z)
    rot = stb.rotation_entries(s)
    plain = np.setdiff1d(np.arange(s.nref), rot)
    assert np.array_equal(got["flags"], want["flags"]) and (want["flags"] == 127 | stb.ZMP).all() and np.array_equal(got["cop"].reshape(B, 3, 2), want["cop"])
    assert sc.bits(got["alpha"].reshape(B, 2)) == sc.bits(want["alpha"]) and sc.bits(got["state"]) == sc.bits(st)
    assert sc.bits(got["ref_out"].reshape(B, -1)[:, plain]) == sc.bits(want["ref_out"][:, plain]) and not (got["ref_out"].reshape(B, -1)[:, 129:141] == 7.0).all(axis=1).any()
    assert np.abs(got["ref_out"].reshape(B, -1)[:, rot] - want["ref_out"][:, rot]).max() <= ROT_BAR


# ---- a float handle ---------------------------------------------------------------------------------------------------------------------------
def test_a_float_handle_reads_float_computes_in_double_writes_float():
    torch, _ = _torch()
    s, z = zc.mini(7)
    ticks = zc.streams(s, z, 43_000)
    B, T = 8, len(ticks)
    as_float = [{k: (v[:B].astype(np.float32).astype(np.float64) if v is not None else None) for k, v in t.items()} for t in ticks]
    state, margins, zm, want = np.zeros((B, stb.state_bytes(7)), np.uint8), [], [], []
    for t in as_float:  # the transcription on what a float handle reads
        want.append(stb.step(s, state, t, margins, zmp=z, zmp_margins=zm))
    stb.clear_margin(margins, 1e-9)
    zc.check_zmp_margins(zm, s.mass)  # (the handle computes in double on exactly these inputs: its decisions are the transcription's)
    h32 = capi.Handle(0, capi.F32)
    try:
        got, _ = run_stream(h32, s, z, upload(as_float, 0, B, torch.float32), 0, T)
    finally:
        h32.close()
    assert got["ref_out"].dtype == np.float32 and got["alpha"].dtype == np.float32
    flags = np.stack([w["flags"] for w in want])
    assert np.array_equal(got["flags"], flags) and (flags & stb.ZMP).any() and sc.states_equal(got["state"][-1], state)
    for k in ("ref_out", "cop", "alpha"):
        w = np.stack([x[k] for x in want])
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        # what the handle writes is the double result rounded to float: one float ulp of the entry at the most (rotation entries: the libm's few double ulp vanish in it)
        r = w.astype(np.float32)
        bad = ~np.isnan(w) & (np.abs(got[k].astype(np.float64) - r.astype(np.float64)) > np.spacing(np.abs(r)).astype(np.float64))
        assert not bad.any(), (k, int(bad.sum()))
    blocks = np.concatenate([np.arange(129, 135), np.arange(135, 141)])
    w = np.stack([x["ref_out"] for x in want])[:, :, blocks]
    assert nan_blind_bits(got["ref_out"][:, :, blocks]) == nan_blind_bits(w.astype(np.float32))  # the force references: exactly the rounded doubles


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_match_between_the_entry_points_and_launch_nothing(handle):
    B = 2
    s0, z0 = zc.mini(3)
    inp = {k: mq.both(v) for k, v in sc.balanced(s0, B).items()}
    out = dict(ref_out=mq.prefilled_both(B * s0.nref), flags=mq.prefilled_both(B, int32=True), cop=mq.prefilled_both(B * 6))
    alpha = mq.prefilled_both(B * 2)
    state = mq.prefilled_both(B * stb.state_bytes(3) // 8)
    O = mq.Out(capi.CStabOutputs, **out)
    I = mq.Out(capi.CStabInputs, **dict(inp, ldp=24, ldx=30))

    def S(**kw):
        return _Struct(capi.c_stabilizer(sc.mini_stab(**{"window": 3, "nref": 141, **kw})), capi.CStabilizer)

    def Z(p=zc.ZMP_P, d=zc.ZMP_D, lf=129, rf=135):
        return _Struct(capi.c_zmp_distributor(stb.ZmpDistributor(p, d, lf, rf)), capi.CZmpDistributor)

    nan6, inf6 = (0.0, np.nan, 0, 0, 0, 0), (0, 0, 0, 0, 0, np.inf)
    bad = [(S(), Z(p=nan6)), (S(), Z(d=inf6)), (S(), Z(lf=-2)), (S(), Z(rf=-2)), (S(), Z(rf=136)), (S(), Z(lf=141)),  # past nref
           (S(), Z(lf=130)), (S(), Z(lf=135)), (S(), Z(lf=128)), (S(), Z(rf=0)), (S(), Z(lf=100, rf=-1)),  # the two overlap; a block overlaps a stabiliser's
           (S(lf_contact_ref=-1, rf_contact_ref=-1), Z()),  # no active foot
           (S(window=0), Z()), (S(dt=0.0), Z()), (S(nref=128), Z(lf=-1, rf=-1))]  # ... and what wbcqp_stabilize refuses
    cases = [(s, z, B, I, state, O, alpha) for s, z in bad]
    cases += [(S(), Z(), -1, I, state, O, alpha), (S(), Z(), B, None, state, O, alpha), (_Struct(None, capi.CStabilizer), Z(), B, I, state, O, alpha)]
    outputs = list(out.values()) + [state, alpha]
    mq.host_refusals_match(handle, "stabilize_zmp", cases, outputs)
    none = mq.Out(capi.CStabOutputs)
    nothing = [(S(), Z(), 0, I, state, O, alpha), (S(), Z(), B, I, None, none, None), (S(), Z(), B, I, None, None, None)]
    mq.host_batch_zero(handle, "stabilize_zmp", nothing, outputs)
    for args in nothing:
        mq.raw(handle, "stabilize_zmp", 0, *args)
    mq._all_unwritten(outputs, "a call with nothing to do wrote something")
    # accepted: offsets of -1; one active foot; alpha as the only output
    for side in (0, 1):
        mq.raw(handle, "stabilize_zmp", side, S(), Z(lf=-1, rf=-1), B, I, None, mq.Out(capi.CStabOutputs, flags=out["flags"]), None)
        mq.raw(handle, "stabilize_zmp", side, S(window=1, lf_contact_ref=-1, lf_force_col=-1), Z(), B, I, None, none, alpha)
    _torch()[0].cuda.synchronize()
    assert not mq.unwritten(out["flags"][1]).any() and not mq.unwritten(out["flags"][0].cpu().numpy()).any()
    assert (alpha[1] == 1.0).all() and (alpha[0].cpu().numpy() == 1.0).all()  # (window 1: the law runs on the first tick; the right foot alone: alpha = 1)
