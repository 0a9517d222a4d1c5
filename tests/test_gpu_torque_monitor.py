"""GPU tests of the torque monitor (wbcqp_detect_torque_collisions, torque_monitor_kernel) against the transcription of the reference's filters and
detector, inria_wbc_amd/torque_monitor.py.  F64: `filtered` and `discrepancy` bit for bit, every integer output equal.

The grid is the whole product n_joints x window x max_invalid x filter x n_ticks x batch of the values below.  The transcription runs once per
(n_joints, window, max_invalid, filter) on the longest stream and the largest batch: the detector is causal and an instance's results depend on its
own rows alone, so a shorter stream is a prefix of that result and a smaller batch its first instances; every launch is compared with that part.

Inputs (streams): per (instance, joint) the wanted discrepancy is piecewise constant -- far outside the threshold with either sign, or well inside it --
over runs of random length between 1 and window + K + 3 ticks (a third of them at most 3 ticks long), and the sensors are the model's column minus that.  A latch needs K ticks after the
filtered discrepancy has crossed, so it can only happen where the longest stream (3 window + 5 ticks) has at least K ticks; cases where it has
at least 2 K + window are asserted to hold latches of both signs, instances without a detection and runs that end before they latch, the others
at least to hold raw-invalid steps.  Over the grid every one of them occurs for every K."""
import ctypes as C

import numpy as np
import pytest

from inria_wbc_amd import capi
from inria_wbc_amd import torque_monitor as tmon
from tests import model_queries as mq

pytestmark = pytest.mark.gpu

N_JOINTS = (1, 22, 63, 64)
WINDOWS = (1, 2, 30, 64)
MAX_INVALID = (0, 1, 5, 31)
FILTERS = (tmon.FILTER_NONE, tmon.FILTER_MEAN, tmon.FILTER_MEDIAN)
BATCHES = mq.BATCHES  # 1, 3, 5, 67
INT_OUT = ("detected", "invalid", "first_tick", "n_detected")
REAL_OUT = ("discrepancy", "filtered")
MARGIN = 1e-9  # no |discrepancy| within MARGIN * max(1, threshold) of its threshold: no decision rests on a last bit


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def handle(built_lib):
    yield from mq.open_handle()


def n_ticks_of(window):
    return (1, window - 1, window, window + 1, 3 * window + 5)


def make_monitor(n, window, max_invalid, filt, seed, with_offset, negative=False):
    """joint: a permutation of more columns than monitored, with a repeat; thresholds between 0.5 and 2, one +inf (never invalid) where there is room
    and, with `negative`, one below zero (always raw-invalid)."""
    rng = np.random.default_rng(seed)
    ldt = n + 3 + int(rng.integers(0, 4))
    joint = rng.permutation(ldt)[:n].astype(np.int32)
    if n >= 2:
        joint[1] = joint[0]
    thr = rng.uniform(0.5, 2.0, n)
    if n >= 8:
        thr[5] = np.inf
        if negative:
            thr[6] = -1.0
    off = rng.uniform(-0.1, 0.1, n) if with_offset else None
    return tmon.Monitor(joint=joint, threshold=thr, offset=off, filter=filt, window=window, max_invalid=max_invalid), ldt


def make_streams(mon, ldt, T, B, seed):
    """tau_model [T][B][ldt], tau_sensor [T][B][n] as the module's docstring says."""
    rng = np.random.default_rng(seed)
    n, K = mon.n_joints, mon.max_invalid + 1
    model = 20.0 * rng.standard_normal((1, B, ldt)) + 0.02 * rng.standard_normal((T, B, ldt))
    scale = np.where(np.isfinite(mon.threshold), np.abs(mon.threshold), 1.0)
    want = np.zeros((T, B, n))
    longest = mon.window + K + 3
    for i in range(B):
        for j in range(n):
            t = 0
            while t < T:
                length = int(rng.integers(1, 4)) if rng.integers(0, 3) == 0 else int(rng.integers(1, longest + 1))
                kind = rng.integers(0, 4)  # outside +, outside -, inside, inside
                want[t:t + length, i, j] = (rng.uniform(3.0, 6.0) * (1 if kind == 0 else -1) if kind < 2 else rng.uniform(-0.3, 0.3)) * scale[j]
                t += length
    if B > 4:
        want[:, 4] = 0.25 * scale  # an instance that never leaves its thresholds (but for a negative one)
    sensor = model[:, :, np.asarray(mon.joint)] - want
    return model, sensor


def assert_streams_decide_clearly(mon, ref, rich):
    thr = np.asarray(mon.threshold, dtype=np.float64)
    d, K = ref["discrepancy"], mon.max_invalid + 1
    fin = np.isfinite(thr)
    assert (np.abs(np.abs(d[..., fin]) - thr[fin]) > MARGIN * np.maximum(1.0, np.abs(thr[fin]))).all()
    raw = ~(np.abs(d) < thr)
    assert raw.any() and not raw[..., thr > 0].all()
    if not rich:
        return
    T, B, n = d.shape
    bits = ((ref["invalid"][..., None] >> np.arange(n, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    assert (bits & (d > 0)).any() and (bits & (d < 0)).any(), "latches of both signs"
    assert (ref["n_detected"] == 0).any(), "an instance without a detection"
    assert (ref["detected"] == 0).any() and (ref["detected"] == 1).any()
    if K > 1:  # a raw-invalid step, not latched, followed by a valid one: a run that ended early
        assert (raw[:-1] & ~bits[:-1] & ~raw[1:]).any(), "interrupted runs"


class Streams:
    """The arrays of one case on the device, and one launch on a part of them."""

    def __init__(self, model, sensor, np_dtype=np.float64):
        torch, dev = _torch()
        self.np_dtype = np_dtype
        self.model = torch.from_numpy(np.ascontiguousarray(model, dtype=np_dtype)).to(dev)
        self.sensor = torch.from_numpy(np.ascontiguousarray(sensor, dtype=np_dtype)).to(dev)

    def launch(self, h, mon, T, lo, hi, state=None, want=capi.TORQUE_CHECKS, t0=0):
        """Ticks t0 .. t0 + T - 1 of instances lo .. hi - 1 as a call of its own, into guarded, prefilled buffers -> {name: numpy array}."""
        torch, dev = _torch()
        B, n, ldt = hi - lo, mon.n_joints, self.model.shape[2]
        td = torch.float64 if self.np_dtype == np.float64 else torch.float32
        model, sensor = self.model[t0:t0 + T, lo:hi].contiguous(), self.sensor[t0:t0 + T, lo:hi].contiguous()
        if T == 0 or B == 0:  # (nothing is read; the pointers must still be given)
            model = sensor = torch.zeros(1, dtype=td, device=dev)
        sizes = {"detected": (T * B, torch.int32), "invalid": (T * B, torch.int64), "discrepancy": (T * B * n, td), "filtered": (T * B * n, td),
                 "first_tick": (B, torch.int32), "n_detected": (B, torch.int32)}
        bufs = {}
        for k in want:
            if k == "invalid":  # (int64 has no NaN: prefilled with UNSET, guarded likewise)
                whole = torch.full((sizes[k][0] + mq.GUARD,), mq.UNSET, dtype=torch.int64, device=dev)
                bufs[k] = (whole, whole[:sizes[k][0]])
            else:
                bufs[k] = mq.guarded(sizes[k][0], sizes[k][1], dev, torch)
        h.detect_torque_collisions(mon, B, T, model, ldt, sensor, state=state, stream=torch.cuda.current_stream().cuda_stream,
                                   **{k: bufs[k][1] for k in want})
        torch.cuda.synchronize()
        shape = {"detected": (T, B), "invalid": (T, B), "discrepancy": (T, B, n), "filtered": (T, B, n), "first_tick": (B,), "n_detected": (B,)}
        out = {}
        for k in want:
            a = bufs[k][0].cpu().numpy()
            N = sizes[k][0]
            if k == "invalid":
                assert (a[N:] == mq.UNSET).all(), (k, "written past the end")
                a = a[:N].view(np.uint64)
            elif a.dtype == np.int32:
                assert (a[N:] == mq.UNSET).all(), (k, "written past the end")
                assert T == 0 or (a[:N] != mq.UNSET).all(), (k, "an element was not written")
                a = a[:N]
            else:
                assert np.isnan(a[N:]).all(), (k, "written past the end")
                a = a[:N]
            out[k] = a.reshape(shape[k])
        return out


def part_of(ref, T, lo, hi):
    """What a call on the first T ticks of instances lo .. hi - 1 must return, from the transcription's result on the whole."""
    out = {k: ref[k][:T, lo:hi] for k in ("detected", "invalid", "discrepancy", "filtered")}
    hit = out["detected"] != 0
    out["n_detected"] = hit.sum(axis=0).astype(np.int32)
    out["first_tick"] = np.where(hit.any(axis=0), hit.argmax(axis=0), -1).astype(np.int32)
    return out


def assert_same(got, want, what, keys=capi.TORQUE_CHECKS):
    for k in keys:
        if k in REAL_OUT:  # bit for bit (a NaN equals a NaN)
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k].astype(got[k].dtype), equal_nan=True), (what, k)
            num = ~np.isnan(got[k])  # (a NaN's sign bit is nobody's business)
            assert np.array_equal(np.signbit(got[k][num]), np.signbit(want[k][num])), (what, k, "sign of a zero")
        else:
            assert np.array_equal(got[k], want[k]), (what, k)


def grid_case(filt, window, n, max_invalid):
    """(monitor, ldt, tau_model, tau_sensor) of one point of the grid on the longest stream and the largest batch; offsets given in half of the cases."""
    seed = 2000 * n + 10 * window + max_invalid  # (a base under which every case's streams pass assert_streams_decide_clearly)
    with_offset = (MAX_INVALID.index(max_invalid) + WINDOWS.index(window)) % 2 == 1
    mon, ldt = make_monitor(n, window, max_invalid, filt, seed, with_offset)
    return (mon, ldt) + make_streams(mon, ldt, 3 * window + 5, max(BATCHES), seed + 1)


def is_rich(filt, window, max_invalid):
    """Whether the longest stream has room for a latch after the filter has let the discrepancy through (the module's docstring)."""
    return 3 * window + 5 >= 2 * (max_invalid + 1) + (window if filt != tmon.FILTER_NONE else 0)


@pytest.mark.parametrize("max_invalid", MAX_INVALID)
@pytest.mark.parametrize("n", N_JOINTS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("filt", FILTERS)
def test_grid_against_the_transcription(handle, filt, window, n, max_invalid):
    mon, ldt, model, sensor = grid_case(filt, window, n, max_invalid)
    ref = tmon.detect(mon, model, sensor)
    assert_streams_decide_clearly(mon, ref, rich=is_rich(filt, window, max_invalid))
    s = Streams(model, sensor)
    for T in n_ticks_of(window):
        for B in BATCHES:
            got = s.launch(handle, mon, T, 0, B)
            if T == 0:  # accepted, nothing launched: first_tick / n_detected stay as they were
                assert (got["first_tick"] == mq.UNSET).all() and (got["n_detected"] == mq.UNSET).all()
                continue
            assert_same(got, part_of(ref, T, 0, B), (filt, window, n, max_invalid, T, B))


SPLIT = [(tmon.FILTER_NONE, 1, 2), (tmon.FILTER_MEAN, 5, 2), (tmon.FILTER_MEDIAN, 4, 0), (tmon.FILTER_MEDIAN, 3, 31)]


@pytest.mark.parametrize("filt,window,max_invalid", SPLIT)
def test_split_invariance(handle, filt, window, max_invalid):
    """T ticks in one call, T calls of one tick and a cut at every tick, the state carried: the same bits in every output and the same state bytes;
    a zeroed state is no state."""
    torch, dev = _torch()
    T, B = 23, 5
    mon, ldt = make_monitor(22, window, min(max_invalid, 3), filt, 77, with_offset=True, negative=True)
    model, sensor = make_streams(mon, ldt, T, B, 78)
    mon.max_invalid = max_invalid
    s = Streams(model, sensor)
    nbytes = capi.torque_monitor_state_bytes(mon)
    assert nbytes == mon.state_bytes()
    fresh = lambda: torch.zeros(B * nbytes, dtype=torch.uint8, device=dev)  # noqa: E731

    def joined(parts, cuts):
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("detected", "invalid", "discrepancy", "filtered")}
        out["n_detected"] = sum(p["n_detected"] for p in parts)
        first = np.full(B, -1, np.int32)
        for p, c in zip(parts, cuts):
            first = np.where((first < 0) & (p["first_tick"] >= 0), p["first_tick"] + c, first)
        out["first_tick"] = first.astype(np.int32)
        return out

    st_whole = fresh()
    whole = s.launch(handle, mon, T, 0, B, state=st_whole)
    assert_same(whole, part_of(tmon.detect(mon, model, sensor), T, 0, B), "one call")
    assert_same(s.launch(handle, mon, T, 0, B, state=None), whole, "no state")
    assert whole["detected"].any() or max_invalid == 31
    assert st_whole.any().item(), "the state was not written"
    st = fresh()
    ticks = [s.launch(handle, mon, 1, 0, B, state=st, t0=t) for t in range(T)]
    assert_same(joined(ticks, range(T)), whole, "T calls of one tick")
    assert torch.equal(st, st_whole)
    for cut in range(1, T):
        st = fresh()
        parts = [s.launch(handle, mon, cut, 0, B, state=st), s.launch(handle, mon, T - cut, 0, B, state=st, t0=cut)]
        assert_same(joined(parts, (0, cut)), whole, ("cut at", cut))
        assert torch.equal(st, st_whole), cut


def test_same_bits_on_two_launches_and_at_any_place_in_a_batch(handle):
    mon, ldt = make_monitor(22, 6, 2, tmon.FILTER_MEDIAN, 91, with_offset=True)
    T, B = 30, 67
    model, sensor = make_streams(mon, ldt, T, B, 92)
    s = Streams(model, sensor)

    def run(lo, hi):
        out = s.launch(handle, mon, T, lo, hi)
        return {k: (np.moveaxis(v, 1, 0) if v.ndim > 1 else v) for k, v in out.items()}  # (instance first)

    a = mq.same_bits_on_two_launches_and_at_any_place_in_a_batch(run, B)
    assert a["detected"].any() and not a["detected"].all()


def test_every_output_is_optional_and_independent(handle):
    torch, dev = _torch()
    mon, ldt = make_monitor(22, 4, 1, tmon.FILTER_MEAN, 93, with_offset=False)
    T, B = 17, 5
    model, sensor = make_streams(mon, ldt, T, B, 94)
    s = Streams(model, sensor)
    nbytes = capi.torque_monitor_state_bytes(mon)
    st_full = torch.zeros(B * nbytes, dtype=torch.uint8, device=dev)
    full = s.launch(handle, mon, T, 0, B, state=st_full)
    for k in capi.TORQUE_CHECKS:
        assert_same(s.launch(handle, mon, T, 0, B, want=(k,)), full, k, keys=(k,))
    pair = s.launch(handle, mon, T, 0, B, want=("invalid", "filtered"))
    assert_same(pair, full, "two outputs", keys=("invalid", "filtered"))
    # every output NULL: with a state the call still runs and advances it; without one there is nothing to do
    st = torch.zeros(B * nbytes, dtype=torch.uint8, device=dev)
    s.launch(handle, mon, T, 0, B, state=st, want=())
    assert torch.equal(st, st_full) and st.any().item()
    s.launch(handle, mon, T, 0, B, want=())
    # the state is guarded too: nothing behind an instance's last byte
    whole = torch.full((B * nbytes + 64,), 0, dtype=torch.uint8, device=dev)
    whole[B * nbytes:] = 0xA5
    s.launch(handle, mon, T, 0, B, state=whole[:B * nbytes], want=())
    assert torch.equal(whole[:B * nbytes], st_full) and (whole[B * nbytes:] == 0xA5).all().item()


def test_the_host_entry_point_is_the_device_one(handle):
    mon, ldt = make_monitor(22, 4, 1, tmon.FILTER_MEDIAN, 95, with_offset=True)
    T, B = 17, 5
    model, sensor = make_streams(mon, ldt, T, B, 96)
    s = Streams(model, sensor)
    torch, dev = _torch()
    nbytes = capi.torque_monitor_state_bytes(mon)
    st_dev = torch.zeros(B * nbytes, dtype=torch.uint8, device=dev)
    first = s.launch(handle, mon, 9, 0, B, state=st_dev)
    st_host = np.zeros((B, nbytes), np.uint8)
    host = handle.detect_torque_collisions_host(mon, model[:9], sensor[:9], state=st_host)
    assert_same(host, first, "host, first part")
    assert np.array_equal(st_host.reshape(-1), st_dev.cpu().numpy())
    second = s.launch(handle, mon, T - 9, 0, B, state=st_dev, t0=9)
    assert_same(handle.detect_torque_collisions_host(mon, model[9:], sensor[9:], state=st_host), second, "host, second part")
    assert np.array_equal(st_host.reshape(-1), st_dev.cpu().numpy())
    only = handle.detect_torque_collisions_host(mon, model, sensor, outputs=("first_tick",))
    assert list(only) == ["first_tick"] and np.array_equal(only["first_tick"], part_of(tmon.detect(mon, model, sensor), T, 0, B)["first_tick"])


def test_f32_handle_rounds_the_f64_result(built_lib):
    """An F32 handle reads float, computes in double and writes float: the F64 result on the float-rounded inputs, rounded; the state stays double."""
    mon, ldt = make_monitor(22, 5, 2, tmon.FILTER_MEAN, 97, with_offset=True)
    T, B = 20, 5
    model, sensor = make_streams(mon, ldt, T, B, 98)
    model32, sensor32 = model.astype(np.float32), sensor.astype(np.float32)
    ref = part_of(tmon.detect(mon, model32.astype(np.float64), sensor32.astype(np.float64)), T, 0, B)
    assert_streams_decide_clearly(mon, ref, rich=False)
    torch, dev = _torch()
    h32 = capi.Handle(0, capi.F32)
    try:
        nbytes = capi.torque_monitor_state_bytes(mon)
        st32 = torch.zeros(B * nbytes, dtype=torch.uint8, device=dev)
        got = Streams(model32, sensor32, np.float32).launch(h32, mon, T, 0, B, state=st32)
        assert got["discrepancy"].dtype == np.float32
        for k in REAL_OUT:
            assert np.array_equal(got[k], ref[k].astype(np.float32)), k
        assert_same(got, ref, "f32", keys=INT_OUT)
        h64 = capi.Handle(0, capi.F64)
        try:
            st64 = torch.zeros(B * nbytes, dtype=torch.uint8, device=dev)
            Streams(model32.astype(np.float64), sensor32.astype(np.float64)).launch(h64, mon, T, 0, B, state=st64)
            assert torch.equal(st32, st64)
        finally:
            h64.close()
    finally:
        h32.close()


def test_a_nan_sample_is_raw_invalid_does_not_latch_and_stays_in_its_instance(handle):
    """Without a filter and under the mean the joint's discrepancy is NaN (for one tick, for `window` ticks): raw-invalid, yet with K = 1 not
    invalid.  Every other joint and every other instance keep the bits of the run without the NaN."""
    for filt, window in ((tmon.FILTER_NONE, 1), (tmon.FILTER_MEAN, 4), (tmon.FILTER_MEDIAN, 4)):
        mon, ldt = make_monitor(22, window, 0, filt, 99, with_offset=False)
        T, B = 16, 5
        model, sensor = make_streams(mon, ldt, T, B, 100)
        clean = Streams(model, sensor).launch(handle, mon, T, 0, B)
        bad = sensor.copy()
        bad[5, 2, 3] = np.nan
        got = Streams(model, bad).launch(handle, mon, T, 0, B)
        assert_same(got, part_of(tmon.detect(mon, model, bad), T, 0, B), ("nan", filt))
        if filt != tmon.FILTER_MEDIAN:
            assert np.isnan(got["discrepancy"][5, 2, 3]) and not (int(got["invalid"][5, 2]) >> 3) & 1  # K = 1: raw-invalid, and still not invalid
        else:  # one NaN among four samples sorts last and is no middle element: the median does not see it
            assert not np.isnan(got["discrepancy"][:, 2, 3]).any()
        others = [i for i in range(B) if i != 2]
        for k in ("detected", "invalid", "discrepancy", "filtered"):
            assert np.array_equal(got[k][:, others], clean[k][:, others]), k
        mask = np.ones(22, bool)
        mask[3] = False
        assert np.array_equal(got["discrepancy"][:, 2][:, mask], clean["discrepancy"][:, 2][:, mask])
        # a NaN where the mean's window holds it: the joint stays NaN for `window` ticks and no longer
        last = 5 + (window if filt == tmon.FILTER_MEAN else 1)
        if filt != tmon.FILTER_MEDIAN:
            assert np.isnan(got["discrepancy"][5:last, 2, 3]).all() and not np.isnan(got["discrepancy"][last:, 2, 3]).any()


def test_refusals_launch_nothing(handle):
    """Every refusal of the header, through both entry points: WBCQP_ERR_INVALID, the same message, outputs and state untouched."""
    torch, dev = _torch()
    T, B, n, ldt = 3, 2, 3, 5
    ok = dict(joint=[4, 0, 4], threshold=[1.0, -2.0, np.inf], offset=None, filter=tmon.FILTER_MEAN, window=4, max_invalid=2)
    mon = lambda **kw: tmon.Monitor(**dict(ok, **kw))  # noqa: E731
    nbytes = mon().state_bytes()
    model, sensor = mq.both(np.ones((T, B, ldt))), mq.both(np.ones((T, B, n)))
    outs = {"detected": mq.prefilled_both(T * B, int32=True), "invalid": mq.prefilled_both(T * B), "discrepancy": mq.prefilled_both(T * B * n),
            "filtered": mq.prefilled_both(T * B * n), "first_tick": mq.prefilled_both(B, int32=True), "n_detected": mq.prefilled_both(B, int32=True)}
    state = mq.prefilled_both(B * nbytes // 8)

    def call(side, m, batch=B, n_ticks=T, tau_model=model, ldt_=ldt, tau_sensor=sensor, st=state, out=True, raw_monitor=None):
        ptr = lambda a: None if a is None else (a[side].ctypes.data if side else a[side].data_ptr())  # noqa: E731
        mb = capi.TorqueMonitorBuffers(m) if raw_monitor is None else None
        mref = C.byref(mb.c) if mb is not None else raw_monitor
        cout = capi.CTorqueChecks(*[ptr(outs[k]) for k in capi.TORQUE_CHECKS])
        args = [handle._h, mref, batch, n_ticks, ptr(tau_model), ldt_, ptr(tau_sensor), ptr(st), C.byref(cout) if out else None]
        if side:
            return handle._check(handle.lib.wbcqp_detect_torque_collisions_host(*args))
        return handle._check(handle.lib.wbcqp_detect_torque_collisions(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    cases = [dict(m=mon(joint=[], threshold=[])), dict(m=mon(joint=list(range(5)) * 13, threshold=[1.0] * 65)), dict(m=mon(window=0)),
             dict(m=mon(window=65)), dict(m=mon(max_invalid=-1)), dict(m=mon(max_invalid=32)), dict(m=mon(filter=3)), dict(m=mon(filter=-1)),
             dict(m=mon(joint=[4, 5, 0])), dict(m=mon(joint=[-1, 0, 1])), dict(m=mon(), ldt_=4), dict(m=mon(threshold=[1.0, np.nan, 1.0])),
             dict(m=mon(offset=[0.0, np.inf, 0.0])), dict(m=mon(offset=[np.nan, 0.0, 0.0])), dict(m=mon(), batch=-1), dict(m=mon(), n_ticks=-1),
             dict(m=mon(), tau_model=None), dict(m=mon(), tau_sensor=None), dict(m=mon(), out=False), dict(m=None, raw_monitor=None)]
    cases[-1] = dict(m=mon(), raw_monitor=C.POINTER(capi.CTorqueMonitor)())  # a NULL monitor
    for kw in cases:
        msgs = [mq.refused(handle, lambda: call(side, **kw)) for side in (1, 0)]
        assert msgs[0] == msgs[1], (kw, msgs)
    mq._all_unwritten(list(outs.values()) + [state], "a refused call wrote something")
    # accepted, nothing to do: batch == 0, n_ticks == 0
    for kw in (dict(batch=0), dict(n_ticks=0)):
        for side in (1, 0):
            call(side, mon(), **kw)
    mq._all_unwritten(list(outs.values()) + [state], "a call with nothing to do wrote something")
    # +-inf and negative thresholds are accepted (the reference's file uses 1e10 as "off"); a window out of range is ignored without a filter
    for side in (1, 0):
        call(side, mon(filter=tmon.FILTER_NONE, window=0), st=None)
    torch.cuda.synchronize()
    assert not mq.unwritten(outs["first_tick"][0].cpu().numpy()).any() and not mq.unwritten(outs["first_tick"][1]).any()


def test_on_a_traced_squat():
    """64 Talos instances squat for 120 ticks.  Model side: inverse dynamics on the trace (entry r's x with entry r - 1's state) + 6, ldt = nv; sensor
    side: the trace's tau.  Thresholds ten times the audit identity's bar (profiles/rnea/INDEX.md): nothing is detected.  Then three instances get an
    extra wrench at the left gripper from tick 40, in a second inverse-dynamics call that serves as the sensors against the trace's tau as the model
    (ldt = na): exactly those three are detected, from the tick and on the joints the transcription names.  All 44 actuated joints are monitored,
    unfiltered, six consecutive violations to latch."""
    from tests.test_inverse_dynamics_host import AUDIT_TOL
    torch, dev = _torch()
    B, K, hit, t_hit = 64, 120, (3, 17, 62), 40
    hand = "gripper_left_joint"

    def prepare(h, m, tm):
        h.set_wrench_frames(0, list(tm.contact_frame) + [m.frame_names.index(hand)])

    h, m, st, tm, trace, q0, v0 = mq.traced_squat(B, K, 1, prepare, more=("x", "tau", "status"))
    try:
        assert (trace["status"] == 0).all().item()
        qb = torch.cat([q0[None], trace["q"][:-1]]).reshape(K * B, -1).contiguous()
        vb = torch.cat([v0[None], trace["v"][:-1]]).reshape(K * B, -1).contiguous()
        x = trace["x"].reshape(K * B, -1).contiguous()
        Tc = torch.from_numpy(np.asarray(st.force_gen()).reshape(st.nc, 6, 12)).to(dev)
        w = torch.zeros(K, B, st.nc + 1, 6, dtype=torch.float64, device=dev)
        w[:, :, :st.nc] = torch.einsum("cij,rbcj->rbci", Tc, trace["x"][..., st.nv:].reshape(K, B, st.nc, 12))
        stream = torch.cuda.current_stream().cuda_stream
        tau_id = torch.full((K * B, m.nv), float("nan"), dtype=torch.float64, device=dev)
        h.inverse_dynamics(0, K * B, qb, tau_id, v=vb, a=x, lda=st.n, wrench=w.reshape(K * B, -1, 6).contiguous(), stream=stream)
        base = m.nv - m.na
        # (no filter: at this threshold a window's lag behind a moving robot's torques would itself be a discrepancy)
        mon = tmon.Monitor(joint=np.arange(m.na), threshold=np.full(m.na, 10 * AUDIT_TOL), filter=tmon.FILTER_NONE, window=1, max_invalid=5)
        out = dict(detected=torch.full((K, B), mq.UNSET, dtype=torch.int32, device=dev), invalid=torch.full((K, B), mq.UNSET, dtype=torch.int64, device=dev),
                   first_tick=torch.full((B,), mq.UNSET, dtype=torch.int32, device=dev), n_detected=torch.full((B,), mq.UNSET, dtype=torch.int32, device=dev))
        # the model's rows are tau_id's, six elements in: no copy
        h.detect_torque_collisions(mon, B, K, tau_id.data_ptr() + 8 * base, m.nv, trace["tau"], stream=stream, **out)
        torch.cuda.synchronize()
        ref = tmon.detect(mon, tau_id.cpu().numpy().reshape(K, B, m.nv)[..., base:], trace["tau"].cpu().numpy())
        for k in out:
            assert np.array_equal(out[k].cpu().numpy().view(ref[k].dtype), ref[k]), k
        assert not out["detected"].any().item() and (out["first_tick"] == -1).all().item()
        print("worst |discrepancy| of the squat: %.3e (threshold %.3e)" % (np.abs(ref["discrepancy"]).max(), 10 * AUDIT_TOL))
        # a push on the left gripper of three robots from tick 40: 15 N along the gripper's own x, 2 N m about its z
        w2 = w.clone()
        for i in hit:
            w2[t_hit:, i, st.nc, 0] = 15.0
            w2[t_hit:, i, st.nc, 5] = 2.0
        tau_hit = torch.full((K * B, m.nv), float("nan"), dtype=torch.float64, device=dev)
        h.inverse_dynamics(0, K * B, qb, tau_hit, v=vb, a=x, lda=st.n, wrench=w2.reshape(K * B, -1, 6).contiguous(), stream=stream)
        sensors = tau_hit.reshape(K, B, m.nv)[..., base:].contiguous()
        for t in out.values():
            t.fill_(mq.UNSET)
        h.detect_torque_collisions(mon, B, K, trace["tau"], m.na, sensors, stream=stream, **out)
        torch.cuda.synchronize()
        ref = tmon.detect(mon, trace["tau"].cpu().numpy(), sensors.cpu().numpy())
        for k in out:
            assert np.array_equal(out[k].cpu().numpy().view(ref[k].dtype), ref[k]), k
        first = out["first_tick"].cpu().numpy()
        assert sorted(np.nonzero(first >= 0)[0].tolist()) == sorted(hit)
        assert (first[list(hit)] == t_hit + mon.max_invalid).all()  # the K-th pushed tick
        arm = [m.joint_names.index("arm_left_%d_joint" % k) - 1 for k in (1, 2, 3, 4)]  # (joint_names[0] is the root)
        last = out["invalid"][-1].cpu().numpy().view(np.uint64)
        for i in hit:
            assert any((int(last[i]) >> j) & 1 for j in arm), "no arm joint among the invalid ones"
    finally:
        h.close()
