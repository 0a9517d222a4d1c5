"""Every kernel that takes WBCQP_FLAG_WARM_START's hint against the HINTED oracle (oracle/wbc_oracle.c, wbco_tick_batch_hint), on hints that
change the path: the cold solution's own mask on heavy QPs, another QP's mask, random bits, the complement (tests/warm_hints.py says how the
QPs and hints were chosen -- by the hinted oracle's event log and its behaviour under one-ulp perturbations with the hint held fixed; nothing
here searches).  Verdicts, as tests/test_gpu_solver_branches.py's for the cold kernels:
  * every QP: the hinted oracle's status; where that is not OPTIMAL the mask that comes back is all zero whatever went in;
  * OPTIMAL QPs: util.assert_parity with its bars as they are (dv, wrench, tau at 1e-8, mask, n_active, objective);
  * class A: the hinted oracle's iteration count;
  * the F32 handle: the suite's f32 bars on rounded inputs (tests/test_gpu_solver_branches.py::test_f32_boundary_on_rounded_inputs);
  * a chain of ticks with the device's own mask carried in place follows the oracle's chain tick by tick;
  * the exact properties of the rule hold bit for bit (KEYS)."""
import numpy as np
import pytest

from tests import solver_branches as sb
from tests import warm_hints as wh
from tests.util import assert_parity, device_outputs, host_outputs, mask_of

pytestmark = pytest.mark.gpu

KEYS = ("x", "tau", "status", "iters", "objective", "n_active", "active_mask")
_REF, _GOT = {}, {}


def _case(name, oracle, f32=False):
    """(st, entries, inputs, hints, hinted oracle outputs) of a structure's selected entries: computed once, never written to."""
    key = (name, f32)
    if key not in _REF:
        from inria_wbc_amd import structure
        st = structure.STRUCTURES[name]()
        entries = wh.load_selection()["f32"] if f32 else wh.entries_of(name)
        assert 0 < len(entries) <= wh.MAX_PER_STRUCTURE
        inputs = sb.stack_inputs(st, entries, f32=f32)
        hints = wh.hints_of(entries)
        ref = oracle.tick_batch(st, inputs, hint=hints)
        for v in list(inputs.values()) + [hints] + [v for v in ref.values() if isinstance(v, np.ndarray)]:
            v.setflags(write=False)
        assert [int(s) for s in ref["status"]] == [e["status"] for e in entries] and [int(i) for i in ref["iters"]] == [e["iters"] for e in entries]
        _REF[key] = (st, entries, inputs, hints, ref)
    return _REF[key]


def _solve(tag, st, inputs, flags, hint=None, f32=False):
    """One launch of the device entry point on a fresh handle; outputs.active_mask holds `hint` ([B, 8]; None: zeros) when it starts.  Cached by tag."""
    key = (tag, flags, f32)
    if key in _GOT:
        return _GOT[key]
    import torch
    from inria_wbc_amd import capi
    dtype, tdt, ndt = (capi.F32, torch.float32, np.float32) if f32 else (capi.F64, torch.float64, np.float64)
    B = inputs["h"].shape[0]
    dev = torch.device("cuda", 0)
    d_in = {k: torch.from_numpy(np.ascontiguousarray(v.astype(ndt))).to(dev) for k, v in inputs.items() if v.size}
    h = capi.Handle(0, dtype, flags=flags)
    try:
        h.set_structure(0, st)
        d_out = device_outputs(B, st, dev, dtype=tdt)
        d_out["x"].fill_(float("nan")); d_out["tau"].fill_(float("nan")); d_out["iters"].fill_(-1)
        if hint is not None:
            d_out["active_mask"].copy_(torch.from_numpy(np.ascontiguousarray(hint).view(np.int32).reshape(B, 8).copy()))
        h.solve_batch(0, B, d_in, d_out, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        h.close()
    _GOT[key] = host_outputs(d_out, st)
    return _GOT[key]


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _verdict(st, entries, got, ref, what, **kw):
    assert np.array_equal(got["status"], ref["status"]), (what, got["status"].tolist(), ref["status"].tolist())
    bad = ref["status"] != 0
    assert not mask_of(got["active_mask"])[bad].any(), (what, "a mask came back where the status is not OPTIMAL")
    info = assert_parity(st, got, ref, what=what, **kw)
    a = np.array([e["class"] == "A" for e in entries])
    differ = np.nonzero(a & (got["iters"] != ref["iters"]))[0]
    assert differ.size == 0, (what, "class-A iteration counts differ from the hinted oracle's",
                              [(entries[i]["seed"], entries[i]["family"], entries[i]["noise"], entries[i]["p"], entries[i]["kind"],
                                int(got["iters"][i]), int(ref["iters"][i])) for i in differ])
    return info


# (structure, flag beside FLAG_WARM_START or None, what runs)
KERNELS = [
    ("talos", None, "queue, Talos's warm twin"),
    ("talos", "FLAG_GENERIC_KERNEL", "queue, generic warm"),
    ("talos", "FLAG_HW_DISPATCH", "hardware dispatch, Talos's warm twin"),
    ("talos_single_support", None, "generic warm"),
    ("icub", None, "generic warm"),
    ("tiago", "FLAG_WORKGROUP_PER_QP", "generic warm, small stack on four waves"),
]


def _flags(flag):
    from inria_wbc_amd import capi
    return capi.FLAG_WARM_START | (getattr(capi, flag) if flag else 0)


@pytest.mark.parametrize("name,flag,what", KERNELS, ids=["%s-%s" % (c[0], c[1] or "default") for c in KERNELS])
def test_every_hinted_kernel_follows_the_hinted_oracle(oracle_mod, name, flag, what):
    st, entries, inputs, hints, ref = _case(name, oracle_mod)
    got = _solve(name, st, inputs, _flags(flag), hints)
    _verdict(st, entries, got, ref, "warm hints: %s, %s" % (name, what))
    # the hint did something here: the cold oracle's iteration counts are others
    assert any(e["differs"] for e in entries)


def test_f32_handle_follows_the_hinted_oracle_on_rounded_inputs(oracle_mod):
    st, entries, inputs, hints, ref = _case("icub", oracle_mod, f32=True)
    got = _solve("icub-f32", st, inputs, _flags(None), hints, f32=True)
    assert np.array_equal(got["status"], ref["status"])
    g64 = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in got.items()}
    assert_parity(st, g64, ref, tol=1e-3, what="warm hints: icub, f32 boundary", active=False)  # (objective / raw forces come back as floats: no 1e-8 bar applies)
    ok = ref["status"] == 0
    assert (np.abs(g64["objective"] - ref["fval"])[ok] <= 1e-5 * np.maximum(1.0, np.abs(ref["fval"]))[ok]).all()
    a = np.array([e["class"] == "A" for e in entries])
    assert np.array_equal(got["iters"][a], ref["iters"][a]), (got["iters"].tolist(), ref["iters"].tolist())


def test_a_chain_of_ticks_carries_the_device_mask_and_follows_the_oracle_chain(oracle_mod):
    """tests/test_gpu_warm.py's squat stream at B = 16: the cold tick, then three ticks each hinted with the mask the tick before left in the
    caller's array -- the device's own, never the oracle's.  The oracle's chain is hinted with the hinted oracle's masks."""
    import torch
    from inria_wbc_amd import capi, structure
    st = structure.STRUCTURES[wh.CHAIN["structure"]]()
    B = wh.CHAIN["batch"]
    rec = wh.load_selection()["chain"]
    ticks = wh.chain(oracle_mod)
    dev = torch.device("cuda", 0)
    h = capi.Handle(0, capi.F64, flags=capi.FLAG_WARM_START)
    try:
        h.set_structure(0, st)
        d_out = device_outputs(B, st, dev)  # active_mask: zeros, the cold tick; from then on whatever the last tick wrote
        for n, t in enumerate(ticks):
            assert [int(v) for v in t["ref"]["iters"]] == rec["iters"][n]
            d_in = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in t["inputs"].items() if v.size}
            went_in = mask_of(d_out["active_mask"].cpu().numpy())
            assert np.array_equal(went_in, t["hint"] if t["hint"] is not None else np.zeros((B, 8), np.uint32)), (n, "the device's mask is not the oracle's")
            h.solve_batch(0, B, d_in, d_out, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = host_outputs(d_out, st)
            entries = [{"class": c, "seed": i, "family": "squat", "noise": 0.0, "p": 0.0, "kind": "chain"} for i, c in enumerate(rec["classes"][n])]
            _verdict(st, entries, got, t["ref"], "warm hints: chain tick %d" % t["t"])
            assert np.array_equal(mask_of(got["active_mask"]), t["ref"]["active_mask"]), (n, "mask")
    finally:
        h.close()


# ---- exact properties: bit for bit on KEYS ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,flag", [("talos", None), ("talos_single_support", None), ("icub", None), ("tiago", "FLAG_WORKGROUP_PER_QP")])
def test_ones_and_zeros_are_the_handle_without_the_flag(oracle_mod, name, flag):
    from inria_wbc_amd import capi
    st, entries, inputs, hints, ref = _case(name, oracle_mod)
    B = len(entries)
    cold = _solve(name + "-cold", st, inputs, _flags(flag) & ~capi.FLAG_WARM_START)
    _same(_solve(name + "-zeros", st, inputs, _flags(flag), np.zeros((B, 8), np.uint32)), cold, (name, "zeros"))
    _same(_solve(name + "-ones", st, inputs, _flags(flag), np.full((B, 8), 0xffffffff, np.uint32)), cold, (name, "ones"))
    # and the selected hints are not that run
    assert not np.array_equal(_solve(name, st, inputs, _flags(flag), hints)["iters"], cold["iters"])


@pytest.mark.parametrize("name,flag", [("talos", None), ("talos_single_support", None), ("icub", None), ("tiago", "FLAG_WORKGROUP_PER_QP")])
def test_bits_at_and_beyond_nin2_mean_nothing(oracle_mod, name, flag):
    st, entries, inputs, hints, ref = _case(name, oracle_mod)
    cleared = wh.cleared_beyond(hints, st.nin2)
    assert (hints != cleared).any()
    _same(_solve(name + "-cleared", st, inputs, _flags(flag), cleared), _solve(name, st, inputs, _flags(flag), hints), name)


def test_talos_twin_is_the_generic_warm_kernel_and_queue_is_hardware_dispatch(oracle_mod):
    st, entries, inputs, hints, ref = _case("talos", oracle_mod)
    own = _solve("talos", st, inputs, _flags(None), hints)
    _same(own, _solve("talos", st, inputs, _flags("FLAG_GENERIC_KERNEL"), hints), "generic")
    _same(own, _solve("talos", st, inputs, _flags("FLAG_HW_DISPATCH"), hints), "hardware dispatch")


@pytest.mark.parametrize("name", ["talos", "icub"])
def test_host_entry_point_with_a_hint_is_the_device_entry_point(oracle_mod, name):
    from inria_wbc_amd import capi
    st, entries, inputs, hints, ref = _case(name, oracle_mod)
    h = capi.Handle(0, capi.F64, flags=capi.FLAG_WARM_START)
    try:
        h.set_structure(0, st)
        got = h.solve_batch_host(0, inputs, hint=hints)
        none = h.solve_batch_host(0, inputs)
    finally:
        h.close()
    dev = _solve(name, st, inputs, _flags(None), hints)
    zeros = _solve(name + "-zeros", st, inputs, _flags(None), np.zeros((len(entries), 8), np.uint32))
    for k in KEYS:
        assert np.array_equal(got[k], dev[k].view(got[k].dtype) if k == "active_mask" else dev[k], equal_nan=True), (name, k)
        assert np.array_equal(none[k], zeros[k].view(none[k].dtype) if k == "active_mask" else zeros[k], equal_nan=True), (name, k, "no hint")
    assert not np.array_equal(got["iters"], none["iters"])


def _random_hints(B, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(B, 8), dtype=np.uint64).astype(np.uint32)


# (structure, flag beside FLAG_WARM_START or None, where its QPs come from): kernels that do not read the hint
DEAF = [("tiago", None, "warm"), ("talos", "FLAG_FULL_LDS", "warm"), ("icub", "FLAG_FULL_LDS", "warm"), ("three_contact", None, "branches")]


@pytest.mark.parametrize("name,flag,source", DEAF, ids=["%s-%s" % (c[0], c[1] or "default") for c in DEAF])
def test_kernels_that_take_no_hint_run_as_without_the_flag_under_any_hint(oracle_mod, name, flag, source):
    from inria_wbc_amd import capi, structure
    if source == "warm":
        st, entries, inputs, hints, _ = _case(name, oracle_mod)
    else:  # three_contact has no entries of its own here: the branch tests' QPs
        st = structure.STRUCTURES[name]()
        entries = sb.entries_of(name)
        inputs = sb.stack_inputs(st, entries)
        hints = _random_hints(len(entries), 31)
    B = len(entries)
    if name == "tiago":
        assert capi.layout_of(st)["wave_per_qp"] == 1
    cold = _solve("%s-deaf-cold" % name, st, inputs, _flags(flag) & ~capi.FLAG_WARM_START)
    for tag, hint in (("sel", hints), ("ones", np.full((B, 8), 0xffffffff, np.uint32)), ("rand", _random_hints(B, 32)), ("zeros", None)):
        got = _solve("%s-deaf-%s" % (name, tag), st, inputs, _flags(flag), hint)
        _same(got, cold, (name, flag, tag))
        assert not mask_of(got["active_mask"])[got["status"] != 0].any()
