"""What the tests of the three model queries on a fleet's states share (tests/test_gpu_observe.py, test_gpu_collision.py,
test_gpu_inverse_dynamics.py and their test_*_facade.py): the cases, the guard-padded output buffers with their two post-conditions, the
refusal helper and the test bodies that are one pattern run with three queries.  A plain module, in the manner of tests/task_laws.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from inria_wbc_amd import capi, refprog, structure
from inria_wbc_amd import model as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 3, 5, 67)  # batches that are no multiple of the four instances of a workgroup, and more than one workgroup
GUARD = 16  # elements behind every output buffer that must stay untouched
UNSET = -77  # what an int32 output buffer holds before a launch (a float one: NaN)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def minimal(m, prefix):
    """The smallest stack a slot accepts for `m`: one SE(3) task on frame 0 (the queries need the tree, not the tasks)."""
    st = structure._mk(prefix + m.name, m.nv, m.na, [], [("a", 3, 1.0)], None, [], False, False, [])
    return st, mdl.build_taskmap(m, st, [dict(name="a", type="se3", tracked=m.frame_names[0], kp=10.0, mask="111000")])


def tree_case(prefix, seed, nb, fb, shape=None, two_on_one_body=False):
    """() -> (model, structure, task map) of a random tree with a frame on body 0 and one on the last body."""
    def f():
        m = mdl.random_tree(seed, nb, fb, nframe=12)
        if shape == "chain":  # (the way three_limbs in tests/test_gpu_terms.py rewrites parents) depth nb - 1: every doubling round moves something
            m.parent = np.arange(-1, nb - 1, dtype=np.int32)
        if shape == "star":   # every body but the root is a leaf: every subtree but the root's is one lane
            m.parent = np.array([-1] + [0] * (nb - 1), dtype=np.int32)
        m.frame_body[0], m.frame_body[1] = 0, nb - 1
        if two_on_one_body:
            m.frame_body[3] = m.frame_body[2]
        m.validate()
        return (m,) + minimal(m, prefix)
    return f


def shipped_case(model, st, stack):
    def f():
        m = model()
        s = st()
        return m, s, mdl.build_taskmap(m, s, stack())
    return f


talos_case = shipped_case(mdl.talos_like, structure.talos_structure, mdl.talos_stack)


def open_handle():
    """The body of the modules' `handle` fixture."""
    h = capi.Handle(0, capi.F64)
    yield h
    h.close()


# ---- guard-padded output buffers -----------------------------------------------------------------------------------------------------------
def guarded(n, td, dev, torch):
    """(whole, part): a prefilled buffer (NaN; UNSET for int32) and its first n elements, the part a query may write."""
    whole = torch.full((n + GUARD,), UNSET if td == torch.int32 else float("nan"), dtype=td, device=dev)
    return whole, whole[:n]


def unwritten(a):
    """Elementwise: the numpy array still holds what `guarded` (or a NaN / UNSET prefilled host array) put there."""
    return a == UNSET if a.dtype == np.int32 else np.isnan(a)


def read_guarded(whole, n, what, finite=True):
    """The n elements a launch had to write: nothing behind them is touched, every one of them is written (finite: and no inf among them)."""
    a = whole.cpu().numpy()
    assert unwritten(a[n:]).all(), (what, "written past the end")
    assert np.isfinite(a[:n]).all() if finite and a.dtype != np.int32 else not unwritten(a[:n]).any(), (what, "an element was not written")
    return a[:n]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(h, call):
    """call() is refused with WBCQP_ERR_INVALID and a message; returns the message."""
    with pytest.raises(capi.WbcqpError) as e:
        call()
    assert e.value.code == 1, e.value  # WBCQP_ERR_INVALID
    msg = (h.lib.wbcqp_last_error(h._h) or b"").decode()
    assert msg.strip(), "no message in wbcqp_last_error"
    return msg


def a_refused_selection_keeps_the_one_before(h, which, nframe, limit, still_stands):
    """which: "observed" or "wrench", on slot 3.  After [3, 5], a selection with an index out of range (through the Handle) and one of limit + 1 frames
    (through the raw library) are refused, and still_stands([3, 5]) asserts that the query answers for [3, 5]."""
    select, raw_set = getattr(h, "set_%s_frames" % which), getattr(h.lib, "wbcqp_set_%s_frames" % which)
    select(3, [3, 5])
    refused(h, lambda: select(3, [0, nframe]))
    refused(h, lambda: h._check(raw_set(h._h, 3, limit + 1, np.zeros(limit + 1, np.int32).ctypes.data_as(capi.c_i32_p))))
    still_stands([3, 5])


# Both entry points of a query through the raw library with the same arguments: an array is a pair (device tensor, numpy array), and so is every
# member of the struct of outputs (Out); side 0 calls wbcqp_<query> on the current stream, side 1 wbcqp_<query>_host
def both(a):
    torch, dev = _torch()
    return torch.from_numpy(a).to(dev), a


def prefilled_both(n, int32=False):
    torch, dev = _torch()
    fill, td, nd = (UNSET, torch.int32, np.int32) if int32 else (float("nan"), torch.float64, np.float64)
    return torch.full((n,), fill, dtype=td, device=dev), np.full(n, fill, nd)


class Out:
    def __init__(self, cls, **members):
        self.cls, self.members = cls, members


def _arg(a, side):
    a = a[side] if isinstance(a, tuple) else a
    if isinstance(a, Out):
        return C.byref(a.cls(*[_arg(a.members.get(k), side) for k, _ in a.cls._fields_]))
    return a if a is None or isinstance(a, int) else (a.ctypes.data if side else a.data_ptr())


def raw(h, query, side, *args):
    stream = () if side else (C.c_void_p(_torch()[0].cuda.current_stream().cuda_stream),)
    h._check(getattr(h.lib, "wbcqp_" + query + ("_host" if side else ""))(h._h, *[_arg(a, side) for a in args], *stream))


def _all_unwritten(outputs, what):
    _torch()[0].cuda.synchronize()
    for dev, host in outputs:
        assert unwritten(dev.cpu().numpy()).all() and unwritten(host).all(), what


def host_refusals_match(h, query, cases, outputs):
    """Every case (the arguments after the handle) is refused by the device-pointer entry point and by the _host one with code 1 and the SAME message, and
    nothing is written to `outputs` on either side."""
    for args in cases:
        assert refused(h, lambda: raw(h, query, 1, *args)) == refused(h, lambda: raw(h, query, 0, *args)), args
    _all_unwritten(outputs, "a refused call wrote something")


def host_batch_zero(h, query, cases, outputs):
    """Every case (batch == 0) is WBCQP_OK through the _host entry point and leaves the caller's prefilled arrays untouched."""
    for args in cases:
        raw(h, query, 1, *args)
    _all_unwritten(outputs, "a call with batch == 0 wrote something")


# ---- one pattern, three queries ------------------------------------------------------------------------------------------------------------
def nothing_else_moves(handle, case, seed, query, observed=None):
    """The rows and the tick of six states (with `observed` frames selected: their observables too) have the same bits before and after
    query(states, the tick before)."""
    m, st, tm = case
    handle.set_structure(3, st)
    handle.set_model(3, m, tm)
    B = 6
    s = mdl.sample_states(m, tm, B, seed, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    tlb, tub, w = np.tile(-m.tau_max, (B, 1)), np.tile(m.tau_max, (B, 1)), np.tile(st.default_weights, (B, 1))
    if observed is not None:
        handle.set_observed_frames(3, observed)

    def snapshot():
        out = [handle.problem_data_host(3, s["q"], s["v"], s["ref"]), handle.tick_host(3, s["q"], s["v"], s["ref"], tlb, tub, w, tm.dt)]
        return out + ([handle.observe_host(3, s["q"], s["v"])] if observed is not None else [])  # (the selection of frames stands)

    before = snapshot()
    query(s, before[1])
    for a, b in zip(before, snapshot()):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert (before[1]["status"] == 0).all()


def same_bits_on_two_launches_and_at_any_place_in_a_batch(run, n):
    """run(lo, hi) -> {name: array} for the rows lo .. hi - 1 of n states as a batch of their own; returns the whole batch's."""
    a, b = run(0, n), run(0, n)
    c = run(10, 16)  # rows 10 .. 15 as a batch of their own: other waves, other workgroups
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][10:16], c[k]), k
    return a


def set_structure_and_set_model_drop(h, case, buffer, query, needle, and_then):
    """After set_structure + set_model, and after set_model alone, on slot 0: query(buf) on buf = buffer() (prefilled, on the device) is refused with
    `needle` in the message and writes nothing; and_then() checks what still works and puts the table back."""
    torch, _ = _torch()
    m, st, tm = case
    for again in ("structure", "model"):
        if again == "structure":
            h.set_structure(0, st)
        h.set_model(0, m, tm)
        buf = buffer()
        with pytest.raises(capi.WbcqpError) as e:
            query(buf)
        assert e.value.code == 1 and needle in str(e.value)
        torch.cuda.synchronize()
        assert unwritten(buf.cpu().numpy()).all()
        and_then()


def traced_squat(B, K, stride, prepare, more=()):
    """A new handle with Talos on slot 0 (prepare(h, m, tm) puts the query's table there) and B instances squatting for K ticks, every stride-th tick
    traced: q, v and, of `more`, x, tau, status.  -> the handle (the caller closes it), m, st, tm, the trace, the initial q and v on the device."""
    torch, dev = _torch()
    m, st, tm = talos_case()
    s = mdl.sample_states(m, tm, B, 97_000, q_noise=0.01, v_noise=0.05, ref_noise=0.01)
    com = next(b for b in tm.blocks if b.kind == mdl.T_COM)
    prog = refprog.move_com_program(tm.nref, com.ref, m.com(m.q0), [[0.0, 0.0, -0.2]], "001", tm.dt, 2.0, loop=True, absolute=False)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    status = lambda *shape: torch.full(shape, -99, dtype=torch.int32, device=dev)  # noqa: E731
    lim = dict(w=up(np.tile(st.default_weights, (B, 1))), tlb=up(np.tile(-m.tau_max, (B, 1))), tub=up(np.tile(m.tau_max, (B, 1))))
    n_rec, width = K // stride, dict(q=m.nq, v=m.nv, x=st.n, tau=st.na)
    trace = {k: status(n_rec, B) if k == "status" else f(n_rec, B, width[k]) for k in ("q", "v") + tuple(more)}
    q0, v0 = up(s["q"]), up(s["v"])
    h = capi.Handle(0, capi.F64)
    try:
        h.set_structure(0, st)
        h.set_model(0, m, tm)
        prepare(h, m, tm)
        stream = torch.cuda.current_stream().cuda_stream
        ref = h.reference_samples(prog, up(s["ref"]), -37 * np.arange(B), 0, K, torch.zeros(K, B, tm.nref, dtype=torch.float64, device=dev), stream=stream)
        out = dict(x=f(B, st.n), tau=f(B, st.na), status=status(B), iters=torch.zeros(B, dtype=torch.int32, device=dev))
        h.rollout_traced(0, B, K, dict(q=q0, v=v0, ref=ref), lim, out, f(B, m.nq), f(B, m.nv), tm.dt, trace=trace, stride=stride, stream=stream)
        torch.cuda.synchronize()
    except BaseException:
        h.close()
        raise
    return h, m, st, tm, trace, q0, v0


# ---- the facade programs -------------------------------------------------------------------------------------------------------------------
def host_build():
    """The body of the facade modules' `host_build` fixture (which asks for built_lib)."""
    from inria_wbc_amd import build
    return build.build_host()


def run_file_source(program, tmp_path, *before_batch):
    """`program --file-source <pos_tracker.yaml> [before_batch ...] <a dumped batch of two Talos QPs>`: a source without a model."""
    from tools import dump_batch
    from inria_wbc_amd import synth
    st = structure.talos_structure()
    path = str(tmp_path / "b.bin")
    dump_batch.dump(path, st, synth.generate(st, 2, synth.SEED_BASE["talos"]))
    return subprocess.run([program, "--file-source", os.path.join(ROOT, "configs/talos/pos_tracker.yaml"), *before_batch, path],
                          capture_output=True, text=True, timeout=120)
