"""The state integration (wbcqp_integrate, wbcqp_integrate_host: csrc/wbcqp_integrate.hpp, integrate_one) against the exact statement of
tests/se3_exact.py, ENTRY BY ENTRY, on every branch: both sides of the exp6 switch and the switch itself, t = 0 and a t whose square underflows,
the four cases of rotation -> quaternion and their ties, the sign flip, the rotation vector on both signs of w, the kept state for every status
code but OPTIMAL, nv across the lane loop, a last block of 1, 3 and 4 wavefronts, ldx > nv, q_solver NULL, K = 256 ticks that must compose, a
drifted input quaternion, and an F32 handle.

The statement's values and scales are the committed fixtures (tests/golden/se3_exact/): no mpmath runs here and nothing is computed but ratios.
    F64 handle   |x - value| <= REF_MULTIPLE K_ORACLE[family][quantity] eps scale          (position, quaternion, rotation vector)
    F32 handle   |x - value| <= eps32 scale: the kernel computes in double and rounds once, a correctly rounded result is within eps32 |x| / 2
    both         v_next, the joints, a kept state's q_next / v_next / position: BIT FOR BIT (scale 0), the identity's rotation vector +0
K_ORACLE is the C oracle's measured worst against the same statement (tests/se3_exact_cases.py, tests/test_se3_exact_host.py) and REF_MULTIPLE = 4
the margin tests/test_gpu_rbd_exact.py gives the device's libm over the host's.  No factor is taken from the kernel under test.  After K ticks the
bar is K times the one-step bar (rounding errors add at worst linearly) and | |q| - 1 | is held to the oracle's own figure times REF_MULTIPLE.
Every output is allocated with a guard row before and after it, filled with a sentinel that is a NaN: the guards come back bit for bit, and an
entry that was not written fails as a NaN.

wbcqp_tick, wbcqp_rollout and the mixed calls (mixed_integrate_kernel) run the same integrate_one and are held BIT FOR BIT to chains of
wbcqp_integrate by tests/test_gpu_rollout.py and tests/test_gpu_mixed_contacts.py: they are not repeated here."""
import numpy as np
import pytest

from tests import se3_exact_cases as X  # (fixtures only: no mpmath here)
from tests.se3_exact_cases import K_ORACLE, KSTEPS, REF_MULTIPLE

pytestmark = pytest.mark.gpu

ERR_INVALID = 1  # WBCQP_ERR_INVALID (include/wbcqp.h)
SENTINEL = {"f64": 0x7FF85E37DEADBEEF, "f32": 0x7FC5E37D}  # quiet NaNs with a payload


@pytest.fixture(scope="module")
def handles(built_lib):
    import torch  # noqa: F401  (share one HIP runtime with torch)
    from inria_wbc_amd import capi
    hs = {"f64": capi.Handle(0, capi.F64), "f32": capi.Handle(0, capi.F32)}
    yield hs
    for h in hs.values():
        h.close()


def _types(tag):
    import torch
    return (torch.float64, torch.int64, np.float64) if tag == "f64" else (torch.float32, torch.int32, np.float32)


def _guarded(rows, cols, tag, dev):
    """(whole, part): [rows + 2, cols] filled with the sentinel, and its rows 1 .. rows: what the call may write."""
    import torch
    td, ti, _ = _types(tag)
    whole = torch.full((rows + 2, cols), SENTINEL[tag], dtype=ti, device=dev).view(td)
    return whole, whole[1:rows + 1]


def _guards_untouched(whole, tag):
    _, ti, _ = _types(tag)
    g = whole.view(ti)[[0, -1]].cpu().numpy()
    return bool((g == SENTINEL[tag]).all())


def _inputs(G, tag):
    _, _, nd = _types(tag)
    q, dq, x = (np.ascontiguousarray(G[k].astype(nd)) for k in ("q", "dq", "x"))
    return q, dq, x, (np.ascontiguousarray(G["status"]) if "status" in G else None)


def _run(handles, G, tag):
    """One launch of wbcqp_integrate on device pointers: the outputs as numpy arrays (q_solver None where the group gives none)."""
    import torch
    dev = torch.device("cuda", 0)
    q, dq, x, status = _inputs(G, tag)
    B, nv, nq = dq.shape[0], int(G["nv"]), q.shape[1]
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    q_, dq_, x_, st_ = t(q), t(dq), t(x), t(status)
    whole = {k: _guarded(B, c, tag, dev) for k, c in (("q_next", nq), ("v_next", nv), ("q_solver", nv))}
    qs = whole["q_solver"][1] if int(G["qs"]) else None
    handles[tag].integrate(B, nv, bool(G["fb"]), float(G["dt"]), q_, dq_, x_, int(G["ldx"]), st_, whole["q_next"][1], whole["v_next"][1], qs,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: w[1].cpu().numpy() for k, w in whole.items()}
    for k, (w, _) in whole.items():
        assert _guards_untouched(w, tag), (k, "a store outside the instance's own rows")
    if qs is None:
        _, ti, _ = _types(tag)
        assert bool((whole["q_solver"][0].view(ti) == SENTINEL[tag]).all()), "q_solver is NULL and something was written"
        out["q_solver"] = None
    return out


def _run_host(handles, G, tag):
    """The same through wbcqp_integrate_host."""
    h = handles[tag]
    q, dq, x, status = _inputs(G, tag)
    B, nv = dq.shape[0], int(G["nv"])
    out = {"q_next": np.zeros_like(q), "v_next": np.zeros_like(dq), "q_solver": np.zeros_like(dq) if int(G["qs"]) else None}
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    h._check(h.lib.wbcqp_integrate_host(h._h, B, nv, int(G["fb"]), float(G["dt"]), p(q), p(dq), p(x), int(G["ldx"]), p(status), p(out["q_next"]),
                                        p(out["v_next"]), p(out["q_solver"])))
    return out


def _bar(family, tag):
    return {k: (REF_MULTIPLE * K_ORACLE[family][k] if tag == "f64" else 1.0) for k in X.QUANTITIES}


def _judge(family, g, tag, G, out, over):
    w, bar = X.worst(G, out, tag), _bar(family, tag)
    print("se3_exact %-9s %-16s %s  %s" % (family, g, tag, "  ".join("%s %.3g (bar %.3g)" % (k, w[k], bar[k]) for k in X.QUANTITIES)))
    over += [(g, tag, k, w[k], bar[k]) for k in X.QUANTITIES if not w[k] <= bar[k]]


CASES = [(f, tag) for f in X.FAMILIES for tag in ("f64", "f32") if any(int(G[tag]) for G in X.load(f).values())]


@pytest.mark.parametrize("family,tag", CASES)
def test_integrate(handles, family, tag):
    over = []
    for g, G in X.load(family).items():
        if not int(G[tag]):
            continue
        out = _run(handles, G, tag)
        _judge(family, g, tag, G, out, over)
        if family == "drifted":
            d = float(X.norm_defect(out["q_next"][:, 3:7]).max())
            print("se3_exact drifted: | |q| - 1 | of the result %.3g (the oracle's %.3g)" % (d, K_ORACLE["drifted"]["norm_abs"]))
            assert d <= K_ORACLE["drifted"]["norm_abs"], d
    assert not over, (family, over)


@pytest.mark.parametrize("family,tag", [c for c in CASES if c[0] in X.HOST_POINTER_FAMILIES])
def test_host_pointers_give_the_same_bits(handles, family, tag):
    for g, G in X.load(family).items():
        if not int(G[tag]):
            continue
        a, b = _run(handles, G, tag), _run_host(handles, G, tag)
        for k in ("q_next", "v_next", "q_solver"):
            assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), (family, g, tag, k)


def test_k_ticks_compose(handles):
    """K launches that ping-pong two buffers at a constant body twist, against the subgroup statement M0 exp6(K dt v)."""
    import torch
    dev = torch.device("cuda", 0)
    G = X.load("ksteps")["all"]
    K, B, nv, dt = int(G["K"]), G["q"].shape[0], int(G["nv"]), float(G["dt"])
    assert K == KSTEPS
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    state = [(t(G["q"]), t(G["dq"])), (torch.zeros(B, nv + 1, dtype=torch.float64, device=dev), torch.zeros(B, nv, dtype=torch.float64, device=dev))]
    x = torch.zeros(B, nv, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for k in range(K):
        (qa, va), (qb, vb) = state[k & 1], state[1 - (k & 1)]
        handles["f64"].integrate(B, nv, True, dt, qa, va, x, nv, None, qb, vb, None, stream=s)
    torch.cuda.synchronize()
    q, v = (a.cpu().numpy() for a in state[K & 1])
    assert v.tobytes() == G["dq"].tobytes()
    w = X.worst(G, {"q_next": q}, prefix="end.")
    norm = float(X.norm_defect(q[:, 3:7]).max() / X.EPS)
    bar = {k: KSTEPS * REF_MULTIPLE * K_ORACLE["ksteps"][k] for k in ("position", "quaternion")}
    print("se3_exact after %d ticks: position %.3g eps scale (bar %.0f), quaternion %.3g eps (bar %.0f), | |q| - 1 | %.3g eps (bar %.2f)" % (
        K, w["position"], bar["position"], w["quaternion"], bar["quaternion"], norm, REF_MULTIPLE * K_ORACLE["ksteps"]["norm"]))
    assert w["position"] <= bar["position"] and w["quaternion"] <= bar["quaternion"], w
    assert norm <= REF_MULTIPLE * K_ORACLE["ksteps"]["norm"], norm


def test_refusals(handles):
    """An in-place call (the kernel's outputs are __restrict__, and the base's twist is read after v_next is stored) and a floating base with
    fewer than six velocities are refused -- the latter by wbcqp_integrate_host before anything is staged."""
    import torch
    from inria_wbc_amd import capi
    dev = torch.device("cuda", 0)
    h = handles["f64"]
    B, nv = 2, 8
    z = lambda c: torch.zeros(B, c, dtype=torch.float64, device=dev)  # noqa: E731
    q, dq, x, qn, vn = z(nv + 1), z(nv), z(nv), z(nv + 1), z(nv)
    for args in ((q, vn), (qn, dq)):
        with pytest.raises(capi.WbcqpError) as e:
            h.integrate(B, nv, True, 1e-3, q, dq, x, nv, None, args[0], args[1], None)
        assert e.value.code == ERR_INVALID
    with pytest.raises(capi.WbcqpError) as e:
        h.integrate(B, 5, True, 1e-3, q, dq, x, 5, None, qn, vn, None)
    assert e.value.code == ERR_INVALID
    a = np.zeros((B, 6))
    rc = h.lib.wbcqp_integrate_host(h._h, B, 5, 1, 1e-3, a.ctypes.data, a.ctypes.data, a.ctypes.data, 5, None, a.ctypes.data, a.ctypes.data, None)
    assert rc == ERR_INVALID and b"floating base" in h.lib.wbcqp_last_error(h._h)
    torch.cuda.synchronize()
    assert not np.any(qn.cpu().numpy()) and not np.any(vn.cpu().numpy())  # nothing ran
