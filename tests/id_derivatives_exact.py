"""The truth of the inverse dynamics' derivatives (wbcqp_inverse_dynamics_derivatives), in mpmath at 80 digits.

tests/rbd_exact.py states tau_aw = M a + nle - sum_k J_k' w_k by d'Alembert's principle from the placement map alone,
    tau_j = sum_b Jc_bj . m (a_c,b - g) + Jw_bj . (I_w alpha_b + w_b x I_w w_b) - sum_k (J_k' w_k)_j,
the Jacobians being central differences (step 1e-20) of the placements along the tangent and the accelerations second differences along the
curve q (+) (t v + t^2 a / 2).  Its entry point takes q as float64 numbers, and a configuration displaced by 1e-20 is none; `tau` below is that
same statement on the joints' coordinates in mpmath (the free-flyer's: (R, p)), made of that module's own pieces -- its tables, T.local,
T.forward, _moved, _on_curve -- without the scales.  tests/test_id_derivatives_host.py holds `tau` at the undisplaced state to the committed
tau_aw of tests/golden/rbd_exact/.

  dtau_dq[i, j]  the central difference, step 1e-20, of tau_i along q (+) e e_j: the perturbation _moved, the one that module's second-order
                 statement uses for H (q_j + e; p + R e_k e and R exp(e e_k^) for the free-flyer, in the base's own axes).  The wrenches are
                 numbers in their frames' axes and stay what they are.  Off by 1e-40 of the value; the second differences inside round at
                 1e-80 / 1e-40, the outer division leaves 1e-20.
  dtau_dv[i, j]  (tau(v + e_j) - tau(v - e_j)) / 2: exact at any step, tau being quadratic in v.

An entry under ZERO_REL = 1e-19 of the largest entry of the state's two matrices is written as 0: the differences' own rounding of an exact zero
(columns 0..2 of dtau_dq on a floating base come out at 1e-23 of the largest entry, the whole of dtau_dv of a single revolute body at 1e-60),
three decades under what float64 can hold beside that largest entry.
Cases, states and wrench frames: tests/rbd_exact_cases.py -- the five SMALL cases with all their states, Talos with its first state.
`python -m tests.id_derivatives_exact --write` makes tests/golden/id_derivatives/<case>.npz.
"""
from __future__ import annotations

import os
import sys
import time
from typing import Dict, Optional, Sequence

import mpmath as mp
import numpy as np

from tests import rbd_exact as X
from tests.id_derivatives_cases import CASES, N_STATES, path
from tests.rbd_exact_cases import model, states, wrench_frames

STEP = "1e-20"
ZERO_REL = 1e-19


def _first(T, x):
    """Placements and first derivatives at the coordinates x: (R, p, dP) with dP[j][b] = (dp, dR) of body b along dof j."""
    h = mp.mpf(STEP)
    loc0 = [T.local(b, x[b]) for b in range(T.nb)]
    R, p = T.forward(loc0)
    dP = []
    for b0, kind, k in T.dofs:
        side = []
        for e in (h, -h):
            loc = list(loc0)
            loc[b0] = T.local(b0, X._moved(T, x[b0], b0, kind, k, e))
            side.append(T.forward(loc, R, p, b0))
        (Ra, pa), (Rb, pb) = side
        dP.append({b: (X._sc(1 / (2 * h), X._sub(pa[b], pb[b])), X._msc(1 / (2 * h), X._msub(Ra[b], Rb[b]))) for b in range(b0, T.last[b0] + 1)})
    return R, p, dP


def tau(T, x, vv, aa, wframes: Sequence[int], wrench, first=None):
    """tau_aw [nv] in mpmath at the joints' coordinates x, the velocity vv and its derivative aa (mpmath numbers), the wrenches (float64
    [len(wframes), 6], in the frames' own axes) at the frames wframes."""
    h = mp.mpf(STEP)
    R, p, dP = first if first is not None else _first(T, x)
    side = [T.forward([T.local(b, X._on_curve(T, x[b], b, vv, aa, t)) for b in range(T.nb)]) for t in (h, -h)]
    (Ra, pa), (Rb, pb) = side
    out = [mp.mpf(0)] * T.nv
    for b in range(T.nb):
        ddp = X._sc(1 / (h * h), X._add(X._sub(pa[b], X._sc(2, p[b])), pb[b]))
        dR = X._msc(1 / (2 * h), X._msub(Ra[b], Rb[b]))
        ddR = X._msc(1 / (h * h), X._madd(X._msub(Ra[b], X._msc(2, R[b])), Rb[b]))
        w, al = X._vee(X._mmt(dR, R[b])), X._vee(X._mmt(ddR, R[b]))
        Iw = X._mm(R[b], X._mmt(T.I[b], R[b]))
        force = X._sc(T.mass[b], X._sub(X._add(ddp, X._mv(ddR, T.c[b])), T.g))
        mom = X._add(X._mv(Iw, al), X._cross(w, X._mv(Iw, w)))
        for j in T.sup[b]:
            dp_, dR_ = dP[j][b]
            out[j] += X._dot(X._add(dp_, X._mv(dR_, T.c[b])), force) + X._dot(X._vee(X._mmt(dR_, R[b])), mom)
    for k, f in enumerate(wframes):
        b = T.fbody[f]
        Rf = X._mm(R[b], T.fR[f])
        wk = [X._f(v_) for v_ in wrench[k]]
        for j in T.sup[b]:
            dp_, dR_ = dP[j][b]
            lin, ang = X._add(dp_, X._mv(dR_, T.fp[f])), X._vee(X._mmt(dR_, R[b]))
            out[j] -= X._dot(X._mtv(Rf, lin), wk[:3]) + X._dot(X._mtv(Rf, ang), wk[3:])
    return out


def _floats(M, nv):
    return np.array([[float(M[i][j]) for j in range(nv)] for i in range(nv)])


def truth(m, q, v, a, wframes: Sequence[int], wrench) -> Dict[str, np.ndarray]:
    """dtau_dq, dtau_dv [nv, nv] and tau [nv] for one state, rounded to float64."""
    T = X._tables(m)  # (sets the precision)
    nv = T.nv
    h = mp.mpf(STEP)
    x0 = X._coords(T, q)
    vv, aa = [X._f(x) for x in v], [X._f(x) for x in a]
    first = _first(T, x0)
    dq = [[None] * nv for _ in range(nv)]
    dv = [[None] * nv for _ in range(nv)]
    for j, (b0, kind, k) in enumerate(T.dofs):
        side = []
        for e in (h, -h):
            x = list(x0)
            x[b0] = X._moved(T, x0[b0], b0, kind, k, e)
            side.append(tau(T, x, vv, aa, wframes, wrench))
        one = mp.mpf(1)
        up, dn = list(vv), list(vv)
        up[j], dn[j] = vv[j] + one, vv[j] - one
        tu, td = tau(T, x0, up, aa, wframes, wrench, first), tau(T, x0, dn, aa, wframes, wrench, first)
        for i in range(nv):
            dq[i][j] = (side[0][i] - side[1][i]) / (2 * h)
            dv[i][j] = (tu[i] - td[i]) / 2
    t0 = tau(T, x0, vv, aa, wframes, wrench, first)
    dq, dv = _floats(dq, nv), _floats(dv, nv)
    big = max(np.abs(dq).max(), np.abs(dv).max())
    dq, dv = (np.where(np.abs(x) < ZERO_REL * big, 0.0, x) for x in (dq, dv))
    return {"dtau_dq": dq, "dtau_dv": dv, "tau": np.array([float(t) for t in t0])}


def compute(name) -> Dict[str, np.ndarray]:
    """The truth of every state of a case that the fixtures hold, stacked; the inputs ride along."""
    m, s = model(name), states(name)
    n = N_STATES[name]
    per = [truth(m, s["q"][i], s["v"][i], s["a"][i], wrench_frames(name), s["wrench"][i]) for i in range(n)]
    out = {k: np.stack([r[k] for r in per]) for k in per[0]}
    out.update({"in." + k: arr[:n] for k, arr in s.items()})
    out["in.wrench_frames"] = np.array(wrench_frames(name), dtype=np.int32)
    return out


def write(names: Optional[Sequence[str]] = None) -> None:
    os.makedirs(os.path.dirname(path(CASES[0])), exist_ok=True)
    for name in names or CASES:
        t0 = time.time()
        np.savez_compressed(path(name), **compute(name))
        print("%-28s %6.1f s  %8d bytes" % (name, time.time() - t0, os.path.getsize(path(name))), flush=True)


if __name__ == "__main__":
    if "--write" in sys.argv:
        write([a for a in sys.argv[1:] if a in CASES] or None)
    else:
        print(__doc__)
