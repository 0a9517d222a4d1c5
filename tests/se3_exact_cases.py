"""The cases of the exact statement of the state integration (tests/se3_exact.py), its committed fixtures and the entrywise bar: everything the
tests need that needs no mpmath.  tests/test_gpu_se3_exact.py uses this module alone -- fixtures only, nothing is computed there;
tests/se3_exact.py (the statement itself) and tests/test_se3_exact_host.py build on it.

A FAMILY is one fixture file (tests/golden/se3_exact/<family>.npz) and holds GROUPS: one group is one launch of wbcqp_integrate (one floating_base,
nv, dt, ldx, batch, status given or NULL, q_solver given or NULL).  A group's keys are "<group>.<key>":
    fb, nv, dt, ldx, qs (q_solver is given), f64 / f32 (the handles it is run with)                      scalars
    q [B, nq], dq [B, nv], x [B, ldx] (NaN past nv, and in the rows of a kept instance), status [B]        inputs; no status: NULL
    q_next, v_next, q_solver                                                                               the statement, rounded to float64
    scale.q_next, scale.q_solver                                                                           the scale of every entry
An F32 handle computes in double and rounds once, so its statement is the same numbers: entries that are bit for bit are float32 of them.
A scale of 0 says BIT FOR BIT (v_next, the joints, a kept state, the exact +0 of an identity's rotation vector): v_next carries no scale array.
A scale of inf says NOT JUDGED (the rotation vector where the result's |w| < 0.05: the axis flips at w = 0) -- but a NaN there still fails.
The K-step family holds, beside the one-step statement of its first tick, K and "end.*": the state after K ticks by the subgroup statement."""
from __future__ import annotations

import functools
import os
from typing import Dict, List

import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se3_exact")
QUANTITIES = ("position", "quaternion", "rotvec")
FAMILIES = ("generic", "switch", "tiny", "rot2quat", "sign", "qsolver", "kept", "sizes", "ksteps", "drifted")
HOST_POINTER_FAMILIES = ("generic", "switch", "kept")  # also through wbcqp_integrate_host, bit for bit
SWITCH = 1e-4  # the kernel's and the oracle's `t > 1e-4`
DT2, DT = 2.0 ** -10, 1e-3
KSTEPS = 256
# the status codes of the HQP_* enumeration (include/wbcqp.h): OPTIMAL is 0
HQP_NOT_OPTIMAL = (-1, 1, 2, 3, 4)
W_MARGIN, DOT_MARGIN = 0.05, 0.1  # |w| of a judged rotation vector's quaternion; |q1 . q0| of every integrated instance

# K_ORACLE[family][quantity]: the worst ratio |x - value| / (eps scale) of the C oracle (oracle/wbc_oracle.c: wbco_integrate) over the family's
# float64 groups.  Measured 2026-10-20 with `pytest -s tests/test_se3_exact_host.py -k oracle_ratio` (the line "K_ORACLE measured", three
# digits), written here rounded UP in the third digit.  "norm": | |q| - 1 | / eps of the result (K steps: after the K ticks), the norm taken
# in long double; "norm_abs" (drifted): | |q| - 1 | itself, which the first-order normalisation leaves at (3/8)(|q0|^2 - 1)^2.
# These are the printed figures, nothing added: a quaternion entry has scale 1, so its ratios are whole multiples of 1/2 and 1.0, 0.5, 3.0 are exact.
K_ORACLE: Dict[str, Dict[str, float]] = {
    "generic": {"position": 1.52, "quaternion": 1.0, "rotvec": 1.59},
    "switch": {"position": 1.62, "quaternion": 1.0, "rotvec": 1.85},
    "tiny": {"position": 3.06, "quaternion": 3.0, "rotvec": 2.50},
    "rot2quat": {"position": 0.999, "quaternion": 1.0, "rotvec": 0.717},
    "sign": {"position": 0.975, "quaternion": 1.0, "rotvec": 1.29},
    "qsolver": {"position": 0.920, "quaternion": 0.5, "rotvec": 0.667},
    "kept": {"position": 0.545, "quaternion": 0.5, "rotvec": 0.955},
    "sizes": {"position": 0.613, "quaternion": 1.0, "rotvec": 0.956},
    "ksteps": {"position": 0.841, "quaternion": 1.0, "rotvec": 1.10, "norm": 0.743},
    # (the values of this family ARE the oracle's outputs, so its own ratios are 0: the bar is the generic family's, whose steps these are)
    "drifted": {"position": 1.52, "quaternion": 1.0, "rotvec": 1.59, "norm_abs": 4.80e-12},
}
assert set(K_ORACLE) == set(FAMILIES)
REF_MULTIPLE = 4  # the device's libm over the host's: the figure of tests/test_gpu_rbd_exact.py


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def _unit(a):
    a = np.asarray(a, dtype=np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _quat_axis_angle(axis, angle, sign=1.0):
    axis = _unit(axis)
    return sign * np.concatenate([np.sin(0.5 * angle) * axis, [np.cos(0.5 * angle)]])


def _random_quats(rng, n):
    u = _unit(rng.standard_normal((n, 4)))
    while np.abs(u[:, 3]).min() < 0.2:  # a small step keeps |w| away from 0, where the rotation vector's axis flips
        u = _unit(rng.standard_normal((n, 4)))
    u[:, 3] = np.abs(u[:, 3]) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)  # both signs of w
    return u


def _exact_quats(rng, n):
    """Unit quaternions that float32 holds EXACTLY: (+-1/2, +-1/2, +-1/2, +-1/2).  With the identity and the half turns about x, y, z these are the
    only ones -- 4^k is a sum of four squares in 24 ways -- so a launch that both handles read takes its integrated instances' quaternions from
    here, w of both signs."""
    u = 0.5 * rng.choice([-1.0, 1.0], size=(n, 4))
    u[:, 3] = 0.5 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return u


def _f32_unit(quat):
    """The float32 quaternion nearest to unit norm within two ulps of each component of float32(quat): what an F32 handle can be given at best.
    Its rotation matrix in the reference's formulation is R + (|q|^2 - 1)(R - I), so what is left of |q|^2 - 1 (1e-9, against eps32 = 1.2e-7)
    counts against the F32 bar."""
    q = np.asarray(quat, dtype=np.float32)
    best, best_d = q, np.inf
    steps = []
    for c in q:
        a = [c]
        lo = hi = c
        for _ in range(2):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            a += [lo, hi]
        steps.append(a)
    for a in steps[0]:
        for b in steps[1]:
            for c in steps[2]:
                for d in steps[3]:
                    u = np.array([a, b, c, d], dtype=np.float64)
                    dd = abs(float((u * u).sum()) - 1.0)
                    if dd < best_d:
                        best, best_d = u, dd
    return best


class _Group:
    """Collects the instances of one launch.  Floating base: nv = 6 + nj."""

    def __init__(self, rng, fb=True, nj=2, dt=DT, ldx_pad=0, qs=True, f64=True, f32=False):
        self.rng, self.fb, self.nj, self.dt, self.ldx_pad, self.qs, self.f64, self.f32 = rng, fb, nj, dt, ldx_pad, qs, f64, f32
        self.q, self.dq, self.dv, self.status = [], [], [], []

    def add(self, p=None, quat=None, v=None, w=None, a=None, status=0):
        """One instance: base position, quaternion, body twist (v, w) such that v_next = (v, w) EXACTLY (dv = 0 on the base) unless a is given
        (the base's accelerations); joints and their velocities and accelerations are random."""
        r, nj = self.rng, self.nj
        if self.fb:
            q = np.concatenate([p, quat, r.uniform(-1.5, 1.5, nj)])
            dq = np.concatenate([v, w, r.standard_normal(nj)])
            dv = np.concatenate([np.zeros(6) if a is None else a, 5.0 * r.standard_normal(nj)])
        else:
            q, dq, dv = r.uniform(-1.5, 1.5, nj), r.standard_normal(nj), 5.0 * r.standard_normal(nj)
        self.q.append(q); self.dq.append(dq); self.dv.append(dv); self.status.append(status)

    def done(self, with_status=None) -> Dict[str, np.ndarray]:
        q, dq, dv = np.array(self.q), np.array(self.dq), np.array(self.dv)
        status = np.array(self.status, dtype=np.int32)
        if self.f32:  # inputs that float32 represents
            quat = q[:, 3:7].copy() if self.fb else None
            q, dq, dv = _f32(q), _f32(dq), _f32(dv)
            for i in range(q.shape[0] if self.fb else 0):
                if status[i] != 0:
                    continue  # (a kept state's rotation vector does not depend on the norm)
                if self.f64:  # both handles read it: unit in double AND a float32
                    assert (q[i, 3:7] * q[i, 3:7]).sum() == 1.0 and np.array_equal(q[i, 3:7], quat[i]), "take it from _exact_quats"
                else:
                    q[i, 3:7] = _f32_unit(quat[i])
        nv = dq.shape[1]
        x = np.full((q.shape[0], nv + self.ldx_pad), np.nan)
        x[:, :nv] = dv
        x[status != 0] = np.nan  # a QP that was not solved left no solution
        g = dict(fb=np.int32(self.fb), nv=np.int32(nv), dt=np.float64(self.dt), ldx=np.int32(nv + self.ldx_pad), qs=np.int32(self.qs),
                 f64=np.int32(self.f64), f32=np.int32(self.f32), q=q, dq=dq, x=x)
        if (status != 0).any() if with_status is None else with_status:
            g["status"] = status
        return g


def _oblique(rng):
    a = _unit(rng.standard_normal(3))
    while np.abs(a).min() < 0.2:  # no component near zero
        a = _unit(rng.standard_normal(3))
    return a


def _generic(rng):
    out = {}
    for f32 in (False, True):
        g = _Group(rng, f64=not f32, f32=f32)
        quats = _random_quats(rng, 16)
        for i, t in enumerate((1e-3, 0.1, 1.0, 2.5) * 4):
            p = _unit(rng.standard_normal(3)) * rng.uniform(1.0, 3.0)
            g.add(p, quats[i], rng.standard_normal(3), _oblique(rng) * t / DT, a=5.0 * rng.standard_normal(6))
        # a screw step that the translation dominates, v parallel to w (w x v = 0: no (1 - cos t) / t^2 loss hides the rest), t up to 1e-3:
        # alpha_v v + alpha_w w = v exactly, and a Taylor series carried too far up (t^4 / 120 = 37 eps at 1e-3) shows
        for i, t in enumerate((1e-3, 0.8e-3, 0.5e-3, 1e-3)):
            ax = _oblique(rng)
            g.add(1e-3 * _unit(rng.standard_normal(3)), quats[i], ax * (1.0 / DT) * (1 if i % 2 else -1), ax * t / DT)
        out["f32" if f32 else "all"] = g.done()
    return out


def switch_ts():
    """t on a coordinate axis: 1e-4 itself, its two neighbouring doubles, 1e-4 (1 +- 2^-k)."""
    ts = [SWITCH, float(np.nextafter(SWITCH, 0.0)), float(np.nextafter(SWITCH, 1.0))]
    return ts + [SWITCH * (1.0 + s * 2.0 ** -k) for k in (1, 10, 20, 40) for s in (-1.0, 1.0)]


def _switch(rng):
    out = {}
    ts = switch_ts()
    for f32 in (False, True):
        for dominant in ("position", "translation"):
            g = _Group(rng, dt=DT2, f64=not f32, f32=f32)
            for kind in ("axis", "oblique"):
                for i, t in enumerate(ts if kind == "axis" else ts[3:]):  # (an oblique t is no chosen double: the ties are the axis's)
                    ax = np.eye(3)[i % 3] * (1.0 if i % 2 else -1.0) if kind == "axis" else _oblique(rng)
                    quat = _random_quats(rng, 2)[i % 2]
                    if dominant == "position":
                        p, v = _unit(rng.standard_normal(3)), _unit(rng.standard_normal(3))
                    else:
                        p, v = 1e-3 * _unit(rng.standard_normal(3)), _oblique(rng) / DT2
                    g.add(p, quat, v, ax * (t / DT2))
            out["%s_%s" % (dominant, "f32" if f32 else "f64")] = g.done()
    return out


def _tiny(rng):
    g = _Group(rng, dt=DT2)
    for dominant in ("position", "translation"):
        for w in (np.zeros(3), np.array([0.0, 1e-8 / DT2, 0.0]), _oblique(rng) * 1e-8 / DT2, np.array([1e-170 / DT2, 0.0, 0.0]),
                  _oblique(rng) * 1e-170 / DT2):
            for quat in _random_quats(rng, 2):
                p, v = (_unit(rng.standard_normal(3)), rng.standard_normal(3)) if dominant == "position" else \
                    (1e-3 * _unit(rng.standard_normal(3)), _oblique(rng) / DT2)
                g.add(p, quat, v, w)
    return {"all": g.done()}


def _rot2quat(rng):
    g = _Group(rng)
    third = 2.0 * np.pi / 3.0
    p = lambda: _unit(rng.standard_normal(3)) * rng.uniform(1.0, 3.0)  # noqa: E731
    for d in (1e-6, -1e-6, 1e-12, -1e-12):  # the trace of the result just either side of 0
        ax = _oblique(rng)
        g.add(p(), _quat_axis_angle(ax, third + d), rng.standard_normal(3), np.zeros(3))                      # as given
        g.add(p(), _quat_axis_angle(ax, 0.5 * third, -1.0), rng.standard_normal(3), ax * (0.5 * third + d) / DT)  # reached by the step
    for k in range(3):  # half turns and near-half turns about x, y, z: the three explicit cases
        e = np.eye(3)[k]
        half = np.concatenate([e, [0.0]])
        g.add(p(), half, rng.standard_normal(3), np.zeros(3))
        g.add(p(), half, rng.standard_normal(3), _oblique(rng) * 1e-3 / DT)
        g.add(p(), _quat_axis_angle(e, np.pi - 1e-9), rng.standard_normal(3), np.zeros(3))
        g.add(p(), _quat_axis_angle(e, np.pi - 1e-9, -1.0), rng.standard_normal(3), _oblique(rng) * 1e-3 / DT)
        g.add(p(), _quat_axis_angle(e, 0.5 * np.pi), rng.standard_normal(3), e * (0.5 * np.pi - 1e-9) / DT)
    for ax in ((1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0)):  # near-ties of two diagonal entries
        g.add(p(), _quat_axis_angle(ax, np.pi - 1e-9), rng.standard_normal(3), np.zeros(3))
        g.add(p(), _quat_axis_angle(ax, 0.5 * np.pi), rng.standard_normal(3), _unit(ax) * (0.5 * np.pi - 1e-9) / DT)
    return {"all": g.done()}


def _sign(rng):
    g = _Group(rng)
    for t in (4.0, 2.5):  # cos(t / 2) = -0.42: the kernel must flip; +0.32: it must not
        for quat in _random_quats(rng, 4):
            g.add(_unit(rng.standard_normal(3)) * rng.uniform(1.0, 3.0), quat, rng.standard_normal(3), _oblique(rng) * t / DT)
    for quat in _random_quats(rng, 4):
        g.add(_unit(rng.standard_normal(3)), -np.abs(quat), rng.standard_normal(3), _oblique(rng) * 1e-2 / DT)  # w < 0 stays w < 0
    return {"all": g.done()}


def _qsolver(rng):
    g = _Group(rng)
    g.add(np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(3))            # identity, zero twist: nn == 0, exact +0
    g.add(np.array([1.0, -2.0, 0.5]), np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(3))
    for angle in (1e-9, 1e-3, 3.0):
        for sign in (1.0, -1.0):
            ax = _oblique(rng)
            g.add(_unit(rng.standard_normal(3)), _quat_axis_angle(ax, angle, sign), np.zeros(3), np.zeros(3))
            g.add(_unit(rng.standard_normal(3)), _quat_axis_angle(ax, angle, sign), rng.standard_normal(3), ax * 1e-3 * min(1.0, angle) / DT)
    return {"all": g.done()}


def _kept(rng):
    out = {}
    codes = (0,) + HQP_NOT_OPTIMAL
    for fb in (True, False):
        g = _Group(rng, fb=fb, nj=3 if fb else 4, ldx_pad=5, f32=True)
        quats = list(_random_quats(rng, 6)) + [np.array([0.0, 0.0, 0.0, 1.0])] * 6 + list(-np.abs(_random_quats(rng, 6)))
        exact = _exact_quats(rng, 18)  # (the integrated rows among them: both handles read this launch)
        for i in range(18):
            g.add(_unit(rng.standard_normal(3)) * 2.0, quats[i] if codes[i % 6] else exact[i], rng.standard_normal(3), rng.standard_normal(3) * (i % 3),
                  a=rng.standard_normal(6), status=codes[i % 6])
        out["floating" if fb else "fixed"] = g.done()
    g = _Group(rng, f32=True)  # status = NULL: every instance is integrated
    for quat in _exact_quats(rng, 5):
        g.add(_unit(rng.standard_normal(3)) * 2.0, quat, rng.standard_normal(3), rng.standard_normal(3), a=rng.standard_normal(6))
    out["null_status"] = g.done(with_status=False)
    return out


SIZES_NV = {True: (6, 7, 63, 64, 65, 126), False: (1, 2, 63, 64, 65, 126)}
# batch -> (ldx - nv, q_solver given): the last block holds 1, 3, 4, 1 wavefronts.  The small nv meet all four; the large ones two each (what a
# large nv can get wrong is the lane loop, what a batch can get wrong is the last block), each with both ldx and both q_solver
SIZES_BATCH = {1: (0, True), 3: (13, False), 4: (13, True), 5: (0, False)}
SIZES_LARGE = {63: ((1, 13, True), (5, 0, False)), 64: ((3, 0, False), (4, 13, True)), 65: ((5, 13, True), (1, 0, False)),
               126: ((3, 13, False), (4, 0, True))}


def sizes_of(nv):
    """(batch, ldx - nv, q_solver given) of every launch at this nv."""
    return SIZES_LARGE.get(nv, tuple((b, pad, qs) for b, (pad, qs) in SIZES_BATCH.items()))


def _sizes(rng):
    out = {}
    for fb in (True, False):
        for nv in SIZES_NV[fb]:
            for batch, pad, qs in sizes_of(nv):
                g = _Group(rng, fb=fb, nj=nv - 6 if fb else nv, ldx_pad=pad, qs=qs, f32=True)
                for i, quat in enumerate(_exact_quats(rng, batch)):
                    # (the fourth of five was not solved: a kept row between integrated ones)
                    g.add(_unit(rng.standard_normal(3)) * 2.0, quat, rng.standard_normal(3), rng.standard_normal(3), a=rng.standard_normal(6),
                          status=1 if (batch == 5 and i == 3) else 0)
                out["%s_nv%d_b%d" % ("fl" if fb else "fx", nv, batch)] = g.done(with_status=batch >= 4)
    return out


def _ksteps(rng):
    g = _Group(rng, nj=0)
    for t in (0.9e-4, 2e-3, 0.05):
        for quat in _random_quats(rng, 4):
            g.add(_unit(rng.standard_normal(3)) * rng.uniform(1.0, 3.0), quat, rng.standard_normal(3), _oblique(rng) * t / DT)
    return {"all": g.done()}


def _drifted(rng):
    g = _Group(rng)
    for i, t in enumerate((1e-3, 0.1, 1.0, 2.5) * 3):
        quat = _random_quats(rng, 2)[i % 2] * (1.0 + (1e-6 if i % 4 < 2 else -1e-6))
        g.add(_unit(rng.standard_normal(3)) * rng.uniform(1.0, 3.0), quat, rng.standard_normal(3), _oblique(rng) * t / DT, a=5.0 * rng.standard_normal(6))
    return {"all": g.done()}


_MAKERS = dict(generic=_generic, switch=_switch, tiny=_tiny, rot2quat=_rot2quat, sign=_sign, qsolver=_qsolver, kept=_kept, sizes=_sizes,
               ksteps=_ksteps, drifted=_drifted)


@functools.lru_cache(maxsize=None)
def inputs(family) -> Dict[str, Dict[str, np.ndarray]]:
    """group -> the inputs of the launch (see the module's docstring), from a generator seeded by the family."""
    return _MAKERS[family](np.random.default_rng(31_000 + FAMILIES.index(family)))


def path(family):
    return os.path.join(GOLDEN, family + ".npz")


@functools.lru_cache(maxsize=None)
def load(family) -> Dict[str, Dict[str, np.ndarray]]:
    """group -> key -> array of the committed fixture."""
    out: Dict[str, Dict[str, np.ndarray]] = {}
    with np.load(path(family)) as z:
        for k in z.files:
            g, key = k.split(".", 1)
            out.setdefault(g, {})[key] = z[k]
    return out


def flat(groups) -> Dict[str, np.ndarray]:
    return {"%s.%s" % (g, k): a for g, G in groups.items() for k, a in G.items()}


def handles(G) -> List[str]:
    return [t for t in ("f64", "f32") if int(G[t])]


# ---- the bar -----------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def ratios(x, value, scale, eps=EPS):
    """|x - value| / (eps scale) per entry.  scale 0: bit for bit (against `value` rounded to x's type: it is representable there), 0 or inf.
    scale inf: not judged, 0.  A NaN or an infinity in x is inf whatever the scale."""
    x, value, scale = np.asarray(x), np.asarray(value, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    assert x.shape == value.shape == scale.shape, (x.shape, value.shape, scale.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(x.astype(np.float64) - value) / (eps * scale)
    r = np.where(np.isinf(scale), 0.0, r)
    r = np.where(scale == 0.0, np.where(_bits(x) == _bits(value.astype(x.dtype)), 0.0, np.inf), r)
    return np.where(np.isfinite(x.astype(np.float64)) & ~np.isnan(r), r, np.inf)


def split(G, what, x, tag="f64", prefix=""):
    """The three judged quantities of one output of group G (what: "q_next" or "q_solver"): quantity -> ratios.  Everything outside the base's
    entries (joints, a fixed base) is bit for bit and is reported with the position."""
    eps = EPS if tag == "f64" else EPS32
    r = ratios(x, G[prefix + what], G["%sscale.%s" % (prefix, what)], eps)
    if not int(G["fb"]):
        return {"position": r}
    if what == "q_next":
        return {"position": np.concatenate([r[:, :3], r[:, 7:]], axis=1), "quaternion": r[:, 3:7]}
    return {"position": np.concatenate([r[:, :3], r[:, 6:]], axis=1), "rotvec": r[:, 3:6]}


def worst(G, outs, tag="f64", prefix="") -> Dict[str, float]:
    """quantity -> the worst ratio over q_next and q_solver (where given) of `outs`; v_next is bit for bit and counts as position."""
    w = {k: 0.0 for k in QUANTITIES}
    for what in ("q_next", "q_solver"):
        if outs.get(what) is not None:
            for k, r in split(G, what, outs[what], tag, prefix).items():
                w[k] = max(w[k], float(r.max()) if r.size else 0.0)
    if outs.get("v_next") is not None:
        v = G[prefix + "v_next"]
        w["position"] = max(w["position"], float(ratios(outs["v_next"], v, np.zeros(v.shape)).max()))
    return w


def norm_defect(quat) -> np.ndarray:
    """| |q| - 1 | per row, the norm in long double (its own rounding is 1e-19)."""
    u = np.asarray(quat).astype(np.longdouble)
    return np.abs(np.sqrt((u * u).sum(axis=-1)) - 1).astype(np.float64)
