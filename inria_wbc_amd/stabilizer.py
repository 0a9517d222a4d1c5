"""The humanoid controllers' stabiliser: a numpy transcription of what the reference does around a solve, the yardstick of wbcqp_stabilize.

    step(stab, state, inputs)      one tick for a batch: CoP estimator (src/estimators/cop.cpp there), its moving averages
                                   (include/inria_wbc/estimators/filtering.hpp), the force filters and the admittance laws
                                   (src/controllers/humanoid_pos_tracker.cpp:134-302, src/stabilizers/stabilizer.cpp) on a reference row
    zmp_distribute, zmp_admittance the ZMP force distributor (stabilizer.cpp:277-311, 340-440): the weight split between the feet, a 6-D force reference each
    ZmpDistributor, ZmpLatch       its gains and reference-row offsets (capi.Handle.stabilize_zmp); which robots have moved to the zmp_w slot of a mixed tick
    euler_012 / recompose          Eigen's eulerAngles(0, 1, 2) [UPSTREAM-RECALL] and Rx Ry Rz back, in any float type (np.longdouble for a scale)
    Stabilizer, from_taskmap       what describes a stabiliser to the library (capi.Handle.stabilize), offsets found by task name
    TALOS_GAINS                    the gains of the reference's shipped stabiliser files, as constants

Everything here runs on the host, one Python float operation per rounding, and is deliberately slow and literal: every product, sum and
quotient rounds once, in the reference's association.  The state is the library's, byte for byte (include/wbcqp.h): per instance
[5]{int32 count, int32 head} of the filters combined / left / right CoP, left / right force z, then the ring [window][8] of samples.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

MAX_WINDOW = 64
FMIN = 30.0  # Cop::fmin(): a float compared as 30.0
COP, LCOP, RCOP, COM, LANKLE, RANKLE, FFDA, ERR_COP, ERR_FORCE = 1, 2, 4, 8, 16, 32, 64, 128, 256
ZMP, ERR_ZMP = 512, 1024
N_FILTERS, N_CHANNELS = 5, 8
F_COP, F_LCOP, F_RCOP, F_LFORCE, F_RFORCE = range(5)
_CHANNELS = ((0, 1), (2, 3), (4, 5), (6,), (7,))  # a filter's channels in the ring

# The reference's shipped stabiliser files (etc/<robot>/stab_fixed_base.yaml, stab_single_support.yaml, stab_double_support.yaml): filter_size, com,
# ankle, ffda per behaviour type, and zmp_p, zmp_d, zmp_w where the file has use_zmp: true (Talos' support files).  The C ABI runs that law
# (wbcqp_stabilize_zmp); the C++ facade does not, so tools/emit_configs.py keeps writing use_zmp: false.
_COM = (0.001, 0.001, 0.0003, 0.0003, 0.00000003, 0.00000003)
_ANKLE = (0.25, 0.25, 0.0001, 0.001, 0.00001, 0.00001)
_ZERO6, _ZERO3 = (0.0,) * 6, (0.0,) * 3
_ZMP_P, _ZMP_D = (0.0, 0.0, 2.0, 10.0, 10.0, 0.0), (0.0, 0.0, 0.0005, 0.0001, 0.002, 0.0)
_ZMP_SS = dict(zmp_p=_ZMP_P, zmp_d=_ZMP_D, zmp_w=(1.0, 1.0, 0.01, 2.0, 2.0, 2.0))
_ZMP_DS = dict(zmp_p=_ZMP_P, zmp_d=_ZMP_D, zmp_w=(1.0, 1.0, 1.0, 2.0, 2.0, 2.0))
_ZMP_OFF = dict(zmp_p=_ZERO6, zmp_d=_ZERO6, zmp_w=_ZERO6)
STAB_FILES = {
    "talos": {"fixed_base": dict(window=7, com_gains=_ZERO6, ankle_gains=_ZERO6, ffda_gains=_ZERO3, **_ZMP_OFF),
              "single_support": dict(window=5, com_gains=_COM, ankle_gains=_ANKLE, ffda_gains=_ZERO3, **_ZMP_SS),
              "double_support": dict(window=7, com_gains=_COM, ankle_gains=_ANKLE, ffda_gains=(0.0003, 0.0, 0.0), **_ZMP_DS)},
    "icub": {"fixed_base": dict(window=7, com_gains=_ZERO6, ankle_gains=_ZERO6, ffda_gains=_ZERO3),
             "single_support": dict(window=7, com_gains=_COM, ankle_gains=_ZERO6, ffda_gains=_ZERO3),
             "double_support": dict(window=7, com_gains=_COM, ankle_gains=_ZERO6, ffda_gains=(0.0003, 0.0, 0.0))},
}
TALOS_GAINS = STAB_FILES["talos"]["double_support"]


def stab_file_text(cfg: dict, use_zmp: bool = False) -> str:
    """A stabiliser file in the reference's schema from one entry of STAB_FILES."""
    fmt = lambda v: "[" + ", ".join(repr(float(x)) for x in v) + "]"  # noqa: E731
    return "filter_size: %d\ncom: %s\nankle: %s\nffda: %s\nuse_zmp: %s\n" % (cfg["window"], fmt(cfg["com_gains"]), fmt(cfg["ankle_gains"]),
                                                                          fmt(cfg["ffda_gains"]), "true" if use_zmp else "false")


@dataclass
class Stabilizer:
    """wbcqp_stabilizer, member for member."""
    window: int
    dt: float
    mass: float
    com_gains: Sequence[float]
    ankle_gains: Sequence[float]
    ffda_gains: Sequence[float]
    nref: int
    com_ref: int
    lf_ref: int
    rf_ref: int
    torso_ref: int
    lf_contact_ref: int = -1
    rf_contact_ref: int = -1
    lf_force_col: int = -1
    rf_force_col: int = -1
    normal: Sequence[float] = (0.0, 0.0, 1.0)
    lf_pos: int = 9   # observed frame 0's translation in a row of wbcqp_observables.placement
    rf_pos: int = 21  # observed frame 1's


@dataclass
class ZmpDistributor:
    """wbcqp_zmp_distributor, member for member: zmp_p, zmp_d and where the two feet's 6-number force references lie in a reference row (-1: not
    written)."""
    p: Sequence[float]
    d: Sequence[float]
    lf_force_ref: int = -1
    rf_force_ref: int = -1


def zmp_from_taskmap(tm, stack: Sequence[dict], p, d, names: Optional[Dict[str, str]] = None) -> ZmpDistributor:
    """The distributor of a task map built with force_refs=True: the feet's blocks of TaskMap.contact_fref by the contacts' names in the WHOLE
    stack's order (the blocks sit at one offset in every contact set's map)."""
    nm = dict(lf_contact="contact_lfoot", rf_contact="contact_rfoot")
    nm.update(names or {})
    contacts = [n["name"] for n in stack if n["type"] == "contact"]
    fref = tm.contact_fref_all if getattr(tm, "contact_fref_all", None) is not None else tm.contact_fref
    assert fref is not None and len(fref) == len(contacts), "build the task map with force_refs=True"
    at = lambda name: int(fref[contacts.index(name)]) if name in contacts else -1  # noqa: E731
    return ZmpDistributor(p=tuple(p), d=tuple(d), lf_force_ref=at(nm["lf_contact"]), rf_force_ref=at(nm["rf_contact"]))


class ZmpLatch:
    """Which slot of a mixed tick every robot is ticked in: the reference sets zmp_w on the contacts the first time the law runs for a robot and never
    sets it back.  update(flags) after a tick's stabilize_zmp; which(default, zmp) -> the int32 `which` array of the next wbcqp_tick_mixed, where
    default / zmp are the indices into wbcqp_mix.slots (scalars, or arrays per robot: three contact sets x two weightings)."""

    def __init__(self, batch: int):
        self.latched = np.zeros(int(batch), bool)

    def update(self, flags) -> np.ndarray:
        self.latched |= (np.asarray(flags).astype(np.int64).reshape(-1) & ZMP) != 0
        return self.latched

    def which(self, default=0, zmp=1) -> np.ndarray:
        return np.where(self.latched, zmp, default).astype(np.int32)


def state_bytes(window: int) -> int:
    return 8 * (N_FILTERS + N_CHANNELS * int(window))


def from_taskmap(model, tm, stack: Sequence[dict], window: int, com_gains, ankle_gains, ffda_gains, contacts: Optional[Sequence[str]] = None,
                 normal: Sequence[float] = (0.0, 0.0, 1.0), lf_slot: int = 0, rf_slot: int = 1, names: Optional[Dict[str, str]] = None) -> Stabilizer:
    """The stabiliser of a task map: the offsets of the tasks `com`, `lf`, `rf`, `torso` and of the contacts `contact_lfoot`, `contact_rfoot` by
    name (names: other names for these six roles).  contacts: the names of tm's contacts in tm's order (default: every contact of the stack, as
    build_taskmap keeps them; a single-support map of contact_set_maps names its one contact) -- a foot whose contact is not among them is not
    active (-1).  lf_slot / rf_slot: which observed frame is the left / right ankle, i.e. the frame its contact tracks."""
    nm = dict(com="com", lf="lf", rf="rf", torso="torso", lf_contact="contact_lfoot", rf_contact="contact_rfoot")
    nm.update(names or {})
    ref = {b.name: int(b.ref) for b in tm.blocks}
    for role in ("com", "lf", "rf", "torso"):
        if nm[role] not in ref:
            raise KeyError("the stabilizer needs the task [%s]" % nm[role])
    if contacts is None:
        contacts = [n["name"] for n in stack if n["type"] == "contact"]
    assert len(contacts) == tm.ncontact, (contacts, tm.ncontact)

    def contact(name):
        if name not in contacts:
            return -1, -1
        c = list(contacts).index(name)
        return int(tm.contact_ref[c]), int(model.nv + 12 * c)

    (lc, lcol), (rc, rcol) = contact(nm["lf_contact"]), contact(nm["rf_contact"])
    return Stabilizer(window=int(window), dt=float(tm.dt), mass=float(model.inertia[:, 0].sum()), com_gains=tuple(com_gains), ankle_gains=tuple(ankle_gains),
                      ffda_gains=tuple(ffda_gains), nref=int(tm.nref), com_ref=ref[nm["com"]], lf_ref=ref[nm["lf"]], rf_ref=ref[nm["rf"]],
                      torso_ref=ref[nm["torso"]], lf_contact_ref=lc, rf_contact_ref=rc, lf_force_col=lcol, rf_force_col=rcol, normal=tuple(normal),
                      lf_pos=12 * lf_slot + 9, rf_pos=12 * rf_slot + 9)


# ---- rotations ------------------------------------------------------------------------------------------------------------------------------
class _Lib:
    """The elementary functions of one float type."""
    def __init__(self, ty, atan2, sin, cos, sqrt):
        self.ty, self.atan2, self.sin, self.cos, self.sqrt = ty, atan2, sin, cos, sqrt


DOUBLE = _Lib(float, math.atan2, math.sin, math.cos, math.sqrt)
LONGDOUBLE = _Lib(np.longdouble, np.arctan2, np.sin, np.cos, np.sqrt)


def euler_012(Rc, lib: _Lib = DOUBLE, margins: Optional[list] = None):
    """Eigen's eulerAngles(0, 1, 2) of a rotation given column-major (9 numbers, a reference's layout) [UPSTREAM-RECALL: Eigen/src/Geometry/
    EulerAngles.h]: the first angle in [0, pi].  -> (e0, e1, e2, whether the r0 > 0 branch was taken)."""
    t = lib.ty
    R00, R10, R20, R01, R11, R21, R02, R12, R22 = (t(x) for x in Rc)
    r0 = lib.atan2(R12, R22)
    c2 = lib.sqrt(R00 * R00 + R01 * R01)
    if margins is not None and not (R12 == 0 and R22 > 0):  # (atan2(+-0, positive) is +-0 in every libm: an exact decision, e.g. an identity)
        margins.append(("r0 > 0", float(r0), 0.0, math.pi))
    flipped = bool(r0 > 0)
    if flipped:
        r0 = r0 - t(math.pi)  # (EIGEN_PI as a double, whatever the type)
        r1 = lib.atan2(-R02, -c2)
    else:
        r1 = lib.atan2(-R02, c2)
    s1, c1 = lib.sin(r0), lib.cos(r0)
    a = s1 * R20
    b = c1 * R10
    c = c1 * R11
    d = s1 * R21
    r2 = lib.atan2(a - b, c - d)
    return -r0, -r1, -r2, flipped


def rot_xyz(a, b, c, lib: _Lib = DOUBLE):
    """Rx(a) Ry(b) Rz(c), column-major; an entry that is zero comes out as +0 (an identity gives back the bits of an identity)."""
    t = lib.ty
    sa, ca, sb, cb, sc, cc = lib.sin(a), lib.cos(a), lib.sin(b), lib.cos(b), lib.sin(c), lib.cos(c)
    sasb = sa * sb
    casb = ca * sb
    z = t(0.0)
    p = [cb * cc, ca * sc, sasb * cc, sa * sc, casb * cc, cb * sc, ca * cc, sasb * sc, sa * cc, casb * sc, sa * cb, ca * cb]
    return [p[0] + z, (p[1] + p[2]) + z, (p[3] - p[4]) + z,
            (-p[5]) + z, (p[6] - p[7]) + z, (p[8] + p[9]) + z,
            sb + z, (-p[10]) + z, p[11] + z]


def recompose(Rc, d0, d1, lib: _Lib = DOUBLE, margins: Optional[list] = None):
    """The rotation Rx(e0 + d0) Ry(e1 + d1) Rz(e2) for (e0, e1, e2) = euler_012(Rc), column-major."""
    e0, e1, e2, _ = euler_012(Rc, lib, margins)
    return rot_xyz(e0 + lib.ty(d0), e1 + lib.ty(d1), e2, lib)


# ---- one tick -------------------------------------------------------------------------------------------------------------------------------
class _Filters:
    """The five moving averages of one instance on the library's state bytes (a float64 row of 5 + 8 window numbers)."""

    def __init__(self, row: np.ndarray, window: int):
        self.w = int(window)
        self.ch = row.view(np.int32)[:2 * N_FILTERS].reshape(N_FILTERS, 2)  # count, head
        self.ring = row[N_FILTERS:].reshape(self.w, N_CHANNELS)

    def push(self, f: int, sample: Sequence[float]) -> List[float]:
        count, head = int(self.ch[f, 0]), int(self.ch[f, 1])
        for c, x in zip(_CHANNELS[f], sample):
            self.ring[head, c] = x
        head = (head + 1) % self.w
        count = min(count + 1, self.w)
        self.ch[f] = (count, head)
        # oldest first, one division by the count, no running sum.  (np.cumsum adds a 1-D array strictly left to right, one rounding per element;
        # the leading 0.0 is the accumulator the sum starts from: it only matters for the sign of a zero)
        order = (head - count + np.arange(count)) % self.w
        return [(0.0 + float(np.cumsum(self.ring[order, c])[-1])) / float(count) for c in _CHANNELS[f]]

    def reset(self, f: int) -> None:
        self.ch[f] = (0, 0)  # (the ring's stale samples stay where they are and are never read)

    def ready(self, f: int) -> bool:
        return int(self.ch[f, 0]) >= self.w


def _foot_cop(pos, torque, force):
    t1 = pos[2] * force[0]
    t2 = pos[2] * force[1]
    return [pos[0] + (-torque[1] - t1) / force[2], pos[1] + (torque[0] - t2) / force[2]]


def _norm(f):
    a, b, c = f[0] * f[0], f[1] * f[1], f[2] * f[2]
    return math.sqrt((a + b) + c)


def _normal_force(n, f12):
    s = 0.0
    for i in range(4):
        a, b, c = n[0] * f12[3 * i], n[1] * f12[3 * i + 1], n[2] * f12[3 * i + 2]
        s = s + ((a + b) + c)
    return s


def _far(x, y, margins):
    if margins is not None:
        margins += [("|cop| >= 10", abs(x), 10.0, 10.0), ("|cop| >= 10", abs(y), 10.0, 10.0)]
    return abs(x) >= 10.0 and abs(y) >= 10.0


def _bump(x, g, angle, den):
    t = g * angle
    return x + t / den


def _div(a, b):
    """a / b as IEEE 754 has it (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _norm2(x, y):
    a, b = x * x, y * y
    return math.sqrt(a + b)


def zmp_distribute(mass, z, PL, PR, left_active=True, right_active=True, margins: Optional[list] = None):
    """stabilizer.cpp:340-440 (zmp_distributor) with closest_point_on_line: -> (alpha, left [6], right [6], ok).  z: the ZMP (2), PL / PR: the xy of
    the left / right contact reference's translation.  Everything is projected to z = 0, so every 3-term sum of the reference has one zero term.
    ok False: the reference throws ("this case should not exists": only non-finite inputs get there); alpha is then NaN and the forces mean nothing."""
    z = [float(z[0]), float(z[1])]
    mass = float(mass)
    ok = True
    if left_active and right_active:
        PL, PR = [float(PL[0]), float(PL[1])], [float(PR[0]), float(PR[1])]
        ux, uy = PR[0] - PL[0], PR[1] - PL[1]
        sq = ux * ux
        t = uy * uy
        sq = sq + t
        if sq > 0.0:  # [UPSTREAM-RECALL: Eigen/src/Core/Dot.h, normalized(): divided by the norm only where the squared norm is > 0]
            ln = math.sqrt(sq)
            ex, ey = ux / ln, uy / ln
        else:
            ex, ey = ux, uy
        a = (z[0] - PR[0]) * ex
        b = (z[1] - PR[1]) * ey
        dd = a + b
        px = PR[0] + ex * dd
        py = PR[1] + ey * dd
        L = _norm2(ux, uy)
        a1 = _norm2(px - PL[0], py - PL[1])
        a2 = _norm2(PR[0] - px, PR[1] - py)
        res = abs((L - a1) - a2)
        if margins is not None:
            margins.append(("on segment", res, 1e-10, 0.0))
        if res < 1e-10:
            alpha = _div(a1, L)  # (coincident feet: 0 / 0, a NaN alpha and no throw)
        else:
            if margins is not None:
                margins.append(("a1 < a2", a1, a2, 0.0))
            if a1 < a2:
                alpha = 0.0
            elif a1 > a2:
                alpha = 1.0
            else:
                alpha, ok = math.nan, False
    elif right_active:
        alpha, PL, PR = 1.0, [0.0, 0.0], [float(PR[0]), float(PR[1])]
    elif left_active:
        alpha, PL, PR = 0.0, [float(PL[0]), float(PL[1])], [0.0, 0.0]
    else:
        raise ValueError("no active foot contact (the reference: is talos jumping ?)")
    f_r = ((-alpha) * mass) * 9.81
    f_l = ((-(1.0 - alpha)) * mass) * 9.81
    tau0 = []
    for k in range(2):
        a = (-(PR[k] - z[k])) * f_r
        b = (PL[k] - z[k]) * f_l
        tau0.append(a - b)
    tauR1 = alpha * tau0[1]
    tauL1 = (1.0 - alpha) * tau0[1]
    if margins is not None:
        margins.append(("tau0[0] < 0", tau0[0], 0.0, mass * 9.81))
    if tau0[0] < 0:
        tauR0, tauL0 = tau0[0], 0.0
    else:
        tauR0, tauL0 = 0.0, tau0[0]
    return alpha, [0.0, 0.0, f_l, tauL1, -tauL0, 0.0], [0.0, 0.0, f_r, tauR1, -tauR0, 0.0], ok


def zmp_admittance(dt, p, d, mass, zmp_ref, cop, PL, PR, left_active=True, right_active=True, margins: Optional[list] = None):
    """stabilizer.cpp:277-311 (zmp_distributor_admittance) without its far-CoP throw (the CoM law's own, on the same CoP): the distribution t of the
    model's ZMP, s of the measured one, fref = (t - p e) - (d e) / dt with e = t - s, per foot and entry.
    -> (left_fref [6], right_fref [6], alpha of the model's ZMP, alpha of the measured one, ok)."""
    at, tl, tr, ok_t = zmp_distribute(mass, zmp_ref, PL, PR, left_active, right_active, margins)
    am, sl, sr, ok_s = zmp_distribute(mass, cop, PL, PR, left_active, right_active, margins)
    out = []
    for t, s in ((tl, sl), (tr, sr)):
        f = []
        for k in range(6):
            e = t[k] - s[k]
            a = float(p[k]) * e
            b = float(d[k]) * e
            f.append((t[k] - a) - b / float(dt))
        out.append(f)
    return out[0], out[1], at, am, ok_t and ok_s


def step(stab: Stabilizer, state: Optional[np.ndarray], inputs: Dict[str, np.ndarray], margins: Optional[list] = None,
         zmp: Optional[ZmpDistributor] = None, zmp_margins: Optional[list] = None) -> Dict[str, np.ndarray]:
    """One tick of the stabiliser for B instances.  inputs: ref [B, nref], wrench [B, 12] (lf_force, lf_torque, rf_force, rf_torque), com [B, 3],
    acom [B, 3], placement [B, ldp], x_prev [B, ldx] or absent / None.  state: a contiguous uint8 array [B, state_bytes(window)], updated in place
    (all-zero bytes: fresh), or None (fresh, discarded).  -> dict(ref_out [B, nref], flags [B] int32, cop [B, 3, 2] with NaN where not valid).
    margins: a list that receives (decision, value, threshold, scale) of every comparison a result depends on.
    zmp: the ZMP force distributor (use_zmp), run exactly when the CoM law runs, after it and before the ankle laws: it writes the two feet's force
    references into their blocks of the row (ZMP), or trips ERR_ZMP like the other guards; the result gains alpha [B, 2] (of the model's ZMP, of the
    measured one; NaN where the law did not run).  zmp_margins: receives the distributor's own decisions ("on segment", "a1 < a2", "tau0[0] < 0")."""
    ref = np.asarray(inputs["ref"], dtype=np.float64)
    B, W = ref.shape[0], int(stab.window)
    wrench, com, acom, place = (np.asarray(inputs[k], dtype=np.float64).reshape(B, -1) for k in ("wrench", "com", "acom", "placement"))
    x_prev = inputs.get("x_prev")
    if x_prev is not None:
        x_prev = np.asarray(x_prev, dtype=np.float64).reshape(B, -1)
    if state is None:
        state = np.zeros((B, state_bytes(W)), np.uint8)
    assert state.dtype == np.uint8 and state.shape == (B, state_bytes(W)) and state.flags["C_CONTIGUOUS"]
    rows = state.view(np.float64)
    out = dict(ref_out=ref.copy(), flags=np.zeros(B, np.int32), cop=np.full((B, 3, 2), np.nan))
    dt = float(stab.dt)
    dt2 = dt * dt
    pc, pa, g, nrm = ([float(x) for x in v] for v in (stab.com_gains, stab.ankle_gains, stab.ffda_gains, stab.normal))
    if zmp is not None:
        assert stab.lf_contact_ref >= 0 or stab.rf_contact_ref >= 0, "no active foot contact (the reference: is talos jumping ?)"
        out["alpha"] = np.full((B, 2), np.nan)
    for i in range(B):
        F = _Filters(rows[i], W)
        lf, lt, rf, rt = ([float(x) for x in wrench[i, 3 * k:3 * k + 3]] for k in range(4))
        lp = [float(x) for x in place[i, stab.lf_pos:stab.lf_pos + 3]]
        rp = [float(x) for x in place[i, stab.rf_pos:stab.rf_pos + 3]]
        if margins is not None:
            margins += [("fz > 30", lf[2], FMIN, FMIN), ("fz > 30", rf[2], FMIN, FMIN), ("|f| > 30", _norm(lf), FMIN, FMIN), ("|f| > 30", _norm(rf), FMIN, FMIN)]
        # ---- the CoP estimator (cop.cpp:10-96) ----
        cops: List[Optional[List[float]]] = [None, None, None]
        lraw = rraw = None
        if lf[2] > FMIN:
            lraw = _foot_cop(lp, lt, lf)
            cops[1] = F.push(F_LCOP, lraw)
        else:
            F.reset(F_LCOP)
        if rf[2] > FMIN:
            rraw = _foot_cop(rp, rt, rf)
            cops[2] = F.push(F_RCOP, rraw)
        else:
            F.reset(F_RCOP)
        if lraw is not None and rraw is not None:
            ratio_l = lf[2] / (lf[2] + rf[2])
            ratio_r = 1.0 - ratio_l
            craw = []
            for k in range(2):
                a = ratio_l * lraw[k]
                b = ratio_r * ((rraw[k] + rp[k]) - lp[k])
                in_l = a + b
                a = ratio_l * ((lraw[k] + lp[k]) - rp[k])
                b = ratio_r * rraw[k]
                in_r = a + b
                a = in_l * ratio_l
                b = in_r * ratio_r
                craw.append(a + b)
            cops[0] = F.push(F_COP, craw)
        for f in (F_COP, F_LCOP, F_RCOP):  # data_ready, then check_nan
            if cops[f] is not None and (not F.ready(f) or math.isnan(cops[f][0]) or math.isnan(cops[f][1])):
                cops[f] = None
        # ---- the force filters (humanoid_pos_tracker.cpp:184-199): only z is ever consumed ----
        fz_l = F.push(F_LFORCE, [lf[2]])[0] if _norm(lf) > FMIN else 0.0
        fz_r = F.push(F_RFORCE, [rf[2]])[0] if _norm(rf) > FMIN else 0.0
        flags = (COP if cops[0] else 0) | (LCOP if cops[1] else 0) | (RCOP if cops[2] else 0)
        for f in range(3):
            if cops[f] is not None:
                out["cop"][i, f] = cops[f]
        valid = cops[0] or cops[1] or cops[2]
        do_l = cops[1] is not None and stab.lf_contact_ref >= 0
        do_r = cops[2] is not None and stab.rf_contact_ref >= 0
        do_f = x_prev is not None and stab.lf_force_col >= 0 and stab.rf_force_col >= 0 and F.ready(F_LFORCE) and F.ready(F_RFORCE)
        # ---- where the reference throws, in its order ----
        err_cop = bool(valid and _far(valid[0], valid[1], margins))
        err_cop = bool(do_l and _far(cops[1][0], cops[1][1], margins)) or err_cop
        err_cop = bool(do_r and _far(cops[2][0], cops[2][1], margins)) or err_cop
        fz = None
        if zmp is not None and valid and not err_cop:  # zmp_distributor_admittance, on the contacts' references as they lie in ref
            la, ra = stab.lf_contact_ref >= 0, stab.rf_contact_ref >= 0
            PL = [float(x) for x in ref[i, stab.lf_contact_ref:stab.lf_contact_ref + 2]] if la else [0.0, 0.0]
            PR = [float(x) for x in ref[i, stab.rf_contact_ref:stab.rf_contact_ref + 2]] if ra else [0.0, 0.0]
            k = float(com[i, 2]) / 9.81
            zref = []
            for c in range(2):
                t = k * float(acom[i, c])
                zref.append(float(com[i, c]) - t)
            fz = zmp_admittance(dt, zmp.p, zmp.d, stab.mass, zref, valid, PL, PR, la, ra, zmp_margins)
        err_zmp = fz is not None and not fz[4]
        err_force = False
        if do_f and not err_cop and not err_zmp:
            mg = stab.mass * 9.81
            ten_mg = 10.0 * mg
            if margins is not None:
                margins.append(("10 M g", abs(fz_l + fz_r), ten_mg, ten_mg))
            err_force = abs(fz_l + fz_r) > ten_mg
        if err_cop or err_zmp or err_force:
            out["flags"][i] = flags | (ERR_COP if err_cop else 0) | (ERR_ZMP if err_zmp else 0) | (ERR_FORCE if err_force else 0)
            continue
        r = out["ref_out"][i]
        if valid:  # com_admittance
            k = float(com[i, 2]) / 9.81
            o = stab.com_ref
            for c in range(2):
                t = k * float(acom[i, c])
                cor = (float(com[i, c]) - t) - valid[c]
                t = pc[c] * cor
                r[o + c] = float(r[o + c]) - t
                t = pc[2 + c] * cor
                r[o + 3 + c] = float(r[o + 3 + c]) - t / dt
                t = pc[4 + c] * cor
                r[o + 6 + c] = float(r[o + 6 + c]) - t / dt2
            flags |= COM
        if fz is not None:
            for o, f in ((zmp.lf_force_ref, fz[0]), (zmp.rf_force_ref, fz[1])):
                if o >= 0:
                    r[o:o + 6] = f
            out["alpha"][i] = (fz[2], fz[3])
            flags |= ZMP
        for do, cop, pos, o, oc, bit in ((do_l, cops[1], lp, stab.lf_ref, stab.lf_contact_ref, LANKLE), (do_r, cops[2], rp, stab.rf_ref, stab.rf_contact_ref, RANKLE)):
            if not do:  # ankle_admittance
                continue
            pitch = pa[0] * (cop[0] - pos[0])
            roll = pa[1] * (cop[1] - pos[1])
            Rn = recompose(r[o + 3:o + 12], roll, pitch, DOUBLE, margins)
            r[o + 12 + 4] = _bump(float(r[o + 12 + 4]), pa[2], pitch, dt)
            r[o + 12 + 3] = _bump(float(r[o + 12 + 3]), pa[3], roll, dt)
            r[o + 18 + 4] = _bump(float(r[o + 18 + 4]), pa[4], pitch, dt2)
            r[o + 18 + 3] = _bump(float(r[o + 18 + 3]), pa[5], roll, dt2)
            r[o + 3:o + 12] = Rn
            r[oc + 3:oc + 12] = Rn
            r[oc + 12:oc + 24] = r[o + 12:o + 24]  # the FOOT TASK's velocity and acceleration, not the contact's own: as the reference
            flags |= bit
        if do_f:  # foot_force_difference_admittance
            nl = _normal_force(nrm, [float(x) for x in x_prev[i, stab.lf_force_col:stab.lf_force_col + 12]])
            nr = _normal_force(nrm, [float(x) for x in x_prev[i, stab.rf_force_col:stab.rf_force_col + 12]])
            zctrl = abs(nl - nr) - abs(fz_l - fz_r)
            troll = g[0] * zctrl
            o = stab.torso_ref
            Rn = recompose(r[o + 3:o + 12], troll, 0.0, DOUBLE, margins)
            r[o + 12 + 3] = _bump(float(r[o + 12 + 3]), g[1], troll, dt)
            r[o + 18 + 3] = _bump(float(r[o + 18 + 3]), g[2], troll, dt2)
            r[o + 3:o + 12] = Rn
            flags |= FFDA
        out["flags"][i] = flags
    return out


def rotation_entries(stab: Stabilizer) -> np.ndarray:
    """Indices into a reference row of the entries that pass through atan2 / sin / cos: the 9 of lf, rf, torso and the active contacts."""
    offs = [stab.lf_ref, stab.rf_ref, stab.torso_ref] + [o for o in (stab.lf_contact_ref, stab.rf_contact_ref) if o >= 0]
    return np.concatenate([np.arange(o + 3, o + 12) for o in offs])


def clear_margin(margins: Sequence[tuple], rel: float = 1e-9) -> None:
    """Asserts that no recorded decision lies within `rel` (relative to its scale) of its threshold."""
    for what, value, threshold, scale in margins:
        assert math.isnan(value) or abs(value - threshold) > rel * max(scale, 1.0), (what, value, threshold)
