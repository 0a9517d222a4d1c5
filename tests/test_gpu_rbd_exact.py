"""The tree kernels' rigid-body terms against the exact statement of tests/rbd_exact.py, ENTRY BY ENTRY: wbcqp_mass_matrix, wbcqp_jacobians,
wbcqp_observe / wbcqp_observe_acom, wbcqp_inverse_dynamics, wbcqp_kinematic_hessians and the rows kernel (wbcqp_problem_data: M, h, the contact
Jacobians, the momentum).

The statement's values and scales are the committed fixtures (tests/golden/rbd_exact/): no mpmath runs here.  The bar of every entry is
    |x - value| <= REF_MULTIPLE K_ORACLE[quantity] eps scale,        a structural zero (scale 0): an exact zero,
K_ORACLE the CPU implementations' measured worst against the same statement (tests/rbd_exact_cases.py, tests/test_rbd_exact_host.py) and REF_MULTIPLE = 4 the figure of
tests/test_gpu_forward_dynamics.py: a second formulation meets each rounding once more.  No factor of it is taken from the kernels under test.
wbcqp_inverse_dynamics and the rows kernel form a subtree's total as scan[last] - scan[body - 1] of whole-robot running totals about the base
(csrc/wbcqp_rnea.hpp, wbcqp_terms.hpp): their M, generalised forces and momentum are held to the same multiple of `scale_total`, and the ratio
against the local `scale` is printed beside it -- the price of the prefix sums on the light links, as a number.  The rows kernel's contact
Jacobians are no running totals: the local scale.

Two corrections of the scale, both read from the kernels' headers and both stated in tests/rbd_exact.py as `scale_world` / `scale_base` (the same
sums with every rotation's lever split at the common origin the kernel forms its columns about):
  * a ZERO LEVER (a frame on its own joint's origin; a leaf whose CoM lies there) has local scale 0, and a body-local recursion writes an exact 0.
    The kernels form every column about one origin -- the world's (wbcqp_jacobians.hpp, wbcqp_observe.hpp), the base (wbcqp_fdyn.hpp,
    wbcqp_terms.hpp) -- and move it to the point: two levers that cancel to rounding.  Where the local scale is 0 and the origin's is not, M, the
    Jacobians, Jcom and Ag are held to the origin's scale; where both are 0 (unrelated branches) to an exact 0; everywhere else to the local scale;
  * the RATES (velocity, vcom, the drifts, acom, dAgv) are sums of products of spatial velocities about the world's origin (wbcqp_observe.hpp:
    ov = R vJ + p x ow, hl = m ov + ow x hc): every term carries the origin's lever, and the scale is `scale_world` throughout.
The multiple does not move and every entry is judged; the ratio against the local scale is printed.  The norm-wise bars of the other test_gpu_*.py
modules stand as they are, next to these.

wbcqp_kinematic_hessians (the fixtures <case>.hessians.npz: H = dJ/dq and dJ/dt in the three conventions) falls under the same two rules, read from
csrc/wbcqp_hessians.hpp:
  * H is a motion cross product of two columns that the kernel forms about the world's origin and moves to the frame ("2. lanes = dofs: lane j's
    world column S_j = (v_j, w_j) about the world's origin", "4. ... lane j forms column j in the convention asked for"): a ZERO LEVER column is two
    levers that cancel to rounding.  H is held to the local scale where it is not 0, to `scale_world` (the same cross product of the columns'
    `scale_world`) where a zero lever leaves the local one 0, to an exact 0 where both are -- the zeros of the header's table, which the statement
    decides from its own values (tests/rbd_exact.py, dependence);
  * dJ is a RATE: "dJ comes in O(1) per column from the bodies' spatial velocities V (world axes, about the world's origin), with
    D_j = V(frame's body) - V(bodyof(j))".  Both path sums hold the whole common ancestry, dof j's own term among it, which the difference and
    S_j x_m S_j cancel to rounding only: `scale_world`, (|V|(frame's body) + |V|(bodyof(j))) x_m |S_j| moved to the frame, throughout.
One launch per entry point (and Jacobian convention) and case, batch = the case's states."""
import numpy as np
import pytest

from inria_wbc_amd import capi, structure
from inria_wbc_amd import model as mdl
from tests import model_queries as mq
from tests import rbd_exact_cases as X  # (fixtures only: no mpmath here)
from tests.rbd_exact_cases import K_ORACLE

pytestmark = pytest.mark.gpu

REF_MULTIPLE = 4
NAMES = list(X.CASES)


@pytest.fixture(scope="module")
def handle():
    yield from mq.open_handle()


def _set(handle, name, slot=3):
    m = X.model(name)
    st, tm = mq.minimal(m, "rbdx_")
    handle.set_structure(slot, st)
    handle.set_model(slot, m, tm)
    return m, X.load(name)


def _local(C, k, origin):
    """(the scale of the bar, the local scale): local, and the origin's where a zero lever leaves the local one at 0."""
    local = C[k + ".scale"]
    return np.where(local == 0.0, C[k + ".scale_" + origin], local), local


def _rate(C, k, origin="world"):
    return C[k + ".scale_" + origin], C[k + ".scale"]


def _judge(kernel, name, checks):
    """checks: (quantity, what the device gave, value, the scale of the bar, the local scale or None).  Prints every ratio over its bar, then asserts."""
    over = []
    for k, x, value, scale, local in checks:
        bar = REF_MULTIPLE * K_ORACLE[k.split(" ")[0]]
        r = X.ratios(x, value, scale)
        zeros_exact = bool(np.isfinite(r).all())
        worst = float(r[np.isfinite(r)].max()) if np.isfinite(r).any() else 0.0
        norm = float(np.abs(x - value).max() / max(1.0, np.abs(value).max()))
        line = "rbd_exact %-18s %-26s %-16s ratio / bar %9.3g  (ratio %9.3g, bar %6.1f)  norm-wise %.1e" % (kernel, name, k, worst / bar, worst, bar, norm)
        if local is not None:
            rl = X.ratios(x, value, local)
            line += "  against the local scale: ratio / bar %9.3g" % (float(rl[np.isfinite(rl)].max()) / bar if np.isfinite(rl).any() else 0.0)
        print(line + ("" if zeros_exact else "  A STRUCTURAL ZERO IS NOT AN EXACT ZERO at %s" % np.argwhere(~np.isfinite(r))[:6].tolist()))
        if not zeros_exact or worst > bar:
            over.append((k, worst / bar, zeros_exact))
    assert not over, (kernel, name, over)


@pytest.mark.parametrize("name", NAMES)
def test_mass_matrix(handle, name):
    m, C = _set(handle, name)
    M = handle.mass_matrix_host(3, C["in.q"])
    _judge("mass_matrix", name, [("M", M, C["M"], *_local(C, "M", "base"))])


@pytest.mark.parametrize("name", NAMES)
def test_jacobians(handle, name):
    m, C = _set(handle, name)
    handle.set_jacobian_frames(3, list(range(m.nframe)))
    q, v = C["in.q"], C["in.v"]
    checks = []
    for rf, key in ((capi.RF_WORLD, "J_world"), (capi.RF_LOCAL, "J_local"), (capi.RF_LOCAL_WORLD_ALIGNED, "J_lwa")):
        got = handle.jacobians_host(3, q, v, rf)
        checks.append((key, got["J"], C[key], *_local(C, key, "world")))
        if rf != capi.RF_WORLD:
            d = "drift_local" if rf == capi.RF_LOCAL else "drift_lwa"
            checks.append((d, got["drift"], C[d], *_rate(C, d)))
        if rf == capi.RF_LOCAL:  # (the three do not depend on the convention: tests/test_gpu_jacobians.py holds them to the same bits)
            checks += [(k, got[k], C[k], *_local(C, k, "world")) for k in ("Jcom", "Ag")] + [("dAgv", got["dAgv"], C["dAgv"], *_rate(C, "dAgv"))]
    _judge("jacobians", name, checks)


@pytest.mark.parametrize("name", NAMES)
def test_observe(handle, name):
    m, C = _set(handle, name)
    handle.set_observed_frames(3, list(range(m.nframe)))
    got = handle.observe_host(3, C["in.q"], C["in.v"], acom=True)
    _judge("observe", name, [(k, got[k], C[k], C[k + ".scale"], None) for k in ("com", "placement")]
           + [(k, got[k], C[k], *_rate(C, k)) for k in ("vcom", "acom", "velocity")])


@pytest.mark.parametrize("name", NAMES)
def test_inverse_dynamics(handle, name):
    m, C = _set(handle, name)
    handle.set_wrench_frames(3, [int(f) for f in C["in.wrench_frames"]])
    q, v, a, w = (C["in." + k] for k in ("q", "v", "a", "wrench"))
    got = {"nle": handle.inverse_dynamics_host(3, q, v), "tau_a": handle.inverse_dynamics_host(3, q, v, a),
           "tau_aw": handle.inverse_dynamics_host(3, q, v, a, wrench=w)}
    _judge("inverse_dynamics", name, [(k, got[k], C[k], C[k + ".scale_total"], C[k + ".scale"]) for k in ("nle", "tau_a", "tau_aw")])


@pytest.mark.parametrize("name", NAMES)
def test_kinematic_hessians(handle, name):
    m, C = _set(handle, name)
    S = X.load_hessians(name)
    handle.set_jacobian_frames(3, [int(f) for f in S["in.hessian_frames"]])
    q, v = C["in.q"], C["in.v"]
    checks = []
    for rf, c in ((capi.RF_WORLD, "world"), (capi.RF_LOCAL, "local"), (capi.RF_LOCAL_WORLD_ALIGNED, "lwa")):
        got = handle.kinematic_hessians_host(3, q, v, rf)
        checks.append(("H_" + c, got["H"], S["H_" + c], *_local(S, "H_" + c, "world")))
        checks.append(("dJ_" + c, got["dJ"], S["dJ_" + c], *_rate(S, "dJ_" + c)))
    _judge("kinematic_hessians", name, checks)


def _stack(name, m):
    if name == "talos":
        st = structure.talos_structure()
        return st, mdl.build_taskmap(m, st, mdl.talos_stack())
    if name == "tree_59_floating":
        # nv = 64: a QP with a contact does not fit one CU's LDS and set_structure refuses it (UNSUPPORTED) -- random_stack with two contacts
        # (n = 88), with one (n = 76), and the minimal stack with one contact (n = 76) were each tried; the rows M, h and the momentum need
        # the tree only, and the contact rows are judged on the three smaller floating cases
        return mq.minimal(m, "rbdx_rows_")
    st, stack = mdl.random_stack(m, 500 + NAMES.index(name), 2)
    return st, mdl.build_taskmap(m, st, stack, dt=2e-3)


@pytest.mark.parametrize("name", NAMES)
def test_rows_kernel(handle, name):
    m, C = X.model(name), X.load(name)
    st, tm = _stack(name, m)
    handle.set_structure(4, st)
    handle.set_model(4, m, tm)
    q, v = C["in.q"], C["in.v"]
    n, nv = q.shape[0], m.nv
    ref = mdl.sample_states(m, tm, n, 97_500)["ref"]
    got = handle.problem_data_host(4, q, v, ref)
    lo = np.tril_indices(nv)
    tri = lambda a: a[:, lo[0], lo[1]]  # noqa: E731  (packed lower triangle: i >= j at i (i + 1) / 2 + j)
    total = np.where(C["M.scale_base"] == 0.0, 0.0, C["M.scale_total"])  # unrelated branches: exact zeros here too
    checks = [("M", got["M"], tri(C["M"]), tri(total), tri(C["M.scale"])),
              ("nle (h)", got["h"], C["nle"], C["nle.scale_total"], C["nle.scale"]),
              ("Agv (momentum)", got["momentum"], C["Agv"], C["Agv.scale_total"], C["Agv.scale"])]
    if tm.ncontact:
        cf = [int(f) for f in tm.contact_frame]
        bar_scale, local = _local(C, "J_local", "base")
        checks.append(("J_local (Ac)", got["Ac"].reshape(n, tm.ncontact, 6, nv), C["J_local"][:, cf], bar_scale[:, cf], local[:, cf]))
    assert tm.ncontact == (2 if m.floating_base and name != "tree_59_floating" else 0)  # contacts wherever there is a base to hold up
    _judge("problem_data", name, checks)
