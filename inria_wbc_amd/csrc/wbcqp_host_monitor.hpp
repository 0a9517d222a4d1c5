// wbcqp_host_monitor.hpp -- host side of wbcqp_detect_torque_collisions and of wbcqp_stabilize (wbcqp_api.hip), the two calls that process a fleet's
// sensor streams with a state of the caller's: per call ONE check that the device-pointer and the host-pointer entry point share (nothing is staged or
// launched before it has passed) and ONE launch of its kernel (torque_monitor_kernel, csrc/wbcqp_monitor.hpp; stabilize_kernel, with a ZMP
// distributor its second instantiation, csrc/wbcqp_stabilize.hpp), one wavefront per instance.  The monitor / the stabiliser travels in the kernel's arguments: no slot, no model, no device
// table.  Host code only; included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_handle.hpp"
#include "wbcqp_monitor.hpp"
#include "wbcqp_stabilize.hpp"

namespace {

static_assert(WBCQP_MAX_MONITORED == kMonitorMaxJoints && WBCQP_MAX_FILTER_WINDOW == kMonitorMaxWindow, "the header and the kernel agree on the monitor's limits");
static_assert(WBCQP_FILTER_NONE == kFilterNone && WBCQP_FILTER_MEAN == kFilterMean && WBCQP_FILTER_MEDIAN == kFilterMedian, "... and on the filters");
static_assert(WBCQP_MAX_INVALID == 31, "K = max_invalid + 1 fits a 32-bit shift register");

// what is wrong with the monitor's own fields (the joints' columns are checked against ldt by the call), or null
const char* monitor_flaw(const wbcqp_torque_monitor* m)
{
    if (!m) return "torque monitor is NULL";
    if (m->n_joints < 1 || m->n_joints > WBCQP_MAX_MONITORED) return "n_joints must be in [1, 64]";
    if (m->filter != WBCQP_FILTER_NONE && m->filter != WBCQP_FILTER_MEAN && m->filter != WBCQP_FILTER_MEDIAN) return "filter must be WBCQP_FILTER_NONE, _MEAN or _MEDIAN";
    if (m->filter != WBCQP_FILTER_NONE && (m->window < 1 || m->window > WBCQP_MAX_FILTER_WINDOW)) return "window must be in [1, 64]";
    if (m->max_invalid < 0 || m->max_invalid > WBCQP_MAX_INVALID) return "max_invalid must be in [0, 31]";
    if (!m->joint || !m->threshold) return "joint / threshold is NULL";
    for (int j = 0; j < m->n_joints; ++j) {
        if (m->joint[j] < 0) return "a monitored joint's column is negative";
        if (std::isnan(m->threshold[j])) return "a threshold is NaN";
        if (m->offset && !std::isfinite(m->offset[j])) return "an offset is not finite";
    }
    return nullptr;
}

// *run: false where the call is accepted and there is nothing to do
int check_torque_monitor(wbcqp_handle* h, const wbcqp_torque_monitor* m, int batch, int n_ticks, const void* tau_model, int ldt, const void* tau_sensor,
                         const void* state, const wbcqp_torque_checks* out, MonitorDev* D, bool* run)
{
    *run = false;
    if (!h) return WBCQP_ERR_INVALID;
    if (const char* flaw = monitor_flaw(m)) return fail(h, WBCQP_ERR_INVALID, flaw);
    for (int j = 0; j < m->n_joints; ++j)
        if (m->joint[j] >= ldt) return fail(h, WBCQP_ERR_INVALID, "a monitored joint's column is outside [0, ldt)");
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (n_ticks < 0) return fail(h, WBCQP_ERR_INVALID, "negative n_ticks");
    if (!tau_model || !tau_sensor) return fail(h, WBCQP_ERR_INVALID, "tau_model and tau_sensor are required");
    if (!out) return fail(h, WBCQP_ERR_INVALID, "torque checks struct is NULL");
    if (batch == 0 || n_ticks == 0) return WBCQP_OK;
    if (!state && !out->detected && !out->invalid && !out->discrepancy && !out->filtered && !out->first_tick && !out->n_detected) return WBCQP_OK;
    *D = MonitorDev{};
    D->n_joints = m->n_joints;
    D->filter = m->filter;
    D->window = m->filter == WBCQP_FILTER_NONE ? 0 : m->window;
    D->k = m->max_invalid + 1;
    D->has_offset = m->offset ? 1 : 0;
    for (int j = 0; j < kMonitorMaxJoints; ++j) {
        const int s = j < m->n_joints ? j : m->n_joints - 1;
        D->joint[j] = m->joint[s];
        D->threshold[j] = m->threshold[s];
        D->offset[j] = m->offset ? m->offset[s] : 0.0;
    }
    *run = true;
    return WBCQP_OK;
}

// batch > 0, n_ticks > 0, arguments checked, the handle's device current; state_in / state_out: the caller's one block, or its two staged copies
int launch_torque_monitor(wbcqp_handle* h, const MonitorDev& D, int batch, int n_ticks, const void* tau_model, int ldt, const void* tau_sensor,
                          const void* state_in, void* state_out, const wbcqp_torque_checks& out, hipStream_t stream)
{
    const size_t ring = monitor_ring_doubles(D.n_joints, D.filter, D.window);
    const int per_block = monitor_per_block(ring);
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const MonitorArgs<TI> a{D, static_cast<const TI*>(tau_model), static_cast<const TI*>(tau_sensor), static_cast<const double*>(state_in),
                                static_cast<double*>(state_out), out.detected, reinterpret_cast<unsigned long long*>(out.invalid),
                                static_cast<TI*>(out.discrepancy), static_cast<TI*>(out.filtered), out.first_tick, out.n_detected, ldt, batch, n_ticks,
                                per_block};
        hipLaunchKernelGGL(torque_monitor_kernel<TI>, dim3((batch + per_block - 1) / per_block), dim3(per_block * kWave), per_block * ring * 8, stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

// ---- the stabiliser ---------------------------------------------------------------------------------------------------------------------------------
static_assert(WBCQP_MAX_STAB_WINDOW == kStabMaxWindow, "the header and the kernel agree on the stabiliser's window");
static_assert(WBCQP_STAB_COP == kStabCop && WBCQP_STAB_LCOP == kStabLcop && WBCQP_STAB_RCOP == kStabRcop && WBCQP_STAB_COM == kStabCom &&
                  WBCQP_STAB_LANKLE == kStabLankle && WBCQP_STAB_RANKLE == kStabRankle && WBCQP_STAB_FFDA == kStabFfda &&
                  WBCQP_STAB_ERR_COP == kStabErrCop && WBCQP_STAB_ERR_FORCE == kStabErrForce && WBCQP_STAB_ZMP == kStabZmp &&
                  WBCQP_STAB_ERR_ZMP == kStabErrZmp,
              "... and on the bits of its flags");

// what is wrong with the stabiliser's own fields (ldp and ldx are the call's), or null
const char* stabilizer_flaw(const wbcqp_stabilizer* s)
{
    if (!s) return "stabilizer is NULL";
    if (s->window < 1 || s->window > WBCQP_MAX_STAB_WINDOW) return "window must be in [1, 64]";
    if (!std::isfinite(s->dt) || !(s->dt > 0.0)) return "dt must be finite and > 0";
    if (!std::isfinite(s->mass) || !(s->mass > 0.0)) return "mass must be finite and > 0";
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(s->com_gains[k]) || !std::isfinite(s->ankle_gains[k])) return "a gain is not finite";
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(s->ffda_gains[k])) return "a gain is not finite";
        if (!std::isfinite(s->normal[k])) return "the contact normal is not finite";
    }
    if (s->nref < 0) return "nref is negative";
    const int off[kStabBlocks] = {s->com_ref, s->lf_ref, s->rf_ref, s->torso_ref, s->lf_contact_ref, s->rf_contact_ref};
    for (int b = 0; b < kStabBlocks; ++b) {
        const int len = b == 0 ? 9 : 24;
        if (off[b] < (b < 4 ? 0 : -1)) return b < 4 ? "com_ref, lf_ref, rf_ref and torso_ref are required (an offset is negative)" : "a contact's reference offset is below -1";
        if (off[b] >= 0 && (int64_t)off[b] + len > s->nref) return "a reference offset runs past nref";
        for (int a = 0; a < b; ++a)
            if (off[a] >= 0 && off[b] >= 0 && off[a] < off[b] + len && off[b] < off[a] + (a == 0 ? 9 : 24)) return "two reference blocks overlap";
    }
    if (s->lf_force_col < -1 || s->rf_force_col < -1) return "a force column is below -1";
    if (s->lf_pos < 0 || s->rf_pos < 0) return "lf_pos and rf_pos are required (an offset is negative)";
    return nullptr;
}

// what is wrong with a ZMP distributor on a stabiliser that has passed stabilizer_flaw, or null
const char* zmp_flaw(const wbcqp_stabilizer* s, const wbcqp_zmp_distributor* z)
{
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(z->p[k]) || !std::isfinite(z->d[k])) return "a ZMP distributor gain is not finite";
    if (s->lf_contact_ref < 0 && s->rf_contact_ref < 0) return "the ZMP distributor needs an active foot contact (lf_contact_ref and rf_contact_ref are both -1)";
    const int off[kStabBlocks] = {s->com_ref, s->lf_ref, s->rf_ref, s->torso_ref, s->lf_contact_ref, s->rf_contact_ref};
    const int foff[2] = {z->lf_force_ref, z->rf_force_ref};
    for (int f = 0; f < 2; ++f) {
        if (foff[f] < -1) return "a force reference offset is below -1";
        if (foff[f] < 0) continue;
        if ((int64_t)foff[f] + 6 > s->nref) return "a force reference runs past nref";
        for (int b = 0; b < kStabBlocks; ++b)
            if (off[b] >= 0 && off[b] < foff[f] + 6 && foff[f] < off[b] + (b == 0 ? 9 : 24)) return "a force reference overlaps a reference block";
    }
    if (foff[0] >= 0 && foff[1] >= 0 && foff[0] < foff[1] + 6 && foff[1] < foff[0] + 6) return "the two force references overlap";
    return nullptr;
}

// *run: false where the call is accepted and there is nothing to do.  z: the ZMP distributor of wbcqp_stabilize_zmp, or null; alpha: its extra output
int check_stabilize(wbcqp_handle* h, const wbcqp_stabilizer* s, const wbcqp_zmp_distributor* z, int batch, const wbcqp_stab_inputs* in, const void* state,
                    const wbcqp_stab_outputs* out, const void* alpha, StabDev* D, bool* run)
{
    *run = false;
    if (!h) return WBCQP_ERR_INVALID;
    if (const char* flaw = stabilizer_flaw(s)) return fail(h, WBCQP_ERR_INVALID, flaw);
    if (z)
        if (const char* flaw = zmp_flaw(s, z)) return fail(h, WBCQP_ERR_INVALID, flaw);
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!in) return fail(h, WBCQP_ERR_INVALID, "stabilizer inputs struct is NULL");
    if (!in->ref || !in->wrench || !in->com || !in->acom || !in->placement) return fail(h, WBCQP_ERR_INVALID, "ref, wrench, com, acom and placement are required");
    if ((int64_t)in->ldp < (int64_t)std::max(s->lf_pos, s->rf_pos) + 3) return fail(h, WBCQP_ERR_INVALID, "ldp is too small for lf_pos + 3 / rf_pos + 3");
    const int last_col = std::max(s->lf_force_col, s->rf_force_col); // (-1: no contact is active, x_prev is not read)
    if (in->x_prev && last_col >= 0 && (int64_t)in->ldx < (int64_t)last_col + 12)
        return fail(h, WBCQP_ERR_INVALID, "ldx is too small for a force column + 12");
    if (batch == 0) return WBCQP_OK;
    if (!state && (!out || (!out->ref_out && !out->flags && !out->cop)) && !(z && alpha)) return WBCQP_OK;
    *D = StabDev{};
    D->window = s->window;
    D->nref = s->nref;
    const int off[kStabBlocks] = {s->com_ref, s->lf_ref, s->rf_ref, s->torso_ref, s->lf_contact_ref, s->rf_contact_ref};
    std::copy(off, off + kStabBlocks, D->off);
    D->lf_col = s->lf_force_col;
    D->rf_col = s->rf_force_col;
    D->lf_pos = s->lf_pos;
    D->rf_pos = s->rf_pos;
    D->dt = s->dt;
    D->mass = s->mass;
    std::copy(s->com_gains, s->com_gains + 6, D->com_gains);
    std::copy(s->ankle_gains, s->ankle_gains + 6, D->ankle_gains);
    std::copy(s->ffda_gains, s->ffda_gains + 3, D->ffda_gains);
    std::copy(s->normal, s->normal + 3, D->normal);
    *run = true;
    return WBCQP_OK;
}

// batch > 0, arguments checked, the handle's device current; state_in / state_out: the caller's one block, or its two staged copies.
// z null: stabilize_kernel; otherwise stabilize_kernel<TI, true>, which also writes alpha (may be null)
int launch_stabilize(wbcqp_handle* h, const StabDev& D, const wbcqp_zmp_distributor* z, int batch, const wbcqp_stab_inputs& in, const void* state_in,
                     void* state_out, const wbcqp_stab_outputs& out, void* alpha, hipStream_t stream)
{
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const StabArgs<TI> a{D, static_cast<const TI*>(in.ref), static_cast<const TI*>(in.wrench), static_cast<const TI*>(in.com),
                             static_cast<const TI*>(in.acom), static_cast<const TI*>(in.placement), static_cast<const TI*>(in.x_prev),
                             static_cast<const double*>(state_in), static_cast<double*>(state_out), static_cast<TI*>(out.ref_out), out.flags,
                             static_cast<TI*>(out.cop), in.ldp, in.ldx, batch};
        const dim3 grid((batch + kObservePerBlock - 1) / kObservePerBlock), block(kObserveThreads);
        if (z) {
            StabZmpArgs<TI> az{};
            static_cast<StabArgs<TI>&>(az) = a;
            std::copy(z->p, z->p + 6, az.p);
            std::copy(z->d, z->d + 6, az.d);
            az.foff[0] = z->lf_force_ref;
            az.foff[1] = z->rf_force_ref;
            az.alpha = static_cast<TI*>(alpha);
            hipLaunchKernelGGL((stabilize_kernel<TI, true>), grid, block, kObservePerBlock * stab_lds_doubles(D.window, true) * 8, stream, az);
        }
        else
            hipLaunchKernelGGL(stabilize_kernel<TI>, grid, block, kObservePerBlock * stab_lds_doubles(D.window) * 8, stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

} // namespace
