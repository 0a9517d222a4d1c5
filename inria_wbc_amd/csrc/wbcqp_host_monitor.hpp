// wbcqp_host_monitor.hpp -- host side of wbcqp_detect_torque_collisions (wbcqp_api.hip): ONE check that the device-pointer and the host-pointer entry
// point share (nothing is staged or launched before it has passed) and ONE launch of torque_monitor_kernel (csrc/wbcqp_monitor.hpp), one wavefront
// per instance.  The monitor travels in the kernel's arguments: no slot, no model, no device table.  Host code only; included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_handle.hpp"
#include "wbcqp_monitor.hpp"

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

} // namespace
