// wbcqp_monitor.hpp -- did a robot of the fleet hit something: the reference's safety::TorqueCollisionDetection (src/safety/torque_collision_detection.cpp
// there) with its filters (include/inria_wbc/estimators/filtering.hpp), for a whole fleet and a whole stream of ticks (wbcqp_detect_torque_collisions).
//
// Per instance and tick: the measured torques of the monitored joints pass a windowed filter (mean, median or none), an offset is added, the result is
// subtracted from the model's torque, and a joint is INVALID when its discrepancy has been outside its threshold, with the same sign, in each of the last
// K = max_invalid + 1 ticks.  This is a stateful stream per joint, not a query on a state:
//   lanes = monitored joints (<= 64); the wave walks its instance's ticks in order
//   window:     a wave-private LDS ring [window][n_joints] doubles; lane j reads and writes column j alone, so nothing in it crosses lanes
//   mean:       the window summed afresh every tick, oldest sample first, one division by the count (no running sum: it drifts, and a stream cut in
//               two calls would then differ from the same stream in one)
//   median:     by rank inside the lane's column, ties broken by age (a NaN ranks above every number, as a sort that puts NaNs last)
//   the rule:   two K-bit shift registers per joint, one for raw-invalid steps with a positive discrepancy and one for negative ones; the reference's ring
//               of signs sums to +-K exactly when one register is full and the other empty, i.e. |popcount(pos) - popcount(neg)| >= K
//   outputs:    `invalid` is a ballot over the joint lanes; detected / first_tick / n_detected leave from lane 0; discrepancy and filtered from lane j
// The state of an instance (count, head, the registers, the ring; all-zero bytes = a fresh detector) comes in at entry and leaves at exit, so a stream may
// be cut into calls anywhere.  One wavefront per instance, up to four per workgroup, nothing shared between the waves: no workgroup barrier, no atomics.
// Only additions, one division and one subtraction: nothing for -ffp-contract to fuse.  F32 handles read float, compute in double, write float.
#pragma once

#include "wbcqp_observe.hpp"

namespace wbcqp {

constexpr int kMonitorMaxJoints = 64; // WBCQP_MAX_MONITORED: one lane each
constexpr int kMonitorMaxWindow = 64; // WBCQP_MAX_FILTER_WINDOW
constexpr int kMonitorLdsBudget = kObservePerBlock * 256 * 4 * 8; // a workgroup's LDS stays within collide_kernel's largest launch (32 KB)
enum { kFilterNone = 0, kFilterMean = 1, kFilterMedian = 2 };

// the monitor as the kernel reads it, by value in the kernel's arguments (entries past n_joints repeat the last joint)
struct MonitorDev {
    int n_joints, filter, window, k; // window: 0 for kFilterNone; k = max_invalid + 1 in 1 .. 32
    int has_offset;
    int joint[kMonitorMaxJoints];
    double threshold[kMonitorMaxJoints];
    double offset[kMonitorMaxJoints];
};

// state of one instance: {int32 count, int32 head}, [n_joints]{uint32 pos, uint32 neg}, [window][n_joints] doubles
inline size_t monitor_ring_doubles(int n_joints, int filter, int window) { return filter == kFilterNone ? 0 : (size_t)window * n_joints; }
inline size_t monitor_state_bytes(int n_joints, int filter, int window) { return 8 + 8 * (size_t)n_joints + 8 * monitor_ring_doubles(n_joints, filter, window); }
// waves (instances) per workgroup for a ring of that size
inline int monitor_per_block(size_t ring_doubles)
{
    const size_t fit = ring_doubles ? (size_t)kMonitorLdsBudget / (ring_doubles * 8) : (size_t)kObservePerBlock;
    return (int)(fit < 1 ? 1 : fit > (size_t)kObservePerBlock ? (size_t)kObservePerBlock : fit);
}

template <typename TI>
struct MonitorArgs {
    MonitorDev M;
    const TI* tau_model;  // row (t, i) at (t * batch + i) * ldt
    const TI* tau_sensor; // [n_ticks][batch][n_joints]
    const double* state_in; // [batch][state doubles] or null (fresh)
    double* state_out;      // the same block (or a staged copy of it), or null (discarded)
    int* detected;                  // [n_ticks][batch] or null
    unsigned long long* invalid;    // [n_ticks][batch] or null
    TI *discrepancy, *filtered;     // [n_ticks][batch][n_joints] or null
    int *first_tick, *n_detected;   // [batch] or null
    int ldt, batch, n_ticks, per_block;
};

#ifdef __HIPCC__

template <typename TI>
__global__ __launch_bounds__(kObserveThreads) void torque_monitor_kernel(const MonitorArgs<TI> args)
{
    extern __shared__ double mon_lds[];
    const MonitorDev& M = args.M;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * args.per_block + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int n = M.n_joints, W = M.window, K = M.k, filter = M.filter;
    const bool mine = lane < n;
    const int j = min(lane, n - 1);
    const size_t ring_doubles = (size_t)W * n; // (W == 0 without a filter)
    const size_t state_doubles = 1 + (size_t)n + ring_doubles;
    double* ring = mon_lds + (size_t)wave * ring_doubles;
    const int col = M.joint[j];
    const double thr = M.threshold[j];
    const double off = M.has_offset ? M.offset[j] : 0.0;
    const unsigned kmask = K >= 32 ? 0xffffffffu : ((1u << K) - 1u);

    // ---- the state comes in: count and head (wave-uniform), the lane's two registers, the ring (zero without a state) ------------------------
    int count = 0, head = 0;
    unsigned pos = 0, neg = 0;
    if (args.state_in) {
        const double* S = args.state_in + (size_t)inst * state_doubles;
        const double w0 = S[0];
        count = min(max(uni(__double2loint(w0)), 0), W); // (bytes that no call of this monitor wrote stay inside the ring)
        head = min(max(uni(__double2hiint(w0)), 0), max(W - 1, 0));
        const double wj = S[1 + j];
        pos = (unsigned)__double2loint(wj);
        neg = (unsigned)__double2hiint(wj);
        for (int r = 0; r < W; ++r)
            if (mine) ring[(size_t)r * n + lane] = S[1 + n + (size_t)r * n + lane];
    }
    else {
        for (int r = 0; r < W; ++r)
            if (mine) ring[(size_t)r * n + lane] = 0.0;
    }

    const size_t B = (size_t)args.batch;
    int first = -1, hits = 0;
    // (the next tick's two loads are issued before this tick's arithmetic: a tick is otherwise one memory round trip long)
    double s_next = (double)args.tau_sensor[(size_t)inst * n + j];
    double m_next = (double)args.tau_model[(size_t)inst * args.ldt + col];
    for (int t = 0; t < args.n_ticks; ++t) {
        const double sample = s_next, model = m_next;
        if (t + 1 < args.n_ticks) {
            const size_t row = (size_t)(t + 1) * B + (size_t)inst;
            s_next = (double)args.tau_sensor[row * n + j];
            m_next = (double)args.tau_model[row * args.ldt + col];
        }
        // ---- 1. the filter ---------------------------------------------------------------------------------------------------------------
        double f = sample;
        if (filter != kFilterNone) {
            if (mine) ring[(size_t)head * n + lane] = sample;
            head = head + 1 == W ? 0 : head + 1;
            count = count < W ? count + 1 : W;
            int oldest = head - count;
            if (oldest < 0) oldest += W;
            const double* colp = ring + j; // (lanes past the last joint read the last joint's column; their result is never stored)
            if (filter == kFilterMean) {
                double sum = 0.0;
                for (int a = 0, r = oldest; a < count; ++a) {
                    sum += colp[(size_t)r * n];
                    r = r + 1 == W ? 0 : r + 1;
                }
                f = sum / (double)count;
            }
            else {
                // element of age a has rank #{b : x_b < x_a, or x_b == x_a and b older}; NaNs rank last among themselves by age
                const int hi_rank = count >> 1, lo_rank = hi_rank - 1;
                double hi = 0.0, lo = 0.0;
                for (int a = 0, ra = oldest; a < count; ++a) {
                    const double xa = colp[(size_t)ra * n];
                    const bool na = xa != xa;
                    int rank = 0;
                    for (int b = 0, rb = oldest; b < count; ++b) {
                        const double xb = colp[(size_t)rb * n];
                        const bool nb = xb != xb;
                        const bool less = na ? !nb : (xb < xa);
                        const bool same = na ? nb : (xb == xa);
                        rank += (less || (same && b < a)) ? 1 : 0;
                        rb = rb + 1 == W ? 0 : rb + 1;
                    }
                    if (rank == hi_rank) hi = xa;
                    if (rank == lo_rank) lo = xa;
                    ra = ra + 1 == W ? 0 : ra + 1;
                }
                f = (count & 1) ? hi : (hi + lo) / 2;
            }
        }
        // ---- 2., 3. offset, discrepancy, raw validity ------------------------------------------------------------------------------------
        if (M.has_offset) f = f + off;
        const double d = model - f;
        const bool raw_invalid = !(fabs(d) < thr); // (a NaN discrepancy is raw-invalid and has no sign)
        // ---- 4. the same sign in each of the last K steps --------------------------------------------------------------------------------
        pos = ((pos << 1) | ((raw_invalid && d > 0) ? 1u : 0u)) & kmask;
        neg = ((neg << 1) | ((raw_invalid && d < 0) ? 1u : 0u)) & kmask;
        const int bal = __popc(pos) - __popc(neg);
        const bool bad = mine && (bal >= K || -bal >= K);
        // ---- 5. any joint ----------------------------------------------------------------------------------------------------------------
        const unsigned long long mask = __ballot(bad);
        const size_t row = (size_t)t * B + (size_t)inst;
        if (mask) {
            if (first < 0) first = t;
            ++hits;
        }
        if (lane == 0) {
            if (args.detected) args.detected[row] = mask ? 1 : 0;
            if (args.invalid) args.invalid[row] = mask;
        }
        if (mine) {
            if (args.discrepancy) args.discrepancy[row * n + lane] = (TI)d;
            if (args.filtered) args.filtered[row * n + lane] = (TI)f;
        }
    }
    if (lane == 0) {
        if (args.first_tick) args.first_tick[inst] = first;
        if (args.n_detected) args.n_detected[inst] = hits;
    }
    // ---- the state leaves --------------------------------------------------------------------------------------------------------------------
    if (args.state_out) {
        double* S = args.state_out + (size_t)inst * state_doubles;
        if (lane == 0) S[0] = __hiloint2double(head, count);
        if (mine) S[1 + lane] = __hiloint2double((int)neg, (int)pos);
        for (int r = 0; r < W; ++r)
            if (mine) S[1 + n + (size_t)r * n + lane] = ring[(size_t)r * n + lane];
    }
}

#endif // __HIPCC__
} // namespace wbcqp
