// wbcqp_refgen.hpp -- the references of a roll-out expanded on the device from a reference program (wbcqp_program, include/wbcqp.h): refgen_kernel.
#pragma once

#include "wbcqp_prims.hpp"

namespace wbcqp {

constexpr int kRefThreads = 256;
constexpr int kRefMaxTracks = 16;
constexpr int kRefSlots = 32;      // components one track may write: an SE3 track has 24, a VEC track 9 or 1
constexpr int kTrackVec = 0, kTrackSe3 = 1;
constexpr int kTrackPoseOnly = 1, kTrackRelative = 2;

// one segment on the device: wbcqp_segment plus its first sample on the timeline
struct RefSeg {
    double T, x0[3], xf[3], R0[9], axis[3], angle;
    int start, n_steps;
};
struct RefTrack {
    int kind, dim, flags, dst0, dst1, seg0, nseg, ncomp; // ncomp: 24 (SE3), 9 (VEC 3), 1 (VEC 1)
};
// travels by value with every launch (536 bytes)
struct RefProg {
    int nref, n_intro, n_cycle, n_tracks;
    double dt;
    RefTrack tr[kRefMaxTracks];
};

template <typename TI>
struct RefGenArgs {
    RefProg P;
    const RefSeg* segs;   // device, all tracks' segments
    const int* offset;    // device [batch]
    const TI* base;       // [batch][nref], or one row (base_stride 0)
    int base_stride;
    TI* out;              // row of (output tick j, instance i) at out + (j batch + i) nref
    int batch;            // instances of the whole call: the tick stride of out
    int inst0;            // blockIdx.x = 0 is instance inst0
    long long tick_first; // tick0 + call tick of output tick 0
    int n_ticks;          // output ticks of this launch
    int ticks_per_block;  // blockIdx.y handles output ticks [y tpb, (y + 1) tpb)
};

// the sample of the timeline that behaviour tick tau plays (model.WalkOnSpotPlan.index)
__host__ __device__ inline int ref_sample_index(long long tau, int n_intro, int n_cycle)
{
    if (tau < 0) return 0;
    if (tau < n_intro) return (int)tau;
    if (n_cycle <= 0) return n_intro > 0 ? n_intro - 1 : 0;
    return n_intro + (int)((tau - n_intro) % n_cycle);
}

// LDS of one workgroup: the row (as doubles' worth of space whatever TI), then per track the origin of a RELATIVE track (position 3, rotation 9 row-major)
__host__ __device__ inline int refgen_lds_bytes(int nref, int n_tracks) { return ((nref + 1) & ~1) * 8 + n_tracks * 12 * 8; }

#ifdef __HIPCC__
template <typename TI> struct alignas(16) RefVec { TI v[16 / sizeof(TI)]; };

// Component c of track t at sample idx of the timeline.  Every operation is written out (fma or a single rounded operation), so the value is a function of
// (segment, idx - start) alone: the same bits whichever chunk, launch or call the tick falls in.  A hold (xf == x0, angle == 0) gives x0 and R0 exactly:
// fma(0, s, x0) = x0, and Rot = I + 0 K + 0 K^2 = I.
__device__ inline double ref_component(const RefTrack& t, const RefSeg* __restrict__ segs, int idx, int c, double dt, const double* __restrict__ org)
{
    const RefSeg* sg = segs + t.seg0;
    for (int s = 0; s + 1 < t.nseg && idx >= sg->start + sg->n_steps; ++s) ++sg;
    const double tt = dt * (double)(idx - sg->start);
    const double td = tt / sg->T;
    const double td2 = td * td, td3 = td2 * td;
    const bool rel = (t.flags & kTrackRelative) != 0;
    int order, comp;  // derivative order, component within it
    bool ang = false; // SE3: an angular part
    if (t.kind == kTrackSe3) {
        if (c < 12) {
            order = 0;
            comp = c;
        }
        else {
            order = c < 18 ? 1 : 2;
            comp = (c - 12) % 6;
            ang = comp >= 3;
            if (ang) comp -= 3;
        }
    }
    else {
        order = c / 3;
        comp = c - 3 * order;
    }
    if (order > 0 && (t.flags & kTrackPoseOnly)) return 0.0;
    double p; // the polynomial of this order, scaled by 1 / T^order
    if (order == 0) p = td3 * fma(td, fma(6.0, td, -15.0), 10.0);
    else if (order == 1) p = td2 * fma(td, fma(30.0, td, -60.0), 30.0) / sg->T;
    else p = td * fma(td, fma(120.0, td, -180.0), 60.0) / (sg->T * sg->T);
    if (t.kind == kTrackVec || (!ang && comp < 3)) { // a translation, or one of its derivatives
        const double d = sg->xf[comp] - sg->x0[comp];
        if (order > 0) return d * p;
        const double x = fma(d, p, sg->x0[comp]);
        return rel ? org[comp] + x : x;
    }
    const double* R0 = sg->R0;
    const double* Rb = org + 3;
    const double ax = sg->axis[0], ay = sg->axis[1], az = sg->axis[2];
    if (ang) { // R0 (angle s' axis), world-oriented; rotated by the origin when relative
        const double w0 = sg->angle * p * ax, w1 = sg->angle * p * ay, w2 = sg->angle * p * az;
        double r[3], out = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = fma(R0[3 * i + 2], w2, fma(R0[3 * i + 1], w1, R0[3 * i] * w0));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double v = rel ? fma(Rb[3 * i + 2], r[2], fma(Rb[3 * i + 1], r[1], Rb[3 * i] * r[0])) : r[i];
            if (i == comp) out = v;
        }
        return out;
    }
    // rotation entry (row, col), column-major in the reference row: R0 (I + sin(a) K + (1 - cos(a)) K K), K the axis' cross-product matrix
    const int e = comp - 3, col = e / 3, row = e - 3 * col;
    const double a = sg->angle * p;
    const double sa = sin(a), ca = 1.0 - cos(a);
    const double K[9] = {0.0, -az, ay, az, 0.0, -ax, -ay, ax, 0.0};
    const double KK[9] = {-(ay * ay + az * az), ax * ay, ax * az, ax * ay, -(ax * ax + az * az), ay * az, ax * az, ay * az, -(ax * ax + ay * ay)};
    double rot[9], Rm[9], out = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) rot[i] = ((i % 4 == 0 ? 1.0 : 0.0) + sa * K[i]) + ca * KK[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rm[3 * i + j] = fma(R0[3 * i + 2], rot[6 + j], fma(R0[3 * i + 1], rot[3 + j], R0[3 * i] * rot[j]));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = rel ? fma(Rb[3 * i + 2], Rm[6 + j], fma(Rb[3 * i + 1], Rm[3 + j], Rb[3 * i] * Rm[j])) : Rm[3 * i + j];
            if (i == row && j == col) out = v;
        }
    return out;
}

// One workgroup per instance and block of ticks.  The instance's base row is read once and kept in LDS; per tick the lanes that own a track's components
// (32 slots per track) overwrite them, then all lanes store the row, consecutive lanes on consecutive addresses, 16 bytes per lane where the row's address
// allows (a Talos row is 305 numbers: every other row starts 8 bytes off a 16-byte boundary, so the first lanes store the odd head singly).  No atomics.
template <typename TI>
__global__ __launch_bounds__(kRefThreads) void refgen_kernel(const RefGenArgs<TI> a)
{
    extern __shared__ double refgen_lds[];
    const RefProg& P = a.P;
    const int tid = threadIdx.x, nref = P.nref;
    const int inst = a.inst0 + (int)blockIdx.x;
    TI* row = reinterpret_cast<TI*>(refgen_lds);
    double* org = refgen_lds + ((nref + 1) & ~1);
    const TI* base = a.base + (size_t)inst * a.base_stride * nref;
    for (int e = tid; e < nref; e += kRefThreads) row[e] = base[e];
    for (int e = tid; e < P.n_tracks * 12; e += kRefThreads) {
        const RefTrack& t = P.tr[e / 12];
        const int c = e % 12;
        double v = 0.0;
        if (t.flags & kTrackRelative) {
            if (c < 3) v = c < t.dim || t.kind == kTrackSe3 ? (double)base[t.dst0 + c] : 0.0;
            else if (t.kind == kTrackSe3) v = (double)base[t.dst0 + 3 + 3 * ((c - 3) % 3) + (c - 3) / 3]; // row-major from the row's column-major
        }
        org[e] = v;
    }
    bsync();
    const long long off = a.offset[inst];
    const int j0 = (int)blockIdx.y * a.ticks_per_block;
    const int j1 = min(a.n_ticks, j0 + a.ticks_per_block);
    constexpr int W = 16 / (int)sizeof(TI);
    for (int j = j0; j < j1; ++j) {
        const int idx = ref_sample_index(a.tick_first + j - off, P.n_intro, P.n_cycle);
        for (int k = tid; k < P.n_tracks * kRefSlots; k += kRefThreads) {
            const RefTrack& t = P.tr[k / kRefSlots];
            const int c = k % kRefSlots;
            if (c >= t.ncomp) continue;
            const TI v = (TI)ref_component(t, a.segs, idx, c, P.dt, org + 12 * (k / kRefSlots));
            row[t.dst0 + c] = v;
            if (t.dst1 >= 0) row[t.dst1 + c] = v;
        }
        bsync();
        TI* dst = a.out + ((size_t)j * a.batch + inst) * nref;
        const int head = min(nref, (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / sizeof(TI)));
        const int nvec = (nref - head) / W;
        if (tid < head) dst[tid] = row[tid];
        for (int v = tid; v < nvec; v += kRefThreads) {
            RefVec<TI> val;
#pragma unroll
            for (int w = 0; w < W; ++w) val.v[w] = row[head + v * W + w];
            *reinterpret_cast<RefVec<TI>*>(dst + head + v * W) = val;
        }
        for (int e = head + nvec * W + tid; e < nref; e += kRefThreads) dst[e] = row[e];
        bsync(); // the next tick's components overwrite the row
    }
}
#endif

} // namespace wbcqp
