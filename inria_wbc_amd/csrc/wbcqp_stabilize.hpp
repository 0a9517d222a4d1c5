// wbcqp_stabilize.hpp -- keep a fleet on its feet: the stabiliser of the reference's humanoid controllers (src/controllers/humanoid_pos_tracker.cpp:134-302,
// src/stabilizers/stabilizer.cpp, src/estimators/cop.cpp, include/inria_wbc/estimators/filtering.hpp there), one tick of it for every robot of a fleet
// (wbcqp_stabilize).  Only a tick's REFERENCES change, never the QP's structure: the kernel reads a reference row, the feet's force/torque samples, the
// model's CoM, its acceleration and the feet's positions, and writes the reference row that wbcqp_problem_data / wbcqp_tick consume unchanged.
//
// Per instance and tick, in double:
//   1. raw centre of pressure of each foot whose fz > 30 (cop.cpp:87-96) and, with both, Kajita's weighted combination (cop.cpp:71-83)
//   2. five moving averages over `window` samples -- combined, left, right CoP (two channels each) and the z of the two foot forces -- in a wave-private
//      LDS ring [window][8], lane c owning channel c: the window summed afresh, oldest first, one division by the count (wbcqp_monitor.hpp's convention).
//      A lifted foot RESETS its CoP filter; the combined filter is neither fed nor reset while a foot is missing; a force filter is fed while |f| > 30 and
//      otherwise left alone (the filtered force of that tick is zero)
//   3. the admittance laws (stabilizer.cpp:31-59, 168-275) on lane 0: CoM against the model's ZMP, the two ankles, the torso roll against the difference
//      of the feet's normal forces (previous solution against filtered sensors)
//   4. the row leaves: all 64 lanes copy the nref elements in consecutive addresses; the elements of the six rewritten blocks come from a wave-private
//      patch in LDS that was filled from the row before lane 0 rewrote it.  No element is stored twice and every element of `ref` is read before any
//      element of `ref_out` is stored, so ref_out may be ref.
// Where the reference throws (a CoP beyond 10 m in both coordinates, a ground force beyond 10 M g), the instance's row leaves unmodified with an error bit
// in its flags; its filters have advanced, as the reference's have at that point.
// State of one instance (all-zero bytes: a fresh stabiliser), always double: [5]{int32 count, int32 head} of the filters 0 combined, 1 left, 2 right CoP,
// 3 left, 4 right force z; then the ring [window][8] (the block is read and written as doubles: 8-byte aligned): channels 0,1 combined x,y; 2,3 left; 4,5 right; 6 left fz; 7 right fz.  A reset sets count and
// head to zero and leaves the ring's stale samples where they are (they are never read).
// One wavefront per instance, four per workgroup, nothing shared between the waves: no workgroup barrier, no atomics.  Every product, sum and quotient
// below is a statement of its own or a __d*_rn call, so -ffp-contract=on has nothing to fuse: the arithmetic equals inria_wbc_amd/stabilizer.py bit for
// bit, except through atan2 / sin / cos (the rotation entries).  F32 handles read float, compute in double, write float.
//
// stabilize_kernel<TI, true> is the same body with the ZMP force distributor compiled in (wbcqp_stabilize_zmp; stabilizer.cpp:277-311, 340-440 there): between the
// CoM law and the ankle laws, exactly when the CoM law runs, the robot's weight is split between the feet by where the ZMP lies between the contacts'
// references (once for the model's ZMP, once for the measured one), and the admittance of the two splits leaves as a 6-number force reference per foot in
// two more blocks of the row.  The patch grows by those twelve numbers (stab_lds_doubles(window, true)); additions, products, quotients and one square
// root, all correctly rounded: the force references are the transcription's bit for bit.  stabilize_kernel<TI> (ZMP false) is the body WITHOUT that code.
#pragma once

#include "wbcqp_observe.hpp"

namespace wbcqp {

constexpr int kStabMaxWindow = 64; // WBCQP_MAX_STAB_WINDOW
constexpr int kStabChannels = 8;
constexpr int kStabFilters = 5;
constexpr int kStabBlocks = 6;   // com, lf, rf, torso, left contact, right contact
constexpr int kStabPatch = 136;  // LDS doubles of the patch: 9 + 5 * 24 = 129, rounded up
constexpr double kStabFmin = 30.0; // Cop::fmin(): a float compared as 30.0
constexpr int kStabZmpPatch = 12; // ... and of the distributor's two force references behind it: left 6, right 6
enum { kStabCop = 1, kStabLcop = 2, kStabRcop = 4, kStabCom = 8, kStabLankle = 16, kStabRankle = 32, kStabFfda = 64, kStabErrCop = 128, kStabErrForce = 256,
       kStabZmp = 512, kStabErrZmp = 1024 };

// the stabiliser as the kernel reads it, by value in the kernel's arguments
struct StabDev {
    int window, nref;
    int off[kStabBlocks]; // com, lf, rf, torso, left contact, right contact; -1: contact not active
    int lf_col, rf_col;   // first of the contact's 12 force variables in a row of x_prev; -1: not active
    int lf_pos, rf_pos;
    double dt, mass;
    double com_gains[6], ankle_gains[6], ffda_gains[3], normal[3];
};

constexpr size_t stab_state_doubles(int window) { return kStabFilters + (size_t)kStabChannels * window; }
constexpr size_t stab_lds_doubles(int window, bool zmp = false) { return (size_t)kStabChannels * window + kStabPatch + (zmp ? kStabZmpPatch : 0); } // per wave

template <typename TI>
struct StabArgs {
    StabDev S;
    const TI *ref, *wrench, *com, *acom, *placement, *x_prev; // x_prev: null on the first tick
    const double* state_in; // [batch][state doubles] or null (fresh)
    double* state_out;      // the same block (or a staged copy of it), or null (discarded)
    TI* ref_out;            // [batch][nref] or null
    int* flags;             // [batch] or null
    TI* cop;                // [batch][3][2] or null
    int ldp, ldx, batch;
};

// the distributor's share of the arguments (stabilize_kernel<TI, true>)
template <typename TI>
struct StabZmpArgs : StabArgs<TI> {
    double p[6], d[6]; // zmp_p, zmp_d
    int foff[2];       // the left / right foot's force reference in a row; -1: not written
    TI* alpha;         // [batch][2] alpha of the model's ZMP, of the measured one (NaN where the law did not run), or null
};
template <typename TI, bool ZMP>
using StabKernelArgs = std::conditional_t<ZMP, StabZmpArgs<TI>, StabArgs<TI>>;

#ifdef __HIPCC__

// Eigen's eulerAngles(0, 1, 2) of a rotation given COLUMN-major (a reference's layout), then the rotation Rx(e0 + d0) Ry(e1 + d1) Rz(e2), column-major.
// [UPSTREAM-RECALL] Eigen/src/Geometry/EulerAngles.h: the first angle lies in [0, pi]; on the r0 > 0 side an added pitch acts with the opposite sign.
__device__ inline void stab_recompose(const double* Rc, double d0, double d1, double* out)
{
    const double R00 = Rc[0], R10 = Rc[1], R20 = Rc[2], R01 = Rc[3], R11 = Rc[4], R21 = Rc[5], R02 = Rc[6], R12 = Rc[7], R22 = Rc[8];
    const double pi = 3.14159265358979323846;
    double r0 = atan2(R12, R22);
    const double c2 = __dsqrt_rn(__dadd_rn(__dmul_rn(R00, R00), __dmul_rn(R01, R01)));
    double r1;
    if (r0 > 0.0) {
        r0 = __dsub_rn(r0, pi);
        r1 = atan2(-R02, -c2);
    }
    else
        r1 = atan2(-R02, c2);
    const double s1 = sin(r0), c1 = cos(r0);
    const double r2 = atan2(__dsub_rn(__dmul_rn(s1, R20), __dmul_rn(c1, R10)), __dsub_rn(__dmul_rn(c1, R11), __dmul_rn(s1, R21)));
    const double a = __dadd_rn(-r0, d0), b = __dadd_rn(-r1, d1), c = -r2;
    const double sa = sin(a), ca = cos(a), sb = sin(b), cb = cos(b), sc = sin(c), cc = cos(c);
    const double sasb = __dmul_rn(sa, sb), casb = __dmul_rn(ca, sb);
    // (+ 0.0: an entry that is zero leaves as +0, so an identity comes back as the bits of an identity)
    out[0] = __dadd_rn(__dmul_rn(cb, cc), 0.0);
    out[1] = __dadd_rn(__dadd_rn(__dmul_rn(ca, sc), __dmul_rn(sasb, cc)), 0.0);
    out[2] = __dadd_rn(__dsub_rn(__dmul_rn(sa, sc), __dmul_rn(casb, cc)), 0.0);
    out[3] = __dadd_rn(-__dmul_rn(cb, sc), 0.0);
    out[4] = __dadd_rn(__dsub_rn(__dmul_rn(ca, cc), __dmul_rn(sasb, sc)), 0.0);
    out[5] = __dadd_rn(__dadd_rn(__dmul_rn(sa, cc), __dmul_rn(casb, sc)), 0.0);
    out[6] = __dadd_rn(sb, 0.0);
    out[7] = __dadd_rn(-__dmul_rn(sa, cb), 0.0);
    out[8] = __dadd_rn(__dmul_rn(ca, cb), 0.0);
}

// x += (g * angle) / dt and y += (g2 * angle) / dt2: one entry of a velocity and of an acceleration (the reference's association)
__device__ inline double stab_bump(double x, double g, double angle, double den) { return __dadd_rn(x, __ddiv_rn(__dmul_rn(g, angle), den)); }

// one foot's raw centre of pressure (cop.cpp:87-96)
__device__ inline void stab_foot_cop(const double* pos, const double* force, const double* torque, double* out)
{
    out[0] = __dadd_rn(pos[0], __ddiv_rn(__dsub_rn(-torque[1], __dmul_rn(pos[2], force[0])), force[2]));
    out[1] = __dadd_rn(pos[1], __ddiv_rn(__dsub_rn(torque[0], __dmul_rn(pos[2], force[1])), force[2]));
}

__device__ inline double stab_norm(const double* f)
{
    return __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(f[0], f[0]), __dmul_rn(f[1], f[1])), __dmul_rn(f[2], f[2])));
}

// tsid Contact6d::getNormalForce [UPSTREAM-RECALL]: sum over the four points of normal . f_i, in that order
__device__ inline double stab_normal_force(const double* n, const double* f12)
{
    double s = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double d = __dadd_rn(__dadd_rn(__dmul_rn(n[0], f12[3 * i]), __dmul_rn(n[1], f12[3 * i + 1])), __dmul_rn(n[2], f12[3 * i + 2]));
        s = __dadd_rn(s, d);
    }
    return s;
}

__device__ inline bool stab_far(double x, double y) { return fabs(x) >= 10.0 && fabs(y) >= 10.0; }

// block of patch element i (0 .. 128) and the block's first patch element
__device__ inline int stab_block_of(int i) { return i < 9 ? 0 : 1 + (i - 9) / 24; }
__device__ inline int stab_base_of(int b) { return b == 0 ? 0 : 9 + 24 * (b - 1); }
// S.off[b] for a b that differs between lanes (a select chain: the kernel's arguments are not indexed by a lane's value)
__device__ inline int stab_off(const StabDev& S, int b)
{
    return b == 0 ? S.off[0] : b == 1 ? S.off[1] : b == 2 ? S.off[2] : b == 3 ? S.off[3] : b == 4 ? S.off[4] : S.off[5];
}

__device__ inline double stab_norm2(double x, double y) { return __dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y))); }

// zmp_distributor (stabilizer.cpp:340-429) with closest_point_on_line (431-440), everything projected to z = 0: alpha and the entries 2, 3, 4 of the left
// and right force reference (the others are +0).  la / ra: the foot's contact is active (one at least).  false: the reference's "this case should not
// exists" (only non-finite inputs get there).
__device__ inline bool stab_zmp_distribute(double mass, const double* z, const double* pl, const double* pr, bool la, bool ra, double* alpha_out,
                                           double* left, double* right)
{
    double PL[2] = {0.0, 0.0}, PR[2] = {0.0, 0.0};
    double alpha = ra ? 1.0 : 0.0;
    bool ok = true;
    if (la) {
        PL[0] = pl[0];
        PL[1] = pl[1];
    }
    if (ra) {
        PR[0] = pr[0];
        PR[1] = pr[1];
    }
    if (la && ra) {
        const double ux = __dsub_rn(PR[0], PL[0]), uy = __dsub_rn(PR[1], PL[1]);
        const double sq = __dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy));
        const double L = __dsqrt_rn(sq);
        double ex = ux, ey = uy; // Eigen's normalized() [UPSTREAM-RECALL] Eigen/src/Core/Dot.h: divided by the norm only where the squared norm is > 0
        if (sq > 0.0) {
            ex = __ddiv_rn(ux, L);
            ey = __ddiv_rn(uy, L);
        }
        const double dd = __dadd_rn(__dmul_rn(__dsub_rn(z[0], PR[0]), ex), __dmul_rn(__dsub_rn(z[1], PR[1]), ey));
        const double px = __dadd_rn(PR[0], __dmul_rn(ex, dd)), py = __dadd_rn(PR[1], __dmul_rn(ey, dd));
        const double a1 = stab_norm2(__dsub_rn(px, PL[0]), __dsub_rn(py, PL[1]));
        const double a2 = stab_norm2(__dsub_rn(PR[0], px), __dsub_rn(PR[1], py));
        if (fabs(__dsub_rn(__dsub_rn(L, a1), a2)) < 1e-10) alpha = __ddiv_rn(a1, L);
        else if (a1 < a2) alpha = 0.0;
        else if (a1 > a2) alpha = 1.0;
        else {
            alpha = __longlong_as_double(0x7ff8000000000000LL);
            ok = false;
        }
    }
    const double f_r = __dmul_rn(__dmul_rn(-alpha, mass), 9.81);
    const double f_l = __dmul_rn(__dmul_rn(-__dsub_rn(1.0, alpha), mass), 9.81);
    double tau0[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) tau0[k] = __dsub_rn(__dmul_rn(-__dsub_rn(PR[k], z[k]), f_r), __dmul_rn(__dsub_rn(PL[k], z[k]), f_l));
    const double tauR1 = __dmul_rn(alpha, tau0[1]), tauL1 = __dmul_rn(__dsub_rn(1.0, alpha), tau0[1]);
    const bool neg = tau0[0] < 0.0;
    const double tauR0 = neg ? tau0[0] : 0.0, tauL0 = neg ? 0.0 : tau0[0];
    left[0] = f_l;
    left[1] = tauL1;
    left[2] = -tauL0;
    right[0] = f_r;
    right[1] = tauR1;
    right[2] = -tauR0;
    *alpha_out = alpha;
    return ok;
}

// one entry of zmp_distributor_admittance (stabilizer.cpp:307-308): t - p (t - s) - d (t - s) / dt
__device__ inline double stab_zmp_entry(double t, double s, double p, double d, double dt)
{
    const double e = __dsub_rn(t, s);
    return __dsub_rn(__dsub_rn(t, __dmul_rn(p, e)), __ddiv_rn(__dmul_rn(d, e), dt));
}

// ZMP false: stabilize_kernel<TI>, what wbcqp_stabilize launches; ZMP true: the second instantiation, with the distributor compiled in
template <typename TI, bool ZMP = false>
__global__ __launch_bounds__(kObserveThreads) void stabilize_kernel(const StabKernelArgs<TI, ZMP> args)
{
    extern __shared__ double stab_lds[];
    const StabDev& S = args.S;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kObservePerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int W = S.window, nref = S.nref;
    double* ring = stab_lds + (size_t)wave * stab_lds_doubles(W, ZMP);
    double* patch = ring + (size_t)kStabChannels * W;
    const size_t state_doubles = stab_state_doubles(W);
    const bool mine = lane < kStabChannels;
    const int ch = lane & (kStabChannels - 1);
    const int fi = ch < 6 ? ch >> 1 : ch - 3; // the channel's filter

    // ---- the state comes in: the lane's filter's count and head, the ring (zero without a state) ----------------------------------------------
    int count = 0, head = 0;
    if (args.state_in) {
        const double* St = args.state_in + (size_t)inst * state_doubles;
        const double w0 = St[fi];
        count = min(max(__double2loint(w0), 0), W); // (bytes that no call of this stabiliser wrote stay inside the ring)
        head = min(max(__double2hiint(w0), 0), W - 1);
        for (int e = lane; e < kStabChannels * W; e += kWave) ring[e] = St[kStabFilters + e]; // (the ring lies in the state as it lies here: 64 lanes, 8 rows a turn)
    }
    else {
        for (int e = lane; e < kStabChannels * W; e += kWave) ring[e] = 0.0;
    }
    // ---- the patch: the six blocks as they lie in the row (an inactive contact's block: zeros, never read again) -------------------------------
    const TI* ref = args.ref + (size_t)inst * nref;
    for (int i = lane; i < 9 + 24 * (kStabBlocks - 1); i += kWave) {
        const int b = stab_block_of(i);
        const int off = stab_off(S, b);
        patch[i] = off >= 0 ? (double)ref[off + (i - stab_base_of(b))] : 0.0;
    }

    // ---- 1. this tick's samples (every lane forms all of them: they are a handful, and wave-uniform) --------------------------------------------
    double lf[3], lt[3], rf[3], rt[3], lp[3], rp[3];
    {
        const TI* w = args.wrench + (size_t)inst * 12;
        const TI* P = args.placement + (size_t)inst * args.ldp;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lf[k] = (double)w[k];
            lt[k] = (double)w[3 + k];
            rf[k] = (double)w[6 + k];
            rt[k] = (double)w[9 + k];
            lp[k] = (double)P[S.lf_pos + k];
            rp[k] = (double)P[S.rf_pos + k];
        }
    }
    const bool has_l = lf[2] > kStabFmin, has_r = rf[2] > kStabFmin, has_b = has_l && has_r;
    double lraw[2] = {0.0, 0.0}, rraw[2] = {0.0, 0.0}, craw[2] = {0.0, 0.0};
    if (has_l) stab_foot_cop(lp, lf, lt, lraw);
    if (has_r) stab_foot_cop(rp, rf, rt, rraw);
    if (has_b) {
        const double ratio_l = __ddiv_rn(lf[2], __dadd_rn(lf[2], rf[2]));
        const double ratio_r = __dsub_rn(1.0, ratio_l);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double in_l = __dadd_rn(__dmul_rn(ratio_l, lraw[k]), __dmul_rn(ratio_r, __dsub_rn(__dadd_rn(rraw[k], rp[k]), lp[k])));
            const double in_r = __dadd_rn(__dmul_rn(ratio_l, __dsub_rn(__dadd_rn(lraw[k], lp[k]), rp[k])), __dmul_rn(ratio_r, rraw[k]));
            craw[k] = __dadd_rn(__dmul_rn(in_l, ratio_l), __dmul_rn(in_r, ratio_r));
        }
    }
    const bool load_l = stab_norm(lf) > kStabFmin, load_r = stab_norm(rf) > kStabFmin;

    // ---- 2. the filters: lane c pushes channel c ----------------------------------------------------------------------------------------------
    const double sample = ch == 0 ? craw[0] : ch == 1 ? craw[1] : ch == 2 ? lraw[0] : ch == 3 ? lraw[1] : ch == 4 ? rraw[0] : ch == 5 ? rraw[1] : ch == 6 ? lf[2] : rf[2];
    const bool push = fi == 0 ? has_b : fi == 1 ? has_l : fi == 2 ? has_r : fi == 3 ? load_l : load_r;
    const bool reset = (fi == 1 && !has_l) || (fi == 2 && !has_r);
    wave_sync(); // the ring and the patch are whole: from here on lane c touches column c of the ring alone
    double fv = 0.0;
    if (push && mine) {
        ring[head * kStabChannels + lane] = sample;
        head = head + 1 == W ? 0 : head + 1;
        count = count < W ? count + 1 : W;
        int r = head - count;
        if (r < 0) r += W;
        double sum = 0.0;
        for (int a = 0; a < count; ++a) {
            sum += ring[r * kStabChannels + ch];
            r = r + 1 == W ? 0 : r + 1;
        }
        fv = sum / (double)count;
    }
    if (reset && mine) {
        count = 0;
        head = 0;
    }
    const int ready = count >= W ? 1 : 0;
    double cp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cp[k] = __shfl(fv, k, kWave);
    const double fz_l = __shfl(fv, 6, kWave), fz_r = __shfl(fv, 7, kWave);
    const bool ok_c = has_b && __shfl(ready, 0, kWave) && cp[0] == cp[0] && cp[1] == cp[1];
    const bool ok_l = has_l && __shfl(ready, 2, kWave) && cp[2] == cp[2] && cp[3] == cp[3];
    const bool ok_r = has_r && __shfl(ready, 4, kWave) && cp[4] == cp[4] && cp[5] == cp[5];
    const bool ready_fl = __shfl(ready, 6, kWave) != 0, ready_fr = __shfl(ready, 7, kWave) != 0;
    const bool any = ok_c || ok_l || ok_r;
    const double vx = ok_c ? cp[0] : ok_l ? cp[2] : cp[4], vy = ok_c ? cp[1] : ok_l ? cp[3] : cp[5];

    // ---- which laws apply, and the reference's two sanity checks (in its order: the first that trips ends the tick) -----------------------------
    const bool do_l = ok_l && S.off[4] >= 0, do_r = ok_r && S.off[5] >= 0;
    const bool do_f = args.x_prev != nullptr && S.lf_col >= 0 && S.rf_col >= 0 && ready_fl && ready_fr;
    const bool err_cop = (any && stab_far(vx, vy)) || (do_l && stab_far(cp[2], cp[3])) || (do_r && stab_far(cp[4], cp[5]));
    // the distributor (every lane forms it: a few dozen wave-uniform operations, and the flags need its guard): after the far-CoP guard, before the force guard
    [[maybe_unused]] double fref[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    [[maybe_unused]] double alpha_t = __longlong_as_double(0x7ff8000000000000LL), alpha_s = alpha_t;
    bool err_zmp = false;
    [[maybe_unused]] bool do_z = false;
    if constexpr (ZMP) {
        if (any && !err_cop) {
            const TI* gc = args.com + (size_t)inst * 3;
            const TI* ga = args.acom + (size_t)inst * 3;
            const double k = __ddiv_rn((double)gc[2], 9.81);
            const double zref[2] = {__dsub_rn((double)gc[0], __dmul_rn(k, (double)ga[0])), __dsub_rn((double)gc[1], __dmul_rn(k, (double)ga[1]))};
            const double zcop[2] = {vx, vy};
            const bool la = S.off[4] >= 0, ra = S.off[5] >= 0; // (the host refuses a call with neither)
            const double* pl = patch + stab_base_of(4); // the contacts' references as they lie in ref: no law has run yet
            const double* pr = patch + stab_base_of(5);
            double tl[3], tr[3], sl[3], sr[3];
            const bool ok_t = stab_zmp_distribute(S.mass, zref, pl, pr, la, ra, &alpha_t, tl, tr);
            const bool ok_s = stab_zmp_distribute(S.mass, zcop, pl, pr, la, ra, &alpha_s, sl, sr);
            err_zmp = !(ok_t && ok_s);
            do_z = !err_zmp;
#pragma unroll
            for (int e = 0; e < 6; ++e) { // entries 0, 1, 5: both splits hold +0 there
                const bool mid = e >= 2 && e <= 4;
                fref[e] = stab_zmp_entry(mid ? tl[e - 2] : 0.0, mid ? sl[e - 2] : 0.0, args.p[e], args.d[e], S.dt);
                fref[6 + e] = stab_zmp_entry(mid ? tr[e - 2] : 0.0, mid ? sr[e - 2] : 0.0, args.p[e], args.d[e], S.dt);
            }
        }
    }
    const double ten_mg = __dmul_rn(10.0, __dmul_rn(S.mass, 9.81));
    const bool err_force = !err_cop && !err_zmp && do_f && fabs(__dadd_rn(fz_l, fz_r)) > ten_mg;
    const bool apply = !err_cop && !err_zmp && !err_force;
    int flags = (ok_c ? kStabCop : 0) | (ok_l ? kStabLcop : 0) | (ok_r ? kStabRcop : 0) | (err_cop ? kStabErrCop : 0) | (err_force ? kStabErrForce : 0);
    if (apply) flags |= (any ? kStabCom : 0) | (do_l ? kStabLankle : 0) | (do_r ? kStabRankle : 0) | (do_f ? kStabFfda : 0);
    if constexpr (ZMP) {
        flags |= err_zmp ? kStabErrZmp : 0;
        do_z = do_z && apply; // (the force guard tripped: the law did not run)
        if (do_z) flags |= kStabZmp;
        else alpha_t = alpha_s = __longlong_as_double(0x7ff8000000000000LL);
    }

    // ---- 3. the laws, on lane 0 -------------------------------------------------------------------------------------------------------------
    if (lane == 0 && apply && args.ref_out) {
        const double dt = S.dt, dt2 = __dmul_rn(S.dt, S.dt);
        if (any) { // stabilizer.cpp:31-59
            const TI* gc = args.com + (size_t)inst * 3;
            const TI* ga = args.acom + (size_t)inst * 3;
            const double k = __ddiv_rn((double)gc[2], 9.81);
            const double cop2[2] = {vx, vy};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double zmp = __dsub_rn((double)gc[c], __dmul_rn(k, (double)ga[c]));
                const double cor = __dsub_rn(zmp, cop2[c]);
                patch[c] = __dsub_rn(patch[c], __dmul_rn(S.com_gains[c], cor));
                patch[3 + c] = __dsub_rn(patch[3 + c], __ddiv_rn(__dmul_rn(S.com_gains[2 + c], cor), dt));
                patch[6 + c] = __dsub_rn(patch[6 + c], __ddiv_rn(__dmul_rn(S.com_gains[4 + c], cor), dt2));
            }
        }
        if constexpr (ZMP) { // stabilizer.cpp:277-311: the two force references (a block that is not written keeps what ref holds)
            if (do_z) {
#pragma unroll
                for (int e = 0; e < kStabZmpPatch; ++e) patch[kStabPatch + e] = fref[e];
            }
        }
        for (int side = 0; side < 2; ++side) { // stabilizer.cpp:168-224
            if (!(side ? do_r : do_l)) continue;
            double* foot = patch + stab_base_of(1 + side);
            double* contact = patch + stab_base_of(4 + side);
            const double* g = S.ankle_gains;
            const double pitch = __dmul_rn(g[0], __dsub_rn(side ? cp[4] : cp[2], side ? rp[0] : lp[0]));
            const double roll = __dmul_rn(g[1], __dsub_rn(side ? cp[5] : cp[3], side ? rp[1] : lp[1]));
            double Rn[9];
            stab_recompose(foot + 3, roll, pitch, Rn);
            foot[12 + 4] = stab_bump(foot[12 + 4], g[2], pitch, dt);
            foot[12 + 3] = stab_bump(foot[12 + 3], g[3], roll, dt);
            foot[18 + 4] = stab_bump(foot[18 + 4], g[4], pitch, dt2);
            foot[18 + 3] = stab_bump(foot[18 + 3], g[5], roll, dt2);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                foot[3 + k] = Rn[k];
                contact[3 + k] = Rn[k];
            }
            for (int k = 12; k < 24; ++k) contact[k] = foot[k]; // (the FOOT TASK's velocity and acceleration, not the contact's own: as the reference)
        }
        if (do_f) { // stabilizer.cpp:226-266
            const TI* x = args.x_prev + (size_t)inst * args.ldx;
            double fl[12], fr[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                fl[k] = (double)x[S.lf_col + k];
                fr[k] = (double)x[S.rf_col + k];
            }
            const double nl = stab_normal_force(S.normal, fl), nr = stab_normal_force(S.normal, fr);
            const double zctrl = __dsub_rn(fabs(__dsub_rn(nl, nr)), fabs(__dsub_rn(fz_l, fz_r)));
            const double troll = __dmul_rn(S.ffda_gains[0], zctrl);
            double* torso = patch + stab_base_of(3);
            double Rn[9];
            stab_recompose(torso + 3, troll, 0.0, Rn);
            torso[12 + 3] = stab_bump(torso[12 + 3], S.ffda_gains[1], troll, dt);
            torso[18 + 3] = stab_bump(torso[18 + 3], S.ffda_gains[2], troll, dt2);
#pragma unroll
            for (int k = 0; k < 9; ++k) torso[3 + k] = Rn[k];
        }
    }
    wave_sync(); // the patch is rewritten

    // ---- 4. the outputs ---------------------------------------------------------------------------------------------------------------------
    if (args.ref_out) {
        TI* out = args.ref_out + (size_t)inst * nref;
        for (int e = lane; e < nref; e += kWave) {
            double v = (double)ref[e];
#pragma unroll
            for (int b = 0; b < kStabBlocks; ++b) {
                const int off = S.off[b], len = b == 0 ? 9 : 24;
                if (off >= 0 && e >= off && e < off + len) v = patch[stab_base_of(b) + (e - off)];
            }
            if constexpr (ZMP) {
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const int off = args.foff[f];
                    if (do_z && off >= 0 && e >= off && e < off + 6) v = patch[kStabPatch + 6 * f + (e - off)];
                }
            }
            out[e] = (TI)v;
        }
    }
    if (lane == 0 && args.flags) args.flags[inst] = flags;
    if constexpr (ZMP) {
        if (lane < 2 && args.alpha) args.alpha[(size_t)inst * 2 + lane] = (TI)(lane == 0 ? alpha_t : alpha_s);
    }
    if (lane < 6 && args.cop) {
        const bool ok = fi == 0 ? ok_c : fi == 1 ? ok_l : ok_r;
        args.cop[(size_t)inst * 6 + lane] = (TI)(ok ? fv : __longlong_as_double(0x7ff8000000000000LL));
    }
    // ---- the state leaves ---------------------------------------------------------------------------------------------------------------------
    if (args.state_out) {
        double* St = args.state_out + (size_t)inst * state_doubles;
        if (mine && (lane >= 6 || !(lane & 1))) St[fi] = __hiloint2double(head, count);
        for (int e = lane; e < kStabChannels * W; e += kWave) St[kStabFilters + e] = ring[e]; // (after the sync that follows the laws: every push is in)
    }
}

#endif // __HIPCC__
} // namespace wbcqp
