// wbcqp_fdyn.hpp -- which accelerations joint torques produce, for a whole fleet (wbcqp_mass_matrix, wbcqp_forward_dynamics, wbcqp_spd_commands):
//     (M(q) + diag(damping)) a = tau - nle(q, v) + sum_k J_k(q)' w_k
// What the reference ships as RobotModel::inertia_matrix() (include/inria_wbc/utils/robot_model.hpp:41 there) and as
// inria_wbc::robot_dart::compute_spd (include/inria_wbc/robot_dart/cmd.hpp:10-38), the stable-PD law of its drivers:
//     qddot = (M + Kd dt)^-1 (-C + p + d + f_c),   commands = p + d - Kd qddot dt,   p = -Kp (q + dq dt - target),   d = -Kd dq
//
// The kernel does NOT compute the bias nle(q, v) - sum_k J_k' w_k: the entry point launches rnea_kernel (a = NULL) into the caller's OUTPUT row
// first and this kernel behind it on the same stream; it reads its own instance's row as the bias and overwrites it with the result.  No hidden
// scratch, no state on the handle, rnea_kernel untouched.  On an F32 handle the bias therefore passes through a float.
//
// Three phases, one wavefront per instance, four instances per workgroup, no workgroup barrier, no atomics:
//   1. CRBA in rnea_kernel's formulation (ONE world-aligned frame at the base; the joint transform and the placement sweep are that kernel's
//      statements, as a copy -- DESIGN 4.15).  lanes = bodies: the body's inertia about the common origin, ten numbers (m, h = m c, I_o), by the
//      statements of rnea_kernel's Io / hc block; composites: every body adds its ten numbers to its parent's, last body first (a serial
//      wave-uniform loop over readlane broadcasts; why not prefix sums: see there).  lanes = dofs: lane j forms S_j and
//      F_j = Y_subtree(j) S_j; M(i, j) = S_i . F_j for i <= j where body(j) lies in the subtree of body(i), an exact zero elsewhere;
//      lane j writes the value to (i, j) AND (j, i): both triangles hold the same bits.
//      The free-flyer's six columns are in the base's own axes, as in rnea_kernel.
//   2. Cholesky of M + diag(damping) in wave-private LDS, [nv] rows of fdyn_row_stride(nv) doubles (odd: a column walk touches 32 banks
//      in turn).  Left-looking, lanes = rows: column k is A(i, k) - sum_{j<k} L(i, j) L(k, j), j ascending.  A pivot that is not > 0 (a NaN is
//      not) ends the instance: info = k + 1 (LAPACK's potrf), the output row all NaN; no other instance notices.
//   3. L y = b, L' a = y with lanes = rows (the running right-hand side stays in a register), then the epilogue.
// Phases 2 and 3 round every product and every sum once (no contraction into fused multiply-adds).
// LDS traffic inside the wave is ordered by the wave_sync() of wbcqp_prims.hpp (release fence / wave_barrier / acquire fence), as in terms_kernel.
#pragma once

#include "wbcqp_rnea.hpp"

namespace wbcqp {

constexpr int kFdynThreads = 256;
constexpr int kFdynPerBlock = kFdynThreads / kWave; // instances per workgroup
constexpr int kFdynMaxDof = 64;

inline int fdyn_row_stride(int nv) { return nv | 1; }
inline int fdyn_lds_bytes(int nv) { return kFdynPerBlock * nv * fdyn_row_stride(nv) * 8; }

template <typename TI>
struct FdynArgs {
    RneaDev D;                   // the tree's tables (the wrench frames are rnea_kernel's business: not read here)
    const TI *q, *v, *rhs;       // [batch][nq]; [batch][nv] or null; rows ldr apart: tau (nv long, or null) / SPD: target (na long)
    TI* out;                     // [batch][nv]: the bias on entry, a / SPD: commands on return (null with M)
    TI* qddot;                   // SPD: [batch][nv] or null
    TI* M;                       // [batch][nv][nv] or null; given: phase 1 alone
    int* info;                   // [batch] or null
    int ldr, batch;
    double dt, kp, kd;           // SPD: the law
    double damping[kFdynMaxDof]; // otherwise: the diagonal, by value
};

#ifdef __HIPCC__

template <typename TI, bool SPD>
__global__ __launch_bounds__(kFdynThreads) void fdyn_kernel(const FdynArgs<TI> args)
{
    extern __shared__ double fdyn_lds[];
    const RneaDev& D = args.D;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kFdynPerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int nb = D.nb, nv = D.nv;
    const int ld = nv | 1;
    double* A = fdyn_lds + (size_t)wave * nv * ld;
    const int* ip = D.ipool;
    const double* dp = D.dpool;
    const TI* gq = args.q + (size_t)inst * D.nq;

    // the constants of this lane's dof (two dependent reads): asked for here, they arrive behind the state
    const bool dof = lane < nv;
    const int cj = min(lane, nv - 1);
    const int bj = ip[D.i_bodyof + cj], kofj = ip[D.i_kof + cj];
    const int lastj = ip[D.i_last + bj], jtypej = ip[D.i_jtype + bj], iqj = ip[D.i_idxq + bj];

    // the right-hand side's ingredients, fetched ahead of phase 1
    const int nbase = D.floating_base ? 6 : 0;
    double bias = 0.0, rhs = 0.0, pd = 0.0, damp = 0.0;
    if (!args.M) {
#pragma clang fp contract(off)
        bias = (double)args.out[(size_t)inst * nv + cj];
        const double vj = args.v ? (double)args.v[(size_t)inst * nv + cj] : 0.0;
        if (SPD) {
            if (cj >= nbase) {
                const double qj = (double)gq[iqj], tj = (double)args.rhs[(size_t)inst * args.ldr + (cj - nbase)];
                const double p = -args.kp * (qj + vj * args.dt - tj);
                const double d = -args.kd * vj;
                pd = p + d;
                damp = args.kd * args.dt;
            }
        }
        else {
            pd = args.rhs ? (double)args.rhs[(size_t)inst * args.ldr + cj] : 0.0;
            damp = args.damping[cj];
        }
        rhs = pd - bias;
    }

    // ---- lanes = bodies: joint transform (lanes past the last body repeat it; nothing reads what they hold) ---------------------
    const int bi = min(lane, nb - 1);
    const int jt = ip[D.i_jtype + bi];
    const int iq = ip[D.i_idxq + bi];
    double Yb[10]; // this body's inertia: fetched now, used after the sweep
#pragma unroll
    for (int r = 0; r < 10; ++r) Yb[r] = dp[D.d_inertia + 10 * bi + r];
    int anc[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) anc[r] = (r < D.nrounds) ? ip[D.i_anc + r * nb + bi] : -1;
    double R[9];
    V3 p;
    {
        const double* P = dp + D.d_place + 12 * bi;
        if (jt == J_FREEFLYER) {
            const double x = (double)gq[3], y = (double)gq[4], z = (double)gq[5], w = (double)gq[6];
            const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
            const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
                         tyz = tz * y, tzz = tz * z;
            R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
            R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
            R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
            p = {0.0, 0.0, 0.0}; // the common origin IS the base: q[0..2] is not read
        }
        else {
            const int a = (jt <= J_RZ) ? jt - J_RX : jt - J_PX;
            const double qj = (double)gq[iq];
            if (jt <= J_RZ) {
                double sn, cs;
                sincos_joint(qj, &sn, &cs);
                // P.R * Rot(axis): the axis column stays, the other two mix
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double c0 = P[3 * r], c1 = P[3 * r + 1], c2 = P[3 * r + 2];
                    const double pa = (a == 0) ? c0 : (a == 1) ? c1 : c2;
                    const double pb = (a == 0) ? c1 : (a == 1) ? c2 : c0;
                    const double pd_ = (a == 0) ? c2 : (a == 1) ? c0 : c1;
                    const double nb_ = cs * pb + sn * pd_, nd_ = cs * pd_ - sn * pb;
                    R[3 * r] = (a == 0) ? pa : (a == 1) ? nd_ : nb_;
                    R[3 * r + 1] = (a == 0) ? nb_ : (a == 1) ? pa : nd_;
                    R[3 * r + 2] = (a == 0) ? nd_ : (a == 1) ? nb_ : pa;
                }
                p = ld3(P + 9);
            }
            else {
#pragma unroll
                for (int r = 0; r < 9; ++r) R[r] = P[r];
                const V3 ax = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
                p = ld3(P + 9) + qj * mv(P, ax);
            }
        }
    }
    // ---- down the tree by ancestor doubling: after round r every body holds the composition over its 2^(r+1) nearest
    //      ancestors-and-self (rigid transforms compose associatively) -------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        if (r < D.nrounds) {
            const int src = anc[r] >= 0 ? anc[r] : lane;
            double Ra[9], Rn[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) Ra[k] = __shfl(R[k], src, kWave);
            const V3 pa = {__shfl(p.x, src, kWave), __shfl(p.y, src, kWave), __shfl(p.z, src, kWave)};
            if (anc[r] >= 0) {
                mm(Ra, R, Rn);
                p = mv(Ra, p) + pa;
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = Rn[k];
            }
        }
    }
    // ---- the body's inertia about the common origin: m, h = m c, I_o ------------------------------------------------------------------
    double sc[10];
    {
        const double m = Yb[0];
        const V3 cw = mv(R, ld3(Yb + 1)) + p;
        const double Ic[9] = {Yb[4], Yb[5], Yb[6], Yb[5], Yb[7], Yb[8], Yb[6], Yb[8], Yb[9]};
        double RI[9], Iw[9], Rt[9];
        mm(R, Ic, RI);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rt[3 * i + j] = R[3 * j + i];
        mm(RI, Rt, Iw);
        const double c2 = dot(cw, cw);
        const V3 hc = m * cw;
        const double Io[6] = {Iw[0] + m * (c2 - cw.x * cw.x), Iw[1] - m * cw.x * cw.y, Iw[2] - m * cw.x * cw.z,
                              Iw[4] + m * (c2 - cw.y * cw.y), Iw[5] - m * cw.y * cw.z, Iw[8] + m * (c2 - cw.z * cw.z)};
        sc[0] = m; sc[1] = hc.x; sc[2] = hc.y; sc[3] = hc.z;
#pragma unroll
        for (int r = 0; r < 6; ++r) sc[4 + r] = Io[r];
    }
    // ---- composites: every body folds its composite into its parent's, last body first.  The bodies are numbered depth-first with parents ahead
    //      of children, so whatever hangs under body i has been folded into it before its own turn.  NOT rnea_kernel's prefix sums
    //      (scan[last] - scan[body - 1]): a difference of two running totals of the whole robot carries the robot's rounding error, 1e-14 kg m^2
    //      on Talos, into the composite of a 8e-6 kg m^2 gripper link -- 1e-9 of that link's M(j, j), which a solve then multiplies by an
    //      acceleration of 1e7 (measured: 2e-8 N m left in the force-space round trip, against 6e-12 with sums that only ever hold a subtree)
    for (int i = nb - 1; i > 0; --i) {
        const int par = __builtin_amdgcn_readlane(anc[0], i); // (anc[0]: the parent)
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const double t = bcast_lane(sc[r], i);
            if (lane == par) sc[r] += t;
        }
    }
    // ---- lanes = dofs: S_j and F_j = Y_subtree(j) S_j ---------------------------------------------------------------------------------------
    double Ys[10], Rb[9];
#pragma unroll
    for (int r = 0; r < 10; ++r) Ys[r] = __shfl(sc[r], bj, kWave);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rb[k] = __shfl(R[k], bj, kWave);
    const V3 pb = {__shfl(p.x, bj, kWave), __shfl(p.y, bj, kWave), __shfl(p.z, bj, kWave)};
    V3 Sv, Sw, Fl, Fa;
    {
        const int a = (jtypej == J_FREEFLYER) ? (kofj % 3) : (jtypej <= J_RZ) ? jtypej - J_RX : jtypej - J_PX;
        const bool ang = (jtypej == J_FREEFLYER) ? (kofj >= 3) : (jtypej <= J_RZ);
        const V3 wax = (a == 0) ? col(Rb, 0) : (a == 1) ? col(Rb, 1) : col(Rb, 2); // world direction of the axis
        Sw = ang ? wax : V3{0.0, 0.0, 0.0};
        Sv = ang ? cross(pb, wax) : wax;
        const V3 h = {Ys[1], Ys[2], Ys[3]};
        Fl = Ys[0] * Sv + cross(Sw, h);
        Fa = symv(Ys + 4, Sw) + cross(h, Sv);
    }
    // ---- M(i, j) = S_i . F_j, i <= j: a wave-uniform loop over the rows, lane j keeps column j and mirrors it ------------------------------
    for (int i = 0; i < nv; ++i) {
        const V3 Svi = {bcast_lane(Sv.x, i), bcast_lane(Sv.y, i), bcast_lane(Sv.z, i)};
        const V3 Swi = {bcast_lane(Sw.x, i), bcast_lane(Sw.y, i), bcast_lane(Sw.z, i)};
        const int bodyi = __builtin_amdgcn_readlane(bj, i), lasti = __builtin_amdgcn_readlane(lastj, i);
        const double dotv = dot(Svi, Fl) + dot(Swi, Fa);
        const double mij = (bodyi <= bj && bj <= lasti) ? dotv : 0.0; // unrelated branches: an exact zero, written as a zero
        if (dof && lane >= i) {
            A[i * ld + lane] = mij;
            A[lane * ld + i] = mij;
        }
    }
    wave_sync();
    if (args.M) {
        TI* gM = args.M + (size_t)inst * nv * nv;
        for (int r = 0; r < nv; ++r)
            if (dof) gM[(size_t)r * nv + lane] = (TI)A[r * ld + lane];
        return;
    }
    // ---- phase 2: Cholesky of M + diag(damping), left-looking, lanes = rows ----------------------------------------------------------------
    {
#pragma clang fp contract(off)
        if (dof) A[lane * ld + lane] = A[lane * ld + lane] + damp;
        wave_sync();
        int failed = 0;
        const double* Ai = A + cj * ld;
        for (int k = 0; k < nv; ++k) {
            const double* Ak = A + k * ld;
            double s = Ai[k];
            for (int j = 0; j < k; ++j) s = s - Ai[j] * Ak[j];
            const double d = bcast_lane(s, k);
            if (!(d > 0.0)) { // (wave-uniform; a NaN pivot lands here too)
                failed = k + 1;
                break;
            }
            const double r = sqrt(d);
            if (dof && lane >= k) A[lane * ld + k] = (lane == k) ? r : s / r;
            wave_sync();
        }
        TI* gout = args.out + (size_t)inst * nv;
        TI* gqdd = (SPD && args.qddot) ? args.qddot + (size_t)inst * nv : nullptr;
        if (failed) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            if (dof) {
                gout[lane] = (TI)nan;
                if (gqdd) gqdd[lane] = (TI)nan;
            }
            if (lane == 0 && args.info) args.info[inst] = failed;
            return;
        }
        // ---- phase 3: L y = b by columns, L' a = y by rows; lane i holds entry i ---------------------------------------------------------
        double b = dof ? rhs : 0.0;
        for (int k = 0; k < nv; ++k) {
            const double yk = bcast_lane(b, k) / A[k * ld + k];
            const double lik = Ai[k];
            if (lane == k) b = yk;
            else if (lane > k) b = b - lik * yk;
        }
        for (int k = nv - 1; k >= 0; --k) {
            const double xk = bcast_lane(b, k) / A[k * ld + k];
            const double lki = A[k * ld + cj];
            if (lane == k) b = xk;
            else if (lane < k) b = b - lki * xk;
        }
        if (dof) {
            if (SPD) {
                const double kdj = (cj >= nbase) ? args.kd : 0.0;
                gout[lane] = (TI)(pd - kdj * b * args.dt);
                if (gqdd) gqdd[lane] = (TI)b;
            }
            else
                gout[lane] = (TI)b;
        }
        if (lane == 0 && args.info) args.info[inst] = 0;
    }
}

#endif // __HIPCC__
} // namespace wbcqp
