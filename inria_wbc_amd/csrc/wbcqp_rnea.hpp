// wbcqp_rnea.hpp -- which joint torques a motion needs under external wrenches, for a whole fleet (wbcqp_inverse_dynamics):
//     tau = M(q) a + nle(q, v) - sum_k J_k(q)' w_k
// What the reference ships as inria_wbc::utils::RobotModel (src/utils/robot_model.cpp there): update() followed by pinocchio::rnea,
// nonLinearEffects (a = 0), computeGeneralizedGravity (a = 0, v = 0) and compute_rnea_double_support (:138-229), which subtracts the LOCAL frame
// Jacobians' transposes times the measured foot wrenches.
//
// Formulation: the rows kernel's (wbcqp_terms.hpp, wave 0) -- ONE frame, world-aligned with its origin at the floating base (the base translation
// is never read: neither the dynamics nor a wrench given in a frame's own axes depends on where the world origin is, and the moments about the
// common origin stay as small as the robot).  Spatial quantities of a subtree are then plain sums over its bodies, and the bodies are numbered
// depth-first, so a subtree is a contiguous lane range:
//   lanes = bodies:  joint transform from q; placement, then velocity, then the FULL acceleration (S_j a_j plus the velocity-product term) down
//                    the tree by nrounds rounds of ancestor doubling over ds_bpermute; gravity enters as the root's acceleration, -g on every body;
//                    body force f_i = I_i a_i + v_i x* I_i v_i about the common origin
//   wrench frames:   a wave-uniform loop over k < n_frames (<= 8): the lane of the frame's body forms the frame's placement, turns w_k into the
//                    common axes, shifts it to the common origin and subtracts it from its own body force (two frames on one body: in loop order)
//   subtree totals:  six inclusive prefix sums over the lanes (wave_scan_incl), then scan[i_last(i)] - scan[i - 1] by ds_bpermute
//   lanes = dofs:    tau_j = S_j . F_subtree(body of j); the free-flyer's six are the root's total in the base's own axes.  Lane j stores tau[j].
// One wavefront per instance, four instances per workgroup, no LDS, no workgroup barrier, no atomics; every sum runs in a fixed order and an
// instance's bits depend on its own rows alone -- the same at whatever index or batch size they arrive.  F32 handles read float, compute in
// double, write float.  The joint transform and the placement sweep are observe_kernel's, statement for statement, as a copy (a
// function shared with an existing kernel changes that kernel's register allocation).
#pragma once

#include "wbcqp_terms.hpp"

namespace wbcqp {

constexpr int kRneaThreads = 256;
constexpr int kRneaPerBlock = kRneaThreads / kWave; // instances per workgroup
constexpr int kMaxWrenchFrames = 8;

// the tree's tables (a copy of the TermsDev fields this kernel reads) and the slot's wrench frames
struct RneaDev {
    int nb, nq, nv, floating_base, nrounds;
    double g[3];
    const int* ipool;
    const double* dpool;
    int i_jtype, i_last, i_idxq, i_idxv, i_anc; // [nb], [nb], [nb], [nb], [nrounds][nb]
    int i_bodyof, i_kof;                        // [nv]
    int d_place, d_inertia;                     // [nb][12], [nb][10]
    int n_frames;                               // wrench frames in use (0 when the call has no wrench)
    const int* frame_body;                      // [n_frames] body of wrench frame k
    const double* frame_place;                  // [n_frames][12] frame in its body's joint frame
};

template <typename TI>
struct RneaArgs {
    RneaDev D;
    const TI *q, *v, *a, *wrench; // [batch][nq]; [batch][nv] or null; rows lda apart or null; [batch][n_frames][6] or null
    TI* tau;                      // [batch][nv]
    int lda, batch;
};

#ifdef __HIPCC__

// (ov, ow) += the same pair of the 2^r-th ancestor, for r = 0 .. nrounds - 1: a path sum down the tree
__device__ __forceinline__ void rnea_path_sum(const int (&anc)[6], int nrounds, int lane, V3& ov, V3& ow)
{
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        if (r < nrounds) {
            const int src = anc[r] >= 0 ? anc[r] : lane;
            const V3 a = {__shfl(ov.x, src, kWave), __shfl(ov.y, src, kWave), __shfl(ov.z, src, kWave)};
            const V3 b = {__shfl(ow.x, src, kWave), __shfl(ow.y, src, kWave), __shfl(ow.z, src, kWave)};
            if (anc[r] >= 0) { ov = ov + a; ow = ow + b; }
        }
    }
}

template <typename TI>
__global__ __launch_bounds__(kRneaThreads) void rnea_kernel(const RneaArgs<TI> args)
{
    const RneaDev& D = args.D;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kRneaPerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int nb = D.nb, nv = D.nv, nf = D.n_frames;
    const int* ip = D.ipool;
    const double* dp = D.dpool;
    const bool vel = args.v != nullptr, acc = args.a != nullptr; // wave-uniform: a sweep whose input is absent is not run
    const TI* gq = args.q + (size_t)inst * D.nq;
    const TI* gv = vel ? args.v + (size_t)inst * nv : nullptr;
    const TI* ga = acc ? args.a + (size_t)inst * args.lda : nullptr;
    const TI* gw = nf ? args.wrench + (size_t)inst * nf * 6 : nullptr;

    // the constants of this lane's dof (two dependent reads): asked for here, they arrive behind the state
    const int cj = min(lane, nv - 1);
    const int bj = ip[D.i_bodyof + cj], kofj = ip[D.i_kof + cj];
    const int lastj = ip[D.i_last + bj], jtypej = ip[D.i_jtype + bj];

    // ---- lanes = bodies: joint transform (lanes past the last body repeat it and count for nothing in the sums) -------------------
    const bool body = lane < nb;
    const int bi = min(lane, nb - 1);
    const int jt = ip[D.i_jtype + bi];
    const int iq = ip[D.i_idxq + bi], iv = ip[D.i_idxv + bi];
    double Yb[10]; // this body's inertia: fetched now, used after the sweeps
#pragma unroll
    for (int r = 0; r < 10; ++r) Yb[r] = dp[D.d_inertia + 10 * bi + r];
    int anc[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) anc[r] = (r < D.nrounds) ? ip[D.i_anc + r * nb + bi] : -1;
    double R[9];
    V3 p, vJ = {0.0, 0.0, 0.0}, wJ = {0.0, 0.0, 0.0}; // joint placement in the parent, joint velocity in the joint's own axes
    V3 aJ = {0.0, 0.0, 0.0}, alJ = {0.0, 0.0, 0.0};   // ... and S_j a_j, likewise
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
            if (vel) {
                vJ = {(double)gv[0], (double)gv[1], (double)gv[2]};
                wJ = {(double)gv[3], (double)gv[4], (double)gv[5]};
            }
            if (acc) {
                aJ = {(double)ga[0], (double)ga[1], (double)ga[2]};
                alJ = {(double)ga[3], (double)ga[4], (double)ga[5]};
            }
        }
        else {
            const int a = (jt <= J_RZ) ? jt - J_RX : jt - J_PX;
            const double qj = (double)gq[iq], qd = vel ? (double)gv[iv] : 0.0, qdd = acc ? (double)ga[iv] : 0.0;
            const V3 e = {a == 0 ? qd : 0.0, a == 1 ? qd : 0.0, a == 2 ? qd : 0.0};
            const V3 ea = {a == 0 ? qdd : 0.0, a == 1 ? qdd : 0.0, a == 2 ? qdd : 0.0};
            if (jt <= J_RZ) {
                double sn, cs;
                sincos_joint(qj, &sn, &cs);
                // P.R * Rot(axis): the axis column stays, the other two mix
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double c0 = P[3 * r], c1 = P[3 * r + 1], c2 = P[3 * r + 2];
                    const double pa = (a == 0) ? c0 : (a == 1) ? c1 : c2;
                    const double pb = (a == 0) ? c1 : (a == 1) ? c2 : c0;
                    const double pd = (a == 0) ? c2 : (a == 1) ? c0 : c1;
                    const double nb_ = cs * pb + sn * pd, nd_ = cs * pd - sn * pb;
                    R[3 * r] = (a == 0) ? pa : (a == 1) ? nd_ : nb_;
                    R[3 * r + 1] = (a == 0) ? nb_ : (a == 1) ? pa : nd_;
                    R[3 * r + 2] = (a == 0) ? nd_ : (a == 1) ? nb_ : pa;
                }
                p = ld3(P + 9);
                wJ = e;
                alJ = ea;
            }
            else {
#pragma unroll
                for (int r = 0; r < 9; ++r) R[r] = P[r];
                const V3 ax = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
                p = ld3(P + 9) + qj * mv(P, ax);
                vJ = e;
                aJ = ea;
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
    // spatial velocity about the common origin, world-aligned: a path sum of the joints' own velocities
    V3 ov = {0.0, 0.0, 0.0}, ow = {0.0, 0.0, 0.0}, jv = ov, jw = ow;
    if (vel) {
        jw = mv(R, wJ);
        jv = mv(R, vJ) + cross(p, jw);
        ov = jv;
        ow = jw;
        rnea_path_sum(anc, D.nrounds, lane, ov, ow);
    }
    // spatial acceleration: a path sum of S_j a_j + v_j x S_j qd_j (motion cross product), then the root's acceleration -g on every body
    V3 oa = {0.0, 0.0, 0.0}, oal = {0.0, 0.0, 0.0};
    if (acc) {
        oal = mv(R, alJ);
        oa = mv(R, aJ) + cross(p, oal);
    }
    if (vel) {
        oa = oa + (cross(ow, jv) + cross(ov, jw));
        oal = oal + cross(ow, jw);
    }
    if (vel || acc) rnea_path_sum(anc, D.nrounds, lane, oa, oal);
    oa = oa - V3{D.g[0], D.g[1], D.g[2]};
    // ---- body force about the common origin: f = Y a + v x* (Y v), Y the body's inertia about the origin -----------------------------
    V3 fl, fa;
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
        const V3 hl = m * ov + cross(ow, hc);
        const V3 ha = symv(Io, ow) + cross(hc, ov);
        fl = m * oa + cross(oal, hc) + cross(ow, hl);
        fa = symv(Io, oal) + cross(hc, oa) + cross(ow, ha) + cross(ov, hl);
    }
    // ---- wrench frames: wave-uniform loop; the frame's body lane keeps the result ---------------------------------------------------------
    for (int k = 0; k < nf; ++k) {
        const int fb = D.frame_body[k]; // (checked on the host: in [0, nb))
        const double* Pf = D.frame_place + 12 * k;
        const V3 wl = {(double)gw[6 * k], (double)gw[6 * k + 1], (double)gw[6 * k + 2]};
        const V3 wa = {(double)gw[6 * k + 3], (double)gw[6 * k + 4], (double)gw[6 * k + 5]};
        // the frame's own axes -> its body's joint frame -> the common axes; the moment moves from the frame's origin to the common one
        const V3 F = mv(R, mv(Pf, wl));
        const V3 pf = mv(R, ld3(Pf + 9)) + p;
        const V3 N = mv(R, mv(Pf, wa)) + cross(pf, F);
        if (lane == fb) { fl = fl - F; fa = fa - N; }
    }
    // ---- subtree totals: inclusive prefix sums over the depth-first lanes, then scan[last] - scan[body - 1] ------------------------------
    double sc[6] = {fl.x, fl.y, fl.z, fa.x, fa.y, fa.z};
#pragma unroll
    for (int r = 0; r < 6; ++r) sc[r] = wave_scan_incl(body ? sc[r] : 0.0);
    // ---- lanes = dofs ---------------------------------------------------------------------------------------------------------------------
    double Fs[6], Rb[9];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double hi = __shfl(sc[r], lastj, kWave), lo = __shfl(sc[r], max(bj - 1, 0), kWave);
        Fs[r] = (bj > 0) ? hi - lo : hi;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Rb[k] = __shfl(R[k], bj, kWave);
    const V3 pb = {__shfl(p.x, bj, kWave), __shfl(p.y, bj, kWave), __shfl(p.z, bj, kWave)};
    {
        const int a = (jtypej == J_FREEFLYER) ? (kofj % 3) : (jtypej <= J_RZ) ? jtypej - J_RX : jtypej - J_PX;
        const bool ang = (jtypej == J_FREEFLYER) ? (kofj >= 3) : (jtypej <= J_RZ);
        const V3 wax = (a == 0) ? col(Rb, 0) : (a == 1) ? col(Rb, 1) : col(Rb, 2); // world direction of the axis
        const V3 Sw = ang ? wax : V3{0.0, 0.0, 0.0};
        const V3 Sv = ang ? cross(pb, wax) : wax;
        const double t = dot(Sv, V3{Fs[0], Fs[1], Fs[2]}) + dot(Sw, V3{Fs[3], Fs[4], Fs[5]});
        if (lane < nv) args.tau[(size_t)inst * nv + lane] = (TI)t;
    }
}

#endif // __HIPCC__
} // namespace wbcqp
