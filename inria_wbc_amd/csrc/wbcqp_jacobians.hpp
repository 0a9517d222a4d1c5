// wbcqp_jacobians.hpp -- where the robots' frames move for a given v: the Jacobians of chosen model frames, the CoM Jacobian, the centroidal momentum
// matrix and their drift terms from (q, v), for a whole fleet (wbcqp_jacobians).  What the reference's RobotModel::update(..., update_jacobians = true)
// fills one robot at a time (src/utils/robot_model.cpp:92-98, 115-126 there: computeJointJacobians, jacobianCenterOfMass, jacobian(name, reference_frame))
// and what its controller reads as momentumJacobian (controller.cpp:245, tsid's task-momentum-equality.cpp:151).
//
// Formulation: everything in the TRUE world frame (the base translation is kept, as in observe_kernel -- NOT rnea_kernel's base-centred frame), so a
// WORLD Jacobian is pinocchio's: the spatial Jacobian about the world's origin.  Five phases, one wavefront per instance:
//   1. lanes = bodies:  joint transform, placement down the tree by ancestor doubling and, with v, the spatial velocity and the bias acceleration
//                       (zero joint accelerations, no gravity) as path sums: observe_kernel's statements, as a copy
//   2. lanes = dofs:    lane j fetches its body's R, p by shuffle and forms its world column S_j = (v_j, w_j) about the world's origin: a revolute
//                       joint (w = axis, v = p x axis), a prismatic joint (v = axis) and the free-flyer's six columns (the base's own axes) each
//                       by their own rule
//   3. lanes = frames:  the selected frame's world placement R_f, p_f and, when asked for, its drift: the frame's classical acceleration
//                       a(p_f) + w x v(p_f) at zero joint accelerations (tsid's Jdot v), written from the frame's lane
//   4. a wave-uniform loop over the selected frames; lane j owns column j: S_j moved to the convention asked for where
//                       bodyof(j) <= frame_body <= last(bodyof(j)) (WORLD: as it is; LOCAL_WORLD_ALIGNED: shifted to p_f; LOCAL: shifted, then
//                       turned by R_f'), an exact +0.0 elsewhere.  Lane j writes J[f][r][j], r = 0..5: six stores of nv consecutive elements
//                       across the wave, coalesced as they are -- nothing is staged
//   5. Jcom / Ag / dAgv: the bodies' inertias about the world's origin (ten numbers: m, h = m c, I_o), composites folded leaf to root
//                       (fdyn_kernel's phase 1, as a copy: why not prefix sums is said there), F_j = Y_subtree(j) S_j; Ag[:, j] = F_j with its
//                       angular part taken about the CoM, Jcom[:, j] = Ag_lin[:, j] / m_total; dAgv = the bodies' bias forces f = Y a + v x* Y v
//                       summed over the wave in wave_sum's fixed order, the torque taken about the CoM
// Four instances per workgroup, nothing shared between the waves, no LDS: no barrier of any kind.  No atomics.  The result of an instance depends on
// its own (q, v) row alone -- the same bits at whatever index or batch size the row arrives.  An F32 handle converts at the loads and stores only.
#pragma once

#include "wbcqp_terms.hpp"

namespace wbcqp {

constexpr int kJacobianThreads = 256;
constexpr int kJacobianPerBlock = kJacobianThreads / kWave; // instances per workgroup
constexpr int kMaxJacobianFrames = 64;                      // one lane per selected frame
// wbcqp_reference_frame (include/wbcqp.h): pinocchio's values
constexpr int kRfWorld = 0, kRfLocal = 1, kRfLocalWorldAligned = 2;

// the tree's tables (a copy of the TermsDev fields this kernel reads) and the slot's Jacobian frames
struct JacobianDev {
    int nb, nq, nv, floating_base, nrounds;
    const int* ipool;
    const double* dpool;
    int i_jtype, i_last, i_idxq, i_idxv, i_anc; // [nb], [nb], [nb], [nb], [nrounds][nb]
    int i_bodyof, i_kof;                        // [nv] body of dof j, its place among the body's dofs
    int d_place, d_inertia;                     // [nb][12], [nb][10]
    int n_frames;
    const int* frame_body;                      // [n_frames] body of selected frame f
    const double* frame_place;                  // [n_frames][12] frame in its body's joint frame
};

template <typename TI>
struct JacobianArgs {
    JacobianDev D;
    const TI *q, *v;                  // [batch][nq], [batch][nv] (v: null when neither drift nor dAgv is asked for)
    TI *J, *Jcom, *Ag, *drift, *dAgv; // [batch][n_frames][6][nv], [batch][3][nv], [batch][6][nv], [batch][n_frames][6], [batch][6]; each may be null
    int rf, batch;                    // rf: kRfWorld / kRfLocal / kRfLocalWorldAligned
};

#ifdef __HIPCC__

template <typename TI>
__global__ __launch_bounds__(kJacobianThreads) void jacobian_kernel(const JacobianArgs<TI> args)
{
    const JacobianDev& D = args.D;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kJacobianPerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int nb = D.nb, nv = D.nv, nf = D.n_frames;
    const int* ip = D.ipool;
    const double* dp = D.dpool;
    const bool vel = args.v != nullptr; // wave-uniform: without v the velocity and acceleration sweeps are not run
    const TI* gq = args.q + (size_t)inst * D.nq;
    const TI* gv = vel ? args.v + (size_t)inst * nv : nullptr;

    // the constants of this lane's dof (two dependent reads): asked for here, they arrive behind the state
    const bool dof = lane < nv;
    const int cj = min(lane, nv - 1);
    const int bj = ip[D.i_bodyof + cj], kofj = ip[D.i_kof + cj];
    const int lastj = ip[D.i_last + bj], jtypej = ip[D.i_jtype + bj];

    // ---- phase 1, lanes = bodies: joint transform (lanes past the last body repeat it and count for nothing in the sums) ---------
    const bool body = lane < nb;
    const int bi = min(lane, nb - 1);
    const int jt = ip[D.i_jtype + bi];
    const int iq = ip[D.i_idxq + bi], iv = ip[D.i_idxv + bi];
    int anc[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) anc[r] = (r < D.nrounds) ? ip[D.i_anc + r * nb + bi] : -1;
    double R[9];
    V3 p, vJ = {0.0, 0.0, 0.0}, wJ = {0.0, 0.0, 0.0}; // joint placement in the parent, joint velocity in the joint's own axes
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
            p = {(double)gq[0], (double)gq[1], (double)gq[2]}; // the base where it IS: the world frame, not the base-centred one
            if (vel) {
                vJ = {(double)gv[0], (double)gv[1], (double)gv[2]};
                wJ = {(double)gv[3], (double)gv[4], (double)gv[5]};
            }
        }
        else {
            const int a = (jt <= J_RZ) ? jt - J_RX : jt - J_PX;
            const double qj = (double)gq[iq], qd = vel ? (double)gv[iv] : 0.0;
            const V3 e = {a == 0 ? qd : 0.0, a == 1 ? qd : 0.0, a == 2 ? qd : 0.0};
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
            }
            else {
#pragma unroll
                for (int r = 0; r < 9; ++r) R[r] = P[r];
                const V3 ax = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
                p = ld3(P + 9) + qj * mv(P, ax);
                vJ = e;
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
    // spatial velocity about the world's origin, world-aligned: a path sum of the joints' own velocities
    V3 ov = {0.0, 0.0, 0.0}, ow = {0.0, 0.0, 0.0};
    // bias acceleration (zero joint accelerations, no gravity): a = a_parent + v x vJ, a path sum as in the rows kernel (wbcqp_terms.hpp, phase 1)
    V3 oa = {0.0, 0.0, 0.0}, oal = {0.0, 0.0, 0.0};
    if (vel) {
        ow = mv(R, wJ);
        ov = mv(R, vJ) + cross(p, ow);
        const V3 jv = ov, jw = ow; // the joint's own velocity, world-aligned
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r < D.nrounds) {
                const int src = anc[r] >= 0 ? anc[r] : lane;
                const V3 a = {__shfl(ov.x, src, kWave), __shfl(ov.y, src, kWave), __shfl(ov.z, src, kWave)};
                const V3 b = {__shfl(ow.x, src, kWave), __shfl(ow.y, src, kWave), __shfl(ow.z, src, kWave)};
                if (anc[r] >= 0) { ov = ov + a; ow = ow + b; }
            }
        }
        oa = cross(ow, jv) + cross(ov, jw);
        oal = cross(ow, jw);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r < D.nrounds) {
                const int src = anc[r] >= 0 ? anc[r] : lane;
                const V3 a = {__shfl(oa.x, src, kWave), __shfl(oa.y, src, kWave), __shfl(oa.z, src, kWave)};
                const V3 b = {__shfl(oal.x, src, kWave), __shfl(oal.y, src, kWave), __shfl(oal.z, src, kWave)};
                if (anc[r] >= 0) { oa = oa + a; oal = oal + b; }
            }
        }
    }

    // ---- phase 2, lanes = dofs: the world column S_j = (Sv, Sw) about the world's origin ----------------------------------------------------------
    V3 Sv, Sw;
    {
        double Rb[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rb[k] = __shfl(R[k], bj, kWave);
        const V3 pb = {__shfl(p.x, bj, kWave), __shfl(p.y, bj, kWave), __shfl(p.z, bj, kWave)};
        const int a = (jtypej == J_FREEFLYER) ? (kofj % 3) : (jtypej <= J_RZ) ? jtypej - J_RX : jtypej - J_PX;
        const bool ang = (jtypej == J_FREEFLYER) ? (kofj >= 3) : (jtypej <= J_RZ);
        const V3 wax = (a == 0) ? col(Rb, 0) : (a == 1) ? col(Rb, 1) : col(Rb, 2); // world direction of the axis
        Sw = ang ? wax : V3{0.0, 0.0, 0.0};
        Sv = ang ? cross(pb, wax) : wax;
    }

    // ---- phases 3 and 4: the selected frames --------------------------------------------------------------------------------------------------------
    if (nf > 0 && (args.J || args.drift)) { // (wave-uniform; refused on the host with no frames selected)
        // lanes = frames: placement in the world
        const int fl = min(lane, nf - 1);
        const int fb = D.frame_body[fl]; // (checked on the host: in [0, nb))
        double Rf[9];
        V3 pf;
        {
            double place[12], Rb[9];
#pragma unroll
            for (int r = 0; r < 12; ++r) place[r] = D.frame_place[12 * fl + r];
            // the body's placement from the body's lane: every lane takes part in the exchange, the frames' lanes keep the result
#pragma unroll
            for (int k = 0; k < 9; ++k) Rb[k] = __shfl(R[k], fb, kWave);
            const V3 pb = {__shfl(p.x, fb, kWave), __shfl(p.y, fb, kWave), __shfl(p.z, fb, kWave)};
            mm(Rb, place, Rf);
            pf = mv(Rb, ld3(place + 9)) + pb;
        }
        if (args.drift) { // (refused on the host without v and with WORLD)
            const V3 bv = {__shfl(ov.x, fb, kWave), __shfl(ov.y, fb, kWave), __shfl(ov.z, fb, kWave)};
            const V3 bw = {__shfl(ow.x, fb, kWave), __shfl(ow.y, fb, kWave), __shfl(ow.z, fb, kWave)};
            const V3 ba = {__shfl(oa.x, fb, kWave), __shfl(oa.y, fb, kWave), __shfl(oa.z, fb, kWave)};
            const V3 bal = {__shfl(oal.x, fb, kWave), __shfl(oal.y, fb, kWave), __shfl(oal.z, fb, kWave)};
            // the spatial quantities moved to the frame's origin; classical = spatial + w x v there
            const V3 vP = bv + cross(bw, pf);
            V3 al = ba + cross(bal, pf) + cross(bw, vP), aw = bal;
            if (args.rf == kRfLocal) {
                al = mtv(Rf, al);
                aw = mtv(Rf, aw);
            }
            if (lane < nf) {
                TI* o = args.drift + ((size_t)inst * nf + lane) * 6;
                o[0] = (TI)al.x; o[1] = (TI)al.y; o[2] = (TI)al.z;
                o[3] = (TI)aw.x; o[4] = (TI)aw.y; o[5] = (TI)aw.z;
            }
        }
        if (args.J) {
            TI* gJ = args.J + (size_t)inst * nf * 6 * nv;
            for (int f = 0; f < nf; ++f) { // wave-uniform: the frame's numbers come from its lane, lane j keeps column j
                const int fbody = __builtin_amdgcn_readlane(fb, f);
                const bool sup = bj <= fbody && fbody <= lastj;
                V3 lin = Sv, ang = Sw;
                if (args.rf != kRfWorld) {
                    const V3 pff = {bcast_lane(pf.x, f), bcast_lane(pf.y, f), bcast_lane(pf.z, f)};
                    lin = Sv + cross(Sw, pff);
                    if (args.rf == kRfLocal) {
                        double Rff[9];
#pragma unroll
                        for (int k = 0; k < 9; ++k) Rff[k] = bcast_lane(Rf[k], f);
                        lin = mtv(Rff, lin);
                        ang = mtv(Rff, ang);
                    }
                }
                if (dof) { // unrelated branches: an exact zero, written as a zero
                    TI* o = gJ + (size_t)f * 6 * nv + lane;
                    o[0] = (TI)(sup ? lin.x : 0.0);
                    o[nv] = (TI)(sup ? lin.y : 0.0);
                    o[2 * nv] = (TI)(sup ? lin.z : 0.0);
                    o[3 * nv] = (TI)(sup ? ang.x : 0.0);
                    o[4 * nv] = (TI)(sup ? ang.y : 0.0);
                    o[5 * nv] = (TI)(sup ? ang.z : 0.0);
                }
            }
        }
    }

    // ---- phase 5: Jcom, Ag, dAgv ----------------------------------------------------------------------------------------------------------------------
    if (!args.Jcom && !args.Ag && !args.dAgv) return;
    // the body's inertia about the world's origin: m, h = m c, I_o
    double sc[10];
    {
        double Yb[10];
#pragma unroll
        for (int r = 0; r < 10; ++r) Yb[r] = dp[D.d_inertia + 10 * bi + r];
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
    // the bodies' bias forces about the world's origin, f = Y a + v x* (Y v), summed over the wave (before the fold: sc is still the body's own)
    V3 fls = {0.0, 0.0, 0.0}, fas = {0.0, 0.0, 0.0};
    if (args.dAgv) { // (refused on the host without v)
        const double m = sc[0];
        const V3 h = {sc[1], sc[2], sc[3]};
        const V3 hl = m * ov + cross(ow, h);
        const V3 ha = symv(sc + 4, ow) + cross(h, ov);
        const V3 fl = m * oa + cross(oal, h) + cross(ow, hl);
        const V3 fa = symv(sc + 4, oal) + cross(h, oa) + cross(ov, hl) + cross(ow, ha);
        fls = {wave_sum(body ? fl.x : 0.0), wave_sum(body ? fl.y : 0.0), wave_sum(body ? fl.z : 0.0)};
        fas = {wave_sum(body ? fa.x : 0.0), wave_sum(body ? fa.y : 0.0), wave_sum(body ? fa.z : 0.0)};
    }
    // ---- composites: every body folds its composite into its parent's, last body first.  The bodies are numbered depth-first with parents ahead
    //      of children, so whatever hangs under body i has been folded into it before its own turn (fdyn_kernel says why not prefix sums)
    for (int i = nb - 1; i > 0; --i) {
        const int par = __builtin_amdgcn_readlane(anc[0], i); // (anc[0]: the parent)
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const double t = bcast_lane(sc[r], i);
            if (lane == par) sc[r] += t;
        }
    }
    // the whole robot is the root's composite: total mass and centre of mass
    const double mt = bcast_lane(sc[0], 0);
    const V3 com = {bcast_lane(sc[1], 0) / mt, bcast_lane(sc[2], 0) / mt, bcast_lane(sc[3], 0) / mt};
    if (args.Jcom || args.Ag) {
        // lanes = dofs: F_j = Y_subtree(j) S_j, its angular part taken about the CoM
        double Ys[10];
#pragma unroll
        for (int r = 0; r < 10; ++r) Ys[r] = __shfl(sc[r], bj, kWave);
        const V3 h = {Ys[1], Ys[2], Ys[3]};
        const V3 Fl = Ys[0] * Sv + cross(Sw, h);
        const V3 Fo = symv(Ys + 4, Sw) + cross(h, Sv);
        const V3 Fa = Fo - cross(com, Fl);
        if (dof) {
            if (args.Ag) {
                TI* o = args.Ag + (size_t)inst * 6 * nv + lane;
                o[0] = (TI)Fl.x; o[nv] = (TI)Fl.y; o[2 * nv] = (TI)Fl.z;
                o[3 * nv] = (TI)Fa.x; o[4 * nv] = (TI)Fa.y; o[5 * nv] = (TI)Fa.z;
            }
            if (args.Jcom) {
                TI* o = args.Jcom + (size_t)inst * 3 * nv + lane;
                o[0] = (TI)(Fl.x / mt); o[nv] = (TI)(Fl.y / mt); o[2 * nv] = (TI)(Fl.z / mt);
            }
        }
    }
    if (args.dAgv) {
        const V3 fc = fas - cross(com, fls);
        if (lane < 6)
            args.dAgv[(size_t)inst * 6 + lane] =
                (TI)(lane == 0 ? fls.x : lane == 1 ? fls.y : lane == 2 ? fls.z : lane == 3 ? fc.x : lane == 4 ? fc.y : fc.z);
    }
}

#endif // __HIPCC__
} // namespace wbcqp
