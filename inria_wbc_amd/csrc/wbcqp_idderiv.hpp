// wbcqp_idderiv.hpp -- how the joint torques of a motion change with the state, for a whole fleet (wbcqp_inverse_dynamics_derivatives):
//     dtau/dq and dtau/dv of   tau = M(q) a + nle(q, v) - sum_k J_k(q)' w_k
// pinocchio's computeRNEADerivatives.  dtau/dq is taken along each dof in the tangent space of wbcqp_integrate's SE(3) integration (the
// convention of wbcqp_kinematic_hessians); the wrenches stay fixed in their frames' own axes.  dtau/da is M (wbcqp_mass_matrix).
//
// Formulation: rnea_kernel's -- ONE frame, world-aligned with its origin at the floating base; q[0..2] is never read.  Motion vectors X = (l, w),
// forces F = (f, n), X . F = l . f + w . n,
//     X x_m Y = (w_X x l_Y + l_X x w_Y, w_X x w_Y),    X x_f F = (w x f, w x n + l x f),    (X x_m Y) . F = -Y . (X x_f F).
// Per body b, as rnea_kernel forms them: the velocity V_b, the acceleration A_b (-g on its linear part), the inertia about the origin
// Y_b = (m, h = m c, I_o), the momentum Y_b V_b = (hl, ha), the body force f_b (wrenches subtracted) and the symmetric
//     D_b = [w]x I_o - I_o [w]x - [l]x [h]x - [h]x [l]x,   (l, w) = V_b.
// Composites over the subtree of c: Y^c (10 numbers), H^c = sum Y_b V_b (6), D^c (6), F^c = sum f_b (6); with hl the linear part of H^c,
//     N^c U := (-hl x U_w, hl x U_l + D^c U_w)
// is all of sum_b (V_b x_f Y_b - Y_b V_b x_m): the symmetric 6 x 6 matrix [[0, -[hl]x], [[hl]x, D]].  28 numbers per body are folded.
// Per dof j with column S_j, body beta, parent body lambda (at the root V_lambda = 0, A_lambda = (-g, 0)):
//     U_j = S_j x_m V_lambda,   W_j = S_j x_m A_lambda - U_j x_m V_lambda,   Z_j = S_j x_m (V_lambda + V_beta).
// For dofs i, j whose bodies lie on one path (two dofs of the free-flyer do), c the deeper of the two bodies:
//     dtau_i/dq_j = S_i . (-Y^c W_j - N^c U_j - U_j x_f H^c)  +  [body(i) a STRICT ancestor of beta]  S_i . (S_j x_f F^beta)
//     dtau_i/dv_j = S_i . ( N^c S_j + S_j x_f H^c - Y^c Z_j)
// and +0.0 everywhere else; columns 0..2 of dtau/dq on a floating base are +0.0 too (nothing depends on where the base is).
//
//   lanes = bodies:  rnea_kernel's joint transform, placement, velocity and acceleration sweeps, body inertia about the origin, body force and
//                    wrench loop, statement for statement, as a copy (a function shared with an existing kernel changes that
//                    kernel's register allocation); D_b beside them
//   composites:      every body adds its 28 numbers to its parent's, last body first, as fdyn_kernel folds its ten (a serial wave-uniform loop
//                    over readlane broadcasts): a sum only ever holds a subtree, so a gripper link's entries keep their digits
//   lanes = dofs:    lane j forms S_j, U_j, W_j, Z_j and, from its own body's composites, the two bracketed 6-vectors above, S_j x_f F^beta,
//                    P_j = Y^beta S_j and E_j = N^beta S_j - S_j x_f H^beta
//   rows:            a wave-uniform loop over i broadcasts S_i, P_i, E_i by readlane; lane j writes entry [i][j] of each matrix asked for.
//                    body(i) is beta or above it: S_i . (the lane's own vectors).  beta strictly above body(i): -P_i . W_j - E_i . U_j for q,
//                    E_i . S_j - P_i . Z_j for v (the pairing identity).  Otherwise a written +0.0.  Every row is one contiguous store.
// One wavefront per instance, four instances per workgroup, no LDS, no workgroup barrier, no atomics; every sum runs in a fixed order and an
// instance's bits depend on its own rows alone.  F32 handles read float, compute in double, write float.  Offsets are 64-bit.
#pragma once

#include "wbcqp_rnea.hpp"

namespace wbcqp {

constexpr int kIdDerivThreads = 256;
constexpr int kIdDerivPerBlock = kIdDerivThreads / kWave; // instances per workgroup

template <typename TI>
struct IdDerivArgs {
    RneaDev D;                    // the tree's tables and the slot's wrench frames (n_frames: 0 when the call has no wrench)
    const TI *q, *v, *a, *wrench; // [batch][nq]; [batch][nv] or null; rows lda apart or null; [batch][n_frames][6] or null
    TI *dtau_dq, *dtau_dv;        // [batch][nv][nv]; each may be null
    int lda, batch;
};

#ifdef __HIPCC__

// a motion or a force vector: the linear part, the angular part
struct Sp6 {
    V3 l, w;
};
__device__ __forceinline__ double idd_dot(Sp6 a, Sp6 b) { return dot(a.l, b.l) + dot(a.w, b.w); }
__device__ __forceinline__ Sp6 idd_xm(Sp6 x, Sp6 y) { return {cross(x.w, y.l) + cross(x.l, y.w), cross(x.w, y.w)}; }
__device__ __forceinline__ Sp6 idd_xf(Sp6 x, Sp6 f) { return {cross(x.w, f.l), cross(x.w, f.w) + cross(x.l, f.l)}; }
__device__ __forceinline__ Sp6 idd_sub(Sp6 a, Sp6 b) { return {a.l - b.l, a.w - b.w}; }
__device__ __forceinline__ Sp6 idd_add(Sp6 a, Sp6 b) { return {a.l + b.l, a.w + b.w}; }
// Y X for Y = (m, h, I_o about the origin: xx xy xz yy yz zz), ten numbers
__device__ __forceinline__ Sp6 idd_inertia(const double* Y, Sp6 x)
{
    const V3 h = {Y[1], Y[2], Y[3]};
    return {Y[0] * x.l + cross(x.w, h), symv(Y + 4, x.w) + cross(h, x.l)};
}
// N U = (-hl x U_w, hl x U_l + D U_w)
__device__ __forceinline__ Sp6 idd_n(V3 hl, const double* Dm, Sp6 u) { return {cross(u.w, hl), cross(hl, u.l) + symv(Dm, u.w)}; }
__device__ __forceinline__ Sp6 idd_bcast(Sp6 x, int i)
{
    return {{bcast_lane(x.l.x, i), bcast_lane(x.l.y, i), bcast_lane(x.l.z, i)}, {bcast_lane(x.w.x, i), bcast_lane(x.w.y, i), bcast_lane(x.w.z, i)}};
}
__device__ __forceinline__ V3 idd_shfl(V3 x, int src) { return {__shfl(x.x, src, kWave), __shfl(x.y, src, kWave), __shfl(x.z, src, kWave)}; }

template <typename TI>
__global__ __launch_bounds__(kIdDerivThreads) void id_derivatives_kernel(const IdDerivArgs<TI> args)
{
    const RneaDev& D = args.D;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kIdDerivPerBlock + wave;
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
    const bool dof = lane < nv;
    const int cj = min(lane, nv - 1);
    const int bj = ip[D.i_bodyof + cj], kofj = ip[D.i_kof + cj];
    const int lastj = ip[D.i_last + bj], jtypej = ip[D.i_jtype + bj];

    // ---- lanes = bodies: joint transform (lanes past the last body repeat it and count for nothing in the sums) -------------------
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
    // ---- per body about the common origin: Y = (m, h, I_o), the momentum Y V, D, and the force f = Y a + v x* (Y v) ---------------------
    //      sc: Y 0..9, H 10..15, D 16..21, F 22..27
    double sc[28];
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
        sc[0] = m; sc[1] = hc.x; sc[2] = hc.y; sc[3] = hc.z;
#pragma unroll
        for (int r = 0; r < 6; ++r) sc[4 + r] = Io[r];
        sc[10] = hl.x; sc[11] = hl.y; sc[12] = hl.z; sc[13] = ha.x; sc[14] = ha.y; sc[15] = ha.z;
        // D = [w]x I_o - I_o [w]x - (h l' + l h' - 2 (l . h) 1), with [l]x [h]x = h l' - (l . h) 1: column j of [w]x I_o is w x (column j of I_o)
        const V3 i0 = {Io[0], Io[1], Io[2]}, i1 = {Io[1], Io[3], Io[4]}, i2 = {Io[2], Io[4], Io[5]};
        const V3 c0 = cross(ow, i0), c1 = cross(ow, i1), c2_ = cross(ow, i2); // columns of [w]x I_o; its transpose is -I_o [w]x
        const double lh = dot(ov, hc);
        sc[16] = (c0.x + c0.x) - (hc.x * ov.x + ov.x * hc.x - 2 * lh);
        sc[17] = (c1.x + c0.y) - (hc.x * ov.y + ov.x * hc.y);
        sc[18] = (c2_.x + c0.z) - (hc.x * ov.z + ov.x * hc.z);
        sc[19] = (c1.y + c1.y) - (hc.y * ov.y + ov.y * hc.y - 2 * lh);
        sc[20] = (c2_.y + c1.z) - (hc.y * ov.z + ov.y * hc.z);
        sc[21] = (c2_.z + c2_.z) - (hc.z * ov.z + ov.z * hc.z - 2 * lh);
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
    sc[22] = fl.x; sc[23] = fl.y; sc[24] = fl.z; sc[25] = fa.x; sc[26] = fa.y; sc[27] = fa.z;
    // ---- composites: every body folds its composite into its parent's, last body first (fdyn_kernel's loop and its reason: a sum only ever
    //      holds a subtree).  Without v the momentum and D are zeros throughout and are not folded ------------------------------------------
    for (int i = nb - 1; i > 0; --i) {
        const int par = __builtin_amdgcn_readlane(anc[0], i); // (anc[0]: the parent)
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const double t = bcast_lane(sc[r], i);
            if (lane == par) sc[r] += t;
        }
        if (vel) {
#pragma unroll
            for (int r = 10; r < 22; ++r) {
                const double t = bcast_lane(sc[r], i);
                if (lane == par) sc[r] += t;
            }
        }
#pragma unroll
        for (int r = 22; r < 28; ++r) {
            const double t = bcast_lane(sc[r], i);
            if (lane == par) sc[r] += t;
        }
    }
    // ---- lanes = dofs: the lane's column, its body's composites, the parent's and the body's motion ------------------------------------------
    const int parj = __shfl(anc[0], bj, kWave);
    const bool rootj = parj < 0;
    const int srcp = rootj ? bj : parj;
    double Ys[10], Dc[6], Rb[9];
#pragma unroll
    for (int r = 0; r < 10; ++r) Ys[r] = __shfl(sc[r], bj, kWave);
    const Sp6 Hc = {{__shfl(sc[10], bj, kWave), __shfl(sc[11], bj, kWave), __shfl(sc[12], bj, kWave)},
                    {__shfl(sc[13], bj, kWave), __shfl(sc[14], bj, kWave), __shfl(sc[15], bj, kWave)}};
#pragma unroll
    for (int r = 0; r < 6; ++r) Dc[r] = __shfl(sc[16 + r], bj, kWave);
    const Sp6 Fc = {{__shfl(sc[22], bj, kWave), __shfl(sc[23], bj, kWave), __shfl(sc[24], bj, kWave)},
                    {__shfl(sc[25], bj, kWave), __shfl(sc[26], bj, kWave), __shfl(sc[27], bj, kWave)}};
#pragma unroll
    for (int k = 0; k < 9; ++k) Rb[k] = __shfl(R[k], bj, kWave);
    const V3 pb = idd_shfl(p, bj);
    const Sp6 Vb = {idd_shfl(ov, bj), idd_shfl(ow, bj)};
    Sp6 Vl = {idd_shfl(ov, srcp), idd_shfl(ow, srcp)}, Al = {idd_shfl(oa, srcp), idd_shfl(oal, srcp)};
    if (rootj) {
        Vl = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        Al = {V3{0.0, 0.0, 0.0} - V3{D.g[0], D.g[1], D.g[2]}, {0.0, 0.0, 0.0}};
    }
    Sp6 S, U, W, Z, Gq, Gv, T, P, E;
    {
        const int a = (jtypej == J_FREEFLYER) ? (kofj % 3) : (jtypej <= J_RZ) ? jtypej - J_RX : jtypej - J_PX;
        const bool ang = (jtypej == J_FREEFLYER) ? (kofj >= 3) : (jtypej <= J_RZ);
        const V3 wax = (a == 0) ? col(Rb, 0) : (a == 1) ? col(Rb, 1) : col(Rb, 2); // world direction of the axis
        S.w = ang ? wax : V3{0.0, 0.0, 0.0};
        S.l = ang ? cross(pb, wax) : wax;
        U = idd_xm(S, Vl);
        W = idd_sub(idd_xm(S, Al), idd_xm(U, Vl));
        Z = idd_xm(S, idd_add(Vl, Vb));
        const Sp6 NS = idd_n(Hc.l, Dc, S), SH = idd_xf(S, Hc);
        P = idd_inertia(Ys, S);
        E = idd_sub(NS, SH);
        Gv = idd_sub(idd_add(NS, SH), idd_inertia(Ys, Z));
        const Sp6 YW = idd_inertia(Ys, W), NU = idd_n(Hc.l, Dc, U), UH = idd_xf(U, Hc);
        Gq = {V3{0.0, 0.0, 0.0} - YW.l - NU.l - UH.l, V3{0.0, 0.0, 0.0} - YW.w - NU.w - UH.w};
        T = idd_xf(S, Fc);
    }
    // ---- rows: a wave-uniform loop over i; lane j writes entry [i][j] of each matrix asked for ---------------------------------------------
    const bool base_col = D.floating_base && lane < 3; // nothing depends on where the base is
    TI* gdq = args.dtau_dq ? args.dtau_dq + (size_t)inst * nv * nv : nullptr;
    TI* gdv = args.dtau_dv ? args.dtau_dv + (size_t)inst * nv * nv : nullptr;
    for (int i = 0; i < nv; ++i) {
        const Sp6 Si = idd_bcast(S, i), Pi = idd_bcast(P, i), Ei = idd_bcast(E, i);
        const int bodyi = __builtin_amdgcn_readlane(bj, i), lasti = __builtin_amdgcn_readlane(lastj, i);
        const bool up = bodyi <= bj && bj <= lasti;   // body(i) is the lane's body or above it
        const bool down = bj < bodyi && bodyi <= lastj; // the lane's body is strictly above body(i)
        if (gdq) {
            const double own = idd_dot(Si, Gq) + ((bodyi != bj) ? idd_dot(Si, T) : 0.0);
            const double under = -idd_dot(Pi, W) - idd_dot(Ei, U);
            const double x = (base_col || !(up || down)) ? 0.0 : up ? own : under; // unrelated branches: an exact zero, written as a zero
            if (dof) gdq[(size_t)i * nv + lane] = (TI)x;
        }
        if (gdv) {
            const double own = idd_dot(Si, Gv);
            const double under = idd_dot(Ei, S) - idd_dot(Pi, Z);
            const double x = !(up || down) ? 0.0 : up ? own : under;
            if (dof) gdv[(size_t)i * nv + lane] = (TI)x;
        }
    }
}

#endif // __HIPCC__
} // namespace wbcqp
