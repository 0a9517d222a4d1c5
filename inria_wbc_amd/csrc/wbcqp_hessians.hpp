// wbcqp_hessians.hpp -- how the robots' frame Jacobians change: the kinematic Hessian H = dJ/dq of the frames of wbcqp_set_jacobian_frames and the
// Jacobian's time variation dJ = sum_k H[.., k] v_k from (q, v), for a whole fleet (wbcqp_kinematic_hessians).  What the reference's
// RobotModel::update(..., update_jacobians = true) fills with computeJointKinematicHessians and RobotModel::hessian(name, reference_frame) hands out
// one robot at a time (src/utils/robot_model.cpp:92-98, 128-135 there), and pinocchio's getFrameJacobianTimeVariation.
//
// The quantity.  J_j = (l_j, w_j) is column j of wbcqp_jacobians' J in the convention asked for, "k <= j" says that dof k's body is dof j's body or
// one of its ancestors (two dofs of the free-flyer are each <= the other), x_m is the motion cross product
// (l1, w1) x_m (l2, w2) = (w1 x l2 + l1 x w2, w1 x w2).  H[f][r][j][k] = d J[f][r][j] / d q_k along dof k in the tangent space (the library's SE(3)
// integration) is, where both j and k move the frame's body,
//     WORLD                 k <= j: J_k x_m J_j                  otherwise: +0.0
//     LOCAL                 k <= j: +0.0                         otherwise: J_j x_m J_k
//     LOCAL_WORLD_ALIGNED   k <= j: (w_k x l_j, w_k x w_j)       otherwise: (w_j x l_k, +0.0)
// and +0.0 everywhere else; every +0.0 is written as a zero, never left to a cross product that cancels (k = j included).  So are the free-flyer's
// TWINS, its translation and its rotation along one axis e of the base (dofs i and i + 3): both columns are made of the one vector R e, the product is
// that vector's with itself (WORLD: all six rows, either order; LOCAL_WORLD_ALIGNED: the linear rows of j the translation, k the rotation) -- the
// base's axis does not move when the base turns about it.  The dofs that move a
// frame lie on one chain, so among them k <= j is bodyof(k) <= bodyof(j) (bodies are numbered with parents ahead of children).
// dJ comes in O(1) per column from the bodies' spatial velocities V (world axes, about the world's origin), with D_j = V(frame's body) - V(bodyof(j))
// the motion of what lies between dof j's body and the frame:
//     WORLD                 V(bodyof(j)) x_m S_j
//     LOCAL                 S_j x_m D_j, carried to the frame
//     LOCAL_WORLD_ALIGNED   (w(bodyof(j)) x l_j + w_j x (D_j's velocity at the frame's origin), w(bodyof(j)) x w_j)
// H is never contracted, and never formed for a call that asks for dJ alone.
//
// Phases, one wavefront per instance:
//   1. lanes = bodies:  joint transform, placement down the tree by ancestor doubling and, with v, the spatial velocity as a path sum
//   2. lanes = dofs:    lane j's world column S_j = (v_j, w_j) about the world's origin
//   3. lanes = frames:  the selected frame's world placement R_f, p_f
//                       -- jacobian_kernel's phases 1 to 3 (csrc/wbcqp_jacobians.hpp), as a copy, without the bias acceleration
//   4. a wave-uniform loop over the selected frames: lane j forms column j in the convention asked for (jacobian_kernel's phase 4) and, for dJ,
//                       its six numbers, stored as J's are: six stores of nv consecutive elements across the wave
//   5. inside it, for H, a wave-uniform loop over the columns j: column j is broadcast with readlane (it lives in scalar registers), the fastest
//                       index k lies across the lanes, and a row H[f][r][j][0 .. nv) is one contiguous store across the wave.  A column j that does
//                       not move the frame is six rows of zeros, stored as zeros: every element of H is written.  The stores are the cost (6 nv^2
//                       numbers per frame), in one of two shapes (the template parameter Wide): one k per lane, or two consecutive k per lane in one
//                       store of twice the width where nv is even and H is aligned to it (profiles/hessians/INDEX.md has both, measured).
// Four instances per workgroup, nothing shared between the waves, no LDS: no barrier of any kind.  No atomics, every sum in a fixed order.  The
// result of an instance depends on its own (q, v) row alone -- the same bits at whatever index or batch size the row arrives.  An F32 handle
// converts at the loads and stores only.  Every output offset is computed in 64 bits.
#pragma once

#include "wbcqp_jacobians.hpp"

namespace wbcqp {

constexpr int kHessianThreads = 256;
constexpr int kHessianPerBlock = kHessianThreads / kWave; // instances per workgroup

template <typename TI>
struct HessianArgs {
    JacobianDev D;     // the tree's tables and the slot's Jacobian frames (n_frames > 0: checked on the host)
    const TI *q, *v;   // [batch][nq], [batch][nv] (v: null when dJ is not asked for)
    TI *H, *dJ;        // [batch][n_frames][6][nv][nv], [batch][n_frames][6][nv]; each may be null
    int rf, batch;     // rf: kRfWorld / kRfLocal / kRfLocalWorldAligned
};

// two consecutive elements of a row, stored at once
template <typename TI>
struct alignas(2 * sizeof(TI)) HessianPair {
    TI a, b;
};

#ifdef __HIPCC__

// H[.][0..6)[j][k] from column k = (lk, wk) and column j = (lj, wj) in the convention rf.  both: j and k move the frame's body; pre: k <= j;
// diag: k == j; twin: k != j, the free-flyer's translation and rotation along one axis.  Whatever the table of this file's head has as +0.0 comes
// out as a written zero
__device__ __forceinline__ void hessian_entry(int rf, bool both, bool pre, bool diag, bool twin, V3 lk, V3 wk, V3 lj, V3 wj, double* o)
{
    // LOCAL, and LOCAL_WORLD_ALIGNED under j: column j acts on column k; otherwise column k on column j
    const bool swap = rf == kRfLocal || (rf == kRfLocalWorldAligned && !pre);
    const V3 aw = swap ? wj : wk, al = swap ? lj : lk, bl = swap ? lk : lj, bw = swap ? wk : wj;
    V3 lin = cross(aw, bl);
    const V3 ang = cross(aw, bw);
    if (rf != kRfLocalWorldAligned) lin = lin + cross(al, bw);
    const bool above = pre && !diag && !twin;
    const bool nzl = both && (rf == kRfWorld ? above : rf == kRfLocal ? !pre : !twin);
    const bool nza = both && (rf == kRfLocal ? !pre : above);
    o[0] = nzl ? lin.x : 0.0; o[1] = nzl ? lin.y : 0.0; o[2] = nzl ? lin.z : 0.0;
    o[3] = nza ? ang.x : 0.0; o[4] = nza ? ang.y : 0.0; o[5] = nza ? ang.z : 0.0;
}

// Two different dofs of one body are the free-flyer's (every other joint has one): twins where they lie three apart, v = (linear, angular)
__device__ __forceinline__ bool hessian_twin(int bk, int bj, int k, int j)
{
    return bk == bj && (k - j == 3 || j - k == 3);
}

// Wide: H's stores.  false (what every call gets by itself: the faster one, profiles/hessians/INDEX.md): one k per lane.  true: two consecutive k
// per lane -- the host launches it only with nv even and H aligned to two elements.  Two instantiations, so that neither pays for the other's registers
template <typename TI, bool Wide = false>
__global__ __launch_bounds__(kHessianThreads) void hessian_kernel(const HessianArgs<TI> args)
{
    const JacobianDev& D = args.D;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kHessianPerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int nb = D.nb, nv = D.nv, nf = D.n_frames;
    const int* ip = D.ipool;
    const double* dp = D.dpool;
    const bool vel = args.v != nullptr; // wave-uniform: without v the velocity sweep is not run
    const TI* gq = args.q + (size_t)inst * D.nq;
    const TI* gv = vel ? args.v + (size_t)inst * nv : nullptr;

    // the constants of this lane's dof (two dependent reads): asked for here, they arrive behind the state
    const bool dof = lane < nv;
    const int cj = min(lane, nv - 1);
    const int bj = ip[D.i_bodyof + cj], kofj = ip[D.i_kof + cj];
    const int lastj = ip[D.i_last + bj], jtypej = ip[D.i_jtype + bj];

    // ---- phase 1, lanes = bodies: joint transform (lanes past the last body repeat it and count for nothing) ---------------------
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
    if (vel) {
        ow = mv(R, wJ);
        ov = mv(R, vJ) + cross(p, ow);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r < D.nrounds) {
                const int src = anc[r] >= 0 ? anc[r] : lane;
                const V3 a = {__shfl(ov.x, src, kWave), __shfl(ov.y, src, kWave), __shfl(ov.z, src, kWave)};
                const V3 b = {__shfl(ow.x, src, kWave), __shfl(ow.y, src, kWave), __shfl(ow.z, src, kWave)};
                if (anc[r] >= 0) { ov = ov + a; ow = ow + b; }
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
    // the spatial velocity of this lane's dof's body: everything up the chain to and with dof j
    const V3 bvj = {__shfl(ov.x, bj, kWave), __shfl(ov.y, bj, kWave), __shfl(ov.z, bj, kWave)};
    const V3 bwj = {__shfl(ow.x, bj, kWave), __shfl(ow.y, bj, kWave), __shfl(ow.z, bj, kWave)};

    // ---- phase 3, lanes = frames: placement in the world ------------------------------------------------------------------------------------------
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

    // ---- phases 4 and 5: the selected frames ------------------------------------------------------------------------------------------------------
    const int rf = args.rf;
    const size_t nvs = (size_t)nv;
    for (int f = 0; f < nf; ++f) { // wave-uniform: the frame's numbers come from its lane, lane j keeps column j
        const int fbody = __builtin_amdgcn_readlane(fb, f);
        const bool sup = dof && bj <= fbody && fbody <= lastj;
        const V3 pff = {bcast_lane(pf.x, f), bcast_lane(pf.y, f), bcast_lane(pf.z, f)};
        double Rff[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rff[k] = bcast_lane(Rf[k], f);
        V3 lin = Sv, ang = Sw; // column j in the convention asked for
        if (rf != kRfWorld) {
            lin = Sv + cross(Sw, pff);
            if (rf == kRfLocal) {
                lin = mtv(Rff, lin);
                ang = mtv(Rff, ang);
            }
        }
        if (args.dJ) { // (refused on the host without v)
            const V3 fv = {bcast_lane(ov.x, fbody), bcast_lane(ov.y, fbody), bcast_lane(ov.z, fbody)};
            const V3 fw = {bcast_lane(ow.x, fbody), bcast_lane(ow.y, fbody), bcast_lane(ow.z, fbody)};
            const V3 Dl = fv - bvj, Dw = fw - bwj; // what moves between dof j's body and the frame
            V3 xl, xw;
            if (rf == kRfWorld) {
                xl = cross(bwj, Sv) + cross(bvj, Sw);
                xw = cross(bwj, Sw);
            }
            else if (rf == kRfLocalWorldAligned) {
                xl = cross(bwj, lin) + cross(ang, Dl + cross(Dw, pff));
                xw = cross(bwj, ang);
            }
            else {
                const V3 yl = cross(Sw, Dl) + cross(Sv, Dw), yw = cross(Sw, Dw);
                xl = mtv(Rff, yl + cross(yw, pff));
                xw = mtv(Rff, yw);
            }
            if (dof) { // dofs that do not move the frame: an exact zero, written as a zero
                TI* o = args.dJ + ((size_t)inst * nf + f) * 6 * nvs + lane;
                o[0] = (TI)(sup ? xl.x : 0.0);
                o[nvs] = (TI)(sup ? xl.y : 0.0);
                o[2 * nvs] = (TI)(sup ? xl.z : 0.0);
                o[3 * nvs] = (TI)(sup ? xw.x : 0.0);
                o[4 * nvs] = (TI)(sup ? xw.y : 0.0);
                o[5 * nvs] = (TI)(sup ? xw.z : 0.0);
            }
        }
        if (!args.H) continue;
        TI* gH = args.H + ((size_t)inst * nf + f) * 6 * nvs * nvs; // this frame's [6][nv][nv]
        const size_t plane = nvs * nvs;
        const int supi = sup ? 1 : 0;
        if constexpr (!Wide) {
            for (int j = 0; j < nv; ++j) { // wave-uniform: column j in scalar registers, k = lane
                TI* o = gH + (size_t)j * nvs + lane;
                double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (__builtin_amdgcn_readlane(supi, j)) { // (wave-uniform; a column that does not move the frame: six rows of zeros)
                    const int bjj = __builtin_amdgcn_readlane(bj, j);
                    const V3 lj = {bcast_lane(lin.x, j), bcast_lane(lin.y, j), bcast_lane(lin.z, j)};
                    const V3 wj = {bcast_lane(ang.x, j), bcast_lane(ang.y, j), bcast_lane(ang.z, j)};
                    hessian_entry(rf, sup, bj <= bjj, lane == j, hessian_twin(bj, bjj, lane, j), lin, ang, lj, wj, e);
                }
                if (dof) {
#pragma unroll
                    for (int r = 0; r < 6; ++r) o[(size_t)r * plane] = (TI)e[r];
                }
            }
        }
        else {
            // lane L holds the columns k = 2L and 2L + 1 (nv is even; the lanes from nv / 2 on hold nothing that is stored)
            const int k0 = 2 * lane, k1 = 2 * lane + 1;
            const bool pairl = k1 < nv;
            const int sup0 = __shfl(supi, k0, kWave), sup1 = __shfl(supi, k1, kWave);
            const int b0 = __shfl(bj, k0, kWave), b1 = __shfl(bj, k1, kWave);
            const V3 l0 = {__shfl(lin.x, k0, kWave), __shfl(lin.y, k0, kWave), __shfl(lin.z, k0, kWave)};
            const V3 w0 = {__shfl(ang.x, k0, kWave), __shfl(ang.y, k0, kWave), __shfl(ang.z, k0, kWave)};
            const V3 l1 = {__shfl(lin.x, k1, kWave), __shfl(lin.y, k1, kWave), __shfl(lin.z, k1, kWave)};
            const V3 w1 = {__shfl(ang.x, k1, kWave), __shfl(ang.y, k1, kWave), __shfl(ang.z, k1, kWave)};
            for (int j = 0; j < nv; ++j) { // wave-uniform
                HessianPair<TI>* o = reinterpret_cast<HessianPair<TI>*>(gH + (size_t)j * nvs + k0);
                double e0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, e1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (__builtin_amdgcn_readlane(supi, j)) {
                    const int bjj = __builtin_amdgcn_readlane(bj, j);
                    const V3 lj = {bcast_lane(lin.x, j), bcast_lane(lin.y, j), bcast_lane(lin.z, j)};
                    const V3 wj = {bcast_lane(ang.x, j), bcast_lane(ang.y, j), bcast_lane(ang.z, j)};
                    hessian_entry(rf, pairl && sup0, b0 <= bjj, k0 == j, hessian_twin(b0, bjj, k0, j), l0, w0, lj, wj, e0);
                    hessian_entry(rf, pairl && sup1, b1 <= bjj, k1 == j, hessian_twin(b1, bjj, k1, j), l1, w1, lj, wj, e1);
                }
                if (pairl) {
#pragma unroll
                    for (int r = 0; r < 6; ++r) o[(size_t)r * (plane / 2)] = HessianPair<TI>{(TI)e0[r], (TI)e1[r]};
                }
            }
        }
    }
}

#endif // __HIPCC__
} // namespace wbcqp
