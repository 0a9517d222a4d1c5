// wbcqp_observe.hpp -- where the robots are: centre of mass and world placements / velocities of chosen model frames from (q, v), for a
// whole fleet (wbcqp_observe).  What the reference's controller exposes one robot at a time as com() and model_frame_pos(name)
// (include/inria_wbc/controllers/controller.hpp:110,141-146 there) and its drivers log every tick beside the task costs.
//
// Formulation: phase 1 of the rows kernel (wbcqp_terms.hpp, wave 0) in the TRUE world frame -- the base translation is kept, so a
// placement comes out as pinocchio's oMf and a body's velocity as its spatial velocity about the world's origin:
//   lanes = bodies:  joint transform from q (sincos_joint, the free-flyer's quaternion); placement, then velocity, down the tree by
//                    nrounds rounds of ancestor doubling over ds_bpermute (the i_anc table wbcqp_set_model uploads);
//                    m (p + R c) and m (v + w x (p + R c)) summed over the wave in a fixed order (wave_sum: no atomics)
//   lanes = frames:  the lane of observed frame f fetches its body's R, p, v, w from the body's lane (18 doubles over ds_bpermute) and
//                    forms the frame's placement and its velocity in its own axes (frame_kin)
//   lanes = output elements: the frames' 12 + 6 numbers go through a wave-private piece of LDS, so that the [n_frames][12] and
//                    [n_frames][6] blocks of an instance leave as consecutive elements of consecutive lanes
// One wavefront per instance, four instances per workgroup, nothing shared between the waves: no workgroup barrier.  The result of an
// instance depends on its own (q, v) row alone -- the same bits at whatever index or batch size the row arrives.
#pragma once

#include "wbcqp_terms.hpp"

namespace wbcqp {

constexpr int kObserveThreads = 256;
constexpr int kObservePerBlock = kObserveThreads / kWave; // instances per workgroup
constexpr int kObsPlaceStride = 13; // LDS doubles per frame: R (9) p (3), odd stride
constexpr int kObsVelStride = 7;    // ... linear (3) angular (3), odd stride

// the tree's tables (a copy of the TermsDev fields this kernel reads) and the slot's observed frames
struct ObserveDev {
    int nb, nq, nv, floating_base, nrounds;
    const int* ipool;
    const double* dpool;
    int i_jtype, i_idxq, i_idxv, i_anc; // [nb], [nb], [nb], [nrounds][nb]
    int d_place, d_inertia;             // [nb][12], [nb][10]
    int n_frames;
    const int* frame_body;              // [n_frames] body of observed frame f
    const double* frame_place;          // [n_frames][12] frame in its body's joint frame
};

template <typename TI>
struct ObserveArgs {
    ObserveDev D;
    const TI *q, *v;                       // [batch][nq], [batch][nv] (v: null when no velocity is asked for)
    TI *com, *vcom, *placement, *velocity; // [batch][3], [batch][3], [batch][n_frames][12], [batch][n_frames][6]; each may be null
    int batch;
    TI* acom;                              // [batch][3] or null: the CoM's acceleration with zero joint accelerations and no gravity
};

// dynamic LDS of one workgroup: every wave stages its instance's frames
inline int observe_lds_bytes(int n_frames) { return kObservePerBlock * n_frames * (kObsPlaceStride + kObsVelStride) * 8; }

#ifdef __HIPCC__

template <typename TI>
__global__ __launch_bounds__(kObserveThreads) void observe_kernel(const ObserveArgs<TI> args)
{
    extern __shared__ double obs_lds[];
    const ObserveDev& D = args.D;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kObservePerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int nb = D.nb, nf = D.n_frames;
    const int* ip = D.ipool;
    const double* dp = D.dpool;
    const bool vel = args.v != nullptr; // wave-uniform: without v the velocity sweep is not run
    const TI* gq = args.q + (size_t)inst * D.nq;
    const TI* gv = vel ? args.v + (size_t)inst * D.nv : nullptr;

    // ---- lanes = bodies: joint transform (lanes past the last body repeat it and count for nothing in the sums) -------------------
    const bool body = lane < nb;
    const int bi = min(lane, nb - 1);
    const int jt = ip[D.i_jtype + bi];
    const int iq = ip[D.i_idxq + bi], iv = ip[D.i_idxv + bi];
    const double mass_b = dp[D.d_inertia + 10 * bi];
    const V3 c_b = ld3(dp + D.d_inertia + 10 * bi + 1);
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
    V3 jv = ov, jw = ow; // the joint's own velocity, world-aligned
    if (vel) {
        ow = mv(R, wJ);
        ov = mv(R, vJ) + cross(p, ow);
        jv = ov;
        jw = ow;
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
    // bias acceleration (zero joint accelerations, no gravity): a = a_parent + v x vJ, a path sum as in the rows kernel (wbcqp_terms.hpp, phase 1)
    V3 oa = {0.0, 0.0, 0.0}, oal = {0.0, 0.0, 0.0};
    if (args.acom) { // wave-uniform; refused on the host without v
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
    // ---- centre of mass, its velocity and its bias acceleration: sums over the bodies in wave_sum's fixed order ------------------
    if (args.com || args.vcom || args.acom) {
        const double m = body ? mass_b : 0.0;
        const V3 hc = m * (mv(R, c_b) + p);
        const double mt = wave_sum(m);
        const double imass = 1.0 / mt;
        if (args.com) {
            const V3 s = {wave_sum(hc.x), wave_sum(hc.y), wave_sum(hc.z)};
            if (lane < 3) args.com[(size_t)inst * 3 + lane] = (TI)(imass * (lane == 0 ? s.x : lane == 1 ? s.y : s.z));
        }
        if (args.vcom) { // (refused on the host without v)
            const V3 hl = m * ov + cross(ow, hc);
            const V3 s = {wave_sum(hl.x), wave_sum(hl.y), wave_sum(hl.z)};
            if (lane < 3) args.vcom[(size_t)inst * 3 + lane] = (TI)(imass * (lane == 0 ? s.x : lane == 1 ? s.y : s.z));
        }
        if (args.acom) { // the bodies' bias forces' linear part, f = m a + al x h_c + w x h_l, over the total mass
            const V3 hl = m * ov + cross(ow, hc);
            const V3 fl = m * oa + cross(oal, hc) + cross(ow, hl);
            const V3 s = {wave_sum(fl.x), wave_sum(fl.y), wave_sum(fl.z)};
            if (lane < 3) args.acom[(size_t)inst * 3 + lane] = (TI)(imass * (lane == 0 ? s.x : lane == 1 ? s.y : s.z));
        }
    }
    // ---- lanes = observed frames ------------------------------------------------------------------------------------------------
    if (nf == 0 || (!args.placement && !args.velocity)) return;
    double* Pl = obs_lds + (size_t)wave * nf * (kObsPlaceStride + kObsVelStride);
    double* Vl = Pl + nf * kObsPlaceStride;
    {
        const int fl = min(lane, nf - 1);
        const int fb = D.frame_body[fl]; // (checked on the host: in [0, nb))
        double place[12];
#pragma unroll
        for (int r = 0; r < 12; ++r) place[r] = D.frame_place[12 * fl + r];
        // the body's kinematics from the body's lane: every lane takes part in the exchange, the frames' lanes keep the result
        double kb[kKinStride];
#pragma unroll
        for (int k = 0; k < 9; ++k) kb[k] = __shfl(R[k], fb, kWave);
        kb[9] = __shfl(p.x, fb, kWave); kb[10] = __shfl(p.y, fb, kWave); kb[11] = __shfl(p.z, fb, kWave);
        if (vel && args.velocity) {
            kb[12] = __shfl(ov.x, fb, kWave); kb[13] = __shfl(ov.y, fb, kWave); kb[14] = __shfl(ov.z, fb, kWave);
            kb[15] = __shfl(ow.x, fb, kWave); kb[16] = __shfl(ow.y, fb, kWave); kb[17] = __shfl(ow.z, fb, kWave);
        }
        else {
#pragma unroll
            for (int k = 12; k < 18; ++k) kb[k] = 0.0;
        }
#pragma unroll
        for (int k = 18; k < kKinStride; ++k) kb[k] = 0.0; // (no accelerations here: what frame_kin makes of them is not kept)
        FrameKin f;
        frame_kin(kb, place, f);
        if (lane < nf) {
            if (args.placement) {
                double* o = Pl + kObsPlaceStride * lane;
#pragma unroll
                for (int r = 0; r < 9; ++r) o[r] = f.R[r];
                st3(o + 9, f.p);
            }
            if (args.velocity) {
                double* o = Vl + kObsVelStride * lane;
                st3(o, f.v);
                st3(o + 3, f.w);
            }
        }
    }
    wave_sync();
    // ---- lanes = output elements: element e of the instance's block from lane e % 64 ----------------------------------------------
    if (args.placement) {
        TI* out = args.placement + (size_t)inst * nf * 12;
        for (int e = lane; e < 12 * nf; e += kWave) {
            const int fr = e / 12;
            out[e] = (TI)Pl[kObsPlaceStride * fr + (e - 12 * fr)];
        }
    }
    if (args.velocity) {
        TI* out = args.velocity + (size_t)inst * nf * 6;
        for (int e = lane; e < 6 * nf; e += kWave) {
            const int fr = e / 6;
            out[e] = (TI)Vl[kObsVelStride * fr + (e - 6 * fr)];
        }
    }
}

#endif // __HIPCC__
} // namespace wbcqp
