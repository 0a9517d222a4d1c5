// wbcqp_collide.hpp -- does a robot's sphere model touch itself: the reference's CollisionCheck::is_colliding (src/safety/collision_check.cpp:27-87
// there), which its controller runs on the solver's own model after every solve, for a whole fleet (wbcqp_check_collisions).
//
// A sphere model is a table of spheres, each carried by a body's joint frame and belonging to a MEMBER (arm_left, torso, ...).  Two spheres of
// different members collide iff the distance of their world centres is below the sum of their radii; spheres of one member are never tested.
//   lanes = bodies:   the world placement of every body from q (collide_body_placement: the walk observe_kernel does)
//   lanes = spheres:  in rounds of 64; the lane of sphere s fetches its body's R, p from the body's lane (12 doubles over ds_bpermute), forms the world
//                     centre R c + p and writes x, y, z and one packed word (float half-diameter, member, place inside the member) into a wave-private
//                     LDS table of 4 doubles per sphere
//   pair loop:        lane = sphere i (rounds of 64), j runs over the WHOLE table for the whole wave: every lane reads the same LDS address, which the
//                     LDS serves as a broadcast without bank conflicts; the pair counts when member[j] > member[i] (every unordered pair once)
//   reductions:       integer sum (pairs in collision), integer minimum of the 24-bit key (member a, member b, i in a, j in b: the pair the
//                     reference's four loops meet first), double minimum (clearance) -- all exact in any order, so a lane assignment changes nothing
//   lanes = output elements: the centres leave from the LDS table as consecutive elements of consecutive lanes
// One wavefront per instance, four per workgroup, nothing shared between the waves: no workgroup barrier, no atomics.  The result of an instance
// depends on its own q row alone.
#pragma once

#include "wbcqp_observe.hpp"

namespace wbcqp {

constexpr int kCollideMaxSpheres = 256; // WBCQP_MAX_SPHERES
constexpr int kCollideStride = 4;       // LDS doubles per sphere: x, y, z, {half-diameter (float) | member << 8 | place inside the member}

// the slot's sphere table on the device (wbcqp_set_collision_spheres)
struct CollideDev {
    int n_spheres;
    const int* body;       // [n_spheres] in [0, nb)
    const int* tag;        // [n_spheres] member << 8 | place inside the member
    const double* centre;  // [n_spheres][3] in the body's joint frame
    const float* half;     // [n_spheres] diameter * 0.5f
};

template <typename TI>
struct CollideArgs {
    ObserveDev D; // the tree's tables (n_frames = 0)
    CollideDev S;
    const TI* q;                            // [batch][nq]
    int *colliding, *first_pair, *n_pairs;  // [batch], [batch][2], [batch]; each may be null
    TI *clearance, *centres;                // [batch], [batch][n_spheres][3]; each may be null
    int batch;
};

inline int collide_lds_bytes(int n_spheres) { return kObservePerBlock * n_spheres * kCollideStride * 8; }

#ifdef __HIPCC__

// World placement R, p of the lane's body bi: joint transform from q, then nrounds rounds of ancestor doubling over ds_bpermute.  This is the position
// part of observe_kernel (wbcqp_observe.hpp), statement for statement, as a copy: lifted into a function that both kernels call, observe_kernel compiled
// to the same resources but another register allocation, and that kernel's code object is not to change (profiles/collision/INDEX.md).
template <typename TI>
__device__ __forceinline__ void collide_body_placement(const ObserveDev& D, const TI* gq, const int lane, const int bi, double (&Rw)[9], V3& pw)
{
    const int* ip = D.ipool;
    const double* dp = D.dpool;
    const int nb = D.nb;
    const int jt = ip[D.i_jtype + bi];
    const int iq = ip[D.i_idxq + bi];
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
            p = {(double)gq[0], (double)gq[1], (double)gq[2]}; // the base where it IS: the world frame
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
                    const double pd = (a == 0) ? c2 : (a == 1) ? c0 : c1;
                    const double nb_ = cs * pb + sn * pd, nd_ = cs * pd - sn * pb;
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
    // down the tree by ancestor doubling: after round r every body holds the composition over its 2^(r+1) nearest ancestors-and-self
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
#pragma unroll
    for (int k = 0; k < 9; ++k) Rw[k] = R[k];
    pw = p;
}

template <typename TI>
__global__ __launch_bounds__(kObserveThreads) void collide_kernel(const CollideArgs<TI> args)
{
    extern __shared__ double col_lds[];
    const ObserveDev& D = args.D;
    const CollideDev& S = args.S;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = uni((int)threadIdx.x >> 6);
    const long long inst = (long long)blockIdx.x * kObservePerBlock + wave;
    if (inst >= args.batch) return; // the whole wave leaves: nothing below waits for another wave
    const int nb = D.nb, ns = S.n_spheres;
    const TI* gq = args.q + (size_t)inst * D.nq;

    // ---- lanes = bodies: world placements (lanes past the last body repeat it; no sphere reads them) ---------------------------------
    const int bi = min(lane, nb - 1);
    double R[9];
    V3 p;
    collide_body_placement(D, gq, lane, bi, R, p);

    // ---- lanes = spheres, in rounds of 64: world centre and the packed word into the wave's table ------------------------------------
    double* T = col_lds + (size_t)wave * ns * kCollideStride;
    const int rounds = (ns + kWave - 1) / kWave; // wave-uniform
    for (int r = 0; r < rounds; ++r) {
        const int s = r * kWave + lane;
        const int sl = min(s, ns - 1);
        const int sb = S.body[sl]; // (checked on the host: in [0, nb))
        const V3 c = ld3(S.centre + 3 * sl);
        // the body's placement from the body's lane: every lane takes part in the exchange, the spheres' lanes keep the result
        double Rb[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rb[k] = __shfl(R[k], sb, kWave);
        const V3 pb = {__shfl(p.x, sb, kWave), __shfl(p.y, sb, kWave), __shfl(p.z, sb, kWave)};
        const V3 w = mv(Rb, c) + pb;
        if (s < ns) {
            double* o = T + kCollideStride * s;
            st3(o, w);
            o[3] = __hiloint2double(S.tag[sl], __float_as_int(S.half[sl]));
        }
    }
    wave_sync();

    // ---- pair loop: lane = sphere i, j the same for the whole wave (a broadcast read) -------------------------------------------------
    if (args.colliding || args.first_pair || args.n_pairs || args.clearance) {
        int hits = 0, best = 0x7fffffff, best_ij = 0;
        double clear = __builtin_huge_val();
        for (int r = 0; r < rounds; ++r) {
            const int i = r * kWave + lane;
            const double* mi = T + kCollideStride * min(i, ns - 1);
            const V3 ci = ld3(mi);
            const int tag_i = (i < ns) ? __double2hiint(mi[3]) : 0x7fffffff; // (a lane without a sphere: no member is above it)
            const float half_i = __int_as_float(__double2loint(mi[3]));
            for (int j = 0; j < ns; ++j) {
                const double* mj = T + kCollideStride * j;
                const V3 d = ld3(mj) - ci;
                const double word = mj[3];
                const int tag_j = __double2hiint(word);
                if ((tag_j >> 8) > (tag_i >> 8)) {
                    const double dist = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
                    const double thr = (double)(__int_as_float(__double2loint(word)) + half_i); // one float addition, as the reference's
                    clear = fmin(clear, dist - thr);
                    if (dist < thr) {
                        ++hits;
                        const int key = ((tag_i >> 8) << 20) | ((tag_j >> 8) << 16) | ((tag_i & 0xff) << 8) | (tag_j & 0xff);
                        if (key < best) {
                            best = key;
                            best_ij = (i << 8) | j;
                        }
                    }
                }
            }
        }
        const int total = wave_sum_int(hits);
        const int first = wave_min_int(best);
        if (args.clearance) {
            const double cmin = wave_min(clear);
            if (lane == 0) args.clearance[inst] = (TI)cmin;
        }
        if (lane == 0) {
            if (args.colliding) args.colliding[inst] = total > 0 ? 1 : 0;
            if (args.n_pairs) args.n_pairs[inst] = total;
        }
        if (args.first_pair) {
            // a key names one pair, so one lane at the most holds the minimum; without a hit lane 0 writes -1 -1
            if (total > 0 ? best == first : lane == 0) {
                args.first_pair[(size_t)inst * 2] = total > 0 ? (best_ij >> 8) : -1;
                args.first_pair[(size_t)inst * 2 + 1] = total > 0 ? (best_ij & 0xff) : -1;
            }
        }
    }
    // ---- lanes = output elements: element e of the instance's [n_spheres][3] block from lane e % 64 -----------------------------------
    if (args.centres) {
        TI* out = args.centres + (size_t)inst * ns * 3;
        for (int e = lane; e < 3 * ns; e += kWave) {
            const int s = e / 3;
            out[e] = (TI)T[kCollideStride * s + (e - 3 * s)];
        }
    }
}

#endif // __HIPCC__
} // namespace wbcqp
