// wbcqp_factor.hpp -- H -> J = U^-1 by blocked elimination in registers (four pivots per synchronisation), and the phases around it that both
// LDS layouts run: staging of the task constants, assembly of H_vv and g, the force blocks, J's final write.
#pragma once

#include "wbcqp_prims.hpp"

namespace wbcqp {
#ifdef __HIPCC__

// ------------------------------------------------------------------------------------------------
// Blocked elimination H -> (pivots, Y) with J = U^-1 = Y diag(1/sqrt(pivot)), four pivots per synchronisation.
// Ownership: a G x G thread grid (G = 1 << LG); thread (ta, te) keeps positions (ta + G u, te + G w), u <= w < NU, of H
// (h) and of Y (y, from zero) in registers for the whole factorisation.  S = [H; Y] (Y from the identity) is reduced by
// column operations: with P the four pivot columns, S(:,k) -= S(:,P) H_PP^-1 H_Pk for every later column k.  Only the
// four pivot rows of H (rb[column][p]) and the four pivot columns of Y (yb[row][p]) travel through LDS, RAW, once per
// panel; every thread factors the 4 x 4 pivot block itself (H_PP = U~' D U~, U~ unit upper triangular, four chained
// reciprocals) and brings its own slices to the state a pivot-by-pivot elimination would have published
// (x' = U~^-T x).  JB = panel start / G is a compile-time constant: only h[u >= JB][.] and y[u <= JB][w >= JB] change.
// WLOCAL: the grid is one wavefront -- LDS operations of a wave execute in order, no workgroup barrier is needed and
// one buffer suffices; otherwise one barrier per panel and two buffers.  Positions past the matrix must hold the identity.
// ------------------------------------------------------------------------------------------------
template <int LG, int NU, bool WLOCAL, int UU>
__device__ __forceinline__ void publish_panel(Ctx& c, double (&h)[NU][NU], double (&y)[NU][NU], int ta, int te, int j0n,
                                              double* RB, double* YB)
{
    // A panel buffer holds four values per index k (the four pivot rows of column k of H; the four pivot columns of row k of Y) in two planes:
    // value p of index k at (p >> 1) HP + 2 k + (p & 1).  A thread reads them as two 16-byte pairs; sixteen lanes with consecutive k then
    // cover 256 contiguous bytes per read, and the 8-byte stores of a publishing row land in distinct banks.  (Until round 4: 4 k + p, the
    // two pairs side by side -- lanes k and k + 8 in the same banks.)
    constexpr int G = 1 << LG, PS = NU * G * 4, HP = PS / 2;
    const int par = WLOCAL ? 0 : ((j0n >> 2) & 1);
    const int grp = (j0n & (G - 1)) >> 2;
    if ((ta >> 2) == grp) { // rows j0n + p, p = ta & 3
        double* dst = RB + par * PS + ((ta >> 1) & 1) * HP + (ta & 1);
#pragma unroll
        for (int w = UU; w < NU; ++w) dst[(te + G * w) * 2] = h[UU][w];
    }
    if ((te >> 2) == grp) { // columns j0n + p of Y, p = te & 3
        const int pp = te & 3;
        double* dst = YB + par * PS + ((te >> 1) & 1) * HP + (te & 1);
#pragma unroll
        for (int u = 0; u < UU; ++u) dst[(ta + G * u) * 2] = y[u][UU];
        const int r = ta + G * UU;
        dst[r * 2] = (r < j0n) ? y[UU][UU] : ((r == j0n + pp) ? 1.0 : 0.0);
    }
}

template <int LG, int NU, bool WLOCAL, int JB>
__device__ __forceinline__ void eliminate_block(Ctx& c, double (&h)[NU][NU], double (&y)[NU][NU], int ta, int te, int npad,
                                                double* RB, double* YB, double* dinv, bool dwriter, int dp)
{
    constexpr int G = 1 << LG, PS = NU * G * 4, HP = PS / 2;
    constexpr int JN = (JB + 1 < NU) ? JB + 1 : JB;
    const int jend = min(G * JB + G, npad);
    for (int j0 = G * JB; j0 < jend; j0 += 4) {
        if (WLOCAL) __builtin_amdgcn_wave_barrier();
        else bsync();
        const int par = WLOCAL ? 0 : ((j0 >> 2) & 1);
        const double* rb = RB + par * PS;
        const double* yb = YB + par * PS;
        // operands: pivot block, this thread's row-role and column-role slices, its rows of Y
        // the pivot block: only its upper triangle is read (H(p,q) = hq[q][p>>1][p&1], p <= q), each piece with a load of exactly its width.
        // (Whole 16-byte pairs for all four columns left half-dead destination registers, which the allocator reused for the next pair:
        // a write-after-write hazard the compiler guards with `s_waitcnt lgkmcnt(0)` right behind the first load of every panel step.)
        double2v hq[4][2], fa[NU][2], fe[NU][2], fr[NU][2];
        hq[0][0].x = rb[j0 * 2];
        hq[1][0] = ld2(rb + (j0 + 1) * 2);
        hq[2][0] = ld2(rb + (j0 + 2) * 2);
        hq[2][1].x = rb[HP + (j0 + 2) * 2];
        hq[3][0] = ld2(rb + (j0 + 3) * 2);
        hq[3][1] = ld2(rb + HP + (j0 + 3) * 2);
#pragma unroll
        for (int u = JB; u < NU; ++u) {
            fe[u][0] = ld2(rb + (te + G * u) * 2);
            fe[u][1] = ld2(rb + HP + (te + G * u) * 2);
            fa[u][0] = ld2(rb + (ta + G * u) * 2);
            fa[u][1] = ld2(rb + HP + (ta + G * u) * 2);
        }
#pragma unroll
        for (int u = 0; u <= JB; ++u) {
            fr[u][0] = ld2(yb + (ta + G * u) * 2);
            fr[u][1] = ld2(yb + HP + (ta + G * u) * 2);
        }
        // H_PP = U~' D U~ : H(p,q) = hq[q][p>>1][p&1] for p <= q
        const double a0 = hq[0][0].x, i0 = fast_rcp(a0);
        const double u01 = hq[1][0].x * i0, u02 = hq[2][0].x * i0, u03 = hq[3][0].x * i0;
        const double a1 = fma(-u01, hq[1][0].x, hq[1][0].y), i1 = fast_rcp(a1);
        const double t12 = fma(-u01, hq[2][0].x, hq[2][0].y), t13 = fma(-u01, hq[3][0].x, hq[3][0].y);
        const double u12 = t12 * i1, u13 = t13 * i1;
        const double a2 = fma(-u12, t12, fma(-u02, hq[2][0].x, hq[2][1].x)), i2 = fast_rcp(a2);
        const double t23 = fma(-u12, t13, fma(-u02, hq[3][0].x, hq[3][1].x));
        const double u23 = t23 * i2;
        const double a3 = fma(-u23, t23, fma(-u13, t13, fma(-u03, hq[3][0].x, hq[3][1].y))), i3 = fast_rcp(a3);
        auto xform = [&](double2v (&x)[2]) __attribute__((always_inline)) { // x' = U~^-T x (also g' = g U~^-1)
            x[0].y = fma(-u01, x[0].x, x[0].y);
            x[1].x = fma(-u12, x[0].y, fma(-u02, x[0].x, x[1].x));
            x[1].y = fma(-u23, x[1].x, fma(-u13, x[0].y, fma(-u03, x[0].x, x[1].y)));
        };
#pragma unroll
        for (int u = JB; u < NU; ++u) {
            xform(fa[u]);
            xform(fe[u]);
            fe[u][0].x *= i0; fe[u][0].y *= i1; fe[u][1].x *= i2; fe[u][1].y *= i3;
        }
        if (te + G * JB < j0 + 4) { // columns up to the end of the panel take no update
            fe[JB][0].x = 0.0; fe[JB][0].y = 0.0; fe[JB][1].x = 0.0; fe[JB][1].y = 0.0;
        }
#pragma unroll
        for (int u = 0; u <= JB; ++u) xform(fr[u]);
#pragma unroll
        for (int u = JB; u < NU; ++u)
#pragma unroll
            for (int w = u; w < NU; ++w)
                h[u][w] = fma(-fa[u][1].y, fe[w][1].y, fma(-fa[u][1].x, fe[w][1].x,
                          fma(-fa[u][0].y, fe[w][0].y, fma(-fa[u][0].x, fe[w][0].x, h[u][w]))));
#pragma unroll
        for (int u = 0; u <= JB; ++u)
#pragma unroll
            for (int w = JB; w < NU; ++w)
                y[u][w] = fma(-fr[u][1].y, fe[w][1].y, fma(-fr[u][1].x, fe[w][1].x,
                          fma(-fr[u][0].y, fe[w][0].y, fma(-fr[u][0].x, fe[w][0].x, y[u][w]))));
        // the pivot columns of Y themselves are final now
        if ((te >> 2) == ((j0 & (G - 1)) >> 2)) {
            const int pp = te & 3;
#pragma unroll
            for (int u = 0; u <= JB; ++u) {
                const double lo = (pp & 1) ? fr[u][0].y : fr[u][0].x;
                const double hi = (pp & 1) ? fr[u][1].y : fr[u][1].x;
                y[u][JB] = (pp & 2) ? hi : lo;
            }
        }
        if (dwriter) { // 1/sqrt(pivot)
            const double lo = (dp & 1) ? a1 : a0, hi = (dp & 1) ? a3 : a2;
            dinv[j0 + dp] = rsqrt((dp & 2) ? hi : lo);
        }
        if (j0 + 4 < npad) {
            if (j0 + 4 < G * JB + G) publish_panel<LG, NU, WLOCAL, JB>(c, h, y, ta, te, j0 + 4, RB, YB);
            else publish_panel<LG, NU, WLOCAL, JN>(c, h, y, ta, te, j0 + 4, RB, YB);
        }
    }
    if constexpr (JB + 1 < NU) {
        if (npad > G * (JB + 1)) eliminate_block<LG, NU, WLOCAL, JB + 1>(c, h, y, ta, te, npad, RB, YB, dinv, dwriter, dp);
    }
}

// ------------------------------------------------------------------------------------------------
// The phases around the elimination that do not depend on where a kernel keeps things in LDS: solve_one (wbcqp_device.hpp) and solve_one_compact
// (wbcqp_compact.hpp) both run these.  Thread (ta, te) = (tid >> 4, tid & 15) of the 16 x 16 grid owns positions (ta + 16 u, te + 16 w), u <= w < NU,
// of the dv block; lane (la, le) = (lane >> 3, lane & 7) of a wave's 8 x 8 grid owns positions (la + 8 u, le + 8 w), u <= w < 2, of a force block.
// ------------------------------------------------------------------------------------------------

// Phase 0, the part no layout changes, in the three pieces its loads, its stores and its barrier cut it into.  What a thread loads for itself:
template <typename TI>
struct TaskConsts {
    TI vb1, vw, vbl, vbu, vtl, vtu, vha; // the short vectors: one (clamped) element per thread each
    int drt;                             // task of dense row tid
    int selc, selt;                      // selection row tid (posture): column, task
    int frt;                             // force variable tid: its contact's force-regularisation task ...
    double ftc[6];                       // ... and its column of F (row of F')
};
// (1) the loads.  qr: the record (b1, h, bounds), qp: the QP's index in the batch (weights, torque limits) -- see solve_one_compact
template <typename TI>
__device__ __forceinline__ void load_task_constants(const GroupArgs<TI>& ga, const DevStruct& S, const Dims& D, size_t qp, size_t qr, int tid, TaskConsts<TI>& t)
{
    t.vb1 = ga.b1[qr * D.r1 + min(tid, D.r1 - 1)];
    t.vw = ga.w[qp * D.n_tasks + min(tid, D.n_tasks - 1)];
    t.vbl = TI(0); t.vbu = TI(0); t.vtl = TI(0); t.vtu = TI(0); t.vha = TI(0);
    if (D.n_bound > 0) {
        t.vbl = ga.blb[qr * D.n_bound + min(tid, D.n_bound - 1)];
        t.vbu = ga.bub[qr * D.n_bound + min(tid, D.n_bound - 1)];
    }
    if (D.act_bounds) {
        t.vtl = ga.tlb[qp * D.na + min(tid, D.na - 1)];
        t.vtu = ga.tub[qp * D.na + min(tid, D.na - 1)];
        t.vha = ga.h[qr * D.nv + D.nu + min(tid, D.na - 1)];
    }
    t.drt = (D.n_dense > 0) ? S.dense_row_task[min(tid, D.n_dense - 1)] : 0;
    // selection rows (posture) and force-regularisation right-hand sides: constants now, arithmetic after the barrier
    t.selc = 0; t.selt = 0; t.frt = 0;
#pragma unroll
    for (int qd = 0; qd < 6; ++qd) t.ftc[qd] = 0.0;
    if (D.n_sel > 0) {
        t.selc = S.sel_col[min(tid, D.n_sel - 1)];
        t.selt = S.sel_task[min(tid, D.n_sel - 1)];
    }
    if (D.nc > 0) {
        const int fm = min(tid, D.k - 1);
        t.frt = S.forcereg_task[fm / 12];
#pragma unroll
        for (int qd = 0; qd < 6; ++qd) t.ftc[qd] = S.ft[(fm / 12) * 72 + (fm % 12) * 6 + qd];
    }
}
// (2) the short vectors land in their slots (b1, w, bounds, tl / tu); z and d start from zero for the selection rows
template <typename TI>
__device__ __forceinline__ void land_task_vectors(Ctx& c, const Dims& D, const TaskConsts<TI>& t)
{
    const int tid = c.tid;
    if (tid < D.r1) c.b1[tid] = (double)t.vb1;
    if (tid < D.n_tasks) c.w[tid] = (double)t.vw;
    if (tid < D.n_bound) {
        c.blb[tid] = (double)t.vbl;
        c.bub[tid] = (double)t.vbu;
    }
    if (D.act_bounds && tid < D.na) { // lb - h_a, ub - h_a (computeProblemData, actuation tasks)
        c.tl[tid] = (double)t.vtl - (double)t.vha;
        c.tu[tid] = (double)t.vtu - (double)t.vha;
    }
    if (tid < D.nv) { // diagonal additions / right-hand sides of the selection rows
        c.z[tid] = 0.0;
        c.d[tid] = 0.0;
    }
}
// (3) behind the barrier that publishes w and b1: what the assembly reads besides the staged rows As
template <typename TI>
__device__ __forceinline__ void stage_task_constants(Ctx& c, const DevStruct& S, const Dims& D, double* As, const TaskConsts<TI>& t)
{
    const int tid = c.tid, n_dense = D.n_dense, n_sel = D.n_sel;
    if (tid < n_dense) { // (row weight, right-hand side) pairs behind the staged rows: one 16-byte read per row
        As[n_dense * 64 + 2 * tid] = c.w[t.drt];
        As[n_dense * 64 + 2 * tid + 1] = c.b1[tid];
    }
    // selection rows (posture): H(c,c) += w, g(c) -= w b  (distinct columns)
    for (int sidx = tid; sidx < n_sel; sidx += kThreads) {
        const int col = (sidx == tid) ? t.selc : S.sel_col[sidx];
        const double wt = c.w[(sidx == tid) ? t.selt : S.sel_task[sidx]];
        c.z[col] = wt;
        c.d[col] = wt * c.b1[n_dense + sidx];
    }
    // force regularisation: g_f = -w F' b
    if (tid < D.k) {
        const double* bb = c.b1 + n_dense + n_sel + 6 * (tid / 12);
        double sacc = 0.0;
#pragma unroll
        for (int qd = 0; qd < 6; ++qd) sacc = fma(t.ftc[qd], bb[qd], sacc);
        c.g[D.nv + tid] = -c.w[t.frt] * sacc;
    }
}

// Phase 1: H_vv = sum_r w_r A(r,:)'A(r,:) + diag(z) + reg I into h (from zero), g_j = -sum_r w_r A(r,j) b(r) - d_j into c.g, the thread's share of
// tr(H) into trace.  As: the nd staged task rows (layout of a staged row: wbcqp_types.hpp, apack), WB: their (weight, right-hand side) pairs
// (stage_task_constants).  The rows of the next task line are in flight while this one multiplies; g rides along.
template <int NU>
__device__ __forceinline__ void assemble_hvv(Ctx& c, const DevStruct& S, const double* As, const double* WB, const int nd, double (&h)[NU][NU], double& trace)
{
    const int ta = c.tid >> 4, te = c.tid & 15, nv = c.nv;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int w = 0; w < NU; ++w) h[u][w] = 0.0;
    double gacc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* Ai = As + ta * 2;
    const double* Aj = As + te * 2;
    auto ldrow = [&](int r, double2v (&ai)[2], double2v (&aj)[2], double2v& wb) __attribute__((always_inline)) {
        ai[0] = ld2(Ai + r * 64);
        ai[1] = ld2(Ai + r * 64 + 32);
        aj[0] = ld2(Aj + r * 64);
        aj[1] = ld2(Aj + r * 64 + 32);
        wb = ld2(WB + 2 * r);
    };
    auto macrow = [&](const double2v (&ai)[2], const double2v (&aj)[2], const double2v& wb) __attribute__((always_inline)) {
        const double a[4] = {ai[0].x, ai[0].y, ai[1].x, ai[1].y};
        const double ajw[4] = {aj[0].x * wb.x, aj[0].y * wb.x, aj[1].x * wb.x, aj[1].y * wb.x};
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int w = u; w < NU; ++w) h[u][w] = fma(a[u], ajw[w], h[u][w]);
#pragma unroll
        for (int w = 0; w < NU; ++w) gacc[w] = fma(ajw[w], wb.y, gacc[w]);
    };
    if (nd > 0) {
        double2v ai0[2], aj0[2], ai1[2], aj1[2], wb0, wb1;
        ldrow(0, ai0, aj0, wb0);
        int r = 0;
        for (; r + 2 <= nd; r += 2) {
            ldrow(r + 1, ai1, aj1, wb1);
            macrow(ai0, aj0, wb0);
            ldrow(min(r + 2, nd - 1), ai0, aj0, wb0);
            macrow(ai1, aj1, wb1);
        }
        if (r < nd) macrow(ai0, aj0, wb0);
    }
    if (ta == 0) {
#pragma unroll
        for (int w = 0; w < NU; ++w) {
            const int col = te + 16 * w;
            if (col < nv) c.g[col] = -gacc[w] - c.d[col];
        }
    }
    if (ta == te) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = ta + 16 * u;
            if (i < nv) {
                h[u][u] += c.z[i] + S.hessian_reg;
                trace += h[u][u];
            }
        }
    }
}

// positions past nv: identity, so that the pivots of the padded last panel are inert
template <int NU>
__device__ __forceinline__ void pad_identity(double (&h)[NU][NU], int ta, int te, int nv)
{
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int w = u; w < NU; ++w) {
            const int r = ta + 16 * u, q = te + 16 * w;
            if (r >= nv || q >= nv) h[u][w] = (r == q) ? 1.0 : 0.0;
        }
}

// the lane's tile of F'F of contact ct (the force-regularisation block is H_ff = w F'F + reg I, 12 x 12 per contact): a constant of the structure,
// fetched ahead of the dv block's elimination so that the loads overlap it
__device__ __forceinline__ void load_ftf_tile(const DevStruct& S, int ct, int la, int le, double (&hF)[2][2])
{
    const double* ftf = S.ftf + ct * 144;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < 2; ++w) hF[u][w] = ftf[min(la + 8 * u, 11) * 12 + min(le + 8 * w, 11)];
}

// One contact's force block on one wave (8 x 8 lane grid, 2 x 2 positions per lane): H_ff = wt F'F + reg I eliminated to (1 / sqrt(pivot), Y) with
// J_ff = Y diag(1 / sqrt(pivot)).  hF enters as the lane's tile of F'F; tF returns the lane's (at most two) diagonal elements of H_ff, in the order the
// kernel adds them to tr(H).  The solve kernels and ffcache_kernel (which makes DevStruct::ffc) both run THIS function: a cached factor is the computed
// one bit for bit.
__device__ __forceinline__ void force_block_factor(Ctx& c, double (&hF)[2][2], double (&yF)[2][2], double (&tF)[2], double wt, double reg, int la, int le,
                                                   double* RBf, double* YBf, double* dinv_out, int lane)
{
    tF[0] = 0.0;
    tF[1] = 0.0;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int r = la + 8 * u, q = le + 8 * w;
            if (r < 12 && q < 12) {
                hF[u][w] = wt * hF[u][w] + ((r == q) ? reg : 0.0);
                if (r == q) tF[u] = hF[u][w]; // (r == q needs u == w: la, le < 8)
            }
            else hF[u][w] = (r == q) ? 1.0 : 0.0;
            yF[u][w] = 0.0;
        }
    publish_panel<3, 2, true, 0>(c, hF, yF, la, le, 0, RBf, YBf);
    eliminate_block<3, 2, true, 0>(c, hF, yF, la, le, 12, RBf, YBf, dinv_out, lane < 4, lane & 3);
}

// final: J(r,q) = Y(r,q) dinv[q], J(r,r) = dinv[r] -- the dv block from the 16 x 16 grid's tiles, a force block (first row and column fb) from a wave's
template <int NU>
__device__ __forceinline__ void store_j_dv(Ctx& c, const double (&y)[NU][NU], int ta, int te)
{
    const int nv = c.nv, ldj = c.ldj;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int w = u; w < NU; ++w) {
            const int r = ta + 16 * u, q = te + 16 * w;
            if (q < nv && r < q) c.J[r * ldj + q] = y[u][w] * c.dinv[q];
            else if (r == q && r < nv) c.J[r * ldj + r] = c.dinv[r];
        }
}
__device__ __forceinline__ void store_j_force(Ctx& c, const double (&yF)[2][2], int fb, int la, int le)
{
    const int ldj = c.ldj;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = u; w < 2; ++w) {
            const int r = la + 8 * u, q = le + 8 * w;
            if (q < 12 && r < q) c.J[(fb + r) * ldj + fb + q] = yF[u][w] * c.dinv[fb + q];
            else if (r == q && r < 12) c.J[(fb + r) * ldj + fb + r] = c.dinv[fb + r];
        }
}

#endif // __HIPCC__
} // namespace wbcqp
