// wbcqp_costs.hpp -- per-task costs of a solved QP record (wbcqp_task_costs, and the cost field of the traced roll-outs).
#pragma once

#include "wbcqp_prims.hpp"

namespace wbcqp {

// cost[t] = || A_t x - b_t ||_2 for every level-1 task t of one instance: the rows exactly as they enter H and g (dense rows over dv,
// the posture's selection rows, F_c f_c per contact with F = diag(w_f) T, the torque task's rows as scale_j tau[joint_j], the cop
// rows over f).  The reference's Controller::cost(task) (controller.hpp:148-152) for the motion tasks.
template <typename TI>
struct CostArgs {
    DevStruct st;         // sizes and the device tables of the structure (row -> task maps, F', the torque task's joints and scales)
    const TI *A, *b1, *Acop;  // the record: [count][n_dense][nv], [count][r1], [count][3][12 nc] (null without a cop task)
    const TI *x, *tau;        // [count][ldx], [count][na] (tau: null without a torque task)
    TI* cost;                 // row j of the record -> cost row perm ? perm[j] : j, [.][ldc]; entries [n_tasks, ldc) are written zero
    const int* perm;
    int count, ldx, ldc;
    int lda;                  // leading dimension of A in LDS (odd: the lanes of the dense rows fall in different banks); 0: A not staged
};

constexpr int kCostThreads = 256;
constexpr int kCostRegs = 16; // elements of A a lane holds while its loads are in flight: every load of a block of up to 4096 is issued before the first wait

// LDS doubles of one instance: A staged (n_dense lda), x, tau, b1, the squared residuals of the rows; then the row -> task map (ints)
__host__ __device__ inline int cost_lds_doubles(const DevStruct& S, int lda) { return S.n_dense * lda + S.n + S.na + 2 * S.r1; }

#ifdef __HIPCC__
// One workgroup per instance.  No atomics: lane r forms row r's residual with its columns in ascending order, lane t sums the squares
// of task t's rows in ascending row order -- the same bits from run to run and between the entry points that launch it.
template <typename TI>
__global__ __launch_bounds__(kCostThreads) void task_costs_kernel(const CostArgs<TI> a)
{
    extern __shared__ double cost_lds[];
    const DevStruct& S = a.st;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int nv = S.nv, na = S.na, k = S.k, n_dense = S.n_dense, n_sel = S.n_sel, r1 = S.r1, lda = a.lda;
    double* sA = cost_lds;
    double* sx = sA + n_dense * lda;
    double* stau = sx + S.n;
    double* sb1 = stau + na;
    double* sres = sb1 + r1;
    int* stask = reinterpret_cast<int*>(sres + r1);
    const TI* Ai = a.A + (size_t)i * n_dense * nv;
    const TI* b1 = a.b1 + (size_t)i * r1;
    // everything the rows need goes into LDS in one phase, its global loads in flight together (one memory latency, not one per loop trip)
    if (lda) // the instance's contiguous block of rows, coalesced
        for (int base = 0; base < n_dense * nv; base += kCostRegs * kCostThreads) {
            TI v[kCostRegs];
#pragma unroll
            for (int j = 0; j < kCostRegs; ++j) {
                const int e = base + tid + j * kCostThreads;
                v[j] = e < n_dense * nv ? Ai[e] : (TI)0;
            }
#pragma unroll
            for (int j = 0; j < kCostRegs; ++j) {
                const int e = base + tid + j * kCostThreads;
                if (e < n_dense * nv) {
                    const int r = e / nv;
                    sA[r * lda + e - r * nv] = (double)v[j];
                }
            }
        }
    for (int e = tid; e < S.n; e += kCostThreads) sx[e] = (double)a.x[(size_t)i * a.ldx + e];
    if (S.n_acteq > 0)
        for (int e = tid; e < na; e += kCostThreads) stau[e] = (double)a.tau[(size_t)i * na + e];
    for (int r = tid; r < r1; r += kCostThreads) {
        sb1[r] = (double)b1[r];
        const int rs = r - n_dense, rf = rs - n_sel, ra = rf - 6 * S.nc;
        stask[r] = r < n_dense ? S.dense_row_task[r] : rs < n_sel ? S.sel_task[rs] : ra < 0 ? S.forcereg_task[rf / 6] : ra < S.n_acteq ? S.acteq_task : S.cop_task;
    }
    bsync();
    for (int r = tid; r < r1; r += kCostThreads) {
        double res;
        if (r < n_dense) {
            double acc = 0.0;
            if (lda) {
#pragma unroll 10
                for (int c = 0; c < nv; ++c) acc += sA[r * lda + c] * sx[c];
            }
            else
                for (int c = 0; c < nv; ++c) acc += (double)Ai[(size_t)r * nv + c] * sx[c];
            res = acc - sb1[r];
        }
        else if (r < n_dense + n_sel) {
            res = sx[S.sel_col[r - n_dense]] - sb1[r];
        }
        else if (r < n_dense + n_sel + 6 * S.nc) {
            const int j = r - n_dense - n_sel, c = j / 6, q = j - 6 * c;
            const double* ft = S.ft + (size_t)c * 72; // F' [12][6]
            const double* f = sx + nv + 12 * c;
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < 12; ++e) acc += ft[e * 6 + q] * f[e];
            res = acc - sb1[r];
        }
        else if (r < n_dense + n_sel + 6 * S.nc + S.n_acteq) {
            const int j = r - n_dense - n_sel - 6 * S.nc;
            res = S.acteq_scale[j] * stau[S.acteq_joint[j]] - sb1[r];
        }
        else {
            const int j = r - n_dense - n_sel - 6 * S.nc - S.n_acteq;
            const TI* Ac = a.Acop + ((size_t)i * 3 + j) * k;
            double acc = 0.0;
            for (int e = 0; e < k; ++e) acc += (double)Ac[e] * sx[nv + e];
            res = acc - sb1[r];
        }
        sres[r] = res * res;
    }
    bsync();
    TI* out = a.cost + (size_t)(a.perm ? a.perm[i] : i) * a.ldc;
    for (int t = tid; t < a.ldc; t += kCostThreads) {
        double s = 0.0;
        if (t < S.n_tasks)
#pragma unroll 8
            for (int r = 0; r < r1; ++r) s += (stask[r] == t) ? sres[r] : 0.0;
        out[t] = (TI)(t < S.n_tasks ? sqrt(s) : 0.0);
    }
}
#endif // __HIPCC__

} // namespace wbcqp
