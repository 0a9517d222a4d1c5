// wbcqp_host_launch.hpp -- host side of the C ABI (wbcqp_api.hip): from checked arguments to kernel launches -- the solve (launch: residency, queue and
// launch order; launch_small), the per-task costs, the force blocks' factor cache, the integration.  Included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_handle.hpp"

namespace {

template <typename TI>
void fill_group(GroupArgs<TI>& g, const Slot& s, bool compact, int batch, const wbcqp_inputs* in, const wbcqp_outputs* out)
{
    static_assert(offsetof(GroupArgs<TI>, Acop) - offsetof(GroupArgs<TI>, M) == offsetof(wbcqp_inputs, Acop), "GroupArgs carries the inputs in wbcqp_inputs' order");
    g.st = compact ? s.host_cp : s.host;
    std::memcpy(&g.M, in, sizeof(*in));
    g.x = static_cast<TI*>(out->x); g.tau = static_cast<TI*>(out->tau); g.objective = static_cast<TI*>(out->objective);
    g.status = out->status; g.iters = out->iters; g.n_active = out->n_active;
    g.amask = out->active_mask; // every kernel writes the mask; only the compact one takes it as the pick hint (g.warm)
    g.warm = 0;
    g.dbg = nullptr;
    g.count = batch;
}

int check_io(wbcqp_handle* h, const Slot& s, int batch, const wbcqp_inputs* in, const wbcqp_outputs* out)
{
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (batch == 0) return WBCQP_OK;
    if (!in || !out) return fail(h, WBCQP_ERR_INVALID, "inputs/outputs struct is NULL");
    const FieldBytes fb = field_bytes(s, 8);
    const Io io(in, out);
    for (Field f : kInputFields)
        if (fb.b[f] > 0 && !io.p[f]) {
            h->err = std::string("input array ") + kField[f].name + " is NULL";
            return WBCQP_ERR_INVALID;
        }
    if (!out->x || !out->status || !out->iters || (s.host.na > 0 && !out->tau))
        return fail(h, WBCQP_ERR_INVALID, "output arrays x, tau, status, iters are required");
    return WBCQP_OK;
}

// which instantiations have a three-per-CU twin: the compact kernel, generic or iCub's.  Not Talos's (two feet: 72 KB of LDS; one foot fits since its layout's
// last diet, 54 480 B, but LOSES there: 8.03 M QP/s at three per CU against 9.32 M at two -- with actuation bounds the loop keeps the actuation rows in 38
// registers, and at 168 they live in scratch, on the chain of every pick; tools/occ3_probe.py --stack talos_single_support).  The generic twin is likewise
// taken only for stacks WITHOUT actuation bounds (launch()).
template <bool CP, int SPEC> constexpr bool kThree = CP && (SPEC == 0 || SPEC == 2);
// which instantiations have a twin with the warm start's pick hint compiled in (WBCQP_FLAG_WARM_START): the generic compact kernel and Talos's; a handle
// with that flag runs every compact launch through one of the two (wbcqp_solve_ragged routes the other stacks to the generic one)
template <bool CP, int SPEC> constexpr bool kWarm = CP && (SPEC == 0 || SPEC == 1);

template <typename TI, bool CP, int SPEC = 0>
int launch(wbcqp_handle* h, GroupTable<TI>& tab, int total, int lds_bytes, hipStream_t stream)
{
    static_assert(SPEC == 0 || CP, "only the compact kernel is specialised");
    if (total == 0) return WBCQP_OK;
    constexpr int V = SPEC > 0 ? 1 + SPEC : (CP ? 1 : 0);
    if (lds_bytes > h->max_lds[V]) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_kernel<TI, CP, SPEC>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_queue_kernel<TI, CP, SPEC>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        if constexpr (kWarm<CP, SPEC>) {
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_kernel_warm<TI, SPEC>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_queue_kernel_warm<TI, SPEC>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        }
        if constexpr (kThree<CP, SPEC>)
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_queue3_kernel<TI, SPEC>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        h->max_lds[V] = lds_bytes;
    }
    // schedule: the order left by the previous launch is used when it is of this very shape and was produced on this
    // stream (stream order then guarantees that it is complete); otherwise index order
    OrderState* osp = h->graph_ord;
    if (!osp) {
        for (size_t i = 0; i < h->streams.size() && !osp; ++i)
            if (h->streams[i].stream == stream) { osp = &h->streams[i].ord; h->last_stream = (int)i; }
        if (!osp && h->streams.size() < kMaxQueues) {
            h->streams.push_back({stream, OrderState{}});
            h->last_stream = (int)h->streams.size() - 1;
            osp = &h->streams.back().ord;
            osp->stream = stream;
        }
        else if (!osp)
            h->last_stream = -1;
    }
    OrderState none{};
    OrderState& os = osp ? *osp : none;
    const bool sched = osp && !(h->flags & WBCQP_FLAG_INDEX_ORDER) && total > 1;
    unsigned long long sig = 1469598103934665603ull;
    ScheduleArgs sa{};
    sa.n = tab.n;
    for (int g = 0; g < tab.n; ++g) {
        sig = (sig ^ (unsigned long long)(uintptr_t)tab.g[g].st.rowmeta) * 1099511628211ull;
        sig = (sig ^ (unsigned long long)tab.g[g].st.lds_doubles) * 1099511628211ull;
        sig = (sig ^ (unsigned long long)tab.g[g].count) * 1099511628211ull;
        sa.iters[g] = tab.g[g].iters;
        sa.count[g] = tab.g[g].count;
    }
    tab.order = (sched && os.total == total && os.sig == sig) ? os.order + (os.packed ? os.cap : 0) : nullptr;
    // The queue pays when a QP is long enough for a hand-over (1 us: atomic + order entry) to vanish and few enough workgroups
    // fit a CU for the dispatcher's binding of a workgroup to one shader engine to leave CUs idle: the humanoid stacks (one
    // or two workgroups per CU; measured on the compact layout, tools/dispatch_sweep.py: 1-2 % over the dispatcher at every
    // batch size).  Small QPs (Franka: 26 KB of LDS) give the dispatcher slack -- measured 27 M QP/s through the queue
    // against 36 M through the hardware.  WBCQP_FLAG_QUEUE forces the queue, WBCQP_FLAG_HW_DISPATCH the dispatcher.
    if (h->queue_lds[V] != lds_bytes) {
        // Resident workgroups per CU of the kernel that will be launched: the runtime's answer, checked against what THIS kernel's own resources admit on
        // the device the handle is bound to (wbcqp_create accepts gfx950 only): k workgroups while k (lds + 16) <= 160 KB (measured, tools/ubench/lds_granule.hip)
        // and k waves per SIMD while k x (its allocated VGPRs, 8-register granule) <= 512 -- both read from the kernel itself (hipFuncGetAttributes), not from a
        // constant.  A runtime that answers LESS than both admit is not believed: seen when a process holds TWO HIP runtimes (the library loaded before torch:
        // the first one then answers 1 for every kernel, tools/occ_state_probe.py); workgroups that do not fit wait their turn, results never depend on it.
        // An answer below the rule for any other reason (registers grown in a variant build, WBCQP_DEBUG_LDS_PAD) moves the rule with it and is kept.
        bool distrust = false;
        auto resident_of = [&](const void* kernel, const char* what, int cap, int& occ_out) -> int {
            int occ = 0;
            HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kThreads, (size_t)lds_bytes));
            hipFuncAttributes fa{};
            HIP_TRY(h, hipFuncGetAttributes(&fa, kernel));
            const int regs = std::max(8, (fa.numRegs + 7) & ~7);
            const int admitted = std::min({(160 * 1024) / (lds_bytes + 16), 512 / regs, cap}); // (+ 16: the granule and the kernel's static word, as measured)
            if (occ < admitted && h->lds_pad == 0) {
                distrust = true;
                occ = admitted;
            }
            if (h->debug_launch)
                std::fprintf(stderr, "wbcqp occupancy: %s lds %d B (+ %d static) VGPRs %d -> %d per CU%s\n", what, lds_bytes, (int)fa.sharedSizeBytes, fa.numRegs, occ,
                             distrust ? " (runtime answered less)" : "");
            occ_out = occ;
            return WBCQP_OK;
        };
        int occ = 0;
        if (int rc = resident_of(reinterpret_cast<const void*>(&solve_queue_kernel<TI, CP, SPEC>), "solve_queue_kernel", 2, occ); rc != WBCQP_OK) return rc;
        if (occ < 1) return fail(h, WBCQP_ERR_HIP, "solve_queue_kernel: no workgroup fits a CU");
        h->queue_occ[V] = occ;
        h->queue_occ_warm[V] = occ;
        if constexpr (kWarm<CP, SPEC>) { // the warm start's twin is a register allocation of its own: its occupancy, not its sibling's
            int occw = 0;
            if (int rc = resident_of(reinterpret_cast<const void*>(&solve_queue_kernel_warm<TI, SPEC>), "solve_queue_kernel_warm", 2, occw); rc != WBCQP_OK) return rc;
            if (occw < 1) return fail(h, WBCQP_ERR_HIP, "solve_queue_kernel_warm: no workgroup fits a CU");
            h->queue_occ_warm[V] = occw;
        }
        h->queue_lds[V] = lds_bytes;
        h->queue_three[V] = false;
        // a workgroup small enough for three on a CU takes the kernel compiled for three waves per SIMD (wbcqp_device.hpp: solve_queue3_kernel)
        if constexpr (kThree<CP, SPEC>) {
            if (lds_bytes <= kLdsThree && h->lds_pad == 0) {
                int occ3 = 0;
                if (int rc = resident_of(reinterpret_cast<const void*>(&solve_queue3_kernel<TI, SPEC>), "solve_queue3_kernel", 3, occ3); rc != WBCQP_OK) return rc;
                if (occ3 >= 3) {
                    h->queue_three[V] = true;
                    h->queue_occ3[V] = occ3;
                }
            }
        }
        if (distrust && !h->warned_occupancy) {
            h->warned_occupancy = true;
            std::fprintf(stderr, "wbcqp: the HIP runtime reports fewer resident workgroups per CU than LDS (%d B) and the kernel's registers admit; launching %d per CU anyway. "
                                 "Two HIP runtimes in this process (libwbcqp.so loaded before torch)?  See INTEGRATION.md.\n", lds_bytes,
                         h->queue_three[V] ? h->queue_occ3[V] : h->queue_occ[V]);
        }
    }
    // three per CU: where the twin holds three AND no group of the launch has actuation bounds (kThree's comment says why)
    bool warm = false; // the handle asked for the warm start's pick hint: the kernels that carry its code
    if constexpr (kWarm<CP, SPEC>) warm = (h->flags & WBCQP_FLAG_WARM_START) != 0;
    bool three = false;
    if constexpr (kThree<CP, SPEC>) {
        three = h->queue_three[V] && !warm;
        for (int g = 0; g < tab.n; ++g) three = three && !tab.g[g].st.act_bounds;
    }
    const int queue_occ = three ? h->queue_occ3[V] : (warm ? h->queue_occ_warm[V] : h->queue_occ[V]);
    if (h->debug_launch)
        std::fprintf(stderr, "wbcqp launch: V %d spec %d total %d lds %d occupancy %d three %d n_cu %d flags 0x%x\n", V, SPEC, total, lds_bytes, queue_occ, (int)three,
                     h->n_cu, (unsigned)h->flags);
    int* queue = nullptr;
    if (osp && !(h->flags & WBCQP_FLAG_HW_DISPATCH) && (lds_bytes >= kQueueMinLds || (three && lds_bytes >= kQueue3MinLds) || (h->flags & WBCQP_FLAG_QUEUE))) {
        if (!os.queue && !h->graph_ord) {
            HIP_TRY(h, hipMalloc(&os.queue, 2 * sizeof(int)));
            HIP_TRY(h, hipMemset(os.queue, 0, 2 * sizeof(int)));
        }
        queue = os.queue;
    }
    if (queue) {
        const long long resident = (long long)queue_occ * h->n_cu;
        if constexpr (kThree<CP, SPEC>) {
            if (three)
                hipLaunchKernelGGL((solve_queue3_kernel<TI, SPEC>), dim3((unsigned)(total < resident ? total : resident)), dim3(kThreads), lds_bytes,
                                   stream, tab, queue, total);
        }
        if constexpr (kWarm<CP, SPEC>) {
            if (warm)
                hipLaunchKernelGGL((solve_queue_kernel_warm<TI, SPEC>), dim3((unsigned)(total < resident ? total : resident)), dim3(kThreads), lds_bytes,
                                   stream, tab, queue, total);
        }
        if (!three && !warm)
            hipLaunchKernelGGL((solve_queue_kernel<TI, CP, SPEC>), dim3((unsigned)(total < resident ? total : resident)), dim3(kThreads), lds_bytes,
                               stream, tab, queue, total);
    }
    else {
        if constexpr (kWarm<CP, SPEC>) {
            if (warm) hipLaunchKernelGGL((solve_kernel_warm<TI, SPEC>), dim3(total), dim3(kThreads), lds_bytes, stream, tab);
        }
        if (!warm) hipLaunchKernelGGL((solve_kernel<TI, CP, SPEC>), dim3(total), dim3(kThreads), lds_bytes, stream, tab);
    }
    HIP_TRY(h, hipGetLastError());
    // the order is renewed every `period` launches: iteration counts drift slowly from tick to tick, the queue absorbs what
    // drift there is, and the two order kernels (4.5 + 15 us) are then a fraction of a launch instead of a twentieth
    const int asked = (h->flags >> WBCQP_FLAG_REFRESH_SHIFT) & 0xff;
    const int period = h->capturing ? 1 : (asked ? asked : kOrderRefresh);
    if (sched && tab.order && os.age + 1 < period)
        ++os.age;
    else if (sched) {
        os.age = 0;
        if (total > os.cap) { // first launch of a larger shape (a graph's buffer has its final size from the start)
            if (h->graph_ord) return fail(h, WBCQP_ERR_INVALID, "captured tick: launch larger than the graph's order buffer");
            HIP_TRY(h, hipStreamSynchronize(stream));
            if (os.order) (void)hipFree(os.order);
            os.order = nullptr;
            os.cap = 0;
            os.total = 0;
            HIP_TRY(h, hipMalloc(&os.order, 2 * sizeof(int) * (size_t)total));
            os.cap = total;
        }
        hipLaunchKernelGGL(schedule_kernel, dim3(1), dim3(1024), 0, stream, sa, os.order, total);
        HIP_TRY(h, hipGetLastError());
        // a few QPs per resident workgroup, one structure, taken from the queue: pack the order (pack_order_kernel)
        const long long resident = queue ? (long long)queue_occ * h->n_cu : 0;
        // (with two workgroups per CU the packed order measured no better than plain longest-first: WBCQP_FLAG_QUEUE asks for it)
        os.packed = queue && !(h->flags & WBCQP_FLAG_NO_PACKING) && (queue_occ == 1 || (h->flags & WBCQP_FLAG_QUEUE)) && tab.n == 1 && resident % kPackSubs == 0 &&
                          total % kPackSubs == 0 && total > resident && total <= 8 * resident && total / kPackSubs <= kPackMaxItems;
        if (os.packed) {
            PackArgs pa{tab.g[0].iters, os.order, os.order + os.cap, total, (int)(resident / kPackSubs)};
            hipLaunchKernelGGL(pack_order_kernel, dim3(kPackSubs), dim3(256), 0, stream, pa);
            HIP_TRY(h, hipGetLastError());
        }
        os.total = total;
        os.sig = sig;
        os.stream = stream;
    }
    return WBCQP_OK;
}

// the small structures of a launch: one wavefront per QP, four per workgroup, in table order (no launch order: the QPs are
// short and alike, and 32 of them are resident per CU)
template <typename TI>
int launch_small(wbcqp_handle* h, GroupTable<TI>& tab, int total, hipStream_t stream)
{
    if (total == 0) return WBCQP_OK;
    tab.order = nullptr;
    const int lds_bytes = kWaves * sm::COUNT * (int)sizeof(double);
    hipLaunchKernelGGL((solve_small_kernel<TI>), dim3((unsigned)((total + kWaves - 1) / kWaves)), dim3(kThreads), lds_bytes, stream, tab, total);
    HIP_TRY(h, hipGetLastError());
    return WBCQP_OK;
}

// per-task costs of `count` solved instances of slot s (task_costs_kernel, wbcqp_costs.hpp): record rows A, b1, Acop, x [count][ldx], tau [count][na];
// cost row perm[j] (or j) of width ldc.  A is staged in LDS where it fits 48 KB (every shipped stack: Talos 16.7 KB); beyond that the lanes read it
// from global memory -- the same products in the same order
constexpr int kCostLdsStage = 48 * 1024;

int launch_costs(wbcqp_handle* h, const Slot& s, int count, const void* A, const void* b1, const void* Acop, const void* x, int ldx, const void* tau,
                 void* cost, int ldc, const int* perm, hipStream_t stream)
{
    if (count <= 0) return WBCQP_OK;
    const DevStruct& D = s.host;
    int lda = odd(D.nv);
    int lds = cost_lds_doubles(D, lda) * 8 + D.r1 * 4;
    if (lds > kCostLdsStage) {
        lda = 0;
        lds = cost_lds_doubles(D, 0) * 8 + D.r1 * 4;
    }
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        CostArgs<TI> a{D, static_cast<const TI*>(A), static_cast<const TI*>(b1), static_cast<const TI*>(Acop), static_cast<const TI*>(x),
                       static_cast<const TI*>(tau), static_cast<TI*>(cost), perm, count, ldx, ldc, lda};
        hipLaunchKernelGGL(task_costs_kernel<TI>, dim3(count), dim3(kCostThreads), lds, stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

// the force blocks' factor for the weights w (one QP's row), by the kernels' own code, ahead of the solve on its stream; waited for once, so that a
// launch on another stream never meets a half-written entry
int build_ffcache(wbcqp_handle* h, Slot& s, const void* w, hipStream_t stream)
{
    WB_TRY(with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        hipLaunchKernelGGL(ffcache_kernel<TI>, dim3(1), dim3(128), 0, stream, s.host_cp, static_cast<const TI*>(w), s.ffc_dev);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    }));
    HIP_TRY(h, hipStreamSynchronize(stream));
    s.ffc_built = true;
    return WBCQP_OK;
}

// the rows kernel's arguments (terms_kernel, wbcqp_terms.hpp) for `batch` instances of slot s: state and record from io
template <typename TI>
void fill_terms(TermsArgs<TI>& a, const wbcqp_handle* h, const Slot& s, int batch, const Io& io)
{
    auto at = [&](Field f) { return static_cast<TI*>(io.p[f]); };
    a.T = s.terms; a.batch = batch; a.dbg = h->dbg;
    a.q = at(F_q); a.v = at(F_v); a.ref = at(F_ref);
    a.M = at(F_M); a.h = at(F_h); a.A = at(F_A); a.b1 = at(F_b1); a.Ac = at(F_Ac); a.bc = at(F_bc); a.blb = at(F_blb); a.bub = at(F_bub); a.Acop = at(F_Acop);
    a.momentum = at(F_mom);
}

int integrate_impl(wbcqp_handle* h, int batch, int nv, int floating_base, double dt, const void* q, const void* dq, const void* x,
                   int ldx, const int32_t* status, void* q_next, void* v_next, void* q_solver, void* stream, const RollAcc& acc)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (batch < 0 || nv <= 0 || ldx < nv) return fail(h, WBCQP_ERR_INVALID, "bad batch / nv / ldx");
    if (floating_base && nv < 6) return fail(h, WBCQP_ERR_INVALID, "a floating base needs nv >= 6");
    if (batch == 0) return WBCQP_OK;
    if (!q || !dq || !x || !q_next || !v_next) return fail(h, WBCQP_ERR_INVALID, "q / dq / x / q_next / v_next is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        hipLaunchKernelGGL(integrate_kernel<TI>, dim3((batch + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), batch, nv, floating_base ? 1 : 0, dt,
                           static_cast<const TI*>(q), static_cast<const TI*>(dq), static_cast<const TI*>(x), ldx, status, static_cast<TI*>(q_next),
                           static_cast<TI*>(v_next), static_cast<TI*>(q_solver), acc);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

} // namespace
