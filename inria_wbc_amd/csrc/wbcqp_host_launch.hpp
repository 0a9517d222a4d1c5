// wbcqp_host_launch.hpp -- host side of the C ABI (wbcqp_api.hip): from checked arguments to kernel launches -- the solve (kernel_set: the kernels of a
// variant by address; launch: order state, residency, the chosen kernel, launch order; launch_small), the per-task costs, the force blocks' factor cache,
// the integration.  Which kernel a launch takes is choose_kernel's answer (wbcqp_host_handle.hpp).  Included by wbcqp_api.hip alone.
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

// The four-wave solve kernels of one variant (wbcqp_device.hpp), by address: the hardware's dispatch, the queue, their twins with the warm start's pick
// hint and the queue's twin compiled for three workgroups per CU; null: the variant has no such twin (spec_has_warm, spec_has_three)
struct KernelSet {
    const void *dispatch, *queue, *dispatch_warm, *queue_warm, *queue3;
};
// ... of the full layout (CP false) or of instantiation SPEC of the compact kernel: the one place that names the kernels
template <typename TI, bool CP, int SPEC>
KernelSet kernel_set()
{
    static_assert(SPEC == 0 || CP, "only the compact kernel is specialised");
    KernelSet k{reinterpret_cast<const void*>(&solve_kernel<TI, CP, SPEC>), reinterpret_cast<const void*>(&solve_queue_kernel<TI, CP, SPEC>), nullptr, nullptr, nullptr};
    if constexpr (CP && spec_has_warm(SPEC)) {
        k.dispatch_warm = reinterpret_cast<const void*>(&solve_kernel_warm<TI, SPEC>);
        k.queue_warm = reinterpret_cast<const void*>(&solve_queue_kernel_warm<TI, SPEC>);
    }
    if constexpr (CP && spec_has_three(SPEC)) k.queue3 = reinterpret_cast<const void*>(&solve_queue3_kernel<TI, SPEC>);
    return k;
}
template <typename TI>
KernelSet kernel_set(int variant)
{
    static_assert(kNumSpecs == 3, "one case per instantiation");
    switch (variant) {
    case 0: return kernel_set<TI, false, 0>();
    case 2: return kernel_set<TI, true, 1>();
    case 3: return kernel_set<TI, true, 2>();
    case 4: return kernel_set<TI, true, 3>();
    default: return kernel_set<TI, true, 0>();
    }
}

// what launch() needs of a group table, whatever its element type: the kernels' argument, where the launch order goes, and the groups' shapes
struct LaunchTable {
    void* kernarg;
    const int** order;
    ScheduleArgs sa;        // the groups' counts and iteration counts (schedule_kernel)
    unsigned long long sig; // shape signature: structures, LDS sizes, counts
    bool act_bounds;        // some group has actuation bounds
};
template <typename TI>
LaunchTable launch_table(GroupTable<TI>& tab)
{
    LaunchTable t{&tab, &tab.order, ScheduleArgs{}, 1469598103934665603ull, false};
    t.sa.n = tab.n;
    for (int g = 0; g < tab.n; ++g) {
        t.sig = (t.sig ^ (unsigned long long)(uintptr_t)tab.g[g].st.rowmeta) * 1099511628211ull;
        t.sig = (t.sig ^ (unsigned long long)tab.g[g].st.lds_doubles) * 1099511628211ull;
        t.sig = (t.sig ^ (unsigned long long)tab.g[g].count) * 1099511628211ull;
        t.sa.iters[g] = tab.g[g].iters;
        t.sa.count[g] = tab.g[g].count;
        t.act_bounds = t.act_bounds || tab.g[g].st.act_bounds;
    }
    return t;
}

// launch(), part 1: the order state of the stream -- the graph's own while a tick is captured, else the handle's for this stream (made on the stream's
// first launch); null beyond kMaxQueues streams: such a launch runs in index order on the dispatcher and leaves no state behind
OrderState* order_state_of(wbcqp_handle* h, hipStream_t stream)
{
    if (h->graph_ord) return h->graph_ord;
    for (size_t i = 0; i < h->streams.size(); ++i)
        if (h->streams[i].stream == stream) {
            h->last_stream = (int)i;
            return &h->streams[i].ord;
        }
    if (h->streams.size() >= kMaxQueues) {
        h->last_stream = -1;
        return nullptr;
    }
    h->streams.push_back({stream, OrderState{}});
    h->last_stream = (int)h->streams.size() - 1;
    h->streams.back().ord.stream = stream;
    return &h->streams.back().ord;
}

// launch(), part 2: the variant's kernels admit lds_bytes of dynamic LDS, and the handle knows how many of their workgroups a CU holds at that size
int prepare_variant(wbcqp_handle* h, const KernelSet& ks, wbcqp_handle::Variant& v, int lds_bytes)
{
    if (lds_bytes > v.max_lds) {
        for (const void* k : {ks.dispatch, ks.queue, ks.dispatch_warm, ks.queue_warm, ks.queue3})
            if (k) HIP_TRY(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        v.max_lds = lds_bytes;
    }
    if (v.occ_lds == lds_bytes) return WBCQP_OK;
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
    WB_TRY(resident_of(ks.queue, "solve_queue_kernel", 2, v.occ));
    if (v.occ < 1) return fail(h, WBCQP_ERR_HIP, "solve_queue_kernel: no workgroup fits a CU");
    v.occ_warm = v.occ;
    if (ks.queue_warm) { // the warm start's twin is a register allocation of its own: its occupancy, not its sibling's
        WB_TRY(resident_of(ks.queue_warm, "solve_queue_kernel_warm", 2, v.occ_warm));
        if (v.occ_warm < 1) return fail(h, WBCQP_ERR_HIP, "solve_queue_kernel_warm: no workgroup fits a CU");
    }
    v.occ_lds = lds_bytes;
    v.three = false;
    // a workgroup small enough for three on a CU takes the kernel compiled for three waves per SIMD (wbcqp_device.hpp: solve_queue3_kernel)
    if (ks.queue3 && lds_bytes <= kLdsThree && h->lds_pad == 0) {
        int occ3 = 0;
        WB_TRY(resident_of(ks.queue3, "solve_queue3_kernel", 3, occ3));
        if (occ3 >= 3) {
            v.three = true;
            v.occ3 = occ3;
        }
    }
    if (distrust && !h->warned_occupancy) {
        h->warned_occupancy = true;
        std::fprintf(stderr, "wbcqp: the HIP runtime reports fewer resident workgroups per CU than LDS (%d B) and the kernel's registers admit; launching %d per CU anyway. "
                             "Two HIP runtimes in this process (libwbcqp.so loaded before torch)?  See INTEGRATION.md.\n", lds_bytes, v.three ? v.occ3 : v.occ);
    }
    return WBCQP_OK;
}

// launch(), part 3: the chosen kernel of the set goes off, through the queue of `resident` workgroups or one workgroup per QP on the dispatcher
int launch_chosen(wbcqp_handle* h, const KernelSet& ks, const KernelChoice& c, void* kernarg, int* queue, long long resident, int total, int lds_bytes, hipStream_t stream)
{
    const void* kernel = queue ? (c.three ? ks.queue3 : (c.warm ? ks.queue_warm : ks.queue)) : (c.warm ? ks.dispatch_warm : ks.dispatch);
    if (!kernel) return fail(h, WBCQP_ERR_INVALID, "no solve kernel for the chosen variant"); // (choose_kernel and kernel_set share spec_has_warm / spec_has_three)
    void* args[3] = {kernarg, &queue, &total}; // (hipLaunchKernel: the runtime entry hipLaunchKernelGGL ends in; a failure is read back below, as after the other launches)
    (void)hipLaunchKernel(kernel, dim3((unsigned)(queue && resident < total ? resident : total)), dim3(kThreads), args, (size_t)lds_bytes, stream);
    HIP_TRY(h, hipGetLastError());
    return WBCQP_OK;
}

// launch(), part 4: the launch order for the next launch of this shape on this stream, from the iteration counts this one leaves
int renew_order(wbcqp_handle* h, OrderState& os, const LaunchTable& t, bool used_order, long long resident, int queue_occ, int total, hipStream_t stream)
{
    // the order is renewed every `period` launches: iteration counts drift slowly from tick to tick, the queue absorbs what
    // drift there is, and the two order kernels (4.5 + 15 us) are then a fraction of a launch instead of a twentieth
    const int asked = (h->flags >> WBCQP_FLAG_REFRESH_SHIFT) & 0xff;
    const int period = h->capturing ? 1 : (asked ? asked : kOrderRefresh);
    if (used_order && os.age + 1 < period) {
        ++os.age;
        return WBCQP_OK;
    }
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
    hipLaunchKernelGGL(schedule_kernel, dim3(1), dim3(1024), 0, stream, t.sa, os.order, total);
    HIP_TRY(h, hipGetLastError());
    // a few QPs per resident workgroup, one structure, taken from the queue (resident > 0): pack the order (pack_order_kernel)
    // (with two workgroups per CU the packed order measured no better than plain longest-first: WBCQP_FLAG_QUEUE asks for it)
    os.packed = resident > 0 && !(h->flags & WBCQP_FLAG_NO_PACKING) && (queue_occ == 1 || (h->flags & WBCQP_FLAG_QUEUE)) && t.sa.n == 1 && resident % kPackSubs == 0 &&
                total % kPackSubs == 0 && total > resident && total <= 8 * resident && total / kPackSubs <= kPackMaxItems;
    if (os.packed) {
        PackArgs pa{t.sa.iters[0], os.order, os.order + os.cap, total, (int)(resident / kPackSubs)};
        hipLaunchKernelGGL(pack_order_kernel, dim3(kPackSubs), dim3(256), 0, stream, pa);
        HIP_TRY(h, hipGetLastError());
    }
    os.total = total;
    os.sig = t.sig;
    os.stream = stream;
    return WBCQP_OK;
}

// `total` QPs of the groups of t on four-wave workgroups of lds_bytes, by the kernel choose_kernel names (c; ks: that variant's kernels)
int launch(wbcqp_handle* h, const KernelSet& ks, KernelChoice c, const LaunchTable& t, int total, int lds_bytes, hipStream_t stream)
{
    if (total == 0) return WBCQP_OK;
    wbcqp_handle::Variant& v = h->variant[c.variant];
    WB_TRY(prepare_variant(h, ks, v, lds_bytes));
    // schedule: the order left by the previous launch is used when it is of this very shape and was produced on this
    // stream (stream order then guarantees that it is complete); otherwise index order
    OrderState* os = order_state_of(h, stream);
    const bool sched = os && !(h->flags & WBCQP_FLAG_INDEX_ORDER) && total > 1;
    *t.order = (sched && os->total == total && os->sig == t.sig) ? os->order + (os->packed ? os->cap : 0) : nullptr;
    // what the device can still overrule: the twin does not hold three workgroups per CU after all (the runtime's occupancy answer, prepare_variant) --
    // then two per CU, and the queue only where it is taken without the twin; and a stream without an order state has no queue counter
    if (c.three && !v.three) {
        c.three = false;
        c.queue = wants_queue(lds_bytes, false, h->flags);
    }
    const int queue_occ = c.three ? v.occ3 : (c.warm ? v.occ_warm : v.occ);
    if (h->debug_launch)
        std::fprintf(stderr, "wbcqp launch: V %d spec %d total %d lds %d occupancy %d three %d n_cu %d flags 0x%x\n", c.variant, c.spec, total, lds_bytes, queue_occ,
                     (int)c.three, h->n_cu, (unsigned)h->flags);
    int* queue = nullptr;
    if (os && c.queue) {
        if (!os->queue && !h->graph_ord) {
            HIP_TRY(h, hipMalloc(&os->queue, 2 * sizeof(int)));
            HIP_TRY(h, hipMemset(os->queue, 0, 2 * sizeof(int)));
        }
        queue = os->queue;
    }
    const long long resident = queue ? (long long)queue_occ * h->n_cu : 0;
    WB_TRY(launch_chosen(h, ks, c, t.kernarg, queue, resident, total, lds_bytes, stream));
    return sched ? renew_order(h, *os, t, *t.order != nullptr, resident, queue_occ, total, stream) : WBCQP_OK;
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
    // the kernel's outputs are __restrict__, and lane 0 reads dq[0..5] after lanes 0..5 have stored v_next[0..5]: in place, the base would be integrated twice
    if (q_next == q || v_next == dq) return fail(h, WBCQP_ERR_INVALID, "q_next / v_next must not be q / dq: the integration is not done in place");
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
