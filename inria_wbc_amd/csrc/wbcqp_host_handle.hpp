// wbcqp_host_handle.hpp -- host side of the C ABI (wbcqp_api.hip): the handle and its slots, error reporting, device and page-locked buffers, the
// ONE description of the per-instance arrays of a call (fields, block layout, staging of the host-pointer entry points), the argument checks the entry
// points share and the F64 / F32 fork; the launch policy (choose_kernel: which kernel runs a launch).  Host code only; included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_device.hpp"
#include "wbcqp_terms.hpp"
#include "wbcqp_dense.hpp"
#include "wbcqp_small.hpp"
#include "wbcqp_costs.hpp"
#include "wbcqp_observe.hpp"
#include "wbcqp_collide.hpp"
#include "wbcqp_rnea.hpp"

#include "../../include/wbcqp.h"

#include <dlfcn.h>
#include <limits>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace wbcqp;

namespace {

thread_local std::string g_create_error;

// a selection of model frames on the device, one allocation: placement [n][12], then body [n]
struct FrameSel {
    int n = 0;
    const int* body = nullptr;
    const double* place = nullptr;
    void* alloc = nullptr;
};

struct Slot {
    bool set = false;
    DevStruct host{};           // sizes, LDS layout and device pointers of the tables: travels by value with every launch
    DevStruct host_cp{};        // the same with the compact LDS layout (wbcqp_compact.hpp); host_cp.compact == 0: not eligible
    std::vector<void*> allocs;  // device arrays owned by this slot
    wbcqp_layout layout{};      // what wbcqp_layout_of reports: the compact layout where the structure is eligible
    int lds_full = 0, lds_cp = 0;
    bool small = false;         // eligible for the one-wavefront-per-QP kernel (wbcqp_small.hpp)
    int spec = 0;               // 1-based index of the compact kernel's instantiation for this very layout (kSpecDims), 0: the generic kernel
    std::vector<int> sel_col_h;       // host copies of what wbcqp_set_model needs of the structure: the posture task's columns
    std::vector<double> force_gen_h;  // and the contacts' force generators (the contact points sit in their skew blocks)
    std::vector<double> forcereg_h;   // forcereg_mat [nc][6][12]: what wbcqp_set_force_references holds the caller's weights against
    double* ffc_dev = nullptr;  // the force blocks' factor for one weight (DevStruct::ffc; owned through `allocs`), null: none (no contacts, not compact, disabled)
    bool ffc_built = false;     // ... made from the first QP of the slot's first compact launch (solve_ragged)
    bool has_model = false;     // wbcqp_set_model: tree + task bindings for wbcqp_problem_data
    std::vector<double> tree;   // ... the tree as numbers (sizes, parents, joint types, placements, inertias, gravity): the slots of a mix must agree on it
    TermsDev terms{};
    std::vector<void*> model_allocs;
    // the model's whole frame table (host copies: only task frames reach the device with the model) and the frames chosen from it, on the device, by
    // wbcqp_set_observed_frames (wbcqp_observe), wbcqp_set_wrench_frames (wbcqp_inverse_dynamics) and wbcqp_set_jacobian_frames (wbcqp_jacobians);
    // dropped with the model
    std::vector<int> frame_body_h;
    std::vector<double> frame_place_h;
    FrameSel observed, wrench, jacobian;
    // wbcqp_check_collisions: the sphere table of wbcqp_set_collision_spheres, one device allocation; dropped with the model
    CollideDev spheres{};
    void* spheres_alloc = nullptr;
};

struct Staging {
    void* dev = nullptr;
    size_t bytes = 0;
};
// page-locked host memory for the host-pointer entry points at small batches: the input arrays of a QP record (eleven, twelve with a cop task; five output
// arrays) cross PCIe as ONE copy each way instead of eleven (five) -- at batch 1 the copies' fixed cost is most of the call
struct Pinned {
    void* host = nullptr;
    size_t bytes = 0;
};
constexpr size_t kPackedBytes = 1u << 20; // above this the arrays go up one by one (the extra host copy would cost more than it saves)

} // namespace

// launch-order state: the order left by one launch for the next one of the same shape on the same stream.  The handle has
// one PER STREAM it has launched on (two launches in flight on two streams share neither the order buffer -- the schedule
// kernel of one would overwrite what the solve kernel of the other is reading -- nor the queue counter); every captured tick
// (wbcqp_graph) and every sub-batch of a roll-out has its own, so that a replay never touches a buffer another launch may
// resize or overwrite (a graph bakes the buffer's address into its kernel nodes).
struct OrderState {
    int* order = nullptr;        // [2][cap]: longest-first, then the packed order (pack_order_kernel)
    bool packed = false;         // the second half is valid for total / sig / stream
    int age = 0;                 // launches that have used the order since it was computed
    int cap = 0;
    int total = 0;               // 0: no valid order
    unsigned long long sig = 0;  // shape of the launch the order belongs to
    hipStream_t stream = nullptr;
    int* queue = nullptr;        // the queue counter pair of solve_queue_kernel that goes with this order (allocated on first use)
};

constexpr size_t kMaxQueues = 16;

// ---- which kernel runs a launch: the ONE statement of the policy (solve_ragged, launch() and wbcqp_layout_of all ask choose_kernel) ------------------
constexpr int kQueueMinLds = 48 * 1024; // workgroups at least this large take their QPs from the queue by default (measured: below it the dispatcher wins, wants_queue)
constexpr int kQueue3MinLds = 40 * 1024; // ... and from 40 KB on where the launch runs three per CU through solve_queue3_kernel (the dispatcher's solve_kernel holds
                                         // two); a 40-48 KB stack that cannot take the twin (actuation bounds, warm start) stays with the dispatcher
constexpr int kLdsThree = 54592;        // the largest dynamic LDS block of which a CU holds three (tools/ubench/lds_granule.hip)
constexpr int kOrderRefresh = 4; // default period of the launch-order renewal (WBCQP_FLAG_REFRESH)

// which instantiations of the compact kernel (0: generic, i: kSpecDims[i - 1]) have a three-per-CU twin: the generic one and iCub's.  Not Talos's (two feet:
// 72 KB of LDS; one foot fits since its layout's last diet, 54 480 B, but LOSES there: 8.03 M QP/s at three per CU against 9.32 M at two -- with actuation
// bounds the loop keeps the actuation rows in 38 registers, and at 168 they live in scratch, on the chain of every pick; tools/occ3_probe.py --stack
// talos_single_support).  The generic twin is likewise taken only for stacks WITHOUT actuation bounds (choose_kernel).
constexpr bool spec_has_three(int spec) { return spec == 0 || spec == 2; }
// ... and which have a twin with the warm start's pick hint compiled in (WBCQP_FLAG_WARM_START): the generic one and Talos's; a handle with that flag runs
// every compact launch through one of the two (the other stacks go to the generic one)
constexpr bool spec_has_warm(int spec) { return spec == 0 || spec == 1; }

// what a launch is, as far as the choice goes
struct LaunchFacts {
    bool compact;    // every group of the launch is eligible for the compact layout
    int lds_bytes;   // dynamic LDS of a workgroup (the largest group's)
    bool act_bounds; // some group has actuation bounds
    int spec;        // the structure's instantiation of the compact kernel (Slot::spec), where the launch is one group
    bool single;     // one group; false: ragged
};
struct KernelChoice {
    int spec;    // the compact kernel's instantiation, 0: the generic one (and the full layout's kernel)
    int variant; // index into wbcqp_handle::variant: 0 full layout, 1 compact, 1 + spec
    bool warm;   // the twin with the warm start's pick hint
    bool three;  // the twin compiled for three workgroups per CU (taken where the launch goes through the queue)
    bool queue;  // the workgroups take their QPs from the queue; false: the hardware's dispatcher
};

// The queue pays when a QP is long enough for a hand-over (1 us: atomic + order entry) to vanish and few enough workgroups
// fit a CU for the dispatcher's binding of a workgroup to one shader engine to leave CUs idle: the humanoid stacks (one
// or two workgroups per CU; measured on the compact layout, tools/dispatch_sweep.py: 1-2 % over the dispatcher at every
// batch size).  Small QPs (Franka: 26 KB of LDS) give the dispatcher slack -- measured 27 M QP/s through the queue
// against 36 M through the hardware.  WBCQP_FLAG_QUEUE forces the queue, WBCQP_FLAG_HW_DISPATCH the dispatcher.
constexpr bool wants_queue(int lds_bytes, bool three, int flags)
{
    return !(flags & WBCQP_FLAG_HW_DISPATCH) && (lds_bytes >= kQueueMinLds || (three && lds_bytes >= kQueue3MinLds) || (flags & WBCQP_FLAG_QUEUE));
}

// flags: wbcqp_desc.flags; lds_pad: the handle's diagnostic padding (WBCQP_DEBUG_LDS_PAD).  Pure: no device, no handle (wbcqp_layout_of asks with flags 0)
constexpr KernelChoice choose_kernel(const LaunchFacts& f, int flags, int lds_pad = 0)
{
    KernelChoice c{0, 0, false, false, false};
    if (f.compact) {
        // a launch of ONE group whose structure is a shipped stack takes that stack's instantiation (sizes and offsets as literals: wbcqp_types.hpp);
        // anything else -- ragged launches, other structures, WBCQP_FLAG_GENERIC_KERNEL -- the generic one.  Same bits.
        if (f.single && !(flags & WBCQP_FLAG_GENERIC_KERNEL) && lds_pad == 0) c.spec = f.spec;
        c.warm = (flags & WBCQP_FLAG_WARM_START) != 0;
        if (c.warm && !spec_has_warm(c.spec)) c.spec = 0;
        c.variant = 1 + c.spec;
        // three per CU: the instantiation has the twin, three workgroups fit the CU's LDS, no warm start and no group has actuation bounds
        c.three = spec_has_three(c.spec) && !c.warm && !f.act_bounds && f.lds_bytes <= kLdsThree && lds_pad == 0;
    }
    c.queue = wants_queue(f.lds_bytes, c.three, flags);
    return c;
}

struct wbcqp_handle {
    int device = 0;
    int dtype = WBCQP_F64;
    std::string err;
    Slot slots[WBCQP_MAX_STRUCTURES];
    Staging stage_in, stage_out;
    Pinned pin_in, pin_out;
    // what the handle remembers per kernel variant (0: full layout, 1: compact, 2 + i: the compact kernel specialised for kSpecDims[i]; KernelSet)
    struct Variant {
        int max_lds = 0;  // largest dynamic LDS size the members' attribute was set for
        int occ_lds = -1; // the LDS size the rest was asked for (-1: never): resident workgroups per CU of the queue kernel, of its warm twin (a
        int occ = 0, occ_warm = 0, occ3 = 0; // register allocation of its own; the queue kernel's where there is none) and of the three-per-CU twin,
        bool three = false;                  // and whether that twin holds three at that size
    };
    Variant variant[2 + kNumSpecs];
    long long* dbg = nullptr; // diagnostic builds only (wbcqp_debug_set_stamp_buffer)
    // longest-first schedule (schedule_kernel): launch order for the next solve of the same shape on the same stream
    int flags = 0;
    // one order state (order buffer + queue counter pair) per stream this handle has launched on; a launch on a stream beyond
    // kMaxQueues distinct ones runs in index order on the hardware's dispatcher and leaves no state behind
    struct StreamState {
        hipStream_t stream;
        OrderState ord;
    };
    std::vector<StreamState> streams;
    int last_stream = -1;            // index of the stream state the most recent launch used (wbcqp_launch_order reports that one)
    OrderState* graph_ord = nullptr; // wbcqp_tick_graph_create: the launches of this tick use the graph's own order state
    bool capturing = false;          // ... and a captured tick always renews its order
    int n_cu = 0;
    int dense_max_lds = 0;
    // wbcqp_solve_dense_host: the reference's HQPOutput, owned by the solver and valid until the next call
    std::vector<double> dense_x, dense_obj;
    std::vector<int32_t> dense_status, dense_iters, dense_nact;
    wbcqp_dense_output dense_out{};
    int lds_pad = 0; // diagnostic (env WBCQP_DEBUG_LDS_PAD): extra dynamic LDS per workgroup, to force a lower residency
    bool debug_launch = false;                                   // env WBCQP_DEBUG_LAUNCH, read once at wbcqp_create (never on the per-tick path)
    bool hessian_wide = false;                                   // env WBCQP_HESSIAN_STORE=wide, read once at wbcqp_create: hessian_kernel's second store shape
    bool no_ffcache = false;                                     // env WBCQP_DEBUG_NO_FFCACHE: every QP eliminates its force blocks itself (what tests compare the cache with)
    bool warned_occupancy = false;                               // the one-time note of launch() when the runtime's occupancy answer is overruled
    // wbcqp_rollout: sub-batches on streams of their own (each with its own launch-order state and queue counter), the record
    // arrays and the state ping-pong of the whole batch
    struct RollSub {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        OrderState ord;
    };
    std::vector<RollSub> roll_subs;
    hipEvent_t roll_start = nullptr;
    hipEvent_t roll_done = nullptr;  // end of the previous roll-out: the next one (on whatever stream) waits for it before it reuses the buffers
    // how many sub-batches a roll-out is cut into is MEASURED, per (slot, batch): the device time of every roll-out lies between
    // roll_start and roll_done (both timed events); the next call reads it without blocking (hipEventQuery) and keeps, per shape, a
    // running figure of microseconds per tick for one sub-batch (= what K calls of wbcqp_tick do) and for two
    struct RollStat {
        int slot = -1, batch = 0, calls = 0;
        double us[3] = {0.0, 0.0, 0.0}; // [S] running mean, 0: never measured
        int cold[3] = {1, 1, 1};        // [S] the next measurement of this form is its first: it paid the form's allocations and stream set-up, it is not kept
    };
    std::vector<RollStat> roll_stats;
    struct RollMeas { // one timed event pair around a roll-out, read by a later call once the device has passed it
        hipEvent_t t0 = nullptr, t1 = nullptr;
        int stat = -1, S = 0, ticks = 0;
        bool pending = false;
    };
    RollMeas roll_meas[4];
    Staging roll_rec, roll_state;
    // wbcqp_tick_mixed / wbcqp_rollout_mixed: the per-tick permutations go up through a ring of page-locked buffers (an entry is reused
    // once the call that last used it is done on the device: four calls ago), the per-set records, gathered weights and outputs, and the
    // state ping-pong of a roll-out
    struct MixPlan {
        Pinned pin;
        int* dev = nullptr;
        size_t cap = 0; // ints
        hipEvent_t done = nullptr;
        bool used = false;
    };
    MixPlan mix_plan[4];
    int mix_next = 0;
    Staging mix_rec, mix_state;
    hipEvent_t mix_done = nullptr; // end of the previous mixed call: the next one (on whatever stream) waits for it before it reuses the buffers
    // reference programs (wbcqp_program): the segments and offsets of a call go up through a ring of page-locked buffers, as the mixed calls' plans do; the
    // rings of generated rows (two chunks of ref_chunk ticks) of the one-slot and of the mixed roll-out; the schedule the mixed one makes on the host
    struct ProgUp {
        Pinned pin;
        void* dev = nullptr;
        size_t cap = 0; // bytes
        hipEvent_t done = nullptr;
        bool used = false;
    };
    ProgUp prog_up[4];
    int prog_next = 0;
    int ref_chunk = 32; // ticks per launch of refgen_kernel (env WBCQP_REFPROG_CHUNK, read at wbcqp_create)
    Staging roll_ref, mix_ref;
    std::vector<int32_t> prog_sched;
};

namespace {

int fail(wbcqp_handle* h, int code, const std::string& msg)
{
    if (h)
        h->err = msg;
    else
        g_create_error = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(h, WBCQP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

#define WB_TRY(expr)                          \
    do {                                      \
        const int rc_ = (expr);               \
        if (rc_ != WBCQP_OK) return rc_;      \
    } while (0)

int ensure_pinned(wbcqp_handle* h, Pinned& p, size_t bytes)
{
    if (p.bytes >= bytes) return WBCQP_OK;
    if (p.host) (void)hipHostFree(p.host);
    p.host = nullptr;
    p.bytes = 0;
    HIP_TRY(h, hipHostMalloc(&p.host, bytes, hipHostMallocDefault));
    p.bytes = bytes;
    return WBCQP_OK;
}

int ensure(wbcqp_handle* h, Staging& s, size_t bytes)
{
    if (s.bytes >= bytes) return WBCQP_OK;
    if (s.dev) (void)hipFree(s.dev);
    s.dev = nullptr;
    s.bytes = 0;
    HIP_TRY(h, hipMalloc(&s.dev, bytes));
    s.bytes = bytes;
    return WBCQP_OK;
}

template <typename T>
int upload(wbcqp_handle* h, Slot& s, const T* src, size_t count, const T** dst)
{
    void* p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    HIP_TRY(h, hipMalloc(&p, bytes));
    s.allocs.push_back(p);
    if (count) HIP_TRY(h, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return WBCQP_OK;
}

void release(FrameSel& f)
{
    if (f.alloc) (void)hipFree(f.alloc);
    f = FrameSel{};
}

void release_spheres(Slot& s)
{
    if (s.spheres_alloc) (void)hipFree(s.spheres_alloc);
    s.spheres_alloc = nullptr;
    s.spheres = CollideDev{};
}

void release_model(Slot& s)
{
    for (void* p : s.model_allocs) (void)hipFree(p);
    s.model_allocs.clear();
    s.has_model = false;
    s.tree.clear();
    s.frame_body_h.clear();
    s.frame_place_h.clear();
    release(s.observed);
    release_spheres(s);
    release(s.wrench);
    release(s.jacobian);
}

void release(Slot& s)
{
    for (void* p : s.allocs) (void)hipFree(p);
    s.allocs.clear();
    s.set = false;
    release_model(s);
}

// ---- the F64 / F32 fork: f(Tag<double>{}) or f(Tag<float>{}) by the handle's dtype -----------------------------------------------------------------
template <typename T> struct Tag { using type = T; };
template <typename F> int with_dtype(const wbcqp_handle* h, F&& f) { return h->dtype == WBCQP_F64 ? f(Tag<double>{}) : f(Tag<float>{}); }
#define WB_TI(tag) typename decltype(tag)::type
inline size_t elem_size(const wbcqp_handle* h) { return h->dtype == WBCQP_F64 ? 8 : 4; }

// ---- the per-instance arrays of a call, described once ----------------------------------------------------------------------------------------------
// In the order of the members of wbcqp_inputs, wbcqp_outputs and wbcqp_state, then the q_next / v_next / q_solver of a tick: the pointers of a call are
// one array indexed by Field (Io), filled from and turned back into the ABI's structs as a whole.
enum Field { F_M, F_h, F_A, F_b1, F_Ac, F_bc, F_blb, F_bub, F_tlb, F_tub, F_w, F_Acop, // wbcqp_inputs
             F_x, F_tau, F_status, F_iters, F_obj, F_nact, F_amask,                   // wbcqp_outputs
             F_q, F_v, F_ref, F_mom,                                                  // wbcqp_state
             F_qn, F_vn, F_qs, F_N };
struct FieldInfo {
    const char* name;
    int elem; // bytes of one element; 0: the handle's dtype
};
constexpr FieldInfo kField[F_N] = {{"M", 0}, {"h", 0}, {"A", 0}, {"b1", 0}, {"Ac", 0}, {"bc", 0}, {"blb", 0}, {"bub", 0}, {"tlb", 0}, {"tub", 0}, {"w", 0}, {"Acop", 0},
                                   {"x", 0}, {"tau", 0}, {"status", 4}, {"iters", 4}, {"objective", 0}, {"n_active", 4}, {"active_mask", 32},
                                   {"q", 0}, {"v", 0}, {"ref", 0}, {"momentum", 0}, {"q_next", 0}, {"v_next", 0}, {"q_solver", 0}};
static_assert(sizeof(wbcqp_inputs) == (F_Acop - F_M + 1) * sizeof(void*) && offsetof(wbcqp_inputs, Acop) == (F_Acop - F_M) * sizeof(void*), "Field follows wbcqp_inputs");
static_assert(sizeof(wbcqp_outputs) == (F_amask - F_x + 1) * sizeof(void*) && offsetof(wbcqp_outputs, objective) == (F_obj - F_x) * sizeof(void*), "Field follows wbcqp_outputs");
static_assert(sizeof(wbcqp_state) == (F_mom - F_q + 1) * sizeof(void*) && offsetof(wbcqp_state, momentum) == (F_mom - F_q) * sizeof(void*), "Field follows wbcqp_state");

// bytes per instance of every field, for slot s and elements of es bytes
struct FieldBytes {
    size_t b[F_N];
};
FieldBytes field_bytes(const Slot& s, size_t es)
{
    const wbcqp_layout& L = s.layout;
    const TermsDev& T = s.terms;
    const int len[F_N] = {L.len_M, L.len_h, L.len_A, L.len_b1, L.len_Ac, L.len_bc, L.len_blb, L.len_bub, L.len_tlb, L.len_tub, L.len_w, L.len_Acop,
                          L.n, s.host.na, 1, 1, 1, 1, 1, T.nq, T.nv, T.nref, 6, T.nq, T.nv, T.nv};
    FieldBytes r;
    for (int f = 0; f < F_N; ++f) r.b[f] = (size_t)len[f] * (kField[f].elem ? (size_t)kField[f].elem : es);
    return r;
}

struct Io {
    void* p[F_N] = {};
    Io() = default;
    Io(const wbcqp_inputs* in, const wbcqp_outputs* out, const wbcqp_state* st = nullptr, void* q_next = nullptr, void* v_next = nullptr, void* q_solver = nullptr)
    {
        if (in) std::memcpy(p + F_M, in, sizeof(*in));
        if (out) std::memcpy(p + F_x, out, sizeof(*out));
        if (st) std::memcpy(p + F_q, st, sizeof(*st));
        p[F_qn] = q_next; p[F_vn] = v_next; p[F_qs] = q_solver;
    }
    wbcqp_inputs inputs() const { wbcqp_inputs r; std::memcpy(&r, p + F_M, sizeof(r)); return r; }
    wbcqp_outputs outputs() const { wbcqp_outputs r; std::memcpy(&r, p + F_x, sizeof(r)); return r; }
    wbcqp_state state() const { wbcqp_state r; std::memcpy(&r, p + F_q, sizeof(r)); return r; }
    wbcqp_tick_io tick_io(double dt) const { return wbcqp_tick_io{state(), inputs(), outputs(), p[F_qn], p[F_vn], p[F_qs], dt}; }
    // the same arrays from instance `first` on (null stays null)
    Io from(size_t first, const FieldBytes& fb) const
    {
        Io r;
        for (int f = 0; f < F_N; ++f) r.p[f] = p[f] ? static_cast<char*>(p[f]) + first * fb.b[f] : nullptr;
        return r;
    }
};

// one array of a block: which field (-1: none of them, elements of the handle's dtype), the caller's side, its size and its place in the block
struct Arr {
    int f;
    void* host;
    size_t bytes, off;
};
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// block layout: the arrays one after the other from byte `at`, each on a 256-byte boundary; returns the end
size_t lay(Arr* a, int n, size_t at = 0)
{
    for (int i = 0; i < n; ++i) {
        a[i].off = at;
        at += al256(a[i].bytes);
    }
    return at;
}
// ... of the fields `fields` of `count` instances (an array is laid out whether or not the caller has one)
size_t lay(const FieldBytes& fb, size_t count, const Field* fields, int n, const Io& host, Arr* a, size_t at = 0)
{
    for (int i = 0; i < n; ++i) a[i] = Arr{fields[i], host.p[fields[i]], count * fb.b[fields[i]], 0};
    return lay(a, n, at);
}
void point(Io& d, void* base, const Arr* a, int n)
{
    for (int i = 0; i < n; ++i) d.p[a[i].f] = static_cast<char*>(base) + a[i].off;
}
constexpr Field kInputFields[12] = {F_M, F_h, F_A, F_b1, F_Ac, F_bc, F_blb, F_bub, F_tlb, F_tub, F_w, F_Acop};
constexpr Field kRecordFields[10] = {F_M, F_h, F_A, F_b1, F_Ac, F_bc, F_blb, F_bub, F_Acop, F_mom}; // what the rows kernel writes: the record (nine), the momentum
constexpr int kNumRecord = 9;

// ---- staging of the host-pointer entry points ---------------------------------------------------------------------------------------------------
// Their arrays cross in the handle's two device blocks (stage_in, stage_out), on the null stream.  packed: through page-locked memory as ONE copy each
// way (at batch 1 the copies' fixed cost is most of the call); async: one asynchronous copy per array; blocking: one hipMemcpy per array;
// blocking_float: the same where the caller's arrays are double and the device's float (wbcqp_solve_dense_host on an F32 handle)
enum class Xfer { packed, async, blocking, blocking_float };

int stage_begin(wbcqp_handle* h, size_t in_bytes, size_t out_bytes, bool packed)
{
    WB_TRY(ensure(h, h->stage_in, in_bytes + 256));
    WB_TRY(ensure(h, h->stage_out, out_bytes + 256));
    if (packed) {
        WB_TRY(ensure_pinned(h, h->pin_in, kPackedBytes));
        WB_TRY(ensure_pinned(h, h->pin_out, kPackedBytes));
    }
    return WBCQP_OK;
}

inline bool is_real(const Arr& a) { return a.f < 0 || kField[a.f].elem == 0; }

// the arrays the caller has go up into the block at dev (packed: the first block_bytes of it in one copy)
int stage_up(wbcqp_handle* h, void* dev, const Arr* a, int n, size_t block_bytes, Xfer how)
{
    char* d = static_cast<char*>(dev);
    if (how == Xfer::packed) {
        char* pin = static_cast<char*>(h->pin_in.host);
        for (int i = 0; i < n; ++i)
            if (a[i].bytes && a[i].host) std::memcpy(pin + a[i].off, a[i].host, a[i].bytes);
        HIP_TRY(h, hipMemcpyAsync(d, pin, block_bytes, hipMemcpyHostToDevice, nullptr));
        return WBCQP_OK;
    }
    for (int i = 0; i < n; ++i) {
        if (!a[i].bytes || !a[i].host) continue;
        if (how == Xfer::blocking_float && is_real(a[i])) {
            const double* sd = static_cast<const double*>(a[i].host);
            std::vector<float> tmp(sd, sd + a[i].bytes / 4);
            HIP_TRY(h, hipMemcpy(d + a[i].off, tmp.data(), a[i].bytes, hipMemcpyHostToDevice));
        }
        else if (how == Xfer::async) HIP_TRY(h, hipMemcpyAsync(d + a[i].off, a[i].host, a[i].bytes, hipMemcpyHostToDevice, nullptr));
        else HIP_TRY(h, hipMemcpy(d + a[i].off, a[i].host, a[i].bytes, hipMemcpyHostToDevice));
    }
    return WBCQP_OK;
}

// ... and come down from it; packed and (unless sync is false) async end in a synchronisation of the null stream
int stage_down(wbcqp_handle* h, const void* dev, const Arr* a, int n, size_t block_bytes, Xfer how, bool sync = true)
{
    const char* d = static_cast<const char*>(dev);
    if (how == Xfer::packed) { // one copy down, then the arrays are taken apart on the host
        char* po = static_cast<char*>(h->pin_out.host);
        HIP_TRY(h, hipMemcpyAsync(po, d, block_bytes, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(h, hipStreamSynchronize(nullptr));
        for (int i = 0; i < n; ++i)
            if (a[i].bytes && a[i].host) std::memcpy(a[i].host, po + a[i].off, a[i].bytes);
        return WBCQP_OK;
    }
    for (int i = 0; i < n; ++i) {
        if (!a[i].bytes || !a[i].host) continue;
        if (how == Xfer::blocking_float && is_real(a[i])) {
            std::vector<float> tmp(a[i].bytes / 4);
            HIP_TRY(h, hipMemcpy(tmp.data(), d + a[i].off, a[i].bytes, hipMemcpyDeviceToHost));
            std::copy(tmp.begin(), tmp.end(), static_cast<double*>(a[i].host));
        }
        else if (how == Xfer::async) HIP_TRY(h, hipMemcpyAsync(a[i].host, d + a[i].off, a[i].bytes, hipMemcpyDeviceToHost, nullptr));
        else HIP_TRY(h, hipMemcpy(a[i].host, d + a[i].off, a[i].bytes, hipMemcpyDeviceToHost));
    }
    if (how == Xfer::async && sync) HIP_TRY(h, hipStreamSynchronize(nullptr));
    return WBCQP_OK;
}

// One staged call of a host-pointer entry point, blocking copies: the arrays of `up` go up, f(u, d) gets the device address of every array of up and of
// dn (null where the caller's pointer is null) and launches on the null stream, the device is waited for, the arrays of dn come down
template <int NU, int ND, typename F>
int staged_call(wbcqp_handle* h, Arr (&up)[NU], Arr (&dn)[ND], F&& f)
{
    WB_TRY(stage_begin(h, lay(up, NU), lay(dn, ND), false));
    WB_TRY(stage_up(h, h->stage_in.dev, up, NU, 0, Xfer::blocking));
    void *u[NU], *d[ND];
    for (int i = 0; i < NU; ++i) u[i] = up[i].host ? static_cast<char*>(h->stage_in.dev) + up[i].off : nullptr;
    for (int i = 0; i < ND; ++i) d[i] = dn[i].host ? static_cast<char*>(h->stage_out.dev) + dn[i].off : nullptr;
    WB_TRY(f(u, d));
    HIP_TRY(h, hipDeviceSynchronize());
    return stage_down(h, h->stage_out.dev, dn, ND, 0, Xfer::blocking);
}

// ---- the argument checks the entry points share ---------------------------------------------------------------------------------------------------
Slot* slot_with_model(wbcqp_handle* h, int slot)
{
    if (slot >= 0 && slot < WBCQP_MAX_STRUCTURES && h->slots[slot].set && h->slots[slot].has_model) return &h->slots[slot];
    fail(h, WBCQP_ERR_INVALID, "slot has no model (wbcqp_set_model)");
    return nullptr;
}

int need_state(wbcqp_handle* h, const TermsDev& T, const wbcqp_state* st)
{
    if (!st || !st->q || !st->v || (T.nref > 0 && !st->ref)) return fail(h, WBCQP_ERR_INVALID, "state arrays q / v / ref are required");
    return WBCQP_OK;
}

int need_rows(wbcqp_handle* h, const wbcqp_layout& L, const wbcqp_inputs* rows)
{
    if (!rows->M || !rows->h || (L.len_A && !rows->A) || (L.len_b1 && !rows->b1) || (L.len_Ac && !rows->Ac) || (L.len_bc && !rows->bc) ||
        (L.len_blb && (!rows->blb || !rows->bub)) || (L.len_Acop && !rows->Acop))
        return fail(h, WBCQP_ERR_INVALID, "row arrays M, h, A, b1, Ac, bc, blb, bub (Acop with a cop task) are required");
    return WBCQP_OK;
}

int need_tick_outputs(wbcqp_handle* h, int na, const wbcqp_outputs& out, const void* q_next, const void* v_next)
{
    if (!out.x || !out.status || !out.iters || (na > 0 && !out.tau) || !q_next || !v_next)
        return fail(h, WBCQP_ERR_INVALID, "x, tau, status, iters, q_next, v_next are required");
    return WBCQP_OK;
}

} // namespace
