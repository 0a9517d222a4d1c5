// wbcqp_api.hip -- C ABI (include/wbcqp.h) over the one-wavefront-per-QP kernel.
//
// Replaces, for B robot instances at once, the two calls the reference makes per control tick
// (/root/reference/src/controllers/controller.cpp:244 computeProblemData [assembly half] and :247
// solver_->solve) plus the decode at :250-251.  There is no CPU path in this library: without a
// gfx950 device wbcqp_create fails with WBCQP_ERR_NO_DEVICE.
//
// This file holds the exported entry points; the host code behind them is in the wbcqp_host_*.hpp headers, included here and nowhere else (the library
// stays ONE translation unit): the handle, the description of a call's arrays and the staging (handle), structure -> sizes and LDS layouts (derive),
// arguments -> kernel launches (launch), reference programs (program), the loops over ticks (rollout), the model queries on a fleet's states (queries),
// the torque monitor on a fleet's streams of joint torques and the stabiliser on its streams of foot wrenches (monitor).
#include "wbcqp_host_handle.hpp"
#include "wbcqp_host_derive.hpp"
#include "wbcqp_host_launch.hpp"
#include "wbcqp_host_program.hpp"
#include "wbcqp_host_rollout.hpp"
#include "wbcqp_host_queries.hpp"
#include "wbcqp_host_monitor.hpp"

namespace {

template <typename TI>
int solve_ragged(wbcqp_handle* h, int n_groups, const wbcqp_group* groups, hipStream_t hs)
{
    int total = 0, lds = 0, used = 0, total_small = 0, used_small = 0, spec = 0;
    GroupTable<TI> tab{}, tab_small{};
    const bool wave_per_qp = !(h->flags & WBCQP_FLAG_WORKGROUP_PER_QP) && !h->dbg; // (the stamped diagnostic build profiles the four-wave kernels)
    // the compact kernel runs a launch whose groups are all eligible; one group that is not puts the launch on the full layout
    bool compact = true;
    for (int g = 0; g < n_groups; ++g) {
        const wbcqp_group& G = groups[g];
        if (G.slot < 0 || G.slot >= WBCQP_MAX_STRUCTURES || !h->slots[G.slot].set)
            return fail(h, WBCQP_ERR_INVALID, "group uses a slot with no structure");
        if (G.batch > 0 && !(wave_per_qp && h->slots[G.slot].small) && !h->slots[G.slot].host_cp.compact) compact = false;
    }
    for (int g = 0; g < n_groups; ++g) {
        const wbcqp_group& G = groups[g];
        Slot& s = h->slots[G.slot];
        WB_TRY(check_io(h, s, G.batch, &G.in, &G.out));
        if (G.batch == 0) continue;
        bool user_capture = false; // (a caller capturing this very call into a graph of its own: no synchronisation there -- the cache waits for a plain launch)
        if (compact && s.ffc_dev && !s.ffc_built && !h->capturing) {
            hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(hs, &cst) != hipSuccess) (void)hipGetLastError();
            user_capture = cst != hipStreamCaptureStatusNone;
        }
        if (compact && s.ffc_dev && !s.ffc_built && !h->capturing && !user_capture && !(wave_per_qp && s.small))
            WB_TRY(build_ffcache(h, s, G.in.w, hs)); // the slot's first compact launch: the force blocks' factor for the weights of its first QP
        if (wave_per_qp && s.small) { // one wavefront per QP: a launch of their own (wbcqp_small.hpp)
            fill_group(tab_small.g[used_small++], s, false, G.batch, &G.in, &G.out);
            total_small += G.batch;
            continue;
        }
        fill_group(tab.g[used], s, compact, G.batch, &G.in, &G.out);
        tab.g[used].dbg = h->dbg;
        tab.g[used].warm = (h->flags & WBCQP_FLAG_WARM_START) ? 1 : 0;
        spec = s.spec; // (what choose_kernel makes of it where this group stays the only one)
        ++used;
        total += G.batch;
        const int need = compact ? s.lds_cp : s.lds_full;
        if (need > lds) lds = need;
    }
    tab.n = used;
    tab_small.n = used_small;
    if (h->lds_pad > 0) lds = std::min(lds + h->lds_pad, 160 * 1024);
    if (total_small > 0) WB_TRY(launch_small<TI>(h, tab_small, total_small, hs));
    const LaunchTable lt = launch_table(tab);
    const KernelChoice c = choose_kernel(LaunchFacts{compact, lds, lt.act_bounds, spec, used == 1}, h->flags, h->lds_pad);
    return launch(h, kernel_set<TI>(c.variant), c, lt, total, lds, hs);
}

} // namespace

extern "C" {

int wbcqp_version(void) { return WBCQP_VERSION; }

const char* wbcqp_last_error(const wbcqp_handle* handle) { return handle ? handle->err.c_str() : g_create_error.c_str(); }

int wbcqp_layout_of(const wbcqp_structure* st, wbcqp_layout* out)
{
    DevStruct D;
    HostBlocks HB;
    wbcqp_layout L;
    std::string why;
    int rc = derive(st, D, HB, L, why);
    if (rc != WBCQP_OK) return fail(nullptr, rc, why);
    DevStruct C;
    if (derive_compact(D, C)) {
        L.specialised = spec_of(C);
        set_lds(L, C.lds_doubles * 8, true, C.act_bounds != 0, L.specialised);
    }
    // how a row of kSpecDims (wbcqp_types.hpp) is made: the derived sizes and offsets of a stack, in the order of struct Dims
    if (std::getenv("WBCQP_DEBUG_DUMP_STRUCT") && C.compact)
        std::fprintf(stderr, "compact: nv %d na %d nc %d k %d n %d nu %d n_dense %d n_tasks %d n_sel %d n_bound %d act_bounds %d neq %d nin2 %d r1 %d max_iter %d "
                     "ldj %d ldb %d o_J %d o_R %d o_vec %d o_int %d o_pan %d act_off %d lds_doubles %d\n", C.nv, C.na, C.nc, C.k, C.n, C.nu, C.n_dense, C.n_tasks,
                     C.n_sel, C.n_bound, C.act_bounds, C.neq, C.nin2, C.r1, C.max_iter, C.ldj, C.ldb, C.o_J, C.o_R, C.o_vec, C.o_int, C.o_pan, C.act_off, C.lds_doubles);
    L.wave_per_qp = small_ok(D, HB) ? 1 : 0;
    if (out) *out = L;
    return WBCQP_OK;
}

int wbcqp_create(const wbcqp_desc* desc, wbcqp_handle** out)
{
    if (!desc || !out) return fail(nullptr, WBCQP_ERR_INVALID, "desc/out is NULL");
    if (desc->dtype != WBCQP_F64 && desc->dtype != WBCQP_F32) return fail(nullptr, WBCQP_ERR_INVALID, "unknown dtype");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, WBCQP_ERR_NO_DEVICE, "no HIP device visible: wbcqp has no CPU fallback");
    if (desc->device < 0 || desc->device >= count) return fail(nullptr, WBCQP_ERR_INVALID, "device ordinal out of range");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, desc->device);
    if (e != hipSuccess) return fail(nullptr, WBCQP_ERR_HIP, hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, WBCQP_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    e = hipSetDevice(desc->device);
    if (e != hipSuccess) return fail(nullptr, WBCQP_ERR_HIP, hipGetErrorString(e));
    wbcqp_handle* h = new wbcqp_handle();
    h->device = desc->device;
    h->dtype = desc->dtype;
    h->flags = desc->flags;
    h->n_cu = prop.multiProcessorCount;
    if (const char* pad = std::getenv("WBCQP_DEBUG_LDS_PAD")) h->lds_pad = std::atoi(pad);
    h->debug_launch = std::getenv("WBCQP_DEBUG_LAUNCH") != nullptr;
    if (const char* shape = std::getenv("WBCQP_HESSIAN_STORE")) h->hessian_wide = !std::strcmp(shape, "wide");
    h->no_ffcache = std::getenv("WBCQP_DEBUG_NO_FFCACHE") != nullptr;
    if (const char* ch = std::getenv("WBCQP_REFPROG_CHUNK")) h->ref_chunk = std::max(1, std::min(std::atoi(ch), 4096));
    *out = h;
    return WBCQP_OK;
}

int wbcqp_destroy(wbcqp_handle* h)
{
    if (!h) return WBCQP_OK;
    (void)hipSetDevice(h->device);
    for (auto& s : h->slots) release(s);
    if (h->stage_in.dev) (void)hipFree(h->stage_in.dev);
    if (h->stage_out.dev) (void)hipFree(h->stage_out.dev);
    if (h->pin_in.host) (void)hipHostFree(h->pin_in.host);
    if (h->pin_out.host) (void)hipHostFree(h->pin_out.host);
    if (h->roll_rec.dev) (void)hipFree(h->roll_rec.dev);
    if (h->roll_state.dev) (void)hipFree(h->roll_state.dev);
    for (auto& r : h->roll_subs) {
        if (r.stream) (void)hipStreamDestroy(r.stream);
        if (r.done) (void)hipEventDestroy(r.done);
        if (r.ord.order) (void)hipFree(r.ord.order);
        if (r.ord.queue) (void)hipFree(r.ord.queue);
    }
    if (h->roll_start) (void)hipEventDestroy(h->roll_start);
    if (h->roll_done) (void)hipEventDestroy(h->roll_done);
    for (auto& mz : h->roll_meas) {
        if (mz.t0) (void)hipEventDestroy(mz.t0);
        if (mz.t1) (void)hipEventDestroy(mz.t1);
    }
    for (auto& ss : h->streams) {
        if (ss.ord.order) (void)hipFree(ss.ord.order);
        if (ss.ord.queue) (void)hipFree(ss.ord.queue);
    }
    for (auto& mp : h->mix_plan) {
        if (mp.pin.host) (void)hipHostFree(mp.pin.host);
        if (mp.dev) (void)hipFree(mp.dev);
        if (mp.done) (void)hipEventDestroy(mp.done);
    }
    if (h->mix_rec.dev) (void)hipFree(h->mix_rec.dev);
    if (h->mix_state.dev) (void)hipFree(h->mix_state.dev);
    if (h->mix_done) (void)hipEventDestroy(h->mix_done);
    for (auto& pu : h->prog_up) {
        if (pu.pin.host) (void)hipHostFree(pu.pin.host);
        if (pu.dev) (void)hipFree(pu.dev);
        if (pu.done) (void)hipEventDestroy(pu.done);
    }
    if (h->roll_ref.dev) (void)hipFree(h->roll_ref.dev);
    if (h->mix_ref.dev) (void)hipFree(h->mix_ref.dev);
    delete h;
    return WBCQP_OK;
}

int wbcqp_set_structure(wbcqp_handle* h, int slot, const wbcqp_structure* st)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (slot < 0 || slot >= WBCQP_MAX_STRUCTURES) return fail(h, WBCQP_ERR_INVALID, "slot out of range");
    DevStruct D;
    HostBlocks HB;
    wbcqp_layout L;
    std::string why;
    int rc = derive(st, D, HB, L, why);
    if (rc != WBCQP_OK) return fail(h, rc, why);
    D.ffc = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    Slot& s = h->slots[slot];
    release(s);
    s.ffc_dev = nullptr;
    s.ffc_built = false;
    const int nc = D.nc;
    // F'F and F' of the force-regularisation block, F = diag(w_f) T  (6 x 12)
    std::vector<double> ftf((size_t)nc * 144 + 1, 0.0), ft((size_t)nc * 72 + 1, 0.0);
    for (int c = 0; c < nc; ++c) {
        const double* F = st->forcereg_mat + (size_t)c * 72;
        for (int a = 0; a < 12; ++a) {
            for (int b = 0; b < 12; ++b) {
                double acc = 0.0;
                for (int q = 0; q < 6; ++q) acc += F[q * 12 + a] * F[q * 12 + b];
                ftf[(size_t)c * 144 + a * 12 + b] = acc;
            }
            for (int q = 0; q < 6; ++q) ft[(size_t)c * 72 + a * 6 + q] = F[q * 12 + a];
        }
    }
#define UP(field, src, count)                                                   \
    do {                                                                        \
        int rc_ = upload(h, s, src, (size_t)(count), &D.field);                 \
        if (rc_ != WBCQP_OK) { release(s); return rc_; }                        \
    } while (0)
    UP(dense_row_task, st->dense_row_task, D.n_dense);
    UP(sel_col, st->sel_col, D.n_sel);
    UP(sel_task, st->sel_task, D.n_sel);
    UP(forcereg_task, st->forcereg_task, nc);
    UP(bound_col, st->bound_col, D.n_bound);
    UP(acteq_joint, st->acteq_joint, D.n_acteq);
    UP(acteq_scale, st->acteq_scale, D.n_acteq);
    UP(force_gen, st->force_gen, nc * 72);
    UP(ftf, ftf.data(), nc * 144);
    UP(ft, ft.data(), nc * 72);
    UP(fric_mat, st->fric_mat, nc * 17 * 12);
    UP(fric_lb, st->fric_lb, nc * 17);
    UP(fric_ub, st->fric_ub, nc * 17);
    {
        std::vector<int> meta((size_t)D.nin2 + 1, 0);
        for (int b = 0; b < HB.n_blocks; ++b) {
            const int rows = HB.blk_rows[b], off = HB.blk_off[b], kind = HB.blk_kind[b];
            for (int r = 0; r < rows; ++r) {
                const int col = (kind == WBCQP_INEQ_BOUNDS) ? st->bound_col[r] : 0;
                const int ct = (kind == WBCQP_INEQ_FORCE) ? HB.blk_arg[b] : 0;
                meta[off + r] = row_meta_pack(kind, 0, r, ct, col);
                meta[off + rows + r] = row_meta_pack(kind, 1, r, ct, col);
            }
        }
        UP(rowmeta, meta.data(), D.nin2);
    }
    {
        std::vector<unsigned> mp((size_t)D.nv * (D.nv + 1) / 2 + 1, 0u);
        for (int i = 0; i < D.nv; ++i)
            for (int j = 0; j <= i; ++j)
                mp[(size_t)i * (i + 1) / 2 + j] = (unsigned)(i * D.ldm + j) | ((unsigned)(j * D.ldm + i) << 16);
        UP(mpack, mp.data(), D.nv * (D.nv + 1) / 2);
    }
    {
        std::vector<unsigned> ap((size_t)D.n_dense * D.nv + 1, 0u);
        for (int r = 0; r < D.n_dense; ++r)
            for (int col = 0; col < D.nv; ++col) ap[(size_t)r * D.nv + col] = (unsigned)(r * 64 + ((col >> 5) & 1) * 32 + (col & 15) * 2 + ((col >> 4) & 1)); // see wbcqp_types.hpp, apack
        UP(apack, ap.data(), D.n_dense * D.nv);
    }
    {
        std::vector<unsigned> cpk((size_t)nc * 6 * D.nv + 1, 0u);
        for (int rr = 0; rr < nc * 6; ++rr)
            for (int kk = 0; kk < D.nv; ++kk) cpk[(size_t)rr * D.nv + kk] = (unsigned)(kk * D.ldb + D.nu + rr);
        UP(acpack, cpk.data(), nc * 6 * D.nv);
    }
#undef UP
    s.host = D;
    s.sel_col_h.assign(st->sel_col, st->sel_col + D.n_sel);
    s.force_gen_h.assign(st->force_gen, st->force_gen + (size_t)nc * 72);
    s.forcereg_h.assign(st->forcereg_mat, st->forcereg_mat + (size_t)nc * 72);
    s.lds_full = D.lds_doubles * 8;
    s.lds_cp = 0;
    s.host_cp = DevStruct{};
    if (!(h->flags & WBCQP_FLAG_FULL_LDS) && derive_compact(D, s.host_cp)) {
        s.lds_cp = s.host_cp.lds_doubles * 8;
        set_lds(L, s.lds_cp, true, s.host_cp.act_bounds != 0, spec_of(s.host_cp));
        if (nc > 0 && !h->no_ffcache) { // room for the force blocks' factor (DevStruct::ffc), invalid (weight NaN) until the slot's first launch makes it
            std::vector<double> init((size_t)nc * kFfcStride, 0.0);
            for (int c = 0; c < nc; ++c) init[(size_t)c * kFfcStride] = std::numeric_limits<double>::quiet_NaN();
            const double* dev = nullptr;
            rc = upload(h, s, init.data(), init.size(), &dev);
            if (rc != WBCQP_OK) { release(s); return rc; }
            s.ffc_dev = const_cast<double*>(dev);
            s.host_cp.ffc = dev;
        }
    }
    s.small = small_ok(D, HB);
    L.wave_per_qp = s.small ? 1 : 0;
    s.spec = s.host_cp.compact ? spec_of(s.host_cp) : 0;
    L.specialised = s.spec;
    s.layout = L;
    s.set = true;
    return WBCQP_OK;
}

int wbcqp_solve_ragged(wbcqp_handle* h, int n_groups, const wbcqp_group* groups, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (n_groups < 0 || n_groups > kMaxGroups) return fail(h, WBCQP_ERR_INVALID, "n_groups must be in [0, 8]");
    if (n_groups > 0 && !groups) return fail(h, WBCQP_ERR_INVALID, "groups is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    return with_dtype(h, [&](auto tag) -> int { return solve_ragged<WB_TI(tag)>(h, n_groups, groups, static_cast<hipStream_t>(stream)); });
}

int wbcqp_solve_batch(wbcqp_handle* h, int slot, int batch, const wbcqp_inputs* in, const wbcqp_outputs* out, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (batch == 0) return WBCQP_OK;
    if (!in || !out) return fail(h, WBCQP_ERR_INVALID, "inputs/outputs struct is NULL");
    wbcqp_group G;
    G.slot = slot;
    G.batch = batch;
    G.in = *in;
    G.out = *out;
    return wbcqp_solve_ragged(h, 1, &G, stream);
}

int wbcqp_task_costs(wbcqp_handle* h, int slot, int batch, const wbcqp_inputs* rows, const void* x, const void* tau, void* cost, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (slot < 0 || slot >= WBCQP_MAX_STRUCTURES || !h->slots[slot].set) return fail(h, WBCQP_ERR_INVALID, "slot has no structure");
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (batch == 0) return WBCQP_OK;
    const Slot& s = h->slots[slot];
    const wbcqp_layout& L = s.layout;
    if (!rows || (L.len_A && !rows->A) || (L.len_b1 && !rows->b1) || (L.len_Acop && !rows->Acop))
        return fail(h, WBCQP_ERR_INVALID, "rows A, b1 (Acop with a cop task) are required");
    if (!x || !cost) return fail(h, WBCQP_ERR_INVALID, "x / cost is NULL");
    if (s.host.n_acteq > 0 && !tau) return fail(h, WBCQP_ERR_INVALID, "tau is required: the stack has a torque task");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_costs(h, s, batch, rows->A, rows->b1, rows->Acop, x, L.n, tau, cost, L.len_w, nullptr, static_cast<hipStream_t>(stream));
}

int wbcqp_solve_batch_host(wbcqp_handle* h, int slot, int batch, const wbcqp_inputs* in, const wbcqp_outputs* out)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (slot < 0 || slot >= WBCQP_MAX_STRUCTURES || !h->slots[slot].set) return fail(h, WBCQP_ERR_INVALID, "slot has no structure");
    const Slot& s = h->slots[slot];
    int rc = check_io(h, s, batch, in, out);
    if (rc != WBCQP_OK || batch == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const FieldBytes fb = field_bytes(s, elem_size(h));
    const Io host(in, out);
    constexpr Field kOut[7] = {F_x, F_tau, F_obj, F_status, F_iters, F_nact, F_amask};
    Arr ai[12], ao[7];
    const size_t in_bytes = lay(fb, batch, kInputFields, 12, host, ai);
    const size_t out_end = lay(fb, batch, kOut, 7, host, ao);
    const size_t out_bytes = ao[6].off + ao[6].bytes + 256;
    const bool packed = in_bytes + ao[6].bytes <= kPackedBytes && out_bytes <= kPackedBytes;
    const Xfer how = packed ? Xfer::packed : Xfer::async;
    WB_TRY(stage_begin(h, in_bytes, out_end, packed));
    WB_TRY(stage_up(h, h->stage_in.dev, ai, 12, in_bytes, how));
    Io d;
    point(d, h->stage_in.dev, ai, 12);
    point(d, h->stage_out.dev, ao, 7);
    if (!out->active_mask) d.p[F_amask] = nullptr;
    else WB_TRY(stage_up(h, h->stage_out.dev, &ao[6], 1, 0, Xfer::async)); // in/out: the hint goes up (zeros where the caller has none), the solution's active set comes back
    const wbcqp_inputs di = d.inputs();
    const wbcqp_outputs dso = d.outputs();
    WB_TRY(wbcqp_solve_batch(h, slot, batch, &di, &dso, nullptr));
    return stage_down(h, h->stage_out.dev, ao, 7, out_bytes, how);
}

int wbcqp_solve_dense(wbcqp_handle* h, int batch, int n, int neq, int nin, int max_iter, const wbcqp_dense_inputs* in,
                      const wbcqp_outputs* out, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (batch < 0 || n <= 0 || neq < 0 || nin < 0) return fail(h, WBCQP_ERR_INVALID, "bad batch / n / neq / nin");
    if (batch == 0) return WBCQP_OK;
    if (!in || !out) return fail(h, WBCQP_ERR_INVALID, "inputs/outputs struct is NULL");
    if (!in->H || !in->g || (neq > 0 && (!in->CE || !in->ce0)) || (nin > 0 && (!in->CI || !in->ci0)))
        return fail(h, WBCQP_ERR_INVALID, "dense QP: H, g and the constraint arrays of non-empty blocks are required");
    if (!out->x || !out->status || !out->iters) return fail(h, WBCQP_ERR_INVALID, "output arrays x, status, iters are required");
    if (n > kDenseMaxVars || nin > kDenseMaxIneq || neq > n) return fail(h, WBCQP_ERR_UNSUPPORTED, "dense QP: n <= 126, nin <= 512, neq <= n");
    DenseArgs a{};
    a.n = n; a.neq = neq; a.nin = nin; a.ldj = odd(n);
    int o = 0;
    auto take = [&](int count) { int at = o; o += (count + 1) & ~1; return at; };
    a.blocked_eq = (neq >= 1 && neq <= 22 && n <= 80) ? 1 : 0;
    a.ldb = 2 * odd((4 * ((neq + 3) / 4) + 1) / 2); // as the structured layout's (derive): rows stay 16-byte aligned for the 4-wide column groups
    a.o_J = take(n * a.ldj);
    int rsize = n * (n + 3) / 2 + 2;
    if (a.blocked_eq && 256 + (n + 17) * a.ldb + 8 > rsize) rsize = 256 + (n + 17) * a.ldb + 8; // B of the blocked equality phase
    a.o_R = take(rsize);
    a.o_vec = take(V_COUNT * kSlot);
    a.o_eqw = take(a.blocked_eq ? (n + 1) * a.ldb + 8 : 0);
    a.o_eqt = take(a.blocked_eq ? neq * (neq + 1) + 4 * neq + 16 : 0);
    a.o_int = o;
    o += kIntCount / 2 + 2;
    const int lds_bytes = o * 8;
    if (lds_bytes > 160 * 1024) return fail(h, WBCQP_ERR_UNSUPPORTED, "dense QP does not fit the 160 KiB LDS of one CU (n <= 99)");
    a.max_iter = max_iter > 0 ? max_iter : 1000;
    a.count = batch;
    a.H = in->H; a.g = in->g; a.CE = in->CE; a.ce0 = in->ce0; a.CI = in->CI; a.ci0 = in->ci0;
    a.x = out->x; a.objective = out->objective; a.status = out->status; a.iters = out->iters; a.n_active = out->n_active;
    HIP_TRY(h, hipSetDevice(h->device));
    if (lds_bytes > h->dense_max_lds) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_dense_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_dense_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        h->dense_max_lds = lds_bytes;
    }
    hipStream_t hs = static_cast<hipStream_t>(stream);
    return with_dtype(h, [&](auto tag) -> int {
        hipLaunchKernelGGL(solve_dense_kernel<WB_TI(tag)>, dim3(batch), dim3(kThreads), lds_bytes, hs, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

int wbcqp_solve_dense_host(wbcqp_handle* h, int batch, int n, int neq, int nin, int max_iter, const wbcqp_dense_inputs* in,
                           const wbcqp_dense_output** result)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!in || !result) return fail(h, WBCQP_ERR_INVALID, "inputs / result is NULL");
    if (batch <= 0 || n <= 0 || neq < 0 || nin < 0) return fail(h, WBCQP_ERR_INVALID, "bad batch / n / neq / nin");
    *result = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    const bool f32 = h->dtype != WBCQP_F64;
    const size_t es = f32 ? 4 : 8;
    const size_t B = (size_t)batch;
    Arr up[6] = {{-1, const_cast<void*>(in->H), (size_t)n * n * B * es, 0},    {-1, const_cast<void*>(in->g), (size_t)n * B * es, 0},
                 {-1, const_cast<void*>(in->CE), (size_t)neq * n * B * es, 0}, {-1, const_cast<void*>(in->ce0), (size_t)neq * B * es, 0},
                 {-1, const_cast<void*>(in->CI), (size_t)nin * n * B * es, 0}, {-1, const_cast<void*>(in->ci0), (size_t)nin * B * es, 0}};
    Arr dn[5] = {{F_x, nullptr, (size_t)n * B * es, 0}, {F_obj, nullptr, B * es, 0}, {F_status, nullptr, B * 4, 0}, {F_iters, nullptr, B * 4, 0}, {F_nact, nullptr, B * 4, 0}};
    const size_t in_bytes = lay(up, 6), out_bytes = lay(dn, 5);
    for (const Arr& u : up)
        if (u.bytes != 0 && !u.host) return fail(h, WBCQP_ERR_INVALID, "dense QP: a required input array is NULL");
    // a small batch (the reference's own use: one QP per call) crosses PCIe as ONE page-locked copy each way, as in
    // wbcqp_solve_batch_host: six pageable copies up and five synchronous ones down were a quarter of a single QP's wall time.
    // The caller's arrays are double (Eigen); an F32 handle carries float at the device boundary
    const bool packed = !f32 && in_bytes <= kPackedBytes && out_bytes <= kPackedBytes;
    WB_TRY(stage_begin(h, in_bytes, out_bytes, packed));
    WB_TRY(stage_up(h, h->stage_in.dev, up, 6, in_bytes, packed ? Xfer::packed : (f32 ? Xfer::blocking_float : Xfer::async)));
    char* din = static_cast<char*>(h->stage_in.dev);
    wbcqp_dense_inputs di = {din + up[0].off, din + up[1].off, neq ? din + up[2].off : nullptr, neq ? din + up[3].off : nullptr,
                             nin ? din + up[4].off : nullptr, nin ? din + up[5].off : nullptr};
    Io d;
    point(d, h->stage_out.dev, dn, 5);
    const wbcqp_outputs dso = d.outputs();
    WB_TRY(wbcqp_solve_dense(h, batch, n, neq, nin, max_iter, &di, &dso, nullptr));
    h->dense_x.assign((size_t)n * B, 0.0);
    h->dense_obj.assign(B, 0.0);
    h->dense_status.assign(B, WBCQP_HQP_UNKNOWN);
    h->dense_iters.assign(B, 0);
    h->dense_nact.assign(B, 0);
    dn[0].host = h->dense_x.data(); dn[1].host = h->dense_obj.data(); dn[2].host = h->dense_status.data(); dn[3].host = h->dense_iters.data();
    dn[4].host = h->dense_nact.data();
    WB_TRY(stage_down(h, h->stage_out.dev, dn, 5, out_bytes, packed ? Xfer::packed : (f32 ? Xfer::blocking_float : Xfer::blocking)));
    h->dense_out = {batch, n, h->dense_x.data(), h->dense_status.data(), h->dense_iters.data(), h->dense_obj.data(), h->dense_nact.data()};
    *result = &h->dense_out;
    return WBCQP_OK;
}

// RCCL is resolved at run time from whatever librccl the process already has (PyTorch's, or the
// system one): the library itself carries no link-time dependency on it.
int wbcqp_allgather_tau(wbcqp_handle* h, void* comm, const void* send, void* recv, size_t count, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!comm || !send || !recv) return fail(h, WBCQP_ERR_INVALID, "comm/send/recv is NULL");
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, void*);
    static allgather_fn fn = nullptr;
    if (!fn) {
        void* sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
        if (!sym) {
            void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (lib) sym = dlsym(lib, "ncclAllGather");
        }
        if (!sym) return fail(h, WBCQP_ERR_RCCL, "ncclAllGather not found (librccl not loadable)");
        fn = reinterpret_cast<allgather_fn>(sym);
    }
    const int nccl_dtype = (h->dtype == WBCQP_F64) ? 8 /* ncclFloat64 */ : 7 /* ncclFloat32 */;
    int rc = fn(send, recv, count, nccl_dtype, comm, stream);
    if (rc != 0) return fail(h, WBCQP_ERR_RCCL, "ncclAllGather failed with code " + std::to_string(rc));
    return WBCQP_OK;
}

// Diagnostic hook, not part of include/wbcqp.h: per-QP phase cycle counters ([batch][20] int64, device memory)
// are written only by a library built with -DWBCQP_STAMPS (inria_wbc_amd/build.py --stamps); single group only.
int wbcqp_launch_order(wbcqp_handle* h, int32_t* order, int32_t capacity, int32_t* packed)
{
    if (!h || !order || capacity < 0) return WBCQP_ERR_INVALID;
    if (packed) *packed = 0;
    if (h->last_stream < 0 || h->last_stream >= (int)h->streams.size()) return 0;
    const OrderState& o = h->streams[h->last_stream].ord; // the stream of the most recent launch
    if (!o.order || o.total <= 0) return 0;
    if (capacity < o.total) return fail(h, WBCQP_ERR_INVALID, "wbcqp_launch_order: capacity below the order's length");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(order, o.order + (o.packed ? o.cap : 0), sizeof(int) * (size_t)o.total, hipMemcpyDeviceToHost));
    if (packed) *packed = o.packed ? 1 : 0;
    return o.total;
}

#ifdef WBCQP_STAMPS
// exported by the DIAGNOSTIC library only (libwbcqp_stamps.so, inria_wbc_amd/build.py --stamps): the product library exports exactly
// what include/wbcqp.h declares
int wbcqp_debug_set_stamp_buffer(wbcqp_handle* h, void* dev_ptr)
{
    if (!h) return WBCQP_ERR_INVALID;
    h->dbg = static_cast<long long*>(dev_ptr);
    return WBCQP_OK;
}
#endif

int wbcqp_integrate(wbcqp_handle* h, int batch, int nv, int floating_base, double dt, const void* q, const void* dq, const void* x,
                    int ldx, const int32_t* status, void* q_next, void* v_next, void* q_solver, void* stream)
{
    return integrate_impl(h, batch, nv, floating_base, dt, q, dq, x, ldx, status, q_next, v_next, q_solver, stream, RollAcc{});
}

int wbcqp_integrate_host(wbcqp_handle* h, int batch, int nv, int floating_base, double dt, const void* q, const void* dq,
                         const void* x, int ldx, const int32_t* status, void* q_next, void* v_next, void* q_solver)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (batch < 0 || nv <= 0 || ldx < nv) return fail(h, WBCQP_ERR_INVALID, "bad batch / nv / ldx");
    if (floating_base && nv < 6) return fail(h, WBCQP_ERR_INVALID, "a floating base needs nv >= 6");  // (before anything is staged)
    if (batch == 0) return WBCQP_OK;
    if (!q || !dq || !x || !q_next || !v_next) return fail(h, WBCQP_ERR_INVALID, "q / dq / x / q_next / v_next is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h);
    const int nq = floating_base ? nv + 1 : nv;
    const size_t nqb = (size_t)batch * nq * es, nvb = (size_t)batch * nv * es;
    Arr up[4] = {{F_q, const_cast<void*>(q), nqb, 0}, {F_v, const_cast<void*>(dq), nvb, 0}, {F_x, const_cast<void*>(x), (size_t)batch * ldx * es, 0},
                 {F_status, const_cast<int32_t*>(status), (size_t)batch * 4, 0}};
    Arr dn[3] = {{F_qn, q_next, nqb, 0}, {F_vn, v_next, nvb, 0}, {F_qs, q_solver, nvb, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return wbcqp_integrate(h, batch, nv, floating_base, dt, u[0], u[1], u[2], ldx, static_cast<const int32_t*>(u[3]), d[0], d[1], d[2], nullptr);
    });
}

int wbcqp_check_model(const wbcqp_structure* st, const wbcqp_model* md, const wbcqp_taskmap* tm, int32_t* lds_bytes)
{
    DevStruct D;
    HostBlocks HB;
    wbcqp_layout L;
    std::string why;
    int rc = derive(st, D, HB, L, why);
    if (rc != WBCQP_OK) return fail(nullptr, rc, why);
    TermsDev T{};
    std::vector<int> ipool;
    std::vector<double> dpool;
    if ((D.n_sel > 0 && !st->sel_col) || (D.nc > 0 && !st->force_gen)) return fail(nullptr, WBCQP_ERR_INVALID, "sel_col / force_gen is NULL");
    rc = derive_terms(nullptr, D, st->sel_col, st->force_gen, md, tm, T, ipool, dpool);
    if (rc == WBCQP_OK && lds_bytes) *lds_bytes = T.lds_doubles * 8;
    return rc;
}

int wbcqp_set_model(wbcqp_handle* h, int slot, const wbcqp_model* md, const wbcqp_taskmap* tm)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (slot < 0 || slot >= WBCQP_MAX_STRUCTURES || !h->slots[slot].set) return fail(h, WBCQP_ERR_INVALID, "slot has no structure");
    Slot& s = h->slots[slot];
    TermsDev T{};
    std::vector<int> ipool;
    std::vector<double> dpool;
    int rc = derive_terms(h, s.host, s.sel_col_h.data(), s.force_gen_h.data(), md, tm, T, ipool, dpool);
    if (rc != WBCQP_OK) return rc;
    const int o = T.lds_doubles;
    HIP_TRY(h, hipSetDevice(h->device));
    release_model(s);
    void *di = nullptr, *dd = nullptr;
    HIP_TRY(h, hipMalloc(&di, ipool.size() * sizeof(int)));
    s.model_allocs.push_back(di);
    HIP_TRY(h, hipMalloc(&dd, dpool.size() * sizeof(double)));
    s.model_allocs.push_back(dd);
    HIP_TRY(h, hipMemcpy(di, ipool.data(), ipool.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(dd, dpool.data(), dpool.size() * sizeof(double), hipMemcpyHostToDevice));
    T.ipool = static_cast<const int*>(di);
    T.dpool = static_cast<const double*>(dd);
    if (o * 8 > 64 * 1024) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&terms_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, o * 8));
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&terms_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, o * 8));
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&terms_kernel<double, true>), hipFuncAttributeMaxDynamicSharedMemorySize, o * 8));
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&terms_kernel<float, true>), hipFuncAttributeMaxDynamicSharedMemorySize, o * 8));
    }
    s.terms = T;
    s.has_model = true;
    const int nb = md->nbody;
    s.tree.assign({(double)nb, (double)(md->floating_base ? 1 : 0), md->gravity[0], md->gravity[1], md->gravity[2]});
    for (int i = 0; i < nb; ++i) {
        s.tree.push_back((double)md->parent[i]);
        s.tree.push_back((double)md->jtype[i]);
    }
    s.tree.insert(s.tree.end(), md->placement, md->placement + 12 * nb);
    s.tree.insert(s.tree.end(), md->inertia, md->inertia + 10 * nb);
    s.frame_body_h.assign(md->frame_body, md->frame_body + md->nframe); // (derive_terms has checked the table)
    s.frame_place_h.assign(md->frame_placement, md->frame_placement + (size_t)12 * md->nframe);
    return WBCQP_OK;
}

int wbcqp_set_force_references(wbcqp_handle* h, int slot, const int32_t* force_ref, const double* weight)
{
    if (!h) return WBCQP_ERR_INVALID;
    Slot* s = slot_with_model(h, slot);
    if (!s) return WBCQP_ERR_INVALID;
    std::vector<int> off;
    WB_TRY(check_force_references(h, *s, force_ref, weight, &off));
    TermsDev& T = s->terms;
    const int nc = T.nc;
    if (nc == 0) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    // (the two tables were given room by wbcqp_set_model; a blocking copy: launches already queued have finished reading the old ones)
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(const_cast<int*>(T.ipool) + T.i_fref, off.data(), (size_t)nc * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(const_cast<double*>(T.dpool) + T.d_fref_w, weight, (size_t)6 * nc * sizeof(double), hipMemcpyHostToDevice));
    T.n_fref = std::any_of(off.begin(), off.end(), [](int o) { return o >= 0; }) ? 6 * nc : 0;
    return WBCQP_OK;
}

int wbcqp_set_observed_frames(wbcqp_handle* h, int slot, int n_frames, const int32_t* frames)
{
    return set_frame_selection(h, slot, &Slot::observed, n_frames, frames, WBCQP_MAX_OBSERVED, "an observed frame", "the observed frames");
}

int wbcqp_observe_acom(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, void* acom, void* stream)
{
    const Slot* s = nullptr;
    const wbcqp_observables none = {};
    if (acom && !out) out = &none; // (acom alone)
    WB_TRY(check_observe(h, slot, batch, q, v, out, acom, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_observe(h, *s, batch, q, v, *out, acom, static_cast<hipStream_t>(stream));
}

int wbcqp_observe(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, void* stream)
{
    return wbcqp_observe_acom(h, slot, batch, q, v, out, nullptr, stream);
}

int wbcqp_observe_acom_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, void* acom)
{
    const Slot* s = nullptr;
    const wbcqp_observables none = {};
    if (acom && !out) out = &none;
    WB_TRY(check_observe(h, slot, batch, q, v, out, acom, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nf = (size_t)s->observed.n;
    Arr up[2] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, const_cast<void*>(v), B * s->terms.nv * es, 0}};
    Arr dn[5] = {{-1, out->com, B * 3 * es, 0}, {-1, out->vcom, B * 3 * es, 0}, {-1, out->placement, B * nf * 12 * es, 0}, {-1, out->velocity, B * nf * 6 * es, 0},
                 {-1, acom, B * 3 * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_observe(h, *s, batch, u[0], u[1], wbcqp_observables{d[0], d[1], d[2], d[3]}, d[4], nullptr);
    });
}

int wbcqp_observe_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out)
{
    return wbcqp_observe_acom_host(h, slot, batch, q, v, out, nullptr);
}

int wbcqp_set_collision_spheres(wbcqp_handle* h, int slot, const wbcqp_sphere_model* sm) { return set_collision_spheres(h, slot, sm); }

int wbcqp_check_collisions(wbcqp_handle* h, int slot, int batch, const void* q, const wbcqp_collisions* out, void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_collisions(h, slot, batch, q, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_collisions(h, *s, batch, q, *out, static_cast<hipStream_t>(stream));
}

int wbcqp_check_collisions_host(wbcqp_handle* h, int slot, int batch, const void* q, const wbcqp_collisions* out)
{
    const Slot* s = nullptr;
    WB_TRY(check_collisions(h, slot, batch, q, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, ns = (size_t)s->spheres.n_spheres;
    Arr up[1] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}};
    Arr dn[5] = {{-1, out->colliding, B * 4, 0}, {-1, out->first_pair, B * 8, 0}, {-1, out->n_pairs, B * 4, 0}, {-1, out->clearance, B * es, 0},
                 {-1, out->centres, B * ns * 3 * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        const wbcqp_collisions dev = {static_cast<int32_t*>(d[0]), static_cast<int32_t*>(d[1]), static_cast<int32_t*>(d[2]), d[3], d[4]};
        return launch_collisions(h, *s, batch, u[0], dev, nullptr);
    });
}

int wbcqp_set_wrench_frames(wbcqp_handle* h, int slot, int n_frames, const int32_t* frames)
{
    return set_frame_selection(h, slot, &Slot::wrench, n_frames, frames, WBCQP_MAX_WRENCH_FRAMES, "a wrench frame", "the wrench frames");
}

int wbcqp_inverse_dynamics(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench, void* tau,
                           void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_inverse_dynamics(h, slot, batch, q, a, lda, wrench, tau, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_inverse_dynamics(h, *s, batch, q, v, a, lda, wrench, tau, static_cast<hipStream_t>(stream));
}

int wbcqp_inverse_dynamics_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench, void* tau)
{
    const Slot* s = nullptr;
    WB_TRY(check_inverse_dynamics(h, slot, batch, q, a, lda, wrench, tau, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv;
    // (a: rows lda apart, the last one nv long -- nothing behind it is the caller's to give)
    Arr up[4] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, const_cast<void*>(v), B * nv * es, 0},
                 {-1, const_cast<void*>(a), ((B - 1) * (size_t)(a ? lda : 0) + nv) * es, 0}, {-1, const_cast<void*>(wrench), B * s->wrench.n * 6 * es, 0}};
    Arr dn[1] = {{-1, tau, B * nv * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_inverse_dynamics(h, *s, batch, u[0], u[1], u[2], lda, u[3], d[0], nullptr);
    });
}

int wbcqp_mass_matrix(wbcqp_handle* h, int slot, int batch, const void* q, void* M, void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_mass_matrix(h, slot, batch, q, M, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_mass_matrix(h, *s, batch, q, M, static_cast<hipStream_t>(stream));
}

int wbcqp_mass_matrix_host(wbcqp_handle* h, int slot, int batch, const void* q, void* M)
{
    const Slot* s = nullptr;
    WB_TRY(check_mass_matrix(h, slot, batch, q, M, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv;
    Arr up[1] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}};
    Arr dn[1] = {{-1, M, B * nv * nv * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) { return launch_mass_matrix(h, *s, batch, u[0], d[0], nullptr); });
}

int wbcqp_forward_dynamics(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* tau, int ldt, const void* wrench,
                           const double* damping, void* a, int32_t* info, void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_forward_dynamics(h, slot, batch, q, tau, ldt, wrench, damping, a, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_forward_dynamics(h, *s, batch, q, v, tau, ldt, wrench, damping, a, info, static_cast<hipStream_t>(stream));
}

int wbcqp_forward_dynamics_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* tau, int ldt, const void* wrench,
                                const double* damping, void* a, int32_t* info)
{
    const Slot* s = nullptr;
    WB_TRY(check_forward_dynamics(h, slot, batch, q, tau, ldt, wrench, damping, a, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv;
    // (tau: rows ldt apart, the last one nv long -- nothing behind it is the caller's to give)
    Arr up[4] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, const_cast<void*>(v), B * nv * es, 0},
                 {-1, const_cast<void*>(tau), ((B - 1) * (size_t)(tau ? ldt : 0) + nv) * es, 0}, {-1, const_cast<void*>(wrench), B * s->wrench.n * 6 * es, 0}};
    Arr dn[2] = {{-1, a, B * nv * es, 0}, {-1, info, B * 4, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_forward_dynamics(h, *s, batch, u[0], u[1], u[2], ldt, u[3], damping, d[0], static_cast<int32_t*>(d[1]), nullptr);
    });
}

int wbcqp_spd_commands(wbcqp_handle* h, int slot, int batch, const wbcqp_spd* law, const void* q, const void* v, const void* target, int ldtarget,
                       const void* wrench, void* commands, void* qddot, int32_t* info, void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_spd_commands(h, slot, batch, law, q, target, ldtarget, wrench, commands, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_spd_commands(h, *s, batch, *law, q, v, target, ldtarget, wrench, commands, qddot, info, static_cast<hipStream_t>(stream));
}

int wbcqp_spd_commands_host(wbcqp_handle* h, int slot, int batch, const wbcqp_spd* law, const void* q, const void* v, const void* target, int ldtarget,
                            const void* wrench, void* commands, void* qddot, int32_t* info)
{
    const Slot* s = nullptr;
    WB_TRY(check_spd_commands(h, slot, batch, law, q, target, ldtarget, wrench, commands, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv, na = nv - (s->terms.floating_base ? 6 : 0);
    // (target: rows ldtarget apart, the last one na long)
    Arr up[4] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, const_cast<void*>(v), B * nv * es, 0},
                 {-1, const_cast<void*>(target), ((B - 1) * (size_t)ldtarget + na) * es, 0}, {-1, const_cast<void*>(wrench), B * s->wrench.n * 6 * es, 0}};
    Arr dn[3] = {{-1, commands, B * nv * es, 0}, {-1, qddot, B * nv * es, 0}, {-1, info, B * 4, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_spd_commands(h, *s, batch, *law, u[0], u[1], u[2], ldtarget, u[3], d[0], d[1], static_cast<int32_t*>(d[2]), nullptr);
    });
}

int wbcqp_set_jacobian_frames(wbcqp_handle* h, int slot, int n_frames, const int32_t* frames)
{
    return set_frame_selection(h, slot, &Slot::jacobian, n_frames, frames, WBCQP_MAX_JACOBIAN_FRAMES, "a jacobian frame", "the jacobian frames");
}

int wbcqp_jacobians(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, int reference_frame, const wbcqp_jacobian_outputs* out, void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_jacobians(h, slot, batch, q, v, reference_frame, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_jacobians(h, *s, batch, q, v, reference_frame, *out, static_cast<hipStream_t>(stream));
}

int wbcqp_jacobians_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, int reference_frame, const wbcqp_jacobian_outputs* out)
{
    const Slot* s = nullptr;
    WB_TRY(check_jacobians(h, slot, batch, q, v, reference_frame, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv, nf = (size_t)s->jacobian.n;
    // (v goes up only where the kernel reads it)
    Arr up[2] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, (out->drift || out->dAgv) ? const_cast<void*>(v) : nullptr, B * nv * es, 0}};
    Arr dn[5] = {{-1, out->J, B * nf * 6 * nv * es, 0}, {-1, out->Jcom, B * 3 * nv * es, 0}, {-1, out->Ag, B * 6 * nv * es, 0}, {-1, out->drift, B * nf * 6 * es, 0},
                 {-1, out->dAgv, B * 6 * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_jacobians(h, *s, batch, u[0], u[1], reference_frame, wbcqp_jacobian_outputs{d[0], d[1], d[2], d[3], d[4]}, nullptr);
    });
}

int wbcqp_kinematic_hessians(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, int reference_frame, const wbcqp_hessian_outputs* out,
                             void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_hessians(h, slot, batch, q, v, reference_frame, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_hessians(h, *s, batch, q, v, reference_frame, *out, static_cast<hipStream_t>(stream));
}

int wbcqp_kinematic_hessians_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, int reference_frame, const wbcqp_hessian_outputs* out)
{
    const Slot* s = nullptr;
    WB_TRY(check_hessians(h, slot, batch, q, v, reference_frame, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv, nf = (size_t)s->jacobian.n;
    // (v goes up only where the kernel reads it)
    Arr up[2] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, out->dJ ? const_cast<void*>(v) : nullptr, B * nv * es, 0}};
    Arr dn[2] = {{-1, out->H, B * nf * 6 * nv * nv * es, 0}, {-1, out->dJ, B * nf * 6 * nv * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_hessians(h, *s, batch, u[0], u[1], reference_frame, wbcqp_hessian_outputs{d[0], d[1]}, nullptr);
    });
}

int wbcqp_inverse_dynamics_derivatives(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench,
                                       const wbcqp_id_derivative_outputs* out, void* stream)
{
    const Slot* s = nullptr;
    WB_TRY(check_inverse_dynamics_derivatives(h, slot, batch, q, v, a, lda, wrench, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_inverse_dynamics_derivatives(h, *s, batch, q, v, a, lda, wrench, *out, static_cast<hipStream_t>(stream));
}

int wbcqp_inverse_dynamics_derivatives_host(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench,
                                            const wbcqp_id_derivative_outputs* out)
{
    const Slot* s = nullptr;
    WB_TRY(check_inverse_dynamics_derivatives(h, slot, batch, q, v, a, lda, wrench, out, &s));
    if (!s) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), B = (size_t)batch, nv = (size_t)s->terms.nv;
    // (a: rows lda apart, the last one nv long -- nothing behind it is the caller's to give)
    Arr up[4] = {{-1, const_cast<void*>(q), B * s->terms.nq * es, 0}, {-1, const_cast<void*>(v), B * nv * es, 0},
                 {-1, const_cast<void*>(a), ((B - 1) * (size_t)(a ? lda : 0) + nv) * es, 0}, {-1, const_cast<void*>(wrench), B * s->wrench.n * 6 * es, 0}};
    Arr dn[2] = {{-1, out->dtau_dq, B * nv * nv * es, 0}, {-1, out->dtau_dv, B * nv * nv * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        return launch_inverse_dynamics_derivatives(h, *s, batch, u[0], u[1], u[2], lda, u[3], wbcqp_id_derivative_outputs{d[0], d[1]}, nullptr);
    });
}

int64_t wbcqp_torque_monitor_state_bytes(const wbcqp_torque_monitor* monitor)
{
    return monitor_flaw(monitor) ? 0 : (int64_t)monitor_state_bytes(monitor->n_joints, monitor->filter, monitor->window);
}

int wbcqp_detect_torque_collisions(wbcqp_handle* h, const wbcqp_torque_monitor* monitor, int batch, int n_ticks, const void* tau_model, int ldt,
                                   const void* tau_sensor, void* state, const wbcqp_torque_checks* out, void* stream)
{
    MonitorDev D;
    bool run = false;
    WB_TRY(check_torque_monitor(h, monitor, batch, n_ticks, tau_model, ldt, tau_sensor, state, out, &D, &run));
    if (!run) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_torque_monitor(h, D, batch, n_ticks, tau_model, ldt, tau_sensor, state, state, *out, static_cast<hipStream_t>(stream));
}

int wbcqp_detect_torque_collisions_host(wbcqp_handle* h, const wbcqp_torque_monitor* monitor, int batch, int n_ticks, const void* tau_model, int ldt,
                                        const void* tau_sensor, void* state, const wbcqp_torque_checks* out)
{
    MonitorDev D;
    bool run = false;
    WB_TRY(check_torque_monitor(h, monitor, batch, n_ticks, tau_model, ldt, tau_sensor, state, out, &D, &run));
    if (!run) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h), rows = (size_t)n_ticks * batch, nj = (size_t)D.n_joints;
    const size_t sb = (size_t)batch * monitor_state_bytes(D.n_joints, D.filter, D.window);
    const int reach = *std::max_element(D.joint, D.joint + D.n_joints) + 1; // (rows ldt apart, the last one read up to its highest monitored column)
    Arr up[3] = {{-1, const_cast<void*>(tau_model), ((rows - 1) * (size_t)ldt + reach) * es, 0}, {-1, const_cast<void*>(tau_sensor), rows * nj * es, 0},
                 {-1, state, sb, 0}};
    Arr dn[7] = {{-1, out->detected, rows * 4, 0}, {-1, out->invalid, rows * 8, 0}, {-1, out->discrepancy, rows * nj * es, 0},
                 {-1, out->filtered, rows * nj * es, 0}, {-1, out->first_tick, (size_t)batch * 4, 0}, {-1, out->n_detected, (size_t)batch * 4, 0},
                 {-1, state, sb, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        const wbcqp_torque_checks dev = {static_cast<int32_t*>(d[0]), static_cast<uint64_t*>(d[1]), d[2], d[3], static_cast<int32_t*>(d[4]),
                                         static_cast<int32_t*>(d[5])};
        return launch_torque_monitor(h, D, batch, n_ticks, u[0], ldt, u[1], u[2], d[6], dev, nullptr);
    });
}

int64_t wbcqp_stabilizer_state_bytes(const wbcqp_stabilizer* stabilizer)
{
    return stabilizer_flaw(stabilizer) ? 0 : (int64_t)(8 * stab_state_doubles(stabilizer->window));
}

int wbcqp_stabilize_zmp(wbcqp_handle* h, const wbcqp_stabilizer* stabilizer, const wbcqp_zmp_distributor* zmp, int batch, const wbcqp_stab_inputs* in,
                        void* state, const wbcqp_stab_outputs* out, void* alpha, void* stream)
{
    StabDev D;
    bool run = false;
    WB_TRY(check_stabilize(h, stabilizer, zmp, batch, in, state, out, alpha, &D, &run));
    if (!run) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_stabilize(h, D, zmp, batch, *in, state, state, out ? *out : wbcqp_stab_outputs{}, alpha, static_cast<hipStream_t>(stream));
}

int wbcqp_stabilize(wbcqp_handle* h, const wbcqp_stabilizer* stabilizer, int batch, const wbcqp_stab_inputs* in, void* state, const wbcqp_stab_outputs* out,
                    void* stream)
{
    return wbcqp_stabilize_zmp(h, stabilizer, nullptr, batch, in, state, out, nullptr, stream);
}

int wbcqp_stabilize_host(wbcqp_handle* h, const wbcqp_stabilizer* stabilizer, int batch, const wbcqp_stab_inputs* in, void* state,
                         const wbcqp_stab_outputs* out)
{
    return wbcqp_stabilize_zmp_host(h, stabilizer, nullptr, batch, in, state, out, nullptr);
}

int wbcqp_stabilize_zmp_host(wbcqp_handle* h, const wbcqp_stabilizer* stabilizer, const wbcqp_zmp_distributor* zmp, int batch, const wbcqp_stab_inputs* in,
                             void* state, const wbcqp_stab_outputs* out, void* alpha)
{
    StabDev D;
    bool run = false;
    WB_TRY(check_stabilize(h, stabilizer, zmp, batch, in, state, out, alpha, &D, &run));
    if (!run) return WBCQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const wbcqp_stab_outputs o = out ? *out : wbcqp_stab_outputs{};
    const size_t es = elem_size(h), B = (size_t)batch, sb = B * 8 * stab_state_doubles(D.window);
    // (placement and x_prev: rows ldp / ldx apart, the last one read up to the feet's translations / the contacts' forces)
    const int last_col = std::max(D.lf_col, D.rf_col);
    const size_t reach_p = (size_t)std::max(D.lf_pos, D.rf_pos) + 3, reach_x = last_col >= 0 ? (size_t)last_col + 12 : 0;
    Arr up[7] = {{-1, const_cast<void*>(in->ref), B * D.nref * es, 0}, {-1, const_cast<void*>(in->wrench), B * 12 * es, 0},
                 {-1, const_cast<void*>(in->com), B * 3 * es, 0}, {-1, const_cast<void*>(in->acom), B * 3 * es, 0},
                 {-1, const_cast<void*>(in->placement), ((B - 1) * (size_t)in->ldp + reach_p) * es, 0},
                 {-1, const_cast<void*>(reach_x ? in->x_prev : nullptr), reach_x ? ((B - 1) * (size_t)in->ldx + reach_x) * es : 0, 0},
                 {-1, state, sb, 0}};
    Arr dn[5] = {{-1, o.ref_out, B * D.nref * es, 0}, {-1, o.flags, B * 4, 0}, {-1, o.cop, B * 6 * es, 0}, {-1, state, sb, 0},
                 {-1, zmp ? alpha : nullptr, B * 2 * es, 0}};
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        const wbcqp_stab_inputs din = {u[0], u[1], u[2], u[3], u[4], in->ldp, u[5], in->ldx};
        return launch_stabilize(h, D, zmp, batch, din, u[6], d[3], wbcqp_stab_outputs{d[0], static_cast<int32_t*>(d[1]), d[2]}, d[4], nullptr);
    });
}

int wbcqp_problem_data(wbcqp_handle* h, int slot, int batch, const wbcqp_state* st, const wbcqp_inputs* rows, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* s = slot_with_model(h, slot);
    if (!s) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (batch == 0) return WBCQP_OK;
    WB_TRY(need_state(h, s->terms, rows ? st : nullptr)); // (no rows: the same refusal)
    WB_TRY(need_rows(h, s->layout, rows));
    HIP_TRY(h, hipSetDevice(h->device));
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        TermsArgs<TI> a{};
        fill_terms(a, h, *s, batch, Io(rows, nullptr, st));
        hipLaunchKernelGGL(terms_kernel<TI>, dim3(batch), dim3(kTermsThreads), s->terms.lds_doubles * 8, static_cast<hipStream_t>(stream), a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

int wbcqp_problem_data_host(wbcqp_handle* h, int slot, int batch, const wbcqp_state* st, const wbcqp_inputs* rows)
{
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* s = slot_with_model(h, slot);
    if (!s) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (batch == 0) return WBCQP_OK;
    if (!st || !rows) return fail(h, WBCQP_ERR_INVALID, "state / rows is NULL");
    WB_TRY(need_state(h, s->terms, st));
    WB_TRY(need_rows(h, s->layout, rows));
    HIP_TRY(h, hipSetDevice(h->device));
    const FieldBytes fb = field_bytes(*s, elem_size(h));
    const Io host(rows, nullptr, st);
    constexpr Field kUp[3] = {F_q, F_v, F_ref};
    Arr up[3], dn[kNumRecord + 1];
    lay(fb, batch, kUp, 3, host, up);
    lay(fb, batch, kRecordFields, kNumRecord + 1, host, dn);
    return staged_call(h, up, dn, [&](void* const* u, void* const* d) {
        Io dev;
        for (int i = 0; i < 3; ++i) dev.p[up[i].f] = u[i];
        for (int i = 0; i < kNumRecord + 1; ++i) dev.p[dn[i].f] = d[i];
        const wbcqp_state ds = dev.state();
        const wbcqp_inputs dr = dev.inputs();
        return wbcqp_problem_data(h, slot, batch, &ds, &dr, nullptr);
    });
}

int wbcqp_tick(wbcqp_handle* h, int slot, int batch, const wbcqp_tick_io* io, void* stream) { return tick_impl(h, slot, batch, io, stream, RollAcc{}); }

int wbcqp_rollout(wbcqp_handle* h, int slot, int batch, int n_ticks, const wbcqp_rollout_io* io, void* stream)
{
    return rollout_impl(h, slot, batch, n_ticks, io, nullptr, stream);
}

int wbcqp_rollout_traced(wbcqp_handle* h, int slot, int batch, int n_ticks, const wbcqp_rollout_io* io, const wbcqp_trace* trace, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (trace && trace->stride < 1) return fail(h, WBCQP_ERR_INVALID, "trace: stride must be >= 1");
    return rollout_impl(h, slot, batch, n_ticks, io, trace_or_null(trace), stream);
}

int wbcqp_tick_mixed(wbcqp_handle* h, const wbcqp_mix* mix, int batch, const int32_t* which, const wbcqp_mixed_io* io, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    const MixCall c{mix, batch, 1, which, io->state, io->out, io->q_next, io->v_next, io->q_solver, io->dt, nullptr, nullptr, nullptr};
    return mixed_call(h, c, stream);
}

int wbcqp_rollout_mixed(wbcqp_handle* h, const wbcqp_mix* mix, int batch, int n_ticks, const int32_t* schedule, const wbcqp_rollout_io* io, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    const MixCall c{mix, batch, n_ticks, schedule, io->state, io->out, io->q_next, io->v_next, io->q_solver, io->dt, io->iters_sum, io->ticks_ok, nullptr};
    return mixed_call(h, c, stream);
}

int wbcqp_rollout_mixed_traced(wbcqp_handle* h, const wbcqp_mix* mix, int batch, int n_ticks, const int32_t* schedule, const wbcqp_rollout_io* io,
                               const wbcqp_trace* trace, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    if (trace && trace->stride < 1) return fail(h, WBCQP_ERR_INVALID, "trace: stride must be >= 1");
    const MixCall c{mix, batch, n_ticks, schedule, io->state, io->out, io->q_next, io->v_next, io->q_solver, io->dt, io->iters_sum, io->ticks_ok,
                    trace_or_null(trace)};
    return mixed_call(h, c, stream);
}

int wbcqp_check_program(const wbcqp_program* prog, int batch, int n_slots) { return check_program(nullptr, prog, batch, n_slots); }

int wbcqp_reference_samples(wbcqp_handle* h, const wbcqp_program* prog, int batch, int tick0, int n_ticks, void* ref_out, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    WB_TRY(check_program(h, prog, batch, 0));
    if (n_ticks < 0) return fail(h, WBCQP_ERR_INVALID, "negative n_ticks");
    if (batch == 0 || n_ticks == 0) return WBCQP_OK;
    if (!prog->base || !ref_out) return fail(h, WBCQP_ERR_INVALID, "program: base / ref_out is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t sm = static_cast<hipStream_t>(stream);
    ProgDev d;
    WB_TRY(upload_program(h, prog, batch, sm, d));
    const int rc = launch_refgen(h, d, batch, 0, batch, tick0, n_ticks, h->ref_chunk, ref_out, sm);
    HIP_TRY(h, hipEventRecord(d.up->done, sm));
    return rc;
}

int wbcqp_rollout_program(wbcqp_handle* h, int slot, int batch, int tick0, int n_ticks, const wbcqp_rollout_io* io, const wbcqp_program* prog,
                          const wbcqp_trace* trace, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (trace && trace->stride < 1) return fail(h, WBCQP_ERR_INVALID, "trace: stride must be >= 1");
    const ProgCall pc{prog, tick0};
    return rollout_impl(h, slot, batch, n_ticks, io, trace_or_null(trace), stream, &pc);
}

int wbcqp_rollout_mixed_program(wbcqp_handle* h, const wbcqp_mix* mix, int batch, int tick0, int n_ticks, const wbcqp_rollout_io* io,
                                const wbcqp_program* prog, const wbcqp_trace* trace, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    if (trace && trace->stride < 1) return fail(h, WBCQP_ERR_INVALID, "trace: stride must be >= 1");
    const ProgCall pc{prog, tick0};
    const MixCall c{mix, batch, n_ticks, nullptr, io->state, io->out, io->q_next, io->v_next, io->q_solver, io->dt, io->iters_sum, io->ticks_ok,
                    trace_or_null(trace), &pc};
    return mixed_call(h, c, stream);
}

int wbcqp_tick_host(wbcqp_handle* h, int slot, int batch, const wbcqp_tick_io* io)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    const Slot* sp = slot_with_model(h, slot);
    if (!sp) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (batch == 0) return WBCQP_OK;
    const Slot& s = *sp;
    const wbcqp_layout& L = s.layout;
    WB_TRY(need_state(h, s.terms, &io->state));
    if ((L.len_tlb && (!io->rows.tlb || !io->rows.tub)) || !io->rows.w) return fail(h, WBCQP_ERR_INVALID, "tlb / tub / w are required");
    WB_TRY(need_tick_outputs(h, s.host.na, io->out, io->q_next, io->v_next));
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t B = (size_t)batch;
    const FieldBytes fb = field_bytes(s, elem_size(h));
    const Io host(&io->rows, &io->out, &io->state, io->q_next, io->v_next, io->q_solver);
    // device staging: inputs | the record, and the outputs (the mask, in/out like wbcqp_solve_batch_host's, where the caller has one)
    constexpr Field kUp[6] = {F_q, F_v, F_ref, F_tlb, F_tub, F_w};
    constexpr Field kDown[11] = {F_x, F_tau, F_obj, F_status, F_iters, F_nact, F_qn, F_vn, F_qs, F_mom, F_amask};
    const int n_dn = io->out.active_mask ? 11 : 10;
    Arr up[6], rec[kNumRecord], dn[11];
    const size_t in_only = lay(fb, B, kUp, 6, host, up); // the inputs lie in front of the record
    const size_t in_bytes = lay(fb, B, kRecordFields, kNumRecord, host, rec, in_only);
    const size_t out_bytes = lay(fb, B, kDown, n_dn, host, dn);
    const bool packed = in_only <= kPackedBytes && out_bytes <= kPackedBytes;
    const Xfer how = packed ? Xfer::packed : Xfer::async;
    WB_TRY(stage_begin(h, in_bytes, out_bytes, packed));
    WB_TRY(stage_up(h, h->stage_in.dev, up, 6, in_only, how));
    Io d;
    point(d, h->stage_in.dev, up, 6);
    point(d, h->stage_in.dev, rec, kNumRecord);
    point(d, h->stage_out.dev, dn, n_dn);
    if (!io->state.momentum) d.p[F_mom] = nullptr;
    if (!io->q_solver) d.p[F_qs] = nullptr;
    if (io->out.active_mask) WB_TRY(stage_up(h, h->stage_out.dev, &dn[10], 1, 0, Xfer::async));
    const wbcqp_tick_io dio = d.tick_io(io->dt);
    WB_TRY(wbcqp_tick(h, slot, batch, &dio, nullptr));
    WB_TRY(stage_down(h, h->stage_in.dev, rec, kNumRecord, 0, Xfer::async, false)); // the rows, where asked for, one by one
    return stage_down(h, h->stage_out.dev, dn, n_dn, out_bytes, how);
}

struct wbcqp_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t capture = nullptr;
    OrderState ord; // the captured kernels read and write THESE buffers on every replay: nothing else ever touches them
};

int wbcqp_tick_graph_destroy(wbcqp_handle* h, wbcqp_graph* g)
{
    if (!g) return WBCQP_OK;
    if (h) (void)hipSetDevice(h->device);
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    if (g->capture) (void)hipStreamDestroy(g->capture);
    if (g->ord.order) (void)hipFree(g->ord.order);
    if (g->ord.queue) (void)hipFree(g->ord.queue);
    delete g;
    return WBCQP_OK;
}

int wbcqp_tick_graph_create(wbcqp_handle* h, int slot, int batch, const wbcqp_tick_io* io, wbcqp_graph** out)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!out || !io) return fail(h, WBCQP_ERR_INVALID, "io / out is NULL");
    if (batch <= 0) return fail(h, WBCQP_ERR_INVALID, "a graph needs a positive batch");
    *out = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    wbcqp_graph* g = new wbcqp_graph();
    hipError_t e = hipStreamCreateWithFlags(&g->capture, hipStreamNonBlocking);
    if (e != hipSuccess) { delete g; return fail(h, WBCQP_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    // the graph's own launch-order buffer and queue counter, at their final size: a replay reads and rewrites them and
    // nothing else does (the handle's own buffer may be resized or overwritten by any other launch)
    e = hipMalloc(&g->ord.order, 2 * sizeof(int) * (size_t)batch);
    if (e == hipSuccess) e = hipMalloc(&g->ord.queue, 2 * sizeof(int));
    if (e == hipSuccess) e = hipMemset(g->ord.queue, 0, 2 * sizeof(int));
    if (e != hipSuccess) { wbcqp_tick_graph_destroy(h, g); return fail(h, WBCQP_ERR_HIP, std::string("graph buffers: ") + hipGetErrorString(e)); }
    g->ord.cap = batch;
    // an ordinary tick on the capture stream first: function attributes are then settled, the graph's order buffer holds a
    // valid order for this stream and shape, and the capture below contains kernel launches only
    h->graph_ord = &g->ord;
    int rc = wbcqp_tick(h, slot, batch, io, g->capture);
    if (rc == WBCQP_OK && hipStreamSynchronize(g->capture) != hipSuccess) rc = fail(h, WBCQP_ERR_HIP, "warm-up tick failed");
    if (rc != WBCQP_OK) { h->graph_ord = nullptr; wbcqp_tick_graph_destroy(h, g); return rc; }
    e = hipStreamBeginCapture(g->capture, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { h->graph_ord = nullptr; wbcqp_tick_graph_destroy(h, g); return fail(h, WBCQP_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e)); }
    h->capturing = true;
    rc = wbcqp_tick(h, slot, batch, io, g->capture);
    h->capturing = false;
    h->graph_ord = nullptr;
    e = hipStreamEndCapture(g->capture, &g->graph);
    if (rc != WBCQP_OK || e != hipSuccess || !g->graph) {
        wbcqp_tick_graph_destroy(h, g);
        return rc != WBCQP_OK ? rc : fail(h, WBCQP_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    }
    e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { wbcqp_tick_graph_destroy(h, g); return fail(h, WBCQP_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
    *out = g;
    return WBCQP_OK;
}

int wbcqp_tick_graph_launch(wbcqp_handle* h, wbcqp_graph* g, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!g || !g->exec) return fail(h, WBCQP_ERR_INVALID, "graph is NULL");
    HIP_TRY(h, hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream)));
    return WBCQP_OK;
}

int wbcqp_sync(wbcqp_handle* h, void* stream)
{
    if (!h) return WBCQP_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return WBCQP_OK;
}

} // extern "C"
