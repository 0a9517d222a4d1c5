// wbcqp_host_queries.hpp -- host side of the model queries on a fleet's states (wbcqp_api.hip): wbcqp_observe, wbcqp_check_collisions and
// wbcqp_inverse_dynamics, each with the set-up call that puts its table on the slot, and wbcqp_mass_matrix, wbcqp_forward_dynamics and
// wbcqp_spd_commands (fdyn_kernel, csrc/wbcqp_fdyn.hpp, behind rnea_kernel for the bias), wbcqp_jacobians (jacobian_kernel,
// csrc/wbcqp_jacobians.hpp), wbcqp_kinematic_hessians (hessian_kernel, csrc/wbcqp_hessians.hpp) and wbcqp_inverse_dynamics_derivatives
// (id_derivatives_kernel, csrc/wbcqp_idderiv.hpp).  Per query: ONE check_* that the device-pointer and the
// host-pointer entry point share (nothing is staged or launched before it has passed) and ONE launch_* of its kernel (csrc/wbcqp_observe.hpp,
// wbcqp_collide.hpp, wbcqp_rnea.hpp), one wavefront per instance.  Host code only; included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_handle.hpp"
#include "wbcqp_fdyn.hpp"
#include "wbcqp_jacobians.hpp"
#include "wbcqp_hessians.hpp"
#include "wbcqp_idderiv.hpp"

namespace {

static_assert(kObservePerBlock == kRneaPerBlock, "the three query kernels hold the same number of instances per workgroup");
static_assert(kFdynPerBlock == kRneaPerBlock && kFdynMaxDof == kWave, "fdyn_kernel: the same instances per workgroup, one lane per dof");
static_assert(kJacobianPerBlock == kRneaPerBlock && WBCQP_MAX_JACOBIAN_FRAMES == kMaxJacobianFrames && kMaxJacobianFrames == kWave,
              "jacobian_kernel: the same instances per workgroup, one lane per selected frame");
static_assert(WBCQP_RF_WORLD == kRfWorld && WBCQP_RF_LOCAL == kRfLocal && WBCQP_RF_LOCAL_WORLD_ALIGNED == kRfLocalWorldAligned,
              "the header and the kernel agree on the reference frames");
static_assert(kHessianPerBlock == kRneaPerBlock, "hessian_kernel: the same instances per workgroup");
static_assert(kIdDerivPerBlock == kRneaPerBlock, "id_derivatives_kernel: the same instances per workgroup");
static_assert(WBCQP_MAX_WRENCH_FRAMES == kMaxWrenchFrames, "the header and the kernel agree on the number of wrench frames");

// workgroups for `batch` instances at one wavefront each
inline int query_blocks(int batch) { return (batch + kObservePerBlock - 1) / kObservePerBlock; }

// the tree of the slot's model as the observe and the collide kernel read it, with `frames` frames of the selection (0: none are read)
// wbcqp_set_force_references' one check on a slot with a model; *off: the offsets as the rows kernel's table holds them
int check_force_references(wbcqp_handle* h, const Slot& s, const int32_t* force_ref, const double* weight, std::vector<int>* off)
{
    const int nc = s.terms.nc, nref = s.terms.nref;
    off->assign(nc, -1);
    if (nc == 0) return WBCQP_OK;
    if (!force_ref || !weight) return fail(h, WBCQP_ERR_INVALID, "force_ref / weight is NULL");
    for (int c = 0; c < nc; ++c) {
        const int o = force_ref[c];
        if (o < -1) return fail(h, WBCQP_ERR_INVALID, "a force reference offset is below -1");
        if (o >= 0 && (int64_t)o + 6 > nref) return fail(h, WBCQP_ERR_INVALID, "a force reference runs past nref");
        for (int a = 0; a < c; ++a)
            if (o >= 0 && force_ref[a] >= 0 && o < force_ref[a] + 6 && force_ref[a] < o + 6) return fail(h, WBCQP_ERR_INVALID, "two force references overlap");
        (*off)[c] = o;
    }
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < 6; ++k) {
            const double w = weight[6 * c + k];
            if (!std::isfinite(w)) return fail(h, WBCQP_ERR_INVALID, "a force regularisation weight is not finite");
            for (int j = 0; j < 12; ++j) {
                volatile double prod = w * s.force_gen_h[(size_t)c * 72 + k * 12 + j]; // (one rounding: the product the caller formed)
                const double have = s.forcereg_h[(size_t)c * 72 + k * 12 + j], got = prod;
                if (!(got == have)) // (exact, no tolerance; a zero of either sign is a zero)
                    return fail(h, WBCQP_ERR_INVALID, "weight[c][k] * force_gen[c][k][j] is not the slot's forcereg_mat[c][k][j]: the weights are not the ones the slot was made with");
            }
        }
    return WBCQP_OK;
}

ObserveDev observe_dev(const TermsDev& T, const FrameSel& sel, bool frames)
{
    return ObserveDev{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, T.ipool, T.dpool, T.i_jtype, T.i_idxq, T.i_idxv, T.i_anc, T.d_place, T.d_inertia,
                      frames ? sel.n : 0, sel.body, sel.place};
}

// ---- the tables of a slot --------------------------------------------------------------------------------------------------------------------------
// A new table is complete on the device, in an allocation of its own, before the caller lets the one before go (a failure leaves that one in place);
// bytes == 0: *fresh is null
int upload_fresh(wbcqp_handle* h, const void* src, size_t bytes, const char* the_table, void** fresh)
{
    *fresh = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    if (bytes == 0) return WBCQP_OK;
    HIP_TRY(h, hipMalloc(fresh, bytes));
    if (hipMemcpy(*fresh, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(*fresh);
        *fresh = nullptr;
        return fail(h, WBCQP_ERR_HIP, std::string("copying ") + the_table + " to the device failed");
    }
    return WBCQP_OK;
}

// wbcqp_set_observed_frames / wbcqp_set_wrench_frames / wbcqp_set_jacobian_frames: frame indices -> (placement, body) of each from the slot's host copy of the model's frame table;
// n_frames == 0 drops the selection
int set_frame_selection(wbcqp_handle* h, int slot, FrameSel Slot::*which, int n_frames, const int32_t* frames, int limit, const char* a_frame,
                        const char* the_frames)
{
    if (!h) return WBCQP_ERR_INVALID;
    Slot* s = slot_with_model(h, slot);
    if (!s) return WBCQP_ERR_INVALID;
    if (n_frames < 0 || n_frames > limit) return fail(h, WBCQP_ERR_INVALID, "n_frames must be in [0, " + std::to_string(limit) + "]");
    if (n_frames > 0 && !frames) return fail(h, WBCQP_ERR_INVALID, "frames is NULL");
    const int nframe = (int)s->frame_body_h.size();
    std::vector<double> store((size_t)12 * n_frames + ((size_t)n_frames + 1) / 2);
    int* body = reinterpret_cast<int*>(store.data() + (size_t)12 * n_frames);
    for (int f = 0; f < n_frames; ++f) {
        if (frames[f] < 0 || frames[f] >= nframe) return fail(h, WBCQP_ERR_INVALID, std::string(a_frame) + " does not exist in the slot's model");
        body[f] = s->frame_body_h[frames[f]];
        std::copy(s->frame_place_h.begin() + (size_t)12 * frames[f], s->frame_place_h.begin() + (size_t)12 * frames[f] + 12, store.begin() + (size_t)12 * f);
    }
    void* fresh = nullptr;
    WB_TRY(upload_fresh(h, store.data(), store.size() * sizeof(double), the_frames, &fresh));
    FrameSel& sel = s->*which;
    release(sel); // (hipFree waits for whatever still reads the previous selection)
    if (n_frames == 0) return WBCQP_OK;
    const double* place = static_cast<const double*>(fresh);
    sel = FrameSel{n_frames, reinterpret_cast<const int*>(place + (size_t)12 * n_frames), place, fresh};
    return WBCQP_OK;
}

int set_collision_spheres(wbcqp_handle* h, int slot, const wbcqp_sphere_model* sm)
{
    if (!h) return WBCQP_ERR_INVALID;
    Slot* s = slot_with_model(h, slot);
    if (!s) return WBCQP_ERR_INVALID;
    if (!sm) return fail(h, WBCQP_ERR_INVALID, "sphere model is NULL");
    const int n = sm->n_spheres;
    if (n < 0 || n > WBCQP_MAX_SPHERES) return fail(h, WBCQP_ERR_INVALID, "n_spheres must be in [0, 256]");
    if (n > 0 && (!sm->body || !sm->member || !sm->centre || !sm->diameter)) return fail(h, WBCQP_ERR_INVALID, "body / member / centre / diameter is NULL");
    // one allocation: centre [n][3] doubles, then body, tag (member << 8 | place inside the member) and half-diameter, 4 bytes each
    std::vector<double> store(((size_t)n * (24 + 12) + 7) / 8); // (doubles: the block's alignment is the centres')
    char* blob = reinterpret_cast<char*>(store.data());
    double* centre = store.data();
    int* body = reinterpret_cast<int*>(blob + (size_t)24 * n);
    int* tag = body + n;
    float* half = reinterpret_cast<float*>(tag + n);
    for (int i = 0, place = 0; i < n; ++i) {
        if (sm->body[i] < 0 || sm->body[i] >= s->terms.nb) return fail(h, WBCQP_ERR_INVALID, "a sphere's body is outside the slot's tree");
        if (sm->member[i] < 0 || sm->member[i] >= WBCQP_MAX_MEMBERS) return fail(h, WBCQP_ERR_INVALID, "a sphere's member must be in [0, 16)");
        if (i > 0 && sm->member[i] < sm->member[i - 1]) return fail(h, WBCQP_ERR_INVALID, "member must be non-decreasing (spheres sorted by member)");
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(sm->centre[3 * i + k])) return fail(h, WBCQP_ERR_INVALID, "a sphere's centre is not finite");
        if (!std::isfinite(sm->diameter[i]) || !(sm->diameter[i] > 0.0f)) return fail(h, WBCQP_ERR_INVALID, "a sphere's diameter must be finite and > 0");
        place = (i > 0 && sm->member[i] == sm->member[i - 1]) ? place + 1 : 0;
        body[i] = sm->body[i];
        tag[i] = (sm->member[i] << 8) | place;
        half[i] = sm->diameter[i] / 2; // a float division, as the reference's sphere.second / 2
        std::copy(sm->centre + 3 * i, sm->centre + 3 * i + 3, centre + 3 * i);
    }
    void* fresh = nullptr;
    WB_TRY(upload_fresh(h, blob, (size_t)n * (24 + 12), "the sphere table", &fresh));
    release_spheres(*s); // (hipFree waits for whatever still reads the previous table)
    if (n == 0) return WBCQP_OK;
    s->spheres_alloc = fresh;
    const int* dbody = reinterpret_cast<const int*>(static_cast<char*>(fresh) + (size_t)24 * n);
    s->spheres = CollideDev{n, dbody, dbody + n, static_cast<const double*>(fresh), reinterpret_cast<const float*>(dbody + 2 * n)};
    return WBCQP_OK;
}

// ---- the checks: what the device-pointer and the host-pointer entry point of a query refuse, before anything is staged or launched ----------------
// *s: the slot, or null where the call is accepted and there is nothing to do (batch == 0, no output asked for)
int check_observe(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, const void* acom, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!out) return fail(h, WBCQP_ERR_INVALID, "observables struct is NULL");
    if ((out->placement || out->velocity) && sl->observed.n == 0)
        return fail(h, WBCQP_ERR_INVALID, "placement / velocity asked for, but no frames are selected (wbcqp_set_observed_frames)");
    if ((out->vcom || out->velocity) && !v) return fail(h, WBCQP_ERR_INVALID, "vcom / velocity asked for, but v is NULL");
    if (acom && !v) return fail(h, WBCQP_ERR_INVALID, "acom asked for, but v is NULL");
    if (batch == 0 || (!out->com && !out->vcom && !out->placement && !out->velocity && !acom)) return WBCQP_OK;
    if (!q) return fail(h, WBCQP_ERR_INVALID, "q is NULL");
    *s = sl;
    return WBCQP_OK;
}

int check_collisions(wbcqp_handle* h, int slot, int batch, const void* q, const wbcqp_collisions* out, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (sl->spheres.n_spheres == 0) return fail(h, WBCQP_ERR_INVALID, "slot has no sphere table (wbcqp_set_collision_spheres)");
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!out) return fail(h, WBCQP_ERR_INVALID, "collisions struct is NULL");
    if (batch == 0 || (!out->colliding && !out->first_pair && !out->n_pairs && !out->clearance && !out->centres)) return WBCQP_OK;
    if (!q) return fail(h, WBCQP_ERR_INVALID, "q is NULL");
    *s = sl;
    return WBCQP_OK;
}

int check_inverse_dynamics(wbcqp_handle* h, int slot, int batch, const void* q, const void* a, int lda, const void* wrench, const void* tau, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!q || !tau) return fail(h, WBCQP_ERR_INVALID, "q and tau are required");
    if (a && lda < sl->terms.nv) return fail(h, WBCQP_ERR_INVALID, "lda must be at least nv");
    if (wrench && sl->wrench.n == 0) return fail(h, WBCQP_ERR_INVALID, "wrench given, but no frames are selected (wbcqp_set_wrench_frames)");
    if (batch > 0) *s = sl;
    return WBCQP_OK;
}

// ---- the launches: batch > 0, arguments checked, the handle's device current ---------------------------------------------------------------------
int launch_observe(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, const wbcqp_observables& out, void* acom, hipStream_t stream)
{
    const ObserveDev D = observe_dev(s.terms, s.observed, out.placement || out.velocity);
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const ObserveArgs<TI> a{D, static_cast<const TI*>(q), (out.vcom || out.velocity || acom) ? static_cast<const TI*>(v) : nullptr,
                                static_cast<TI*>(out.com), static_cast<TI*>(out.vcom), static_cast<TI*>(out.placement), static_cast<TI*>(out.velocity), batch,
                                static_cast<TI*>(acom)};
        hipLaunchKernelGGL(observe_kernel<TI>, dim3(query_blocks(batch)), dim3(kObserveThreads), observe_lds_bytes(D.n_frames), stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

int launch_collisions(wbcqp_handle* h, const Slot& s, int batch, const void* q, const wbcqp_collisions& out, hipStream_t stream)
{
    const ObserveDev D = observe_dev(s.terms, FrameSel{}, false);
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const CollideArgs<TI> a{D, s.spheres, static_cast<const TI*>(q), out.colliding, out.first_pair, out.n_pairs, static_cast<TI*>(out.clearance),
                                static_cast<TI*>(out.centres), batch};
        hipLaunchKernelGGL(collide_kernel<TI>, dim3(query_blocks(batch)), dim3(kObserveThreads), collide_lds_bytes(s.spheres.n_spheres), stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

int launch_inverse_dynamics(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench, void* tau,
                            hipStream_t stream)
{
    const TermsDev& T = s.terms;
    const RneaDev D{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, {T.g[0], T.g[1], T.g[2]}, T.ipool, T.dpool, T.i_jtype, T.i_last, T.i_idxq, T.i_idxv, T.i_anc,
                    T.i_bodyof, T.i_kof, T.d_place, T.d_inertia, wrench ? s.wrench.n : 0, s.wrench.body, s.wrench.place};
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const RneaArgs<TI> args{D, static_cast<const TI*>(q), static_cast<const TI*>(v), static_cast<const TI*>(a), static_cast<const TI*>(wrench),
                                static_cast<TI*>(tau), a ? lda : 0, batch};
        hipLaunchKernelGGL(rnea_kernel<TI>, dim3(query_blocks(batch)), dim3(kRneaThreads), 0, stream, args);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

// ---- forward dynamics: wbcqp_mass_matrix, wbcqp_forward_dynamics, wbcqp_spd_commands ----------------------------------------------------------------
int check_mass_matrix(wbcqp_handle* h, int slot, int batch, const void* q, const void* M, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!q || !M) return fail(h, WBCQP_ERR_INVALID, "q and M are required");
    if (batch > 0) *s = sl;
    return WBCQP_OK;
}

int check_forward_dynamics(wbcqp_handle* h, int slot, int batch, const void* q, const void* tau, int ldt, const void* wrench, const double* damping,
                           const void* a, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!q || !a) return fail(h, WBCQP_ERR_INVALID, "q and a are required");
    if (tau && ldt < sl->terms.nv) return fail(h, WBCQP_ERR_INVALID, "ldt must be at least nv");
    if (wrench && sl->wrench.n == 0) return fail(h, WBCQP_ERR_INVALID, "wrench given, but no frames are selected (wbcqp_set_wrench_frames)");
    for (int j = 0; damping && j < sl->terms.nv; ++j)
        if (!std::isfinite(damping[j]) || damping[j] < 0.0) return fail(h, WBCQP_ERR_INVALID, "damping must be finite and >= 0");
    if (batch > 0) *s = sl;
    return WBCQP_OK;
}

int check_spd_commands(wbcqp_handle* h, int slot, int batch, const wbcqp_spd* law, const void* q, const void* target, int ldtarget, const void* wrench,
                       const void* commands, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (!law) return fail(h, WBCQP_ERR_INVALID, "spd law is NULL");
    if (!std::isfinite(law->dt) || !(law->dt > 0.0)) return fail(h, WBCQP_ERR_INVALID, "dt must be finite and > 0");
    if (!std::isfinite(law->kp) || !std::isfinite(law->kd)) return fail(h, WBCQP_ERR_INVALID, "kp / kd is not finite");
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!q || !target || !commands) return fail(h, WBCQP_ERR_INVALID, "q, target and commands are required");
    if (ldtarget < sl->terms.nv - (sl->terms.floating_base ? 6 : 0)) return fail(h, WBCQP_ERR_INVALID, "ldtarget must be at least na");
    if (wrench && sl->wrench.n == 0) return fail(h, WBCQP_ERR_INVALID, "wrench given, but no frames are selected (wbcqp_set_wrench_frames)");
    if (batch > 0) *s = sl;
    return WBCQP_OK;
}

// fdyn_kernel<TI, SPD> on arguments filled by `fill(FdynArgs<TI>&)`, behind whatever the stream already holds
template <bool SPD, typename F> int launch_fdyn(wbcqp_handle* h, const Slot& s, int batch, hipStream_t stream, F&& fill)
{
    const TermsDev& T = s.terms;
    const RneaDev D{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, {T.g[0], T.g[1], T.g[2]}, T.ipool, T.dpool, T.i_jtype, T.i_last, T.i_idxq, T.i_idxv, T.i_anc,
                    T.i_bodyof, T.i_kof, T.d_place, T.d_inertia, 0, nullptr, nullptr};
    const int lds = fdyn_lds_bytes(T.nv);
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        FdynArgs<TI> args{};
        args.D = D;
        args.batch = batch;
        fill(args);
        if (lds > 64 * 1024)
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&fdyn_kernel<TI, SPD>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL((fdyn_kernel<TI, SPD>), dim3(query_blocks(batch)), dim3(kFdynThreads), lds, stream, args);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

int launch_mass_matrix(wbcqp_handle* h, const Slot& s, int batch, const void* q, void* M, hipStream_t stream)
{
    return launch_fdyn<false>(h, s, batch, stream, [&](auto& a) {
        using TI = std::remove_const_t<std::remove_pointer_t<decltype(a.q)>>;
        a.q = static_cast<const TI*>(q);
        a.M = static_cast<TI*>(M);
    });
}

// the bias nle(q, v) - sum_k J_k' w_k by rnea_kernel into the output row, then fdyn_kernel on it
int launch_forward_dynamics(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, const void* tau, int ldt, const void* wrench,
                            const double* damping, void* a, int32_t* info, hipStream_t stream)
{
    WB_TRY(launch_inverse_dynamics(h, s, batch, q, v, nullptr, 0, wrench, a, stream));
    return launch_fdyn<false>(h, s, batch, stream, [&](auto& g) {
        using TI = std::remove_const_t<std::remove_pointer_t<decltype(g.q)>>;
        g.q = static_cast<const TI*>(q);
        g.v = static_cast<const TI*>(v);
        g.rhs = static_cast<const TI*>(tau);
        g.ldr = tau ? ldt : 0;
        g.out = static_cast<TI*>(a);
        g.info = info;
        if (damping) std::copy(damping, damping + s.terms.nv, g.damping);
    });
}

int launch_spd_commands(wbcqp_handle* h, const Slot& s, int batch, const wbcqp_spd& law, const void* q, const void* v, const void* target, int ldtarget,
                        const void* wrench, void* commands, void* qddot, int32_t* info, hipStream_t stream)
{
    WB_TRY(launch_inverse_dynamics(h, s, batch, q, v, nullptr, 0, wrench, commands, stream));
    return launch_fdyn<true>(h, s, batch, stream, [&](auto& g) {
        using TI = std::remove_const_t<std::remove_pointer_t<decltype(g.q)>>;
        g.q = static_cast<const TI*>(q);
        g.v = static_cast<const TI*>(v);
        g.rhs = static_cast<const TI*>(target);
        g.ldr = ldtarget;
        g.out = static_cast<TI*>(commands);
        g.qddot = static_cast<TI*>(qddot);
        g.info = info;
        g.dt = law.dt;
        g.kp = law.kp;
        g.kd = law.kd;
    });
}

// ---- differential kinematics: wbcqp_jacobians --------------------------------------------------------------------------------------------------------
int check_jacobians(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, int rf, const wbcqp_jacobian_outputs* out, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!out) return fail(h, WBCQP_ERR_INVALID, "jacobian outputs struct is NULL");
    if (rf != WBCQP_RF_WORLD && rf != WBCQP_RF_LOCAL && rf != WBCQP_RF_LOCAL_WORLD_ALIGNED)
        return fail(h, WBCQP_ERR_INVALID, "unknown reference_frame (WBCQP_RF_WORLD, WBCQP_RF_LOCAL or WBCQP_RF_LOCAL_WORLD_ALIGNED)");
    if (!out->J && !out->Jcom && !out->Ag && !out->drift && !out->dAgv) return fail(h, WBCQP_ERR_INVALID, "every output is NULL: nothing is asked for");
    if ((out->J || out->drift) && sl->jacobian.n == 0)
        return fail(h, WBCQP_ERR_INVALID, "J / drift asked for, but no frames are selected (wbcqp_set_jacobian_frames)");
    if ((out->drift || out->dAgv) && !v) return fail(h, WBCQP_ERR_INVALID, "drift / dAgv asked for, but v is NULL");
    if (out->drift && rf == WBCQP_RF_WORLD)
        return fail(h, WBCQP_ERR_INVALID, "drift asked for with WBCQP_RF_WORLD: a classical acceleration is LOCAL or LOCAL_WORLD_ALIGNED");
    if (batch == 0) return WBCQP_OK;
    if (!q) return fail(h, WBCQP_ERR_INVALID, "q is NULL");
    *s = sl;
    return WBCQP_OK;
}

int launch_jacobians(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, int rf, const wbcqp_jacobian_outputs& out, hipStream_t stream)
{
    const TermsDev& T = s.terms;
    const bool frames = out.J || out.drift;
    const JacobianDev D{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, T.ipool, T.dpool, T.i_jtype, T.i_last, T.i_idxq, T.i_idxv, T.i_anc, T.i_bodyof, T.i_kof,
                        T.d_place, T.d_inertia, frames ? s.jacobian.n : 0, s.jacobian.body, s.jacobian.place};
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const JacobianArgs<TI> a{D, static_cast<const TI*>(q), (out.drift || out.dAgv) ? static_cast<const TI*>(v) : nullptr, static_cast<TI*>(out.J),
                                 static_cast<TI*>(out.Jcom), static_cast<TI*>(out.Ag), static_cast<TI*>(out.drift), static_cast<TI*>(out.dAgv), rf, batch};
        hipLaunchKernelGGL(jacobian_kernel<TI>, dim3(query_blocks(batch)), dim3(kJacobianThreads), 0, stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

// ---- second-order kinematics: wbcqp_kinematic_hessians -----------------------------------------------------------------------------------------------
int check_hessians(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, int rf, const wbcqp_hessian_outputs* out, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!out) return fail(h, WBCQP_ERR_INVALID, "hessian outputs struct is NULL");
    if (rf != WBCQP_RF_WORLD && rf != WBCQP_RF_LOCAL && rf != WBCQP_RF_LOCAL_WORLD_ALIGNED)
        return fail(h, WBCQP_ERR_INVALID, "unknown reference_frame (WBCQP_RF_WORLD, WBCQP_RF_LOCAL or WBCQP_RF_LOCAL_WORLD_ALIGNED)");
    if (!out->H && !out->dJ) return fail(h, WBCQP_ERR_INVALID, "every output is NULL: nothing is asked for");
    if (sl->jacobian.n == 0) return fail(h, WBCQP_ERR_INVALID, "H / dJ asked for, but no frames are selected (wbcqp_set_jacobian_frames)");
    if (out->dJ && !v) return fail(h, WBCQP_ERR_INVALID, "dJ asked for, but v is NULL");
    if (batch == 0) return WBCQP_OK;
    if (!q) return fail(h, WBCQP_ERR_INVALID, "q is NULL");
    *s = sl;
    return WBCQP_OK;
}

// H's store shape.  One k per lane (narrow) everywhere, unless the handle was created with WBCQP_HESSIAN_STORE=wide in the environment AND nv is
// even AND H is aligned to two elements: then two consecutive k per lane in one store of twice the width.  Narrow is the faster one; wide is kept
// so that tools/hessians_bench.py can put the two side by side (profiles/hessians/INDEX.md has the figures)
bool hessian_wide_stores(const wbcqp_handle* h, const void* H, int nv, size_t elem)
{
    return h->hessian_wide && H && !(nv & 1) && reinterpret_cast<uintptr_t>(H) % (2 * elem) == 0;
}

int launch_hessians(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, int rf, const wbcqp_hessian_outputs& out, hipStream_t stream)
{
    const TermsDev& T = s.terms;
    const JacobianDev D{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, T.ipool, T.dpool, T.i_jtype, T.i_last, T.i_idxq, T.i_idxv, T.i_anc, T.i_bodyof, T.i_kof,
                        T.d_place, T.d_inertia, s.jacobian.n, s.jacobian.body, s.jacobian.place};
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        // (v goes to the kernel only where dJ is asked for: H has the bits of the call with v)
        const HessianArgs<TI> a{D, static_cast<const TI*>(q), out.dJ ? static_cast<const TI*>(v) : nullptr, static_cast<TI*>(out.H), static_cast<TI*>(out.dJ),
                                rf, batch};
        if (hessian_wide_stores(h, out.H, T.nv, sizeof(TI)))
            hipLaunchKernelGGL((hessian_kernel<TI, true>), dim3(query_blocks(batch)), dim3(kHessianThreads), 0, stream, a);
        else
            hipLaunchKernelGGL((hessian_kernel<TI, false>), dim3(query_blocks(batch)), dim3(kHessianThreads), 0, stream, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

// ---- the inverse dynamics' derivatives: wbcqp_inverse_dynamics_derivatives ------------------------------------------------------------------------------
int check_inverse_dynamics_derivatives(wbcqp_handle* h, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench,
                                       const wbcqp_id_derivative_outputs* out, const Slot** s)
{
    *s = nullptr;
    if (!h) return WBCQP_ERR_INVALID;
    const Slot* sl = slot_with_model(h, slot);
    if (!sl) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!out) return fail(h, WBCQP_ERR_INVALID, "inverse dynamics derivative outputs struct is NULL");
    if (!out->dtau_dq && !out->dtau_dv) return fail(h, WBCQP_ERR_INVALID, "every output is NULL: nothing is asked for");
    if (out->dtau_dv && !v) return fail(h, WBCQP_ERR_INVALID, "dtau_dv asked for, but v is NULL");
    if (a && lda < sl->terms.nv) return fail(h, WBCQP_ERR_INVALID, "lda must be at least nv");
    if (wrench && sl->wrench.n == 0) return fail(h, WBCQP_ERR_INVALID, "wrench given, but no frames are selected (wbcqp_set_wrench_frames)");
    if (batch == 0) return WBCQP_OK;
    if (!q) return fail(h, WBCQP_ERR_INVALID, "q is NULL");
    *s = sl;
    return WBCQP_OK;
}

int launch_inverse_dynamics_derivatives(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench,
                                        const wbcqp_id_derivative_outputs& out, hipStream_t stream)
{
    const TermsDev& T = s.terms;
    const RneaDev D{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, {T.g[0], T.g[1], T.g[2]}, T.ipool, T.dpool, T.i_jtype, T.i_last, T.i_idxq, T.i_idxv, T.i_anc,
                    T.i_bodyof, T.i_kof, T.d_place, T.d_inertia, wrench ? s.wrench.n : 0, s.wrench.body, s.wrench.place};
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const IdDerivArgs<TI> args{D, static_cast<const TI*>(q), static_cast<const TI*>(v), static_cast<const TI*>(a), static_cast<const TI*>(wrench),
                                   static_cast<TI*>(out.dtau_dq), static_cast<TI*>(out.dtau_dv), a ? lda : 0, batch};
        hipLaunchKernelGGL(id_derivatives_kernel<TI>, dim3(query_blocks(batch)), dim3(kIdDerivThreads), 0, stream, args);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

} // namespace
