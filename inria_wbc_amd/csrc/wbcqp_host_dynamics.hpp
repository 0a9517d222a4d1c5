// wbcqp_host_dynamics.hpp -- host side of wbcqp_set_wrench_frames / wbcqp_inverse_dynamics (wbcqp_api.hip): the argument checks the device-pointer and
// the host-pointer entry point share, and the launch of rnea_kernel (csrc/wbcqp_rnea.hpp).  Host code only; included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_handle.hpp"

namespace {

// what both wbcqp_inverse_dynamics and wbcqp_inverse_dynamics_host refuse, before anything is staged or launched; *s: the slot
int check_inverse_dynamics(wbcqp_handle* h, int slot, int batch, const void* q, const void* a, int lda, const void* wrench, const void* tau, const Slot** s)
{
    *s = slot_with_model(h, slot);
    if (!*s) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (!q || !tau) return fail(h, WBCQP_ERR_INVALID, "q and tau are required");
    if (a && lda < (*s)->terms.nv) return fail(h, WBCQP_ERR_INVALID, "lda must be at least nv");
    if (wrench && (*s)->n_wrench == 0) return fail(h, WBCQP_ERR_INVALID, "wrench given, but no frames are selected (wbcqp_set_wrench_frames)");
    return WBCQP_OK;
}

// one wavefront per instance, kRneaPerBlock instances per workgroup; batch > 0, arguments checked
int launch_inverse_dynamics(wbcqp_handle* h, const Slot& s, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench, void* tau,
                            hipStream_t stream)
{
    const TermsDev& T = s.terms;
    const RneaDev D{T.nb, T.nq, T.nv, T.floating_base, T.nrounds, {T.g[0], T.g[1], T.g[2]}, T.ipool, T.dpool, T.i_jtype, T.i_last, T.i_idxq, T.i_idxv, T.i_anc,
                    T.i_bodyof, T.i_kof, T.d_place, T.d_inertia, wrench ? s.n_wrench : 0, s.wrench_body, s.wrench_place};
    const int blocks = (batch + kRneaPerBlock - 1) / kRneaPerBlock;
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        const RneaArgs<TI> args{D, static_cast<const TI*>(q), static_cast<const TI*>(v), static_cast<const TI*>(a), static_cast<const TI*>(wrench),
                                static_cast<TI*>(tau), a ? lda : 0, batch};
        hipLaunchKernelGGL(rnea_kernel<TI>, dim3(blocks), dim3(kRneaThreads), 0, stream, args);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

} // namespace
