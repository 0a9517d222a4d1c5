// wbcqp_host_rollout.hpp -- host side of the C ABI (wbcqp_api.hip): one tick, and the two loops over ticks -- rollout_impl (one slot: wbcqp_rollout,
// wbcqp_rollout_traced) and mixed_run (one robot model, its instances in different contact sets: wbcqp_tick_mixed, wbcqp_rollout_mixed,
// wbcqp_rollout_mixed_traced) -- with the trace writer and the state ping-pong they share.  Included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_launch.hpp"
#include "wbcqp_host_program.hpp"

namespace {

// a trace whose fields are all NULL is no trace
const wbcqp_trace* trace_or_null(const wbcqp_trace* tr)
{
    return (tr && (tr->q || tr->v || tr->x || tr->tau || tr->status || tr->iters || tr->objective || tr->cost)) ? tr : nullptr;
}

// Where the ticks of a roll-out of B instances write what a trace records.  A recorded tick's solve and integration write into the trace's entry (the
// next tick reads its state from there); a recorded LAST tick writes the caller's own arrays where there are any and is copied into its entry by finish()
struct TraceWriter {
    const wbcqp_trace* tr; // null: no trace
    size_t B;
    int n_ticks;
    bool recorded(int t) const { return tr && (t + 1) % tr->stride == 0; }
    size_t row0(int t) const { return (size_t)((t + 1) / tr->stride - 1) * B; } // first row of tick t's entry
    void* field(Field f) const
    {
        switch (f) {
        case F_qn: return tr->q;
        case F_vn: return tr->v;
        case F_x: return tr->x;
        case F_tau: return tr->tau;
        case F_obj: return tr->objective;
        case F_status: return tr->status;
        case F_iters: return tr->iters;
        default: return nullptr;
        }
    }
    // where tick t writes field f (`bytes` per instance): its entry's, or `other` -- the tick is not recorded, the trace has no such field, or it is the last
    // tick and `other` is the caller's array
    void* dest(int t, Field f, size_t bytes, void* other) const
    {
        if (!recorded(t) || !field(f) || (t + 1 == n_ticks && other)) return other;
        return static_cast<char*>(field(f)) + row0(t) * bytes;
    }
    int finish(wbcqp_handle* h, const Io& io, const FieldBytes& fb, hipStream_t sm) const
    {
        if (!recorded(n_ticks - 1)) return WBCQP_OK;
        for (Field f : {F_qn, F_vn, F_x, F_tau, F_obj, F_status, F_iters})
            if (field(f) && io.p[f] && fb.b[f])
                HIP_TRY(h, hipMemcpyAsync(static_cast<char*>(field(f)) + row0(n_ticks - 1) * fb.b[f], io.p[f], B * fb.b[f], hipMemcpyDeviceToDevice, sm));
        return WBCQP_OK;
    }
};

// The state between the ticks of a roll-out: two halves of a device block, written in turn.  The first tick reads the caller's q / v in place, the last
// one writes the caller's q_next / v_next: the block is touched by the ticks in between only
struct PingPong {
    char* base;
    size_t qb, vb; // bytes of one half of q, of v
    static size_t bytes(size_t qb, size_t vb) { return 2 * (qb + vb); }
    void* q(int half) const { return base + (half & 1) * qb; }
    void* v(int half) const { return base + 2 * qb + (half & 1) * vb; }
};

int tick_impl(wbcqp_handle* h, int slot, int batch, const wbcqp_tick_io* io, void* stream, const RollAcc& acc)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    const Slot* s = slot_with_model(h, slot);
    if (!s) return WBCQP_ERR_INVALID;
    if (batch < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch");
    if (batch == 0) return WBCQP_OK;
    if (!io->q_next || !io->v_next) return fail(h, WBCQP_ERR_INVALID, "q_next / v_next is NULL");
    WB_TRY(wbcqp_problem_data(h, slot, batch, &io->state, &io->rows, stream));
    WB_TRY(wbcqp_solve_batch(h, slot, batch, &io->rows, &io->out, stream));
    return integrate_impl(h, batch, s->terms.nv, s->terms.floating_base, io->dt, io->state.q, io->state.v, io->out.x, s->host.n,
                          io->out.status, io->q_next, io->v_next, io->q_solver, stream, acc);
}

// need_state for a call whose references may come from a program (then state.ref is not read)
int need_state_or_program(wbcqp_handle* h, const TermsDev& T, const wbcqp_state* st, const ProgCall* pc)
{
    if (!pc) return need_state(h, T, st);
    if (!st->q || !st->v) return fail(h, WBCQP_ERR_INVALID, "state arrays q / v are required");
    return WBCQP_OK;
}

// the refusals of a roll-out by program that follow the plain call's: wbcqp_check_program's, then nref and base
int check_program_call(wbcqp_handle* h, const ProgCall& pc, int batch, int n_slots, int nref)
{
    WB_TRY(check_program(h, pc.prog, batch, n_slots));
    if (pc.prog->nref != nref)
        return fail(h, WBCQP_ERR_INVALID, "program: nref " + std::to_string(pc.prog->nref) + " is not the slot's " + std::to_string(nref));
    if (!pc.prog->base) return fail(h, WBCQP_ERR_INVALID, "program: base is NULL");
    return WBCQP_OK;
}

// pc: the references come from a program (wbcqp_rollout_program); null: from io->state.ref
int rollout_impl(wbcqp_handle* h, int slot, int batch, int n_ticks, const wbcqp_rollout_io* io, const wbcqp_trace* tr, void* stream,
                 const ProgCall* pc = nullptr)
{
    if (!h) return WBCQP_ERR_INVALID;
    if (!io) return fail(h, WBCQP_ERR_INVALID, "io is NULL");
    const Slot* sp = slot_with_model(h, slot);
    if (!sp) return WBCQP_ERR_INVALID;
    if (tr && tr->cost && sp->host.n_acteq > 0 && !tr->tau && !io->out.tau)
        return fail(h, WBCQP_ERR_INVALID, "trace: the costs of a stack with a torque task need tau (trace->tau or io->out.tau)");
    if (batch < 0 || n_ticks < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch / n_ticks");
    if (batch == 0 || n_ticks == 0) return WBCQP_OK;
    const Slot& s = *sp;
    const wbcqp_layout& L = s.layout;
    WB_TRY(need_state_or_program(h, s.terms, &io->state, pc));
    if ((L.len_tlb && (!io->tlb || !io->tub)) || !io->w) return fail(h, WBCQP_ERR_INVALID, "tlb / tub / w are required");
    WB_TRY(need_tick_outputs(h, s.host.na, io->out, io->q_next, io->v_next));
    if (pc) WB_TRY(check_program_call(h, *pc, batch, 0, s.terms.nref));
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t sm = static_cast<hipStream_t>(stream);
    const size_t es = elem_size(h);
    const size_t B = (size_t)batch;
    // One sub-batch (what K calls of wbcqp_tick do) or two.  Two pay where a tick's solve has a long tail -- one instance far
    // above the rest, B = 1024: 1.04x -- and cost where it has none (every instance heavy: 0.76x) or where the launch is large
    // enough to hide its tail by itself (B = 4096: 0.93x); three gain less (1.02x), four queue behind one another (0.57x)
    // [tools/rollout_bench.py].  Which regime a caller is in is not knowable from the arguments, so it is measured: the first
    // roll-outs of a (slot, batch) run one sub-batch, then two, each timed on the device by an event pair a LATER call reads
    // without blocking -- the first sample of either form is discarded (it pays that form's allocations, stream creation and a
    // device synchronisation) --; from then on the faster of the two, the other one tried again every 64th call (a workload drifts).  WBCQP_ROLLOUT_STREAMS overrides (1 .. 8).  The result does not depend on the choice, bit for bit.
    for (auto& mz : h->roll_meas) {
        if (!mz.pending || hipEventQuery(mz.t1) != hipSuccess) continue;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, mz.t0, mz.t1) == hipSuccess && mz.ticks > 0 && mz.S >= 1 && mz.S <= 2 && mz.stat >= 0 &&
            mz.stat < (int)h->roll_stats.size()) {
            auto& stt = h->roll_stats[mz.stat];
            double& slot_us = stt.us[mz.S];
            const double us = (double)ms * 1e3 / mz.ticks;
            if (stt.cold[mz.S]) stt.cold[mz.S] = 0; // (the form runs once more before it is compared)
            else slot_us = slot_us > 0.0 ? 0.5 * (slot_us + us) : us;
        }
        mz.pending = false;
    }
    (void)hipGetLastError(); // (hipEventQuery's hipErrorNotReady is not an error of this call)
    int stat_i = -1;
    for (size_t i = 0; i < h->roll_stats.size(); ++i)
        if (h->roll_stats[i].slot == slot && h->roll_stats[i].batch == batch) stat_i = (int)i;
    if (stat_i < 0) {
        if (h->roll_stats.size() >= 64) { // (an index into the table is kept by the pending measurements: start over)
            h->roll_stats.clear();
            for (auto& mz : h->roll_meas) mz.stat = -1;
        }
        h->roll_stats.emplace_back();
        stat_i = (int)h->roll_stats.size() - 1;
        h->roll_stats[stat_i].slot = slot;
        h->roll_stats[stat_i].batch = batch;
    }
    int S = 1;
    {
        auto& stt = h->roll_stats[stat_i];
        if (batch >= 512) {
            bool two_in_flight = false; // a roll-out with two sub-batches is on the device and not measured yet
            for (const auto& mz : h->roll_meas) two_in_flight = two_in_flight || (mz.pending && mz.stat == stat_i && mz.S == 2);
            if (stt.us[1] <= 0.0) S = 1;
            else if (stt.us[2] <= 0.0) S = two_in_flight ? 1 : 2;
            else {
                S = stt.us[2] < stt.us[1] ? 2 : 1;
                const int other = 3 - S;
                if (stt.calls % 64 == 63) S = other; // the other form again, whatever its last figure: a workload drifts, and one inflated sample must not pin the choice
            }
        }
        ++stt.calls;
    }
    if (const char* ev = std::getenv("WBCQP_ROLLOUT_STREAMS")) S = std::max(1, std::min({std::atoi(ev), 8, batch}));
    if (std::getenv("WBCQP_ROLLOUT_DEBUG"))
        std::fprintf(stderr, "wbcqp_rollout: slot %d batch %d ticks %d -> %d sub-batch(es); measured us per tick: one %.1f, two %.1f\n", slot, batch,
                     n_ticks, S, h->roll_stats[stat_i].us[1], h->roll_stats[stat_i].us[2]);
    for (int k = 0; k < S; ++k) { // the handle owns a sub-batch's stream, event and counters from the moment they exist (a failure half
        // way leaves them to wbcqp_destroy)
        if ((int)h->roll_subs.size() <= k) h->roll_subs.emplace_back();
        wbcqp_handle::RollSub& r = h->roll_subs[k];
        if (!r.stream) HIP_TRY(h, hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
        if (!r.done) HIP_TRY(h, hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
        if (!r.ord.queue) {
            HIP_TRY(h, hipMalloc(&r.ord.queue, 2 * sizeof(int)));
            HIP_TRY(h, hipMemset(r.ord.queue, 0, 2 * sizeof(int)));
        }
    }
    if (!h->roll_start) HIP_TRY(h, hipEventCreateWithFlags(&h->roll_start, hipEventDisableTiming));
    const bool had_roll = h->roll_done != nullptr;
    if (!h->roll_done) HIP_TRY(h, hipEventCreateWithFlags(&h->roll_done, hipEventDisableTiming));
    // the record of every instance (the rows kernel's output, the solve's input) and the state ping-pong
    const FieldBytes fb = field_bytes(s, es);
    Arr rec_a[kNumRecord];
    const size_t rec_bytes = lay(fb, B, kRecordFields, kNumRecord, Io{}, rec_a);
    const size_t qb = al256(B * fb.b[F_q]), vb = al256(B * fb.b[F_v]);
    const int sub_cap = (batch + S - 1) / S;
    const size_t ring_bytes = pc ? RefFeed::ring_bytes(B, fb.b[F_ref], h->ref_chunk) : 0;
    bool grow = h->roll_rec.bytes < rec_bytes || h->roll_state.bytes < PingPong::bytes(qb, vb) || h->roll_ref.bytes < ring_bytes;
    for (int k = 0; k < S; ++k) grow = grow || h->roll_subs[k].ord.cap < sub_cap;
    if (grow) { // first call of a larger shape: nothing of an earlier call may still be running on what is replaced
        HIP_TRY(h, hipDeviceSynchronize());
        WB_TRY(ensure(h, h->roll_rec, rec_bytes));
        WB_TRY(ensure(h, h->roll_state, PingPong::bytes(qb, vb)));
        WB_TRY(ensure(h, h->roll_ref, ring_bytes));
        for (int k = 0; k < S; ++k) {
            OrderState& os = h->roll_subs[k].ord;
            if (os.cap < sub_cap) {
                if (os.order) (void)hipFree(os.order);
                os.order = nullptr;
                os.cap = os.total = 0;
                HIP_TRY(h, hipMalloc(&os.order, 2 * sizeof(int) * (size_t)sub_cap));
                os.cap = sub_cap;
            }
        }
    }
    const PingPong pp{static_cast<char*>(h->roll_state.dev), qb, vb};
    // the sub-streams of the previous roll-out may still be on the ping-pong buffers and the record when this one comes in on
    // another stream: wait for that roll-out's end first (on the same stream the wait is already implied)
    if (had_roll) HIP_TRY(h, hipStreamWaitEvent(sm, h->roll_done, 0));
    wbcqp_handle::RollMeas* meas = nullptr; // a free event pair: this roll-out is measured
    for (auto& mz : h->roll_meas)
        if (!mz.pending && !meas) meas = &mz;
    if (meas) {
        if (!meas->t0) HIP_TRY(h, hipEventCreate(&meas->t0));
        if (!meas->t1) HIP_TRY(h, hipEventCreate(&meas->t1));
        HIP_TRY(h, hipEventRecord(meas->t0, sm));
    }
    ProgDev prog_dev; // the program's tables go up on the caller's stream, ahead of roll_start: every sub-batch's stream sees them
    if (pc) WB_TRY(upload_program(h, pc->prog, batch, sm, prog_dev));
    HIP_TRY(h, hipEventRecord(h->roll_start, sm));
    int rc_all = WBCQP_OK;
    // one sub-batch: the ticks go out on the caller's own stream with that stream's launch-order state -- K calls of wbcqp_tick, minus
    // the caller's loop (on a stream of its own the same sequence measured 1.5 % slower than the tick loop: fork, join, a second queue)
    const bool own_stream = S == 1;
    if (!own_stream)
        for (int k = 0; k < S; ++k) HIP_TRY(h, hipStreamWaitEvent(h->roll_subs[k].stream, h->roll_start, 0));
    const TraceWriter tw{tr, B, n_ticks};
    // the caller's arrays of the whole batch; per tick: the record, the state it starts from and the one it leaves, the outputs' destinations
    Io call(nullptr, &io->out, &io->state, io->q_next, io->v_next, io->q_solver);
    call.p[F_tlb] = const_cast<void*>(io->tlb); call.p[F_tub] = const_cast<void*>(io->tub); call.p[F_w] = const_cast<void*>(io->w);
    point(call, h->roll_rec.dev, rec_a, kNumRecord);
    // tick t's references: the caller's array, or the ring a chunk of generated rows ahead
    const RefFeed feed = pc ? RefFeed{static_cast<char*>(h->roll_ref.dev), fb.b[F_ref], B, n_ticks, h->ref_chunk, &prog_dev, pc->tick0}
                            : RefFeed{static_cast<char*>(call.p[F_ref]), fb.b[F_ref], B, n_ticks};
    Io tick = call;
    // tick t of every sub-batch is enqueued before tick t + 1 of any: the streams then advance together on the device (enqueued one
    // sub-batch after the other, the last stream's first tick would reach the device when the first stream is almost through), and the
    // tail of one sub-batch's solve (its longest QP) runs beside the bulk of another's
    for (int t = 0; t < n_ticks && rc_all == WBCQP_OK; ++t) {
        const bool last = t + 1 == n_ticks;
        tick.p[F_ref] = feed.at(t);
        tick.p[F_qn] = tw.dest(t, F_qn, fb.b[F_qn], last ? io->q_next : pp.q(t + 1));
        tick.p[F_vn] = tw.dest(t, F_vn, fb.b[F_vn], last ? io->v_next : pp.v(t + 1));
        for (Field f : {F_x, F_tau, F_obj, F_status, F_iters}) tick.p[f] = tw.dest(t, f, fb.b[f], call.p[f]);
        tick.p[F_mom] = last ? call.p[F_mom] : nullptr;
        tick.p[F_qs] = last ? call.p[F_qs] : nullptr;
        for (int k = 0; k < S && rc_all == WBCQP_OK; ++k) {
            const size_t b0 = (size_t)k * batch / S, b1 = (size_t)(k + 1) * batch / S;
            const int nb = (int)(b1 - b0);
            if (nb == 0) continue;
            wbcqp_handle::RollSub& sub = h->roll_subs[k];
            const wbcqp_tick_io d = tick.from(b0, fb).tick_io(io->dt);
            if ((rc_all = feed.prepare(h, t, (int)b0, nb, own_stream ? sm : sub.stream)) != WBCQP_OK) break;
            h->graph_ord = own_stream ? nullptr : &sub.ord; // a sub-batch's own launch-order state and queue counter (as a captured tick has)
            const RollAcc acc = {d.out.iters, io->iters_sum ? io->iters_sum + b0 : nullptr, io->ticks_ok ? io->ticks_ok + b0 : nullptr, t == 0 ? 1 : 0};
            rc_all = tick_impl(h, slot, nb, &d, own_stream ? sm : sub.stream, acc); // (the per-instance totals ride along with the integration)
            h->graph_ord = nullptr;
            if (rc_all == WBCQP_OK && tw.recorded(t) && tr->cost) // (before the next tick's rows kernel overwrites the record: same stream)
                rc_all = launch_costs(h, s, nb, d.rows.A, d.rows.b1, L.len_Acop ? d.rows.Acop : nullptr, d.out.x, L.n, d.out.tau,
                                      static_cast<char*>(tr->cost) + (tw.row0(t) + b0) * fb.b[F_w], L.len_w, nullptr, own_stream ? sm : sub.stream);
        }
        tick.p[F_q] = tick.p[F_qn]; // the state the next tick starts from
        tick.p[F_v] = tick.p[F_vn];
    }
    for (int k = 0; k < S && !own_stream; ++k) {
        HIP_TRY(h, hipEventRecord(h->roll_subs[k].done, h->roll_subs[k].stream));
        HIP_TRY(h, hipStreamWaitEvent(sm, h->roll_subs[k].done, 0));
    }
    if (rc_all == WBCQP_OK) rc_all = tw.finish(h, call, fb, sm);
    if (pc) HIP_TRY(h, hipEventRecord(prog_dev.up->done, sm));
    HIP_TRY(h, hipEventRecord(h->roll_done, sm));
    if (meas && rc_all == WBCQP_OK) {
        HIP_TRY(h, hipEventRecord(meas->t1, sm));
        meas->stat = stat_i; meas->S = S; meas->ticks = n_ticks; meas->pending = true;
    }
    return rc_all;
}

// ---- wbcqp_tick_mixed / wbcqp_rollout_mixed: one robot model, its instances in different contact sets ----------------------------------------
// Per tick: the rows kernel once per non-empty set (terms_kernel<., true>: instances gathered through the tick's permutation, the record of
// the set written contiguously), ONE solve launch over the sets (wbcqp_solve_ragged), one kernel that scatters the outputs back to instance
// order and integrates every instance from its set's x (mixed_integrate_kernel).  The host makes the plan: which instances each set holds
// on each tick.
struct MixCall { // the checked arguments of a mixed call
    const wbcqp_mix* mix;
    int batch, n_ticks;
    const int32_t* which;  // [n_ticks][batch]
    wbcqp_state state;     // ref: [n_ticks][batch][nref]
    wbcqp_outputs out;
    void *q_next, *v_next, *q_solver;
    double dt;
    int32_t *iters_sum, *ticks_ok;
    const wbcqp_trace* trace; // null: untraced
    const ProgCall* prog = nullptr; // the references come from a program and `which` is made from its set_of (wbcqp_rollout_mixed_program)
};

int check_mix(wbcqp_handle* h, const MixCall& c)
{
    if (h->flags & WBCQP_FLAG_WARM_START) return fail(h, WBCQP_ERR_UNSUPPORTED, "mixed contact sets: no warm start (a hint does not carry across a change of contact set)");
    const wbcqp_mix* mix = c.mix;
    if (!mix) return fail(h, WBCQP_ERR_INVALID, "mix is NULL");
    if (mix->n_slots < 1 || mix->n_slots > kMaxGroups) return fail(h, WBCQP_ERR_INVALID, "mix: n_slots must be in [1, 8]");
    if (!mix->slots || !mix->w) return fail(h, WBCQP_ERR_INVALID, "mix: slots / w is NULL");
    const Slot* s0 = nullptr;
    for (int k = 0; k < mix->n_slots; ++k) {
        const int sl = mix->slots[k];
        if (sl < 0 || sl >= WBCQP_MAX_STRUCTURES || !h->slots[sl].set || !h->slots[sl].has_model)
            return fail(h, WBCQP_ERR_INVALID, "mix: slot " + std::to_string(sl) + " has no structure and model (wbcqp_set_model)");
        const Slot& s = h->slots[sl];
        if (!s0) { s0 = &s; continue; }
        if (s.tree != s0->tree || s.terms.nq != s0->terms.nq || s.terms.nv != s0->terms.nv || s.terms.na != s0->terms.na)
            return fail(h, WBCQP_ERR_INVALID, "mix: slot " + std::to_string(sl) + " has another robot model than slot " + std::to_string(mix->slots[0]));
        if (s.terms.nref != s0->terms.nref || s.terms.dt != s0->terms.dt)
            return fail(h, WBCQP_ERR_INVALID, "mix: slot " + std::to_string(sl) + " has another reference length (nref) or dt than slot " + std::to_string(mix->slots[0]));
    }
    if (c.batch < 0 || c.n_ticks < 0) return fail(h, WBCQP_ERR_INVALID, "negative batch / n_ticks");
    if (c.batch == 0 || c.n_ticks == 0) return WBCQP_OK;
    if (!c.which && !c.prog) return fail(h, WBCQP_ERR_INVALID, "which / schedule is NULL");
    bool used[kMaxGroups] = {};
    const size_t N = c.which ? (size_t)c.batch * c.n_ticks : 0; // (a call by program comes here twice: before its schedule exists, and with it)
    for (size_t e = 0; e < N; ++e) {
        const int k = c.which[e];
        if (k < 0 || k >= mix->n_slots)
            return fail(h, WBCQP_ERR_INVALID, "which / schedule entry " + std::to_string(e) + " = " + std::to_string(k) + " is outside [0, n_slots)");
        used[k] = true;
    }
    for (int k = 0; k < mix->n_slots; ++k) {
        if (!used[k]) continue;
        const Slot& s = h->slots[mix->slots[k]];
        if (s.layout.len_w > 0 && !mix->w[k]) return fail(h, WBCQP_ERR_INVALID, "mix: w of slot " + std::to_string(mix->slots[k]) + " is NULL and instances use it");
        if (s.layout.len_tlb > 0 && (!mix->tlb || !mix->tub)) return fail(h, WBCQP_ERR_INVALID, "mix: tlb / tub are required (a slot in use has actuation bounds)");
    }
    WB_TRY(need_state_or_program(h, s0->terms, &c.state, c.prog));
    return need_tick_outputs(h, s0->terms.na, c.out, c.q_next, c.v_next);
}

// one set's arrays in the record scratch of a tick: the rows kernel's output (9), the gathered w, tlb, tub, the solve's outputs
constexpr Field kMixFields[] = {F_M, F_h, F_A, F_b1, F_Ac, F_bc, F_blb, F_bub, F_Acop, F_w, F_tlb, F_tub, F_x, F_tau, F_obj, F_status, F_iters, F_nact, F_amask};
constexpr int kNumMix = (int)(sizeof(kMixFields) / sizeof(kMixFields[0]));

template <typename TI>
int mixed_run(wbcqp_handle* h, const MixCall& c, hipStream_t sm)
{
    const wbcqp_mix& mix = *c.mix;
    const int B = c.batch, K = mix.n_slots;
    const Slot& s0 = h->slots[mix.slots[0]];
    const TermsDev& T0 = s0.terms;
    constexpr size_t es = sizeof(TI);
    int ldx = 0, ldc = 0;
    for (int k = 0; k < K; ++k) ldx = std::max(ldx, h->slots[mix.slots[k]].layout.n);
    for (int k = 0; k < K; ++k) ldc = std::max(ldc, h->slots[mix.slots[k]].layout.len_w);
    // the caller's arrays by instance: the model's sizes, x rows ldx wide (the largest n over the mix)
    FieldBytes fb = field_bytes(s0, es);
    fb.b[F_x] = (size_t)ldx * es;
    const Io call(nullptr, &c.out, &c.state, c.q_next, c.v_next, c.q_solver);
    const TraceWriter tw{c.trace, (size_t)B, c.n_ticks};
    // the plan: per tick, the instances of set 0, then of set 1, ... (ascending within a set), and the sets' counts
    std::vector<int> counts((size_t)c.n_ticks * K, 0);
    for (int t = 0; t < c.n_ticks; ++t)
        for (int i = 0; i < B; ++i) ++counts[(size_t)t * K + c.which[(size_t)t * B + i]];
    Arr ga[kNumMix];
    size_t rec_bytes = 0;
    for (int t = 0; t < c.n_ticks; ++t) {
        size_t bytes = 0;
        for (int k = 0; k < K; ++k)
            if (counts[(size_t)t * K + k]) bytes += lay(field_bytes(h->slots[mix.slots[k]], es), counts[(size_t)t * K + k], kMixFields, kNumMix, Io{}, ga);
        rec_bytes = std::max(rec_bytes, bytes);
    }
    const size_t plan_ints = (size_t)c.n_ticks * B;
    const size_t qb = al256((size_t)B * fb.b[F_q]), vb = al256((size_t)B * fb.b[F_v]);
    const size_t state_bytes = c.n_ticks > 1 ? PingPong::bytes(qb, vb) : 0;
    wbcqp_handle::MixPlan& P = h->mix_plan[h->mix_next];
    h->mix_next = (h->mix_next + 1) % 4;
    if (P.used) HIP_TRY(h, hipEventSynchronize(P.done)); // (the call that last filled this entry: four calls ago)
    if (!P.done) HIP_TRY(h, hipEventCreateWithFlags(&P.done, hipEventDisableTiming));
    const bool had_mix = h->mix_done != nullptr;
    if (!h->mix_done) HIP_TRY(h, hipEventCreateWithFlags(&h->mix_done, hipEventDisableTiming));
    const size_t ring_bytes = c.prog ? RefFeed::ring_bytes((size_t)B, fb.b[F_ref], h->ref_chunk) : 0;
    if (P.cap < plan_ints || h->mix_rec.bytes < rec_bytes || h->mix_state.bytes < state_bytes || h->mix_ref.bytes < ring_bytes) {
        // first call of a larger shape: nothing of an earlier call may still be running on what is replaced
        HIP_TRY(h, hipDeviceSynchronize());
        if (P.cap < plan_ints) {
            if (P.dev) (void)hipFree(P.dev);
            P.dev = nullptr;
            P.cap = 0;
            HIP_TRY(h, hipMalloc(&P.dev, plan_ints * sizeof(int)));
            P.cap = plan_ints;
        }
        WB_TRY(ensure(h, h->mix_rec, rec_bytes));
        if (state_bytes) WB_TRY(ensure(h, h->mix_state, state_bytes));
        WB_TRY(ensure(h, h->mix_ref, ring_bytes));
    }
    WB_TRY(ensure_pinned(h, P.pin, plan_ints * sizeof(int)));
    int* perm_h = static_cast<int*>(P.pin.host);
    for (int t = 0; t < c.n_ticks; ++t) {
        int pos[kMaxGroups];
        for (int k = 0, o = 0; k < K; ++k) { pos[k] = o; o += counts[(size_t)t * K + k]; }
        for (int i = 0; i < B; ++i) perm_h[(size_t)t * B + pos[c.which[(size_t)t * B + i]]++] = i;
    }
    // the force blocks' factor cache of every slot of the mix, before the first tick (a cache made in the middle of a roll-out would wait for it)
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(sm, &cst) != hipSuccess) (void)hipGetLastError();
    for (int k = 0; k < K && cst == hipStreamCaptureStatusNone; ++k) {
        Slot& s = h->slots[mix.slots[k]];
        const bool wave_small = !(h->flags & WBCQP_FLAG_WORKGROUP_PER_QP) && !h->dbg && s.small;
        if (s.host_cp.compact && s.ffc_dev && !s.ffc_built && !h->capturing && !wave_small && mix.w[k]) WB_TRY(build_ffcache(h, s, mix.w[k], sm));
    }
    if (had_mix) HIP_TRY(h, hipStreamWaitEvent(sm, h->mix_done, 0)); // the previous mixed call is done with the records and the ping-pong
    HIP_TRY(h, hipMemcpyAsync(P.dev, perm_h, plan_ints * sizeof(int), hipMemcpyHostToDevice, sm));
    P.used = true;
    ProgDev prog_dev;
    if (c.prog) WB_TRY(upload_program(h, c.prog->prog, B, sm, prog_dev));
    const RefFeed feed = c.prog ? RefFeed{static_cast<char*>(h->mix_ref.dev), fb.b[F_ref], (size_t)B, c.n_ticks, h->ref_chunk, &prog_dev, c.prog->tick0}
                                : RefFeed{static_cast<char*>(call.p[F_ref]), fb.b[F_ref], (size_t)B, c.n_ticks};
    char* rec = static_cast<char*>(h->mix_rec.dev);
    const PingPong pp{static_cast<char*>(h->mix_state.dev), qb, vb};
    Io tick = call; // the arrays of one tick, by instance: the state it starts from and the one it leaves, the outputs' destinations
    for (int t = 0; t < c.n_ticks; ++t) {
        const bool last = t + 1 == c.n_ticks;
        tick.p[F_ref] = feed.at(t);
        WB_TRY(feed.prepare(h, t, 0, B, sm));
        tick.p[F_mom] = last ? call.p[F_mom] : nullptr;
        tick.p[F_qn] = tw.dest(t, F_qn, fb.b[F_qn], last ? c.q_next : pp.q(t));
        tick.p[F_vn] = tw.dest(t, F_vn, fb.b[F_vn], last ? c.v_next : pp.v(t));
        const int* perm = P.dev + (size_t)t * B;
        wbcqp_group groups[kMaxGroups];
        MixedScatterArgs<TI> sa{};
        int ng = 0, o = 0;
        size_t base = 0;
        for (int k = 0; k < K; ++k) {
            const int cnt = counts[(size_t)t * K + k];
            if (cnt == 0) continue;
            const Slot& s = h->slots[mix.slots[k]];
            Io g = tick; // the set's record, gathered weights and outputs in the scratch; the state by instance
            const size_t bytes = lay(field_bytes(s, es), cnt, kMixFields, kNumMix, Io{}, ga);
            point(g, rec + base, ga, kNumMix);
            base += bytes;
            auto at = [&](Field f) -> TI* { return static_cast<TI*>(g.p[f]); };
            const bool tl = s.layout.len_tlb > 0;
            TermsGatherArgs<TI> a{};
            fill_terms(a, h, s, cnt, g);
            a.perm = perm + o;
            a.w_src = static_cast<const TI*>(mix.w[k]); a.w_dst = at(F_w); a.n_tasks = s.layout.len_w;
            a.tlb_src = tl ? static_cast<const TI*>(mix.tlb) : nullptr; a.tub_src = tl ? static_cast<const TI*>(mix.tub) : nullptr;
            a.tlb_dst = tl ? at(F_tlb) : nullptr; a.tub_dst = tl ? at(F_tub) : nullptr;
            hipLaunchKernelGGL((terms_kernel<TI, true>), dim3(cnt), dim3(kTermsThreads), s.terms.lds_doubles * 8, sm, a);
            HIP_TRY(h, hipGetLastError());
            if (!tl) g.p[F_tlb] = g.p[F_tub] = nullptr;
            if (!s.layout.len_Acop) g.p[F_Acop] = nullptr;
            wbcqp_group& G = groups[ng];
            G.slot = mix.slots[k];
            G.batch = cnt;
            G.in = g.inputs();
            G.out = g.outputs();
            MixedGroupOut<TI>& M = sa.g[ng];
            M.x = at(F_x); M.tau = at(F_tau); M.objective = at(F_obj);
            M.status = G.out.status; M.iters = G.out.iters; M.n_active = G.out.n_active; M.amask = G.out.active_mask;
            M.n = s.layout.n;
            sa.off[ng] = o;
            o += cnt;
            ++ng;
        }
        sa.off[ng] = o;
        WB_TRY(wbcqp_solve_ragged(h, ng, groups, sm));
        sa.n_groups = ng; sa.total = B; sa.nv = T0.nv; sa.na = T0.na; sa.floating_base = T0.floating_base; sa.ldx = ldx;
        sa.perm = perm; sa.dt = c.dt; sa.q = static_cast<const TI*>(tick.p[F_q]); sa.v = static_cast<const TI*>(tick.p[F_v]);
        sa.q_next = static_cast<TI*>(tick.p[F_qn]); sa.v_next = static_cast<TI*>(tick.p[F_vn]);
        sa.q_solver = last ? static_cast<TI*>(c.q_solver) : nullptr;
        // the caller's outputs are those of the last tick only (what a roll-out reports); a recorded tick before it writes its entry
        auto dest = [&](Field f) { return tw.dest(t, f, fb.b[f], last ? call.p[f] : nullptr); };
        sa.x = static_cast<TI*>(dest(F_x)); sa.tau = static_cast<TI*>(dest(F_tau)); sa.objective = static_cast<TI*>(dest(F_obj));
        sa.status = static_cast<int*>(dest(F_status)); sa.iters = static_cast<int*>(dest(F_iters));
        if (last) { sa.n_active = c.out.n_active; sa.amask = c.out.active_mask; }
        sa.iters_sum = c.iters_sum; sa.ticks_ok = c.ticks_ok; sa.first = t == 0 ? 1 : 0;
        hipLaunchKernelGGL(mixed_integrate_kernel<TI>, dim3((B + 3) / 4), dim3(256), 0, sm, sa);
        HIP_TRY(h, hipGetLastError());
        if (tw.recorded(t) && c.trace->cost) // every set's costs from its own record and outputs, rows put in instance order and ldc wide (before the next tick's rows kernels)
            for (int g = 0; g < ng; ++g)
                WB_TRY(launch_costs(h, h->slots[groups[g].slot], groups[g].batch, groups[g].in.A, groups[g].in.b1, groups[g].in.Acop, groups[g].out.x,
                                    sa.g[g].n, groups[g].out.tau, static_cast<TI*>(c.trace->cost) + tw.row0(t) * ldc, ldc, perm + sa.off[g], sm));
        tick.p[F_q] = tick.p[F_qn];
        tick.p[F_v] = tick.p[F_vn];
    }
    WB_TRY(tw.finish(h, call, fb, sm));
    if (c.prog) HIP_TRY(h, hipEventRecord(prog_dev.up->done, sm));
    HIP_TRY(h, hipEventRecord(P.done, sm));
    HIP_TRY(h, hipEventRecord(h->mix_done, sm));
    return WBCQP_OK;
}

int mixed_call(wbcqp_handle* h, const MixCall& c0, void* stream)
{
    int rc = check_mix(h, c0);
    if (rc != WBCQP_OK || c0.batch == 0 || c0.n_ticks == 0) return rc;
    MixCall c = c0;
    if (c.prog) { // the program's refusals, then the schedule from its set_of and what the plain call checks of a schedule
        WB_TRY(check_program_call(h, *c.prog, c.batch, c.mix->n_slots, h->slots[c.mix->slots[0]].terms.nref));
        if (!c.prog->prog->set_of) return fail(h, WBCQP_ERR_INVALID, "program: a mixed roll-out needs set_of");
        program_schedule(c.prog->prog, c.batch, c.prog->tick0, c.n_ticks, h->prog_sched);
        c.which = h->prog_sched.data();
        WB_TRY(check_mix(h, c));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return with_dtype(h, [&](auto tag) -> int { return mixed_run<WB_TI(tag)>(h, c, static_cast<hipStream_t>(stream)); });
}

} // namespace
