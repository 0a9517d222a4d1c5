// wbcqp_host_program.hpp -- host side of the C ABI (wbcqp_api.hip): reference programs (wbcqp_program) -- the checks, the tables' way to the device, the
// launches of refgen_kernel, the schedule of a mixed roll-out, and RefFeed: where the references of tick t of a roll-out live, whether the caller brought
// them as an array or the library generates them.  Included by wbcqp_host_rollout.hpp.
#pragma once
#include "wbcqp_host_launch.hpp"
#include "wbcqp_refgen.hpp"

namespace {

inline int track_ncomp(const wbcqp_track& t) { return t.kind == WBCQP_TRACK_SE3 ? 24 : (t.dim == 3 ? 9 : 1); }

// wbcqp_check_program; h may be null (the device-free entry point)
int check_program(wbcqp_handle* h, const wbcqp_program* p, int batch, int n_slots)
{
    auto bad = [&](const std::string& m) { return fail(h, WBCQP_ERR_INVALID, "program: " + m); };
    if (!p) return bad("is NULL");
    if (batch < 0) return bad("negative batch");
    if (p->n_tracks < 0 || p->n_tracks > WBCQP_MAX_TRACKS) return bad(std::to_string(p->n_tracks) + " tracks, at most " + std::to_string(WBCQP_MAX_TRACKS));
    if (p->n_intro < 0 || p->n_cycle < 0 || (long long)p->n_intro + p->n_cycle < 1) return bad("empty timeline (n_intro + n_cycle < 1)");
    if (p->nref < 1) return bad("nref < 1");
    if (!(p->dt > 0.0)) return bad("dt <= 0");
    if (batch > 0 && !p->offset) return bad("offset is NULL");
    if (p->n_tracks > 0 && !p->tracks) return bad("tracks is NULL");
    const long long len = (long long)p->n_intro + p->n_cycle;
    struct Extent { int lo, hi, track; };
    std::vector<Extent> ext;
    for (int k = 0; k < p->n_tracks; ++k) {
        const wbcqp_track& t = p->tracks[k];
        const std::string tk = "track " + std::to_string(k) + ": ";
        if (t.kind != WBCQP_TRACK_VEC && t.kind != WBCQP_TRACK_SE3) return bad(tk + "unknown kind " + std::to_string(t.kind));
        if (t.kind == WBCQP_TRACK_VEC && t.dim != 1 && t.dim != 3) return bad(tk + "dim " + std::to_string(t.dim) + " is not 1 or 3");
        if (t.n_segments < 1 || !t.segments) return bad(tk + "no segments");
        long long sum = 0;
        for (int s = 0; s < t.n_segments; ++s) {
            const wbcqp_segment& g = t.segments[s];
            const std::string sk = tk + "segment " + std::to_string(s) + ": ";
            if (g.n_steps < 1) return bad(sk + "n_steps < 1");
            if (!(g.T > 0.0)) return bad(sk + "T <= 0");
            if (t.kind == WBCQP_TRACK_SE3) {
                const double n2 = g.axis[0] * g.axis[0] + g.axis[1] * g.axis[1] + g.axis[2] * g.axis[2];
                if (!(std::fabs(n2 - 1.0) <= 1e-9)) return bad(sk + "axis is not a unit vector");
            }
            sum += g.n_steps;
        }
        if (sum != len) return bad(tk + "segments cover " + std::to_string(sum) + " ticks, the timeline has " + std::to_string(len));
        const int nc = track_ncomp(t);
        for (int d = 0; d < 2; ++d) {
            if (d == 1 && t.dst[1] < 0) continue;
            if (t.dst[d] < 0 || (long long)t.dst[d] + nc > p->nref)
                return bad(tk + "destination [" + std::to_string(t.dst[d]) + ", " + std::to_string((long long)t.dst[d] + nc) + ") leaves [0, nref = " + std::to_string(p->nref) + ")");
            for (const Extent& e : ext)
                if (t.dst[d] < e.hi && e.lo < t.dst[d] + nc)
                    return bad(tk + "destination [" + std::to_string(t.dst[d]) + ", " + std::to_string(t.dst[d] + nc) + ") overlaps track " + std::to_string(e.track) + "'s");
            ext.push_back({t.dst[d], t.dst[d] + nc, k});
        }
    }
    if (p->set_of && n_slots > 0)
        for (long long i = 0; i < len; ++i)
            if (p->set_of[i] < 0 || p->set_of[i] >= n_slots)
                return bad("set_of[" + std::to_string(i) + "] = " + std::to_string(p->set_of[i]) + " is outside [0, n_slots = " + std::to_string(n_slots) + ")");
    return WBCQP_OK;
}

// a checked program on the device: the header (by value with every launch), the segments and the offsets (one block, one copy per call)
struct ProgDev {
    RefProg P{};
    const RefSeg* segs = nullptr;
    const int* offset = nullptr;
    const void* base = nullptr;
    int base_stride = 0;
    wbcqp_handle::ProgUp* up = nullptr;
};

int upload_program(wbcqp_handle* h, const wbcqp_program* p, int batch, hipStream_t sm, ProgDev& d)
{
    RefProg& P = d.P;
    P.nref = p->nref; P.n_intro = p->n_intro; P.n_cycle = p->n_cycle; P.n_tracks = p->n_tracks; P.dt = p->dt;
    int nseg = 0;
    for (int k = 0; k < p->n_tracks; ++k) nseg += p->tracks[k].n_segments;
    const size_t seg_bytes = al256((size_t)std::max(nseg, 1) * sizeof(RefSeg)), bytes = seg_bytes + (size_t)batch * sizeof(int);
    wbcqp_handle::ProgUp& U = h->prog_up[h->prog_next];
    h->prog_next = (h->prog_next + 1) % 4;
    if (U.used) HIP_TRY(h, hipEventSynchronize(U.done)); // (the call that last filled this entry: four calls ago)
    if (!U.done) HIP_TRY(h, hipEventCreateWithFlags(&U.done, hipEventDisableTiming));
    if (U.cap < bytes) {
        if (U.dev) (void)hipFree(U.dev);
        U.dev = nullptr;
        U.cap = 0;
        HIP_TRY(h, hipMalloc(&U.dev, bytes));
        U.cap = bytes;
    }
    WB_TRY(ensure_pinned(h, U.pin, bytes));
    RefSeg* sh = static_cast<RefSeg*>(U.pin.host);
    int s0 = 0;
    for (int k = 0; k < p->n_tracks; ++k) {
        const wbcqp_track& t = p->tracks[k];
        P.tr[k] = RefTrack{t.kind, t.kind == WBCQP_TRACK_SE3 ? 3 : t.dim, t.flags, t.dst[0], t.dst[1] < 0 ? -1 : t.dst[1], s0, t.n_segments, track_ncomp(t)};
        int start = 0;
        for (int s = 0; s < t.n_segments; ++s) {
            const wbcqp_segment& g = t.segments[s];
            RefSeg& r = sh[s0 + s];
            r.T = g.T; r.angle = g.angle; r.start = start; r.n_steps = g.n_steps;
            std::memcpy(r.x0, g.x0, sizeof(r.x0)); std::memcpy(r.xf, g.xf, sizeof(r.xf));
            std::memcpy(r.R0, g.R0, sizeof(r.R0)); std::memcpy(r.axis, g.axis, sizeof(r.axis));
            start += g.n_steps;
        }
        s0 += t.n_segments;
    }
    std::memcpy(static_cast<char*>(U.pin.host) + seg_bytes, p->offset, (size_t)batch * sizeof(int));
    HIP_TRY(h, hipMemcpyAsync(U.dev, U.pin.host, bytes, hipMemcpyHostToDevice, sm));
    U.used = true;
    d.segs = static_cast<const RefSeg*>(U.dev);
    d.offset = reinterpret_cast<const int*>(static_cast<char*>(U.dev) + seg_bytes);
    d.base = p->base;
    d.base_stride = p->base_stride ? 1 : 0;
    d.up = &U;
    return WBCQP_OK;
}

// rows of instances [inst0, inst0 + n_inst) for n_ticks ticks from behaviour-time tick_first on, to out (tick stride: batch rows), ticks_per_block per workgroup
int launch_refgen(wbcqp_handle* h, const ProgDev& d, int batch, int inst0, int n_inst, long long tick_first, int n_ticks, int ticks_per_block, void* out,
                  hipStream_t sm)
{
    if (n_inst <= 0 || n_ticks <= 0) return WBCQP_OK;
    return with_dtype(h, [&](auto tag) -> int {
        using TI = WB_TI(tag);
        RefGenArgs<TI> a{d.P, d.segs, d.offset, static_cast<const TI*>(d.base), d.base_stride, static_cast<TI*>(out), batch, inst0, tick_first, n_ticks, ticks_per_block};
        const dim3 grid((unsigned)n_inst, (unsigned)((n_ticks + ticks_per_block - 1) / ticks_per_block));
        hipLaunchKernelGGL(refgen_kernel<TI>, grid, dim3(kRefThreads), refgen_lds_bytes(d.P.nref, d.P.n_tracks), sm, a);
        HIP_TRY(h, hipGetLastError());
        return WBCQP_OK;
    });
}

// A roll-out by program: the call's tick0 and the program.  The roll-outs check it, send it up and build a RefFeed from it
struct ProgCall {
    const wbcqp_program* prog;
    int tick0;
};

// Where tick t's references live.  The caller's array [n_ticks][batch][nref], or a ring of two chunks of C ticks that refgen_kernel fills one chunk ahead
// of the ticks that read it: chunk c + 1 is enqueued when chunk c's first tick is, on the stream that runs these instances' ticks, so it writes the half
// that chunk c - 1's ticks -- enqueued before it on that stream -- are done with.
struct RefFeed {
    char* base = nullptr;      // the array, or the ring
    size_t row_bytes = 0;      // one instance's row
    size_t batch = 0;
    int n_ticks = 0;
    int C = 0;                 // 0: the caller's array
    const ProgDev* prog = nullptr;
    long long tick0 = 0;
    static size_t ring_bytes(size_t batch, size_t row_bytes, int C) { return 2 * (size_t)C * batch * row_bytes; }
    void* at(int t) const
    {
        if (!base) return nullptr;
        const size_t row = C ? (size_t)((t / C) & 1) * C + (size_t)(t % C) : (size_t)t;
        return base + row * batch * row_bytes;
    }
    // before tick t of instances [inst0, inst0 + n_inst) is enqueued on sm
    int prepare(wbcqp_handle* h, int t, int inst0, int n_inst, hipStream_t sm) const
    {
        if (!C || t % C) return WBCQP_OK;
        const int c = t / C;
        for (int g = c == 0 ? 0 : c + 1; g <= c + 1; ++g) {
            const int t0 = g * C, n = std::min(C, n_ticks - t0);
            if (n <= 0) break;
            WB_TRY(launch_refgen(h, *prog, (int)batch, inst0, n_inst, tick0 + t0, n, n, at(t0), sm));
        }
        return WBCQP_OK;
    }
};

// the schedule of a mixed roll-out [n_ticks][batch] from set_of, offset and tick0
void program_schedule(const wbcqp_program* p, int batch, int tick0, int n_ticks, std::vector<int32_t>& out)
{
    out.resize((size_t)batch * n_ticks);
    for (int t = 0; t < n_ticks; ++t)
        for (int i = 0; i < batch; ++i)
            out[(size_t)t * batch + i] = p->set_of[ref_sample_index((long long)tick0 + t - p->offset[i], p->n_intro, p->n_cycle)];
}

} // namespace
