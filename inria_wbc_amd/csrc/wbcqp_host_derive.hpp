// wbcqp_host_derive.hpp -- host side of the C ABI (wbcqp_api.hip): what a structure, a tree and its task bindings are turned into before anything is
// uploaded -- sizes, the LDS layouts (full and compact), the rows kernel's tables.  Pure host arithmetic: wbcqp_layout_of and wbcqp_check_model run it
// without a device.  Included by wbcqp_api.hip alone.
#pragma once
#include "wbcqp_host_handle.hpp"

namespace {

int odd(int v) { return v | 1; }
void set_lds(wbcqp_layout& L, int lds_bytes, bool compact = false, bool act_bounds = false, int spec = 0);

// Validates a structure and derives sizes + LDS layout. Pure host code.
int derive(const wbcqp_structure* st, DevStruct& D, HostBlocks& HB, wbcqp_layout& L, std::string& why)
{
    if (!st) { why = "structure is NULL"; return WBCQP_ERR_INVALID; }
    if (st->nv <= 0 || st->na < 0 || st->na > st->nv || st->nc < 0) { why = "bad nv/na/nc"; return WBCQP_ERR_INVALID; }
    if (st->n_dense < 0 || st->n_sel < 0 || st->n_tasks <= 0 || st->n_bound < 0) { why = "bad level-1 sizes"; return WBCQP_ERR_INVALID; }
    if (st->n_ineq_blocks < 0 || st->n_ineq_blocks > WBCQP_MAX_INEQ_BLOCKS) { why = "too many inequality blocks"; return WBCQP_ERR_INVALID; }
    std::memset(&D, 0, sizeof(D));
    std::memset(&L, 0, sizeof(L));
    D.nv = st->nv; D.na = st->na; D.nc = st->nc; D.k = 12 * st->nc; D.n = D.nv + D.k; D.nu = D.nv - D.na;
    if (D.n > WBCQP_MAX_VARS) { why = "n = nv + 12 nc exceeds WBCQP_MAX_VARS"; return WBCQP_ERR_UNSUPPORTED; }
    if (D.nv > 64) { why = "nv exceeds 64 (the dv block is factorised on a 64 x 64 register grid)"; return WBCQP_ERR_UNSUPPORTED; }
    if (st->nc > 15) { why = "more than 15 contacts"; return WBCQP_ERR_UNSUPPORTED; }
    if (st->n_tasks > kSlot || st->n_dense > kSlot || st->n_bound > kSlot || 6 * st->nc > kSlot) { why = "a per-QP vector exceeds 128 entries"; return WBCQP_ERR_UNSUPPORTED; }
    D.n_dense = st->n_dense; D.n_tasks = st->n_tasks; D.n_sel = st->n_sel; D.n_bound = st->n_bound;
    D.act_bounds = st->act_bounds ? 1 : 0;
    D.neq = D.nu + 6 * D.nc;
    // level-1 tasks that couple the blocks of H ("torque", "cop"): H dense, full layout
    D.n_acteq = st->n_acteq;
    D.acteq_task = st->acteq_task;
    D.cop_task = st->cop_task;
    if (D.n_acteq < 0 || D.n_acteq > D.na) { why = "n_acteq outside [0, na]"; return WBCQP_ERR_INVALID; }
    if (D.n_acteq > 0) {
        if (!st->acteq_joint || !st->acteq_scale) { why = "acteq_joint / acteq_scale is NULL"; return WBCQP_ERR_INVALID; }
        if (D.acteq_task < 0 || D.acteq_task >= D.n_tasks) { why = "acteq_task out of range"; return WBCQP_ERR_INVALID; }
        for (int j = 0; j < D.n_acteq; ++j)
            if (st->acteq_joint[j] < 0 || st->acteq_joint[j] >= D.na || (j > 0 && st->acteq_joint[j] <= st->acteq_joint[j - 1])) { why = "acteq_joint must be ascending in [0, na)"; return WBCQP_ERR_INVALID; }
    }
    if (D.cop_task >= D.n_tasks) { why = "cop_task out of range"; return WBCQP_ERR_INVALID; }
    if (D.cop_task < 0) D.cop_task = -1;
    if (D.cop_task >= 0 && D.nc == 0) { why = "a cop task needs a contact"; return WBCQP_ERR_INVALID; }
    if (D.cop_task >= 0) {
        // A cop task is a task of its own: its index into w is shared with no other row.  This is also what catches the C idiom the field is a trap
        // for -- a zero-initialised (memset) structure says cop_task = 0, which is some dense or selection task's index in every real stack
        bool shared = (D.n_acteq > 0 && D.acteq_task == D.cop_task);
        for (int r = 0; r < st->n_dense && st->dense_row_task && !shared; ++r) shared = st->dense_row_task[r] == D.cop_task;
        for (int r = 0; r < st->n_sel && st->sel_task && !shared; ++r) shared = st->sel_task[r] == D.cop_task;
        for (int c2 = 0; c2 < st->nc && st->forcereg_task && !shared; ++c2) shared = st->forcereg_task[c2] == D.cop_task;
        if (shared) {
            why = "cop_task " + std::to_string(D.cop_task) + " is also the task of other level-1 rows: a cop task has a weight of its own (a structure WITHOUT a cop "
                  "task sets cop_task = -1; zero-initialisation alone declares one on task 0)";
            return WBCQP_ERR_INVALID;
        }
    }
    D.dense_h = (D.n_acteq > 0 || D.cop_task >= 0) ? 1 : 0;
    if (D.dense_h && D.n > 80) { why = "a torque / cop task makes H dense: supported for n <= 80 (the dense seam, wbcqp_solve_dense, carries n <= 99)"; return WBCQP_ERR_UNSUPPORTED; }
    if (D.cop_task >= 0 && 3 * D.k > kSlot) { why = "cop rows exceed one 128-entry slot"; return WBCQP_ERR_UNSUPPORTED; }
    D.r1 = D.n_dense + D.n_sel + 6 * D.nc + D.n_acteq + (D.cop_task >= 0 ? 3 : 0);
    HB.n_blocks = st->n_ineq_blocks;
    int off = 0;
    bool has_act = false;
    int act_off = -1, n_act_blocks = 0;
    for (int b = 0; b < HB.n_blocks; ++b) {
        const int kind = st->ineq_kind[b];
        int rows;
        if (kind == WBCQP_INEQ_BOUNDS) rows = D.n_bound;
        else if (kind == WBCQP_INEQ_ACTUATION) { rows = D.na; has_act = true; act_off = off; ++n_act_blocks; }
        else if (kind == WBCQP_INEQ_FORCE) {
            rows = 17;
            if (st->ineq_arg[b] < 0 || st->ineq_arg[b] >= D.nc) { why = "force block names a missing contact"; return WBCQP_ERR_INVALID; }
        }
        else { why = "unknown inequality kind"; return WBCQP_ERR_INVALID; }
        HB.blk_kind[b] = kind; HB.blk_arg[b] = st->ineq_arg[b]; HB.blk_off[b] = off; HB.blk_rows[b] = rows;
        off += 2 * rows;
    }
    if (has_act != (D.act_bounds != 0)) { why = "act_bounds flag and inequality blocks disagree"; return WBCQP_ERR_INVALID; }
    D.nin2 = off;
    D.act_off = (n_act_blocks == 1) ? act_off : -1;
    if (D.nin2 > 4 * kSlot) { why = "more than 512 one-sided inequality rows"; return WBCQP_ERR_UNSUPPORTED; }
    if (D.r1 > 2 * kSlot) { why = "more than 256 level-1 rows"; return WBCQP_ERR_UNSUPPORTED; }
    if (D.neq > D.n) { why = "more equalities than variables"; return WBCQP_ERR_INVALID; }
    for (int r = 0; r < D.n_dense; ++r)
        if (st->dense_row_task[r] < 0 || st->dense_row_task[r] >= D.n_tasks) { why = "dense_row_task out of range"; return WBCQP_ERR_INVALID; }
    for (int r = 0; r < D.n_sel; ++r)
        if (st->sel_col[r] < 0 || st->sel_col[r] >= D.nv || st->sel_task[r] < 0 || st->sel_task[r] >= D.n_tasks) { why = "selection row out of range"; return WBCQP_ERR_INVALID; }
    for (int r = 0; r < D.n_bound; ++r)
        if (st->bound_col[r] < 0 || st->bound_col[r] >= D.nv) { why = "bound_col out of range"; return WBCQP_ERR_INVALID; }
    for (int c = 0; c < D.nc; ++c)
        if (st->forcereg_task[c] < 0 || st->forcereg_task[c] >= D.n_tasks) { why = "forcereg_task out of range"; return WBCQP_ERR_INVALID; }
    D.max_iter = st->max_iter > 0 ? st->max_iter : 1000;
    D.hessian_reg = st->hessian_reg;

    // ---- LDS layout (doubles) ----
    const int n = D.n, nv = D.nv;
    D.ldj = odd(n); D.ldm = odd(nv); D.ldc = odd(nv); D.ldb = 2 * odd((4 * ((D.neq + 3) / 4) + 1) / 2); // twice an odd number: rows stay 16-byte aligned for the 4-wide column groups (which may read past m) and 16 rows still hit 16 distinct bank groups
    int o = 0;
    auto take = [&](int count) { int at = o; o += (count + 1) & ~1; return at; }; // keep 16-byte alignment
    D.o_J = take(n * D.ldj);
    int rsize = n * (n + 3) / 2 + 2;
    if (D.n_dense * 66 + 8 > rsize) rsize = D.n_dense * 66 + 8; // staged task rows: 64 columns (transposed groups) + (w, b) pairs
    if (D.neq > 0 && 256 + (n + 17) * D.ldb + 8 > rsize) rsize = 256 + (n + 17) * D.ldb + 8; // B of the blocked equality phase + 16 zero rows // + 64: the 4x4 H tiles may read past the last staged row
    D.o_R = take(rsize);
    D.o_M = take(nv * D.ldm);
    D.o_Jc = take(D.k * D.ldc);
    D.o_Ac = take(D.nc * 6 * nv);
    D.o_vec = take(V_COUNT * kSlot);
    D.o_eqw = take(D.neq > 0 ? (n + 1) * D.ldb + 8 : 0);
    D.o_eqt = take(D.neq > 0 ? D.neq * (D.neq + 1) + 4 * D.neq + 16 : 0);
    D.fric_lds = (D.nc > 0 && (o - D.o_eqw) >= 238 * D.nc) ? 1 : 0;
    D.o_int = o;
    o += kIntCount / 2 + 2;
    D.lds_doubles = o;
    D.compact = 0;

    std::memset(&L, 0, sizeof(L));
    L.n = n; L.neq = D.neq; L.nin = D.nin2 / 2; L.nin2 = D.nin2; L.r1 = D.r1;
    L.len_M = nv * (nv + 1) / 2; L.len_h = nv; L.len_A = D.n_dense * nv; L.len_b1 = D.r1;
    L.len_Ac = D.nc * 6 * nv; L.len_bc = D.nc * 6; L.len_blb = D.n_bound; L.len_bub = D.n_bound;
    L.len_tlb = D.act_bounds ? D.na : 0; L.len_tub = L.len_tlb; L.len_w = D.n_tasks;
    L.len_Acop = D.cop_task >= 0 ? 3 * D.k : 0;
    L.dense_h = D.dense_h;
    set_lds(L, o * 8);
    const int64_t n_in = (int64_t)L.len_M + L.len_h + L.len_A + L.len_b1 + L.len_Ac + L.len_bc + L.len_blb + L.len_bub +
                         L.len_tlb + L.len_tub + L.len_w + L.len_Acop;
    L.algorithmic_bytes = 8 * (n_in + n + D.na) + 8;
    if (L.lds_bytes > 160 * 1024) { why = "QP does not fit the 160 KiB LDS of one CU"; return WBCQP_ERR_UNSUPPORTED; }
    return WBCQP_OK;
}

// one wavefront per QP (wbcqp_small.hpp): fixed base, no contacts, n = nv <= 16, bounds as the only inequality rows
bool small_ok(const DevStruct& D, const HostBlocks& HB)
{
    if (D.dense_h) return false;
    if (!(D.nc == 0 && D.nu == 0 && D.neq == 0 && D.n == D.nv && D.n >= 1 && D.n <= 16 && D.na <= 16 && D.n_dense <= 16 && D.n_sel <= 16 &&
          D.n_tasks >= 1 && D.n_tasks <= 16 && D.n_bound <= 16 && D.nin2 <= 32 && D.r1 >= 1 && D.r1 <= 32 && !D.act_bounds))
        return false;
    for (int b = 0; b < HB.n_blocks; ++b)
        if (HB.blk_kind[b] != WBCQP_INEQ_BOUNDS) return false;
    return true;
}

// The compact LDS layout of an eligible structure (wbcqp_compact.hpp): J region | R region | vectors | ints; everything
// else is staged inside the first two while they are idle, or never enters LDS.  Returns false when not eligible.
bool derive_compact(const DevStruct& F, DevStruct& D)
{
    D = F;
    D.compact = 0;
    if (F.dense_h) return false; // a torque / cop task: H is one n x n matrix, the compact kernel factors a dv block and 12 x 12 blocks
    const int n = F.n, nv = F.nv;
    // (n <= 78: the 80-entry vector slots hold a zero pad pair behind column n for the loop's 16-byte row passes)
    if (!(n <= 78 && F.neq <= 22 && nv <= 52 && F.nc <= 2 && F.nu <= 8 && F.na <= 64 && F.n_bound <= 64 && F.nin2 <= 256 &&
          F.r1 <= 128 && F.n_tasks <= 64 && (!F.act_bounds || F.act_off >= 0) && n - F.neq <= 64))
        return false;
    // The loop publishes an actuation row into np with its force padding, up to entry nv + 23.  With 64-entry slots (n <= 62) and nv > 40 that runs into the
    // slot behind np, d, whose entries from neq on are live: zeros land on the pending v (a fixed base at nv = 52: dv off by twice |x|,
    // tests/size_edges.py: fixed52).  Such a stack keeps the full layout.
    if (F.act_bounds && cp::vec_stride(n, nv) == 64 && nv + 23 - 64 >= F.neq) return false;
    int o = 0;
    auto take = [&](int count) { int at = o; o += (count + 1) & ~1; return at; };
    // rows of J: 16-byte aligned, a zero pad pair behind column n, and 2 x odd long -- sixteen rows then start in sixteen
    // different bank groups for 8-byte and for 16-byte accesses alike
    {
        int l = ((n + 1) & ~1) + 2;
        while ((l & 3) != 2) l += 2;
        // n itself is 2 x odd and there are equality columns to spare: the pad pair of a row is the next row's (dead, zeroed) columns 0-1 in the
        // loop, two more doubles end the last row
        if ((n & 3) == 2 && F.neq >= 2) l = n;
        D.ldj = l;
    }
    const int as_size = (F.n_dense * 66 + 8 + 1) & ~1;   // staged task rows: 64 columns + (w, b) pairs
    int jsize = n * D.ldj + 2;
    if (as_size + 1024 > jsize) jsize = as_size + 1024;  // + the elimination's panels (2 x 2 x 256)
    D.o_pan = as_size;
    D.o_J = take(jsize);
    int rs = 512;                                        // packed R of the equalities (neq <= 22 columns)
    if (F.neq > 0 && (n + 4) * F.ldb + 8 > rs) rs = (n + 4) * F.ldb + 8; // N = CE', then B = J0'N (from the region's start: the packed R follows it in time)
    {   // the inequality loop: Ri (row-packed, n - neq rows, one spare element per row; reads past its end land in what follows), four doubles per
        // rotation of a drop, the friction rows' table (one sign)
        const int mmax = n - F.neq;
        const int fric = cp::fric_in_j(n, F.neq, F.nc) != 0 ? 0 : F.nc * 17 * 12; // (with fourteen equalities the table lives in J's dead columns: wbcqp_compact.hpp)
        const int need = ((2 + mmax * (mmax + 3) / 2 + 1) & ~1) + 4 * (mmax + 2) + fric + 2; // (reads past Ri's last row reach at most mmax + 8 doubles into the 4 (mmax + 2) of the rotation table)
        if (need > rs) rs = need;
    }
    D.o_R = take(rs);
    D.o_vec = take(cp::vec_map(n, nv, F.act_bounds).COUNT);
    D.o_int = o;
    o += cp::ICOUNT / 2;
    D.o_M = D.o_Jc = D.o_Ac = D.o_eqw = D.o_eqt = 0;
    D.fric_lds = 0;
    D.lds_doubles = o;
    D.compact = 1;
    return true;
}

void set_lds(wbcqp_layout& L, int lds_bytes, bool compact, bool act_bounds, int spec)
{
    L.lds_bytes = lds_bytes;
    L.waves_per_cu = lds_bytes > 0 ? (160 * 1024) / lds_bytes : 0;
    // registers: the solve kernels allocate up to 256 VGPRs = two waves per SIMD = two workgroups per CU; the compact layout has a twin compiled
    // for three (solve_queue3_kernel), taken when three workgroups fit the CU's LDS: measured (tools/ubench/lds_granule.hip) the third one fits
    // up to 54 592 bytes of dynamic LDS beside the kernel's static word -- no coarser granule than 16 bytes (the launch asks the runtime itself).
    // Whether a launch of this structure alone, on a handle without flags, takes that twin is choose_kernel's answer, not a rule of this function's
    const KernelChoice c = choose_kernel(LaunchFacts{compact, lds_bytes, act_bounds, spec, true}, 0);
    const int cap = (c.three && c.queue) ? 3 : 2;
    if (L.waves_per_cu > cap) L.waves_per_cu = cap;
}

// Validates a tree + task bindings against a structure and derives the rows kernel's tables and LDS layout.  Pure host code
// (wbcqp_check_model runs it without a device; wbcqp_set_model uploads what it returns).
// sel_host [D.n_sel]: the posture task's columns; force_gen_host [D.nc][6][12]: the contacts' force generators (host copies)
int derive_terms(wbcqp_handle* h, const DevStruct& D, const int* sel_host, const double* force_gen_host, const wbcqp_model* md,
                        const wbcqp_taskmap* tm, TermsDev& T, std::vector<int>& ipool, std::vector<double>& dpool)
{
    if (!md || !tm) return fail(h, WBCQP_ERR_INVALID, "model / taskmap is NULL");
    const int nb = md->nbody, fb = md->floating_base ? 1 : 0;
    if (nb <= 0 || !md->parent || !md->jtype || !md->placement || !md->inertia) return fail(h, WBCQP_ERR_INVALID, "empty model");
    if (nb > kWave) return fail(h, WBCQP_ERR_UNSUPPORTED, "more than 64 bodies (one lane per body)");
    const int nv = nb + (fb ? 5 : 0), nq = nb + (fb ? 6 : 0), na = nv - (fb ? 6 : 0);
    if (nv != D.nv || na != D.na) return fail(h, WBCQP_ERR_INVALID, "model and structure disagree on nv / na");
    if (tm->n_contact != D.nc) return fail(h, WBCQP_ERR_INVALID, "taskmap and structure disagree on the number of contacts");
    if ((tm->bounds ? na : 0) != D.n_bound) return fail(h, WBCQP_ERR_INVALID, "taskmap and structure disagree on the bounds rows");
    if (tm->n_task < 0 || (tm->n_task > 0 && !tm->task) || tm->nref < 0 || !(tm->dt > 0.0)) return fail(h, WBCQP_ERR_INVALID, "bad taskmap");
    // tree: parents first, depth-first numbering (a subtree is a contiguous range)
    std::vector<int> depth(nb, 0), last(nb), idxq(nb), idxv(nb), bodyof(nv), kof(nv);
    for (int i = 0; i < nb; ++i) {
        last[i] = i;
        if (i == 0 ? md->parent[0] != -1 : (md->parent[i] < 0 || md->parent[i] >= i)) return fail(h, WBCQP_ERR_INVALID, "parent[i] must be in [0, i), -1 for body 0");
        const int jt = md->jtype[i];
        if (jt < WBCQP_J_FREEFLYER || jt > WBCQP_J_PZ || ((jt == WBCQP_J_FREEFLYER) != (fb && i == 0)))
            return fail(h, WBCQP_ERR_INVALID, "joint type out of range, or a free-flyer that is not body 0 of a floating-base model");
        if (i) depth[i] = depth[md->parent[i]] + 1;
        idxq[i] = fb ? (i == 0 ? 0 : 6 + i) : i;
        idxv[i] = fb ? (i == 0 ? 0 : 5 + i) : i;
    }
    for (int i = nb - 1; i > 0; --i) last[md->parent[i]] = std::max(last[md->parent[i]], last[i]);
    for (int i = 1; i < nb; ++i) {
        // depth-first: the parent of i is the body just before it or one of that body's ancestors
        bool on_path = false;
        for (int b = i - 1; b >= 0 && !on_path; b = md->parent[b]) on_path = (b == md->parent[i]);
        if (!on_path) return fail(h, WBCQP_ERR_INVALID, "bodies are not numbered depth-first");
    }
    int maxdepth = 0;
    for (int i = 0; i < nb; ++i) {
        maxdepth = std::max(maxdepth, depth[i]);
        const int cnt = (md->jtype[i] == WBCQP_J_FREEFLYER) ? 6 : 1;
        for (int k = 0; k < cnt; ++k) { bodyof[idxv[i] + k] = i; kof[idxv[i] + k] = k; }
    }
    if (md->nframe < 0 || (md->nframe > 0 && (!md->frame_body || !md->frame_placement))) return fail(h, WBCQP_ERR_INVALID, "bad frame tables");
    for (int f = 0; f < md->nframe; ++f)
        if (md->frame_body[f] < 0 || md->frame_body[f] >= nb) return fail(h, WBCQP_ERR_INVALID, "a frame hangs on a body that does not exist");
    auto frame_ok = [&](int f) { return f >= 0 && f < md->nframe; };
    // tasks -> law lanes (SE3 blocks then contacts), self-collision pairs, blocks
    std::vector<int> law_body, law_mask, law_row, law_ref, law_va, law_contact, pair_bt, pair_ba;
    std::vector<int> blk_kind, blk_mask, blk_row, blk_ref, blk_pair0, blk_npair;
    std::vector<double> law_place, law_kp, law_kd, scf_place, pair_par, blk_kp, blk_kd;
    std::vector<int> scf_frame, scf_body, pair_ft, pair_fa;
    auto scf_index = [&](int f) {
        for (size_t k = 0; k < scf_frame.size(); ++k)
            if (scf_frame[k] == f) return (int)k;
        scf_frame.push_back(f); scf_body.push_back(md->frame_body[f]);
        scf_place.insert(scf_place.end(), md->frame_placement + 12 * f, md->frame_placement + 12 * f + 12);
        return (int)scf_frame.size() - 1;
    };
    auto popc = [](int m, int bits) { int c = 0; for (int i = 0; i < bits; ++i) c += (m >> i) & 1; return c; };
    int row = 0;
    for (int t = 0; t < tm->n_task; ++t) {
        const wbcqp_task& K = tm->task[t];
        blk_kind.push_back(K.kind); blk_mask.push_back(K.mask); blk_row.push_back(row); blk_ref.push_back(K.ref);
        blk_kp.push_back(K.kp); blk_kd.push_back(K.kd);
        blk_pair0.push_back((int)pair_bt.size()); blk_npair.push_back(0);
        int need = 0;
        if (K.kind == WBCQP_T_SE3) {
            if (!frame_ok(K.frame)) return fail(h, WBCQP_ERR_INVALID, "SE3 task tracks a frame that does not exist");
            law_body.push_back(md->frame_body[K.frame]); law_mask.push_back(K.mask & 63); law_row.push_back(row);
            law_ref.push_back(K.ref); law_va.push_back(1); law_contact.push_back(-1);
            law_kp.push_back(K.kp); law_kd.push_back(K.kd);
            law_place.insert(law_place.end(), md->frame_placement + 12 * K.frame, md->frame_placement + 12 * K.frame + 12);
            row += popc(K.mask, 6); need = 24;
        }
        else if (K.kind == WBCQP_T_COM) { row += popc(K.mask, 3); need = 9; blk_mask.back() = K.mask & 7; }
        else if (K.kind == WBCQP_T_MOMENTUM) { row += popc(K.mask, 6); need = 12; blk_mask.back() = K.mask & 63; }
        else if (K.kind == WBCQP_T_SELFCOLLISION) {
            if (!frame_ok(K.frame) || K.n_avoided < 0 || (K.n_avoided > 0 && (!K.avoided_frame || !K.avoided_r0)))
                return fail(h, WBCQP_ERR_INVALID, "bad self-collision task");
            if (!(K.m > 0.0) || !(K.margin > 0.0)) return fail(h, WBCQP_ERR_INVALID, "self-collision needs m > 0 and margin > 0");
            // constants of the 5PL repulsor (task-self-collision.cpp:147-149)
            const double k5 = -std::log(std::pow(-1e-5 + 1., -1. / K.m) - 1.) / K.margin;
            const double s_p = -1. / k5 * std::log(-1 + std::pow(2, 1. / K.m));
            for (int a = 0; a < K.n_avoided; ++a) {
                const int fa = K.avoided_frame[a];
                if (!frame_ok(fa)) return fail(h, WBCQP_ERR_INVALID, "self-collision task avoids a frame that does not exist");
                pair_bt.push_back(md->frame_body[K.frame]); pair_ba.push_back(md->frame_body[fa]);
                pair_ft.push_back(scf_index(K.frame)); pair_fa.push_back(scf_index(fa));
                const double par[6] = {K.avoided_r0[a] + K.radius, k5, s_p, K.m, K.kp, K.kd};
                pair_par.insert(pair_par.end(), par, par + 6);
            }
            blk_npair.back() = K.n_avoided;
            row += 1;
        }
        else return fail(h, WBCQP_ERR_INVALID, "unknown task kind");
        if (need && (K.ref < 0 || K.ref + need > tm->nref)) return fail(h, WBCQP_ERR_INVALID, "a task reference lies outside the reference vector");
    }
    if (row != D.n_dense) return fail(h, WBCQP_ERR_INVALID, "the tasks' rows do not add up to the structure's n_dense");
    for (int c = 0; c < tm->n_contact; ++c) {
        const int f = tm->contact_frame[c];
        if (!frame_ok(f)) return fail(h, WBCQP_ERR_INVALID, "contact frame does not exist");
        if (tm->contact_ref[c] < 0 || tm->contact_ref[c] + 24 > tm->nref) return fail(h, WBCQP_ERR_INVALID, "a contact reference lies outside the reference vector");
        law_body.push_back(md->frame_body[f]); law_mask.push_back(63); law_row.push_back(0); law_ref.push_back(tm->contact_ref[c]);
        law_va.push_back(1); law_contact.push_back(c); law_kp.push_back(tm->contact_kp[c]); law_kd.push_back(tm->contact_kd[c]);
        law_place.insert(law_place.end(), md->frame_placement + 12 * f, md->frame_placement + 12 * f + 12);
    }
    if ((int)law_body.size() > kWave || (int)blk_kind.size() > kWave || (int)scf_frame.size() > kWave)
        return fail(h, WBCQP_ERR_UNSUPPORTED, "more than 64 framed tasks or self-collision frames (one lane each)");
    if (D.n_sel > 0 && (tm->posture_ref < 0 || tm->posture_ref + na > tm->nref)) return fail(h, WBCQP_ERR_INVALID, "the posture reference lies outside the reference vector");
    if (D.n_bound > 0 && (!md->q_lb || !md->q_ub || !md->dq_max)) return fail(h, WBCQP_ERR_INVALID, "bounds need q_lb / q_ub / dq_max");

    T = TermsDev{};
    T.nb = nb; T.nq = nq; T.nv = nv; T.na = na; T.floating_base = fb;
    int nrounds = 0;
    while ((1 << nrounds) < maxdepth + 1) ++nrounds;
    T.nrounds = nrounds; // <= 6 for 64 bodies
    std::vector<int> anc((size_t)std::max(nrounds, 1) * nb, -1);
    for (int i = 0; i < nb; ++i) anc[i] = md->parent[i];
    for (int r = 1; r < nrounds; ++r)
        for (int i = 0; i < nb; ++i) {
            const int a = anc[(size_t)(r - 1) * nb + i];
            anc[(size_t)r * nb + i] = (a >= 0) ? anc[(size_t)(r - 1) * nb + a] : -1;
        }
    T.nlaw = (int)law_body.size(); T.npair = (int)pair_bt.size(); T.nscf = (int)scf_frame.size(); T.nblock = (int)blk_kind.size(); T.nc = D.nc;
    T.n_dense = D.n_dense; T.n_sel = D.n_sel; T.n_bound = D.n_bound; T.r1 = D.r1; T.nref = tm->nref;
    T.posture_ref = tm->posture_ref; T.posture_kp = tm->posture_kp; T.posture_kd = tm->posture_kd; T.dt = tm->dt;
    for (int k = 0; k < 3; ++k) T.g[k] = md->gravity[k];
    ipool.clear();
    dpool.clear();
    auto puti = [&](const int* a, size_t n) { int at = (int)ipool.size(); ipool.insert(ipool.end(), a, a + n); ipool.push_back(0); return at; };
    auto putd = [&](const double* a, size_t n) { int at = (int)dpool.size(); dpool.insert(dpool.end(), a, a + n); dpool.push_back(0.0); return at; };
    // the posture task's columns: the actuated joints its mask keeps (tasks.cpp:197-217), from the structure
    std::vector<int> sel(D.n_sel);
    for (int r = 0; r < D.n_sel; ++r) {
        sel[r] = sel_host[r];
        if (sel[r] < nv - na || sel[r] >= nv) return fail(h, WBCQP_ERR_INVALID, "a posture row selects a column that is not an actuated joint");
    }
    // cop task (tasks.cpp:156-178): the rows kernel forms its three rows from the contact frames; the contact points are the skew
    // blocks of the force generators, T(3.., 3 p ..) = skew(p): x = T(5, 3p + 1), y = T(3, 3p + 2), z = T(4, 3p)
    std::vector<double> cop_pts;
    T.cop = D.cop_task >= 0 ? 1 : 0;
    if (T.cop)
        for (int c = 0; c < D.nc; ++c)
            for (int p = 0; p < 4; ++p) {
                const double* Tg = force_gen_host + (size_t)c * 72;
                cop_pts.push_back(Tg[5 * 12 + 3 * p + 1]);
                cop_pts.push_back(Tg[3 * 12 + 3 * p + 2]);
                cop_pts.push_back(Tg[4 * 12 + 3 * p]);
            }
    T.i_jtype = puti(md->jtype, nb); T.i_last = puti(last.data(), nb);
    T.i_anc = puti(anc.data(), (size_t)nrounds * nb);
    T.i_idxq = puti(idxq.data(), nb); T.i_idxv = puti(idxv.data(), nb); T.i_bodyof = puti(bodyof.data(), nv); T.i_kof = puti(kof.data(), nv);
    T.i_law_body = puti(law_body.data(), law_body.size()); T.i_law_mask = puti(law_mask.data(), law_mask.size());
    T.i_law_row = puti(law_row.data(), law_row.size()); T.i_law_ref = puti(law_ref.data(), law_ref.size());
    T.i_law_va = puti(law_va.data(), law_va.size()); T.i_law_contact = puti(law_contact.data(), law_contact.size());
    T.i_pair_bt = puti(pair_bt.data(), pair_bt.size());
    T.i_pair_ba = puti(pair_ba.data(), pair_ba.size());
    T.i_pair_ft = puti(pair_ft.data(), pair_ft.size()); T.i_pair_fa = puti(pair_fa.data(), pair_fa.size());
    T.i_scf_body = puti(scf_body.data(), scf_body.size());
    T.i_blk_kind = puti(blk_kind.data(), blk_kind.size()); T.i_blk_mask = puti(blk_mask.data(), blk_mask.size());
    T.i_blk_row = puti(blk_row.data(), blk_row.size()); T.i_blk_ref = puti(blk_ref.data(), blk_ref.size());
    T.i_blk_pair0 = puti(blk_pair0.data(), blk_pair0.size());
    T.i_blk_npair = puti(blk_npair.data(), blk_npair.size()); T.i_sel_col = puti(sel.data(), sel.size());
    // room for the contacts' force references (wbcqp_set_force_references fills it in place): none yet
    const std::vector<int> no_fref(D.nc, -1);
    const std::vector<double> no_fref_w((size_t)6 * D.nc, 0.0);
    T.n_fref = 0;
    T.i_fref = puti(no_fref.data(), no_fref.size());
    T.d_place = putd(md->placement, (size_t)nb * 12); T.d_inertia = putd(md->inertia, (size_t)nb * 10);
    T.d_law_place = putd(law_place.data(), law_place.size()); T.d_law_kp = putd(law_kp.data(), law_kp.size());
    T.d_law_kd = putd(law_kd.data(), law_kd.size());
    T.d_scf_place = putd(scf_place.data(), scf_place.size());
    T.d_pair_par = putd(pair_par.data(), pair_par.size());
    T.d_blk_kp = putd(blk_kp.data(), blk_kp.size()); T.d_blk_kd = putd(blk_kd.data(), blk_kd.size());
    T.d_cop_pts = putd(cop_pts.data(), cop_pts.size());
    T.d_fref_w = putd(no_fref_w.data(), no_fref_w.size());
    T.d_qlb = putd(md->q_lb, D.n_bound ? na : 0); T.d_qub = putd(md->q_ub, D.n_bound ? na : 0); T.d_dqmax = putd(md->dq_max, D.n_bound ? na : 0);
    int o = 0;
    auto take = [&](int count) { int at = o; o += (count + 1) & ~1; return at; };
    T.o_state = take(nq + nv + tm->nref);
    T.o_kin = take(nb * kKinStride);
    T.o_scan = take((nb + 1) * kScanStride);
    T.o_tot = take(8); // momentum totals (6), the frames-published flag
    T.o_sf = take(nv * kSFStride);
    T.o_law = take(T.nlaw * kLawStride);
    T.o_pair = take(T.npair * kPairStride);
    T.o_scf = take(T.nscf * kScfStride);
    T.o_b1 = take(D.r1);
    T.o_bc = take(6 * D.nc);
    T.lds_doubles = o;
    if ((size_t)o * 8 > 160 * 1024) return fail(h, WBCQP_ERR_UNSUPPORTED, "the working set of one instance exceeds the LDS");
    return WBCQP_OK;
}

} // namespace
