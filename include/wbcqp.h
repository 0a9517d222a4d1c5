/*
 * wbcqp.h -- C ABI of the MI355X batched whole-body QP ("one control tick of inria_wbc, B robots at once").
 *
 * This is the drop-in boundary for the single hot path of resibots/inria_wbc
 * (citations are into /root/reference/):
 *
 *   Controller::_solve                         src/controllers/controller.cpp:231-313
 *     tsid_->computeProblemData(t, q, dq)      src/controllers/controller.cpp:244   (assembly half: HQPData)
 *     solver_->solve(HQPData)                  src/controllers/controller.cpp:247   (tsid SolverHQuadProgFast
 *                                                                                    + eiquadprog-fast GI solve)
 *     getActuatorForces / getAccelerations     src/controllers/controller.cpp:250-251
 *     getContactForces                         src/controllers/controller.cpp:260
 *
 * One "QP" below = that sequence for one robot instance.  Inputs are what the step before the path
 * produces (pinocchio terms + each task's compute(): M, h, task rows, contact Jacobians, bounds);
 * outputs are x = [dv; f], tau, status, active-set iterations.
 *
 * Plain pointers and sizes only; no C++/torch types.  Nothing throws across this boundary: every
 * entry point returns a wbcqp_status and wbcqp_last_error() gives the text.  A handle is bound to one
 * HIP device and is not thread-safe: one host thread at a time calls into it; distinct handles may be
 * used concurrently (the reference's Controller is single-threaded and non-copyable,
 * controller.hpp:50-51).  That one thread may launch on SEVERAL HIP streams: the handle keeps its
 * launch-order buffer and its queue counter per stream (up to 16 distinct streams; a launch on a 17th runs
 * in index order on the hardware's dispatcher and keeps no state), so launches in flight on two streams
 * share nothing -- tests/test_gpu_streams.py interleaves two streams on one handle and compares bit for
 * bit.  A stream's state is keyed by the stream handle's value: destroy a stream only after its launches
 * have completed.  wbcqp_rollout waits for the previous roll-out of the same handle (on whatever stream it
 * ran) before it reuses the handle's roll-out buffers.  The device-pointer solve entry points allocate
 * nothing in the steady state (upstream's solver runs under EIGEN_MALLOC_NOT_ALLOWED); the FIRST launch
 * on a stream of a larger batch than any before it on that stream (launch-order buffer, 8 bytes per QP,
 * with one synchronisation of that stream) and the first launch on a new stream (an 8-byte queue counter)
 * do allocate.  A captured tick (wbcqp_tick_graph_create) owns its buffers and never does.  The first solve of a slot after
 * wbcqp_set_structure also synchronises its stream once (the force blocks' factor cache, interface history 151).
 */
#ifndef WBCQP_H
#define WBCQP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Interface history (WBCQP_VERSION = 100 major + 10 minor + patch; round 5 changed no declaration of this header -- wbcqp_layout.waves_per_cu may now be 3,
 * and wbcqp_structure.max_iter no longer decides whether a shipped stack runs its own instantiation):
 *   151  no declaration changed.  wbcqp_tick_host fills wbcqp_outputs.active_mask when given; the numbering of active_mask's bits is documented (below);
 *        a slot's FIRST solve on the compact layout makes the force blocks' factor for the force-regularisation weights of its first QP (one small kernel
 *        and one synchronisation of the launch's stream, once per wbcqp_set_structure; never inside a stream capture) -- later QPs that carry those weights
 *        take the factor from there, others compute it as before: the same bits either way (env WBCQP_DEBUG_NO_FFCACHE=1, read at wbcqp_create, turns it off).
 *        Added without a change of version: wbcqp_mix, wbcqp_mixed_io, wbcqp_tick_mixed and wbcqp_rollout_mixed (instances of one robot model in
 *        different contact sets, one call); wbcqp_trace, wbcqp_task_costs, wbcqp_rollout_traced and wbcqp_rollout_mixed_traced (per-task costs on
 *        the device, per-tick results of a roll-out); wbcqp_program, wbcqp_track, wbcqp_segment, wbcqp_check_program, wbcqp_reference_samples,
 *        wbcqp_rollout_program and wbcqp_rollout_mixed_program (the references of a roll-out generated on the device from a reference program);
 *        wbcqp_observables, wbcqp_set_observed_frames, wbcqp_observe and wbcqp_observe_host (centre of mass and world placements / velocities of
 *        chosen model frames from (q, v) on the device); wbcqp_set_model now keeps the model's whole frame table on the host;
 *        wbcqp_sphere_model, wbcqp_collisions, wbcqp_set_collision_spheres, wbcqp_check_collisions and wbcqp_check_collisions_host (self-collision
 *        of a robot's sphere model from q on the device); wbcqp_set_wrench_frames, wbcqp_inverse_dynamics and wbcqp_inverse_dynamics_host (the joint
 *        torques of a motion under external wrenches at model frames, on the device); wbcqp_torque_monitor, wbcqp_torque_checks,
 *        wbcqp_torque_monitor_state_bytes, wbcqp_detect_torque_collisions and wbcqp_detect_torque_collisions_host (external collisions of a fleet
 *        from the discrepancy of model and measured joint torques over a stream of ticks, on the device); wbcqp_observe_acom and wbcqp_observe_acom_host (wbcqp_observe with
 *        the CoM's bias acceleration as one more output); wbcqp_stabilizer, wbcqp_stab_inputs, wbcqp_stab_outputs,
 *        wbcqp_stabilizer_state_bytes, wbcqp_stabilize and wbcqp_stabilize_host (the humanoid controllers' stabiliser: CoP estimator, filters and
 *        admittance laws that rewrite a tick's references, on the device); wbcqp_set_force_references (contact force references carried by a tick's
 *        reference row), wbcqp_zmp_distributor, wbcqp_stabilize_zmp, wbcqp_stabilize_zmp_host, WBCQP_STAB_ZMP and WBCQP_STAB_ERR_ZMP (the stabiliser's
 *        ZMP force distributor); wbcqp_spd, wbcqp_mass_matrix, wbcqp_forward_dynamics, wbcqp_spd_commands and their _host forms (M(q), the
 *        accelerations joint torques produce, and the reference's stable-PD torque commands, on the device); wbcqp_reference_frame,
 *        wbcqp_jacobian_outputs, wbcqp_set_jacobian_frames, wbcqp_jacobians and wbcqp_jacobians_host (frame Jacobians, the CoM Jacobian, the
 *        centroidal momentum matrix and their drift terms, on the device); wbcqp_hessian_outputs, wbcqp_kinematic_hessians and
 *        wbcqp_kinematic_hessians_host (the frames' kinematic Hessians dJ/dq and the Jacobians' time variation, on the device);
 *        wbcqp_id_derivative_outputs, wbcqp_inverse_dynamics_derivatives and wbcqp_inverse_dynamics_derivatives_host (dtau/dq and dtau/dv of the
 *        inverse dynamics, on the device).  151 therefore names more than one set of declarations: every one of them
 *        contains the one before it unchanged (nothing was removed or resized), so a caller checks for a symbol, not for the number
 *   150  launch-order state per (handle, stream), active_mask written by every kernel, torque / cop task rows
 *        (wbcqp_structure.n_acteq, cop_*), posture mask
 *   140  wbcqp_rollout, wbcqp_outputs.active_mask (WBCQP_FLAG_WARM_START), wbcqp_state.momentum, wbcqp_layout.wave_per_qp
 *        (WBCQP_FLAG_WORKGROUP_PER_QP)
 *   130  wbcqp_integrate, wbcqp_set_model / wbcqp_problem_data / wbcqp_tick and companions
 *   121  queue + packed launch order, wbcqp_launch_order */
#define WBCQP_VERSION 151
#define WBCQP_MAX_STRUCTURES 16
#define WBCQP_MAX_INEQ_BLOCKS 16
#define WBCQP_MAX_VARS 126 /* n = nv + 12*nc: every per-QP vector fits one 128-entry LDS slot, n + 2 <= 128.  A task stack meets another limit first: it is
                            * admitted only if its full layout (WBCQP_FLAG_FULL_LDS) fits one CU's 160 KiB of LDS, which no stack with n > 77 does (nv 29 and
                            * four contacts on a fixed base); with a floating base and two contacts that ends at Talos' size, nv 50, n 74 */

/* ---- return codes of the API itself ---- */
typedef enum {
    WBCQP_OK = 0,
    WBCQP_ERR_INVALID = 1,     /* bad argument / inconsistent structure */
    WBCQP_ERR_HIP = 2,         /* HIP runtime error (text in wbcqp_last_error) */
    WBCQP_ERR_UNSUPPORTED = 3, /* size outside what the kernels support */
    WBCQP_ERR_NO_DEVICE = 4,   /* no gfx950 device: there is NO CPU fallback */
    WBCQP_ERR_RCCL = 5
} wbcqp_status;

/* ---- per-QP solver status: the tsid HQP status values the reference switches on
 *      (controller.cpp:249, 284-307) ---- */
typedef enum {
    WBCQP_HQP_UNKNOWN = -1,
    WBCQP_HQP_OPTIMAL = 0,
    WBCQP_HQP_INFEASIBLE = 1,
    WBCQP_HQP_UNBOUNDED = 2,
    WBCQP_HQP_MAX_ITER_REACHED = 3,
    WBCQP_HQP_ERROR = 4 /* redundant equalities */
} wbcqp_hqp_status;

/* kinds of level-0 inequality blocks, in the order the task stack added them
 * (pos_tracker.cpp:161-189 walks tasks.yaml in file order) */
typedef enum {
    WBCQP_INEQ_BOUNDS = 0,    /* "bounds"           tasks.cpp:274-300  rows = +-e_col          */
    WBCQP_INEQ_ACTUATION = 1, /* "actuation-bounds" tasks.cpp:303-324  rows = +-[M_a | -J_a']  */
    WBCQP_INEQ_FORCE = 2      /* contact friction   tasks.cpp:329-368  17 x 12 per contact     */
} wbcqp_ineq_kind;

typedef enum {
    WBCQP_F64 = 0, /* inputs/outputs double (the reference's Eigen double) */
    WBCQP_F32 = 1  /* inputs/outputs float at the boundary; the solve still runs in f64 */
} wbcqp_dtype;

/*
 * Constant structure of one task stack = what PosTracker::parse_tasks + tasks.cpp factories fix at
 * construction time.  Variables x = [dv (nv); f (12 per contact)], n = nv + 12 nc.
 * All arrays are HOST pointers, copied by wbcqp_set_structure.
 */
typedef struct {
    int32_t nv, na, nc;
    /* level 1 (cost): H = sum_t w_t A_t' A_t + hessian_reg I, g = -sum_t w_t A_t' b_t */
    int32_t n_dense;               /* dense motion rows (se3 / com / momentum / self-collision), nv wide   */
    int32_t n_tasks;               /* length of the per-QP weight vector w                                 */
    const int32_t* dense_row_task; /* [n_dense] row -> index into w; rows of one task are consecutive      */
    int32_t n_sel;                 /* selection rows (posture task, tasks.cpp:181-224): A = e_col'          */
    const int32_t* sel_col;        /* [n_sel] column in [0, nv)                                            */
    const int32_t* sel_task;       /* [n_sel] row -> index into w                                          */
    const double* forcereg_mat;    /* [nc][6][12] diag(w_f) T   (Contact6d force regularisation task)      */
    const int32_t* forcereg_task;  /* [nc] -> index into w      (weight w_force_feet, tasks.hpp:23)        */
    /* level 0 (hard constraints) */
    const double* force_gen;       /* [nc][6][12] T: contact-point forces -> 6-D wrench; Jc = T' A_c       */
    const double* fric_mat;        /* [nc][17][12] friction pyramid + normal force rows                    */
    const double* fric_lb;         /* [nc][17] */
    const double* fric_ub;         /* [nc][17] */
    int32_t n_bound;               /* rows of the joint bounds task                                        */
    const int32_t* bound_col;      /* [n_bound] column in [0, nv)                                          */
    int32_t act_bounds;            /* 1 if an actuation-bounds task exists (na rows)                       */
    int32_t n_ineq_blocks;
    const int32_t* ineq_kind;      /* [n_ineq_blocks] wbcqp_ineq_kind                                      */
    const int32_t* ineq_arg;       /* [n_ineq_blocks] contact index for WBCQP_INEQ_FORCE                   */
    double hessian_reg;            /* tsid default 1e-8                                                    */
    int32_t max_iter;              /* eiquadprog-fast default 1000                                         */
    /* Two level-1 task types of the reference's factory that no shipped stack uses.  Each couples blocks of H that every other
     * task keeps apart (dv with f, one contact's forces with another's), so a stack that has one runs the full LDS layout with H
     * assembled and factored as ONE n x n matrix (wbcqp_layout.dense_h; n <= 80) instead of a dv block and a 12 x 12 block per
     * contact.  CE, CI and the decode are what they are without them: level-1 tasks only enter H and g.
     *  "torque" (tasks.cpp:227-271, tsid TaskActuationEquality): n_acteq rows, one per 1 of the task's mask,
     *      scale_j [M_a(joint_j, :) | -J_a(:, joint_j)'] x = scale_j tau_ref_j - scale_j h_a(joint_j)   (SURVEY A.1 step 6);
     *      scale = the task's weight vector (`scaling:`, tasks.cpp:256-261), tau_ref = 0 in the reference (tasks.cpp:263-265); the
     *      products scale_j tau_ref_j are the task's entries of wbcqp_inputs.b1.
     *  "cop" (tasks.cpp:156-178, tsid TaskCopEquality): 3 rows over ALL 12 nc force variables (the task is associated with no
     *      single contact), given per QP in wbcqp_inputs.Acop -- they depend on the contact frames' placements; right-hand side in b1. */
    int32_t n_acteq;               /* rows of the torque task; 0: none                                     */
    const int32_t* acteq_joint;    /* [n_acteq] actuated joint in [0, na), ascending                       */
    const double* acteq_scale;     /* [n_acteq]                                                            */
    int32_t acteq_task;            /* -> index into w                                                      */
    int32_t cop_task;              /* -> index into w, a task of its own (shared with no other row); -1: no cop task.  A zero-initialised structure must set it
                                      to -1: 0 declares a cop task on task 0 -- wbcqp_set_structure refuses that when task 0 has other rows, as it has in every stack */
} wbcqp_structure;

/* Sizes derived from a structure (what PosTracker prints under `verbose`, pos_tracker.cpp:150-158). */
typedef struct {
    int32_t n;    /* tsid nVar */
    int32_t neq;  /* tsid nEq  = (nv - na) + 6 nc */
    int32_t nin;  /* tsid nIn  (two-sided rows) */
    int32_t nin2; /* one-sided rows of eiquadprog's CI = 2 nin */
    int32_t r1;   /* level-1 rows = n_dense + n_sel + 6 nc + n_acteq + (3 if a cop task) */
    /* element counts of the per-QP input arrays below */
    int32_t len_M, len_h, len_A, len_b1, len_Ac, len_bc, len_blb, len_bub, len_tlb, len_tub, len_w;
    int32_t lds_bytes;         /* dynamic LDS one QP (one 256-thread workgroup) needs */
    int32_t waves_per_cu;      /* resident QPs (workgroups) per CU a launch of THIS structure alone runs with on a handle without flags: 1 (full
                                  layout), 2 (compact layout: the kernels' registers admit two), or 3 where the launch takes the queue kernel compiled
                                  for three waves per SIMD.  That is the library's one choosing function asked about this structure (choose_kernel,
                                  csrc/wbcqp_host_handle.hpp): the kernel the structure runs has such a twin (the generic compact kernel and iCub's),
                                  no WBCQP_FLAG_WARM_START, no group of the launch has actuation bounds, lds_bytes <= 54592 and no
                                  WBCQP_DEBUG_LDS_PAD -- and the launch goes through the queue: lds_bytes >= 40 KB and no WBCQP_FLAG_HW_DISPATCH
                                  (iCub on one or two feet).  env WBCQP_DEBUG_LAUNCH=1 prints the residency of every launch */
    int64_t algorithmic_bytes; /* compact in+out bytes per QP at WBCQP_F64 */
    int32_t wave_per_qp;       /* 1: the structure runs one WAVEFRONT per QP (n <= 16, fixed base, no contacts, bounds only: Franka, Tiago),
                                  four QPs per workgroup, 7.7 KB of LDS per QP; lds_bytes / waves_per_cu then describe the four-wave
                                  kernel that WBCQP_FLAG_WORKGROUP_PER_QP selects */
    int32_t dense_h;           /* 1: the stack has a torque or a cop task -- full layout, H factored as one n x n matrix (never compact) */
    int32_t len_Acop;          /* element count of wbcqp_inputs.Acop: 3 * 12 nc with a cop task, else 0 */
    int32_t specialised;       /* > 0: the library holds an instantiation of the compact kernel with THIS layout's sizes and offsets as literals
                                  (the shipped stacks: 1 Talos, 2 iCub, 3 Talos in single support); a launch of one such group runs it unless
                                  WBCQP_FLAG_GENERIC_KERNEL.  Bit for bit the generic kernel's results, about 10 % less time per QP */
} wbcqp_layout;

/*
 * Per-QP inputs, each a contiguous [batch][len] row-major array of the handle's dtype.
 * One workgroup reads one QP's rows, so consecutive lanes read consecutive addresses.
 */
typedef struct {
    const void* M;   /* [batch][nv(nv+1)/2] inertia matrix, packed lower triangle (i>=j at i(i+1)/2+j)      */
    const void* h;   /* [batch][nv]  non-linear effects                                                     */
    const void* A;   /* [batch][n_dense][nv] dense level-1 task rows (TaskSE3Equality & co: ex_task.cpp:175-247,
                        task-momentum-equality.cpp:144-173, task-self-collision.cpp:84-203)                   */
    const void* b1;  /* [batch][r1] level-1 right-hand sides: dense | selection | force-regularisation
                        | torque task (scale_j tau_ref_j, n_acteq) | cop task (3)                             */
    const void* Ac;  /* [batch][nc][6][nv] contact motion-task matrices (local frame)                       */
    const void* bc;  /* [batch][nc][6]     contact motion-task right-hand sides                             */
    const void* blb; /* [batch][n_bound]   acceleration bounds                                              */
    const void* bub; /* [batch][n_bound]                                                                    */
    const void* tlb; /* [batch][na]        torque bounds, before the -h_a shift (NULL if !act_bounds)       */
    const void* tub; /* [batch][na]                                                                         */
    const void* w;   /* [batch][n_tasks]   level-1 task weights (PosTracker::update_task_weights)           */
    const void* Acop;/* [batch][3][12 nc]  rows of the cop task over the force variables (NULL without one)      */
} wbcqp_inputs;

typedef struct {
    void* x;          /* [batch][n]  = [dv; f]        (getAccelerations / getContactForces)  */
    void* tau;        /* [batch][na] actuator torques (getActuatorForces)                    */
    int32_t* status;  /* [batch] wbcqp_hqp_status                                            */
    int32_t* iters;   /* [batch] active-set iterations (eiquadprog `iter`)                   */
    void* objective;  /* [batch] 0.5x'Hx + g'x (SolverHQPBase::getObjectiveValue), may be NULL */
    int32_t* n_active;/* [batch] size of the final active set incl. equalities, may be NULL  */
    uint32_t* active_mask; /* [batch][8], may be NULL.  OUT: bit r of the 256-bit mask (bit r % 32 of word r / 32) = one-sided inequality row r is
                         active at the solution (HQPOutput::activeSet's inequality entries).  r IS eiquadprog's CI row index, i.e. the row
                         SolverHQuadProgFast::solve stacks: the level-0 inequality blocks in the order of wbcqp_structure.ineq_kind / ineq_arg
                         (= the order tasks.yaml added them, pos_tracker.cpp:161-189), each two-sided block of m rows lb <= A x <= ub as
                         rows [k, k + m) = +A with ci0 = -lb (the LOWER side) followed by rows [k + m, k + 2m) = -A with ci0 = ub (the UPPER
                         side); m = n_bound for the bounds block (row j: joint bound_col[j]), na for the actuation bounds (row j: actuated
                         joint j, limits shifted by -h_a), 17 for a contact's force block (rows 0-15 the friction pyramid of the four points,
                         row 16 the normal-force sum).  Talos: bounds 0-43 / 44-87, torque 88-131 / 132-175, first contact 176-192 / 193-209,
                         second contact 210-226 / 227-243.  Equalities (always active; eiquadprog tags them -i-1) have no bit: popcount =
                         n_active - nEq.  tests/util.py:assert_parity compares the mask with the oracle's active list bit for bit on every
                         parity case.  With WBCQP_FLAG_WARM_START also IN: the mask a previous tick left for the same instance (zeros: no
                         hint).  Device pointer on the device entry points.  Written by every kernel (rows beyond the 256th have no bit;
                         all zero where the status is not OPTIMAL); READ as the hint by the compact-layout kernel only -- structures on
                         the one-wavefront-per-QP kernel (wbcqp_layout.wave_per_qp) and on the full layout ignore the hint. */
} wbcqp_outputs;

/* wbcqp_desc.flags */
#define WBCQP_FLAG_INDEX_ORDER 1 /* launch the QPs of a batch in index order.  Default (0): longest-first -- a launch is
                                    ordered by the active-set iteration counts of the previous launch of the same shape on
                                    the same stream (control ticks change little); results do not depend on the order */
#define WBCQP_FLAG_HW_DISPATCH 2 /* one workgroup per QP, handed to the CUs by the hardware's dispatcher (the default for
                                    structures whose workgroup is under 48 KB of LDS: Franka, Tiago).  Default (0) for the
                                    humanoid stacks: as many workgroups as the chip holds (two per CU on the compact layout)
                                    take QPs from a queue in the launch order (the dispatcher binds workgroup i to one shader
                                    engine of XCD i % 8 and waits for it; the queue does not); results do not depend on it */
#define WBCQP_FLAG_QUEUE 8       /* the queue also for small structures, and the bin-packed order also where two workgroups share
                                    a CU (measured no better than longest-first there: tools/dispatch_sweep.py) */
#define WBCQP_FLAG_NO_PACKING 4  /* keep the plain longest-first order for the queue.  Default (0): where one workgroup fills a
                                    CU and a launch holds between one and eight QPs per resident workgroup, the order is
                                    bin-packed from the predicted costs (setup + iterations of the previous launch) */
#define WBCQP_FLAG_FULL_LDS 16    /* keep every structure on the layout that holds M, Jc and A_c in LDS for the QP's whole life
                                    (Talos: one QP per CU).  Default (0): structures within n <= 80, nEq <= 22, nv <= 52, two
                                    contacts (every stack the reference ships) use the compact layout -- half the LDS, two
                                    QPs resident per CU; same algorithm, results agree to rounding */

#define WBCQP_FLAG_WORKGROUP_PER_QP 32 /* keep the small structures (n <= 16 without contacts: Franka, Tiago) on the four-wave kernels too.
                                     Default (0): one WAVEFRONT per QP for them, four QPs per 256-thread workgroup and no workgroup
                                     barrier (csrc/wbcqp_small.hpp); in a ragged launch they go out as a launch of their own */
#define WBCQP_FLAG_WARM_START 64 /* OPT-IN, not what the reference does: among the violated constraints the active-set loop first picks
                                    those that were active at the previous tick's solution (wbcqp_outputs.active_mask, in/out), the most
                                    violated of them first; when none of them is violated, eiquadprog's rule (the most violated row).
                                    Still Goldfarb-Idnani -- any violated constraint is a legal pick, the QP is strictly convex, so the
                                    EXACT solution is the cold start's -- but eiquadprog's loop ends on |sum min(s, 0)| <= nIneq eps
                                    tr(H) tr(J) 100 (about 0.3 for the humanoid stacks), so x and tau equal the cold start's only up to
                                    that termination tolerance: the two pick orders may end on different iterates (measured on the
                                    squat stream: 2-4 of 1024 QPs per tick, |dx| up to 4e-4 relative; bench.py's warm_start.parity
                                    counts them, tests/test_gpu_warm.py bounds them).  What it buys: the add / drop churn of a cold
                                    start is avoided, iteration counts fall to about the number of constraints active at the solution.
                                    eiquadprog-fast has no such thing: bench.py reports it BESIDE the headline, never as it */
#define WBCQP_FLAG_GENERIC_KERNEL 128 /* never the shipped stacks' own instantiations of the compact kernel (wbcqp_layout.specialised): the generic
                                     kernel for every structure (what the specialised ones are tested against, bit for bit) */
#define WBCQP_FLAG_REFRESH_SHIFT 8
#define WBCQP_FLAG_REFRESH(n) (((n) & 0xff) << WBCQP_FLAG_REFRESH_SHIFT) /* renew the launch order every n-th launch of a shape
                                    (1: after every launch; 0: the default, 4).  Between renewals the same order is used:
                                    iteration counts drift slowly between control ticks and the queue absorbs the drift.
                                    A captured tick (wbcqp_tick_graph_create) renews it on every replay */

typedef struct {
    int32_t device;   /* HIP device ordinal */
    int32_t dtype;    /* wbcqp_dtype of every input/output array */
    int32_t flags;    /* WBCQP_FLAG_* */
} wbcqp_desc;

/* one homogeneous group of a ragged (mixed-robot) batch */
typedef struct {
    int32_t slot;     /* structure slot */
    int32_t batch;
    wbcqp_inputs in;  /* DEVICE pointers */
    wbcqp_outputs out;
} wbcqp_group;

typedef struct wbcqp_handle wbcqp_handle;

int wbcqp_version(void);
/* text of the last error on this handle (or of the last failed wbcqp_create if handle == NULL) */
const char* wbcqp_last_error(const wbcqp_handle* handle);

/* Binds to a gfx950 device. Fails with WBCQP_ERR_NO_DEVICE when none is present (no CPU path). */
int wbcqp_create(const wbcqp_desc* desc, wbcqp_handle** out);
int wbcqp_destroy(wbcqp_handle* handle);

/* Uploads a task stack into `slot` (0..WBCQP_MAX_STRUCTURES-1): the analogue of
 * solver_->resize(nVar, nEq, nIn) at pos_tracker.cpp:102 plus the constant blocks. */
int wbcqp_set_structure(wbcqp_handle* handle, int slot, const wbcqp_structure* st);
/* Pure host computation; handle may be NULL (usable without a GPU). */
int wbcqp_layout_of(const wbcqp_structure* st, wbcqp_layout* out);

/* Solve `batch` QPs of one structure. All pointers are DEVICE pointers on the handle's device;
 * the launch is asynchronous on `stream` (a hipStream_t, NULL = default stream). */
int wbcqp_solve_batch(wbcqp_handle* handle, int slot, int batch,
                      const wbcqp_inputs* in, const wbcqp_outputs* out, void* stream);
/* Same with HOST pointers: stages through device buffers owned by the handle, blocks until done. */
int wbcqp_solve_batch_host(wbcqp_handle* handle, int slot, int batch,
                           const wbcqp_inputs* in, const wbcqp_outputs* out);
/* Mixed-robot batch: one launch over several homogeneous groups (per-QP n differs between groups). */
int wbcqp_solve_ragged(wbcqp_handle* handle, int n_groups, const wbcqp_group* groups, void* stream);

/* ---- The narrow seam: one dense QP the way tsid's solver hands it to eiquadprog --------------------------
 * What stands behind `solver_->resize(nVar, nEq, nIn)` (pos_tracker.cpp:102) and `const HQPOutput& solver_->solve(const
 * HQPData&)` (controller.cpp:247) once SolverHQuadProgFast has stacked the HQPData:
 *      min 1/2 x'Hx + g'x   s.t.  CE x + ce0 = 0,  CI x + ci0 >= 0
 * H [n][n] (symmetric, the lower triangle is read), g [n], CE [neq][n], ce0 [neq], CI [nin][n], ci0 [nin], all row-major,
 * nin = the rows eiquadprog sees (tsid stacks every two-sided row twice: [A; -A], ci0 = [-lb; ub]).  No structure is
 * assumed and none is needed: this is the compatibility path for a caller that owns its HQPData (INTEGRATION.md section
 * 3 shows the tsid SolverHQPBase subclass); wbcqp_solve_batch on a task stack is the fast path.  n <= 99 (J, R and the vectors of one QP must fit one CU's 160 KiB of LDS:
 * 163 392 bytes at n = 99, whatever neq), nin <= 512.
 * Status values are tsid's (wbcqp_hqp_status: eiquadprog UNBOUNDED -> INFEASIBLE, REDUNDANT_EQUALITIES -> ERROR). */
typedef struct {
    const void *H, *g, *CE, *ce0, *CI, *ci0; /* [batch][...] of the handle's dtype; CE / ce0 may be NULL when neq == 0, CI / ci0 when nin == 0 */
} wbcqp_dense_inputs;

/* DEVICE pointers, asynchronous on `stream`; out->tau is not written (a dense QP has no actuation model), out->x is [batch][n]. */
int wbcqp_solve_dense(wbcqp_handle* handle, int batch, int n, int neq, int nin, int max_iter,
                      const wbcqp_dense_inputs* in, const wbcqp_outputs* out, void* stream);

/* HQPOutput of the reference: owned by the solver, valid until the next call on the same handle (the reference returns a
 * reference to solver-owned storage, controller.cpp:247). */
typedef struct {
    int32_t batch, n;
    const double* x;         /* [batch][n] */
    const int32_t* status;   /* [batch] wbcqp_hqp_status */
    const int32_t* iters;    /* [batch] */
    const double* objective; /* [batch] SolverHQPBase::getObjectiveValue (pos_tracker.hpp:44) */
    const int32_t* n_active; /* [batch] */
} wbcqp_dense_output;

/* HOST pointers to double arrays (whatever the handle's dtype: the reference's Eigen matrices are double), blocks until
 * done; *result points into storage owned by the handle. */
int wbcqp_solve_dense_host(wbcqp_handle* handle, int batch, int n, int neq, int nin, int max_iter,
                           const wbcqp_dense_inputs* in, const wbcqp_dense_output** result);

/* Optional exchange step: all-gather joint torques of a batch sharded over ranks.
 * `comm` is an ncclComm_t created by the caller (RCCL). send: [count] elements, recv: [nranks*count]. */
int wbcqp_allgather_tau(wbcqp_handle* handle, void* comm, const void* send, void* recv,
                        size_t count, void* stream);

/* After the path -- what Controller::_solve does with an optimal solution, controller.cpp:250-272:
 *   v_next = dq + dt dv;  q_next = pinocchio::integrate(model, q, dt v_next);  q_solver = q_next with the base orientation
 *   repacked from quaternion to angle * axis (floating base) or q_next itself.
 * Model: free-flyer root (q = [p, quat(x,y,z,w)], v = [v_lin, w] in the body frame, nq = nv + 1) followed by revolute
 * joints when floating_base != 0, revolute joints only otherwise (nq = nv).  x is the solver output [batch][ldx], dv its
 * first nv entries.  status may be NULL; an instance whose status is not WBCQP_HQP_OPTIMAL keeps its state (the
 * reference throws there, controller.cpp:284-307).  q_solver ([batch][nv]) may be NULL.  DEVICE pointers of the handle's
 * dtype, asynchronous on `stream`.
 * q_next, v_next and q_solver must not overlap q, dq or x: the integration is not done in place (the base's twist is read
 * after v_next has been stored).  q_next == q or v_next == dq is refused with WBCQP_ERR_INVALID; any other overlap is the
 * caller's to avoid.  tests/se3_exact.py states every output exactly; tests/test_gpu_se3_exact.py holds the kernel to it. */
int wbcqp_integrate(wbcqp_handle* handle, int batch, int nv, int floating_base, double dt,
                    const void* q, const void* dq, const void* x, int ldx, const int32_t* status,
                    void* q_next, void* v_next, void* q_solver, void* stream);

/* Same with HOST pointers: stages through device buffers owned by the handle, blocks until done. */
int wbcqp_integrate_host(wbcqp_handle* handle, int batch, int nv, int floating_base, double dt,
                         const void* q, const void* dq, const void* x, int ldx, const int32_t* status,
                         void* q_next, void* v_next, void* q_solver);

/* ---- Before the path: from the robot state to the rows of the QP -------------------------
 * What the upstream half of tsid_->computeProblemData (controller.cpp:244) produces: pinocchio's rigid-body terms (call
 * set of RobotModel::update, src/utils/robot_model.cpp:83-113) and every task's compute() (example_project/src/tsid/
 * ex_task.cpp:175-247, src/tsid/task-momentum-equality.cpp:144-173, src/tsid/task-self-collision.cpp:84-203, gains and
 * masks of src/controllers/tasks.cpp:38-404).  The kinematic tree and the task bindings are DATA (no URDF / YAML parser
 * behind this boundary). */
typedef enum { WBCQP_J_FREEFLYER = 0, WBCQP_J_RX = 1, WBCQP_J_RY = 2, WBCQP_J_RZ = 3, WBCQP_J_PX = 4, WBCQP_J_PY = 5, WBCQP_J_PZ = 6 } wbcqp_joint_type;
typedef enum { WBCQP_T_SE3 = 0, WBCQP_T_COM = 1, WBCQP_T_MOMENTUM = 2, WBCQP_T_SELFCOLLISION = 3 } wbcqp_task_kind;

/* A kinematic tree (what pinocchio::Model holds).  Bodies are numbered depth-first (parent[i] < i and every subtree is a
 * contiguous index range, as pinocchio numbers joints); body 0 hangs on the world by a free-flyer (floating_base: q =
 * [p, quat(x,y,z,w)], v = [linear, angular] in the body frame) or by its own joint.  nq = nbody + 6 / nbody,
 * nv = nbody + 5 / nbody.  Placements are 12 doubles: rotation row-major (9), translation (3).  HOST pointers. */
typedef struct {
    int32_t nbody, floating_base;
    const int32_t* parent;         /* [nbody], -1 for body 0 */
    const int32_t* jtype;          /* [nbody] wbcqp_joint_type */
    const double* placement;       /* [nbody][12] joint frame in the parent's joint frame */
    const double* inertia;         /* [nbody][10] mass, centre of mass (3), inertia at the com: xx xy xz yy yz zz */
    double gravity[3];             /* pinocchio's default (0, 0, -9.81) */
    int32_t nframe;
    const int32_t* frame_body;     /* [nframe] */
    const double* frame_placement; /* [nframe][12] frame in its body's joint frame */
    const double* q_lb;            /* [na] position limits of the actuated joints (tasks.cpp:291-292) */
    const double* q_ub;            /* [na] */
    const double* dq_max;          /* [na] velocity limits (tasks.cpp:287); acceleration limit = dq_max / dt (:288) */
} wbcqp_model;

/* One level-1 task that yields dense rows, in the order of the addMotionTask calls (= file order of tasks.yaml, with the
 * self-collision tasks last as in the shipped stacks): its rows are consecutive in wbcqp_inputs.A / b1. */
typedef struct {
    int32_t kind;    /* wbcqp_task_kind */
    int32_t frame;   /* tracked frame (SE3, self-collision) */
    int32_t mask;    /* bit i = row i kept (tasks.cpp:27-35 convert_mask: character i of the yaml string) */
    double kp, kd;
    int32_t ref;     /* offset of the task's reference inside one instance's reference vector:
                        SE3: placement 12 (translation, rotation COLUMN-major: tsid SE3ToVector, src/trajs/loader.cpp:11-53),
                             velocity 6, acceleration 6 (world-oriented);  CoM: pos 3, vel 3, acc 3;
                             momentum: reference 6, its derivative 6;  self-collision: none */
    int32_t n_avoided;              /* self-collision */
    const int32_t* avoided_frame;   /* [n_avoided] */
    const double* avoided_r0;       /* [n_avoided] */
    double radius, margin, m;       /* self-collision (tasks.cpp:380-383) */
} wbcqp_task;

typedef struct {
    int32_t n_task;
    const wbcqp_task* task;
    double posture_kp, posture_kd;  /* the structure's selection rows (tasks.cpp:181-224) */
    int32_t posture_ref;            /* offset of the na reference positions */
    int32_t n_contact;              /* must equal the structure's nc */
    const int32_t* contact_frame;   /* [n_contact] */
    const double* contact_kp;       /* [n_contact] (tasks.cpp:359-360) */
    const double* contact_kd;
    const int32_t* contact_ref;     /* [n_contact] offset of the contact motion task's reference, 24 numbers like an SE3 task:
                                       placement 12 (tasks.cpp:361-362 sets it), velocity 6, acceleration 6 (zero unless a
                                       behaviour moves the contact: PosTracker::set_contact_se3_ref(sample), pos_tracker.cpp:240-244) */
    int32_t bounds;                 /* 1: the structure's n_bound = na joint-bounds rows are computed (tasks.cpp:274-300) */
    double dt;                      /* CONTROLLER.dt */
    int32_t nref;                   /* reference doubles per instance */
} wbcqp_taskmap;

typedef struct {
    const void* q;    /* [batch][nq] */
    const void* v;    /* [batch][nv] */
    const void* ref;  /* [batch][nref] */
    void* momentum;   /* OUT, may be NULL: [batch][6] centroidal momentum Ag(q) v of this state -- linear (3), then angular about the CoM
                         (3): what Controller::_solve keeps as momentum_ = momentumJacobian(data).bottomRows(3) * dq
                         (controller.cpp:245) is entries 3..5.  The rows kernel forms it anyway (momentum task, CoM velocity). */
} wbcqp_state;

/* Binds a tree and its task bindings to a slot that already holds the matching structure (same nv, na, nc, n_dense,
 * n_sel, n_bound).  A later wbcqp_set_structure on the slot drops the model with the old structure: bind it again (a
 * contact added or removed changes both, pos_tracker.cpp:246-263). */
int wbcqp_set_model(wbcqp_handle* handle, int slot, const wbcqp_model* model, const wbcqp_taskmap* map);
/* Contact force references carried by a tick's reference row (tsid's Contact6d::setForceReference; the stabiliser's ZMP distributor writes them).
 * After wbcqp_set_model, dropped with the model.  force_ref: HOST [nc] offset of contact c's 6-number force reference in a reference row, -1: none (that
 * contact's entries of b1 stay +0).  weight: HOST [nc][6], the w_f the slot's forcereg_mat = diag(w_f) T was made with (T: force_gen).
 * With it the rows kernel writes b1[n_dense + n_sel + 6 c + k] = weight[c][k] * ref[force_ref[c] + k] -- one product, in double -- through every path
 * that runs it: wbcqp_problem_data, wbcqp_tick, wbcqp_tick_host, wbcqp_tick_mixed, the roll-outs (a captured wbcqp_tick_graph keeps what was set when
 * it was created).  The solve consumes it as any right-hand side: the block's cost is |forcereg_mat f - b1|^2 = |diag(w_f) (T f - f_ref)|^2.
 * A slot on which the call was never made, or made with every offset -1, produces the bits it produced before this call existed.
 * WBCQP_ERR_INVALID: a slot without a model; force_ref or weight NULL (nc > 0); an offset below -1; a block [offset, offset + 6) that runs past nref or
 * overlaps another of these blocks; a weight that is not finite; a weight with weight[c][k] * T[c][k][j] != forcereg_mat[c][k][j] for some j, exactly
 * (no tolerance; zeros of either sign are equal; a slot whose weights the caller misstates must not solve silently against the wrong right-hand side). */
int wbcqp_set_force_references(wbcqp_handle* handle, int slot, const int32_t* force_ref, const double* weight);
/* The checks of wbcqp_set_model without a device (pure host computation, like wbcqp_layout_of): is this tree + these task
 * bindings a valid companion of that structure, and how much LDS does one instance of the rows kernel need.  Error text through
 * wbcqp_last_error(NULL). */
int wbcqp_check_model(const wbcqp_structure* st, const wbcqp_model* model, const wbcqp_taskmap* map, int32_t* lds_bytes);
/* Writes the M, h, A, b1, Ac, bc, blb, bub arrays of `rows` (DEVICE pointers, the layout wbcqp_solve_batch reads; tlb, tub
 * and w are not touched: constant limits and weights) for `batch` instances.  Asynchronous on `stream`. */
int wbcqp_problem_data(wbcqp_handle* handle, int slot, int batch, const wbcqp_state* state, const wbcqp_inputs* rows,
                       void* stream);
/* Same with HOST pointers; blocks until done. */
int wbcqp_problem_data_host(wbcqp_handle* handle, int slot, int batch, const wbcqp_state* state, const wbcqp_inputs* rows);

/* ---- One whole control tick on the device: all of Controller::_solve (controller.cpp:231-313) for `batch` instances ----
 * rows (wbcqp_problem_data) -> QP (wbcqp_solve_batch) -> state integration (wbcqp_integrate), ordered on one stream.
 * All pointers are DEVICE pointers. `rows` is the QP record: M, h, A, b1, Ac, bc, blb, bub are scratch the rows kernel
 * writes and the solve reads; tlb, tub, w are supplied by the caller (constant limits, task weights). */
typedef struct {
    wbcqp_state state;
    wbcqp_inputs rows;
    wbcqp_outputs out;
    void* q_next;    /* [batch][nq] */
    void* v_next;    /* [batch][nv]; q_next / v_next must not be state.q / state.v: refused with WBCQP_ERR_INVALID, as wbcqp_integrate refuses it */
    void* q_solver;  /* [batch][nv] or NULL */
    double dt;
} wbcqp_tick_io;

int wbcqp_tick(wbcqp_handle* handle, int slot, int batch, const wbcqp_tick_io* io, void* stream);
/* Same with HOST pointers; blocks until done.  Only the state, the references and the constant tlb / tub / w cross to the
 * device and only x, tau, status, iters (objective, n_active, active_mask if given) and the integrated state come back: about 4 KB per
 * Talos instance instead of the 34 KB record.  The row arrays M .. bub of io->rows may be NULL; where given they receive the
 * rows of this tick (what Controller::cost() reads). */
int wbcqp_tick_host(wbcqp_handle* handle, int slot, int batch, const wbcqp_tick_io* io);

/* ---- K ticks of every instance in one call, without the batch barrier ----
 * Instance i's tick t + 1 depends on instance i's tick t only (controller.cpp:254-256), never on the batch; a loop of wbcqp_tick calls
 * makes every tick wait for the slowest QP of the WHOLE batch, and on the squat stream that one QP is 0.29 ms long while the rest of a
 * 1024-QP batch is worth 0.13 ms of the chip.  wbcqp_rollout enqueues all K ticks up front (rows -> QP -> integration, the kernels of
 * wbcqp_tick; the host waits for nothing), either as ONE stream of ticks -- what K calls of wbcqp_tick are -- or, for 512 instances and
 * more, as TWO sub-batches on HIP streams of their own (each with its own launch-order state and queue counter), whose launches overlap
 * on the device: the tail of one sub-batch's solve runs beside the bulk of the other's.  Which of the two is faster depends on the
 * workload, measured (tools/rollout_bench.py, profiles/r03/rollout_bench.log, profiles/r04/): two sub-batches 1.04x of the tick loop at
 * B = 1024 where one instance stays the hard one, but 0.76x where every instance is heavy (nothing idles in a tick's tail) and 0.93x at
 * B = 4096 (the launch hides its own tail); three sub-batches 1.02x, four 0.57x.  So the library MEASURES: every roll-out is timed on
 * the device by an event pair that a later call reads without blocking; the first roll-outs of a (slot, batch) run as one stream, then
 * as two -- the first sample of either form is not kept: it pays that form's allocations, stream creation and a device synchronisation
 * (so the first TWO calls of each form block on the device once) --, from then on whichever was faster, the other one tried again every
 * 64th call whatever its last figure.  With both measured it is the tick loop or better, up to what a drifting workload changes between
 * two such retries; what it buys is bounded by the slowest INSTANCE's own chain of K ticks (round 5, B = 1024: 1.06x with two sub-batches,
 * 1.09x with three -- a tick's solve is 0.12 ms of which the hard instance's own chain is 0.10 -- profiles/r05/).  Bit for bit the result of K
 * calls of wbcqp_tick with q_next / v_next fed back, whatever the choice.  (A single persistent kernel running the three phases back to back per instance was built and measured first: 0.69x of the tick
 * loop -- the three phases together do not fit 256 VGPRs, and an instance's rows phase runs at 8 waves per CU instead of 16;
 * profiles/r03/fused_rollout_kernel_not_kept.log, DESIGN.md.)  Loop shape: qp_timer_test.cpp:55-63.  All pointers are DEVICE pointers.
 * Ordered after everything already on `stream`; everything enqueued on `stream` afterwards sees the results. */
typedef struct {
    wbcqp_state state;   /* q, v: the state before the first tick; ref: [n_ticks][batch][nref], one reference sample per tick;
                            momentum: of the LAST tick's state, or NULL */
    const void* tlb;     /* [batch][na] torque bounds (NULL if !act_bounds), constant over the ticks */
    const void* tub;
    const void* w;       /* [batch][n_tasks] */
    wbcqp_outputs out;   /* x, tau, status, iters (objective, n_active) of the LAST tick */
    void* q_next;        /* [batch][nq] the state after n_ticks ticks */
    void* v_next;        /* [batch][nv]; with n_ticks == 1 the call is one wbcqp_tick: q_next / v_next equal to state.q / state.v are refused there */
    void* q_solver;      /* [batch][nv] or NULL */
    double dt;
    int32_t* iters_sum;  /* [batch] active-set iterations over all ticks, may be NULL */
    int32_t* ticks_ok;   /* [batch] ticks whose QP was solved (a tick that is not keeps the state, like wbcqp_integrate), may be NULL */
} wbcqp_rollout_io;
/* The slot needs a model (wbcqp_set_model).  The first call of a larger shape allocates the record arrays and the state ping-pong (and
 * synchronises the device to do it); WBCQP_ROLLOUT_STREAMS in the environment fixes the number of sub-batches (1 .. 8; 1: a plain tick loop)
 * instead of the measured choice. */
int wbcqp_rollout(wbcqp_handle* handle, int slot, int batch, int n_ticks, const wbcqp_rollout_io* io, void* stream);

/* ---- A fleet: instances of ONE robot model in DIFFERENT contact sets, one call ----
 * Under a walk, the QP changes size at every lift-off and touchdown (remove_contact / add_contact, pos_tracker.cpp:246-263): one library
 * slot per contact set (a structure and a model each).  wbcqp_tick and wbcqp_rollout take one slot, so every instance of a call is in the
 * same set.  The two calls below take a MIX of slots and, per instance, which of them it uses this tick: the rows kernel runs once per
 * non-empty set and tick on that set's instances (read where they lie, written as a contiguous record), the QPs of all sets go out as ONE
 * launch (wbcqp_solve_ragged: the generic compact kernel when several sets are present), and one kernel puts the outputs back in instance
 * order and integrates each instance from its own set's x.  Bit for bit, instance i's results are those of wbcqp_tick on its slot.
 *
 * Everything is in INSTANCE order: q, v, ref ([batch][nref]), momentum, q_next, v_next, q_solver, and the outputs tau, status, iters,
 * objective, n_active, active_mask.  x is [batch][ldx] with ldx = the largest n over the mix's slots: instance i's row is in the layout of
 * ITS slot ([dv; the forces of that slot's contacts]), zero past its n; active_mask numbers the rows of its own slot's CI.
 * Every slot of a mix holds a structure and a model (wbcqp_set_model), all with the same tree (nq, nv, na, floating base, bodies), the same
 * nref and the same dt: ONE reference row serves every contact set (a single-support task map points its remaining contact's contact_ref at
 * the offset the double-support map uses).  Refused with WBCQP_ERR_INVALID, before anything is launched: a mix that breaks that rule,
 * n_slots outside 1 .. 8, a `which` / `schedule` entry outside [0, n_slots), a NULL w for a slot some instance uses, tlb / tub NULL
 * where a slot in use has actuation bounds.  A handle with WBCQP_FLAG_WARM_START gets WBCQP_ERR_UNSUPPORTED (a hint does not carry across
 * a change of contact set).  The force blocks' factor cache of every slot of the mix is made before the first tick is enqueued (from the
 * weights of instance 0 of that slot's w; the same bits whichever QP it comes from).  The library owns the per-set records (about the
 * size of the instances' own records) and the plan (the per-tick permutation, 4 bytes per instance and tick, copied up once per call);
 * the first call of a larger shape allocates them after a device synchronisation.  DEVICE pointers, asynchronous on `stream`; a call
 * waits on the device for the previous mixed call of the handle (on whatever stream) before it reuses the handle's buffers. */
typedef struct {
    int32_t n_slots;          /* 1 .. 8: one slot per contact set of the same robot model */
    const int32_t* slots;     /* [n_slots] HOST */
    const void* const* w;     /* [n_slots] HOST array of DEVICE pointers, w[k]: [batch][n_tasks of slots[k]], indexed by INSTANCE; may be
                                 NULL for a slot no instance uses */
    const void* tlb;          /* [batch][na] torque bounds by instance (NULL when no slot has actuation bounds) */
    const void* tub;
} wbcqp_mix;

typedef struct {              /* wbcqp_tick_io without the record: the library keeps the per-set records */
    wbcqp_state state;        /* q [batch][nq], v [batch][nv], ref [batch][nref], momentum [batch][6] or NULL */
    wbcqp_outputs out;        /* x [batch][ldx], tau [batch][na], status, iters (objective, n_active, active_mask) by instance */
    void* q_next;             /* [batch][nq] */
    void* v_next;             /* [batch][nv]; q_next / v_next must not be state.q / state.v (the integration is not done in place; NOT checked on this path) */
    void* q_solver;           /* [batch][nv] or NULL */
    double dt;
} wbcqp_mixed_io;

/* One tick; which: HOST [batch], instance i uses mix->slots[which[i]]. */
int wbcqp_tick_mixed(wbcqp_handle* handle, const wbcqp_mix* mix, int batch, const int32_t* which, const wbcqp_mixed_io* io, void* stream);
/* n_ticks ticks enqueued up front (the host waits for nothing; one stream of ticks); schedule: HOST [n_ticks][batch] index into mix->slots.
 * io->state.ref is [n_ticks][batch][nref]; io->w, io->tlb, io->tub are not read (the mix's are); out holds the LAST tick's outputs,
 * iters_sum / ticks_ok the per-instance totals; an instance whose QP fails keeps its state for that tick, as wbcqp_integrate does.
 * Bit for bit n_ticks calls of wbcqp_tick_mixed with q_next / v_next fed back. */
int wbcqp_rollout_mixed(wbcqp_handle* handle, const wbcqp_mix* mix, int batch, int n_ticks, const int32_t* schedule, const wbcqp_rollout_io* io,
                        void* stream);

/* ---- Per-task costs and per-tick traces ----
 * The cost of level-1 task t of an instance (the index space of wbcqp_inputs.w, n_tasks entries) is
 *     cost[t] = || A_t x - b_t ||_2
 * over the rows of task t exactly as they enter H = sum_t w_t A_t' A_t + hessian_reg I and g = -sum_t w_t A_t' b_t:
 *     dense row r (dense_row_task):    A[r] . dv - b1[r]
 *     selection row r (posture):       dv[sel_col[r]] - b1[n_dense + r]
 *     force regularisation, contact c: F_c f_c - b1[n_dense + n_sel + 6 c ..], F = diag(w_f) T (forcereg_mat)
 *     torque task row j:               acteq_scale[j] tau[acteq_joint[j]] - b1[..]   (the row scale_j [M_a | -J_a'] x = scale_j tau_ref_j -
 *                                      scale_j h_a(joint_j) with the decoded tau = M_a dv + h_a - J_a' f)
 *     cop task:                        Acop f - b1[..]
 * For the dense and selection rows this is the reference's Controller::cost(task) (controller.hpp:148-152: the norm of A ddq - b), what
 * `-l cost_<task>` logs every tick (src/robot_dart/talos.cpp:504-505).  Identity: objective = 1/2 sum_t w_t (cost_t^2 - ||b_t||^2) +
 * 1/2 hessian_reg ||x||^2, b_t the right-hand side as it enters g (b1; on the torque rows scale_j tau_ref_j - scale_j h_a(joint_j)).  Costs are formed from x and tau as written, whatever the status: the caller masks by status.  One workgroup per
 * instance, no atomics, a fixed order of summation: the same bits from run to run and between the three entry points below (F32 handles
 * read float, sum in double, write float). */
typedef struct {
    int32_t stride;      /* tick t (0-based) is recorded when (t + 1) % stride == 0: n_rec = n_ticks / stride entries; >= 1 */
    void* q;             /* [n_rec][batch][nq]  the state AFTER the recorded tick (each field may be NULL: not recorded) */
    void* v;             /* [n_rec][batch][nv] */
    void* x;             /* [n_rec][batch][ldx] ldx = n (one slot) / the largest n over the mix's slots, as wbcqp_mixed_io.out.x */
    void* tau;           /* [n_rec][batch][na] */
    int32_t* status;     /* [n_rec][batch] */
    int32_t* iters;      /* [n_rec][batch] */
    void* objective;     /* [n_rec][batch] */
    void* cost;          /* [n_rec][batch][ldc] ldc = n_tasks (one slot) / the largest n_tasks over the mix's slots; zero past the own slot's n_tasks */
} wbcqp_trace;

/* The costs of a solved record: rows as given to wbcqp_solve_batch (A, b1 and Acop are read), x [batch][n] and tau [batch][na] as it wrote
 * them (tau may be NULL when the stack has no torque task); cost [batch][n_tasks].  DEVICE pointers, asynchronous on `stream`. */
int wbcqp_task_costs(wbcqp_handle* handle, int slot, int batch, const wbcqp_inputs* rows, const void* x, const void* tau, void* cost,
                     void* stream);
/* wbcqp_rollout / wbcqp_rollout_mixed that also keep every stride-th tick's results in `trace` (DEVICE pointers).  trace == NULL, or one
 * whose fields are all NULL, is the untraced call.  The outputs of io, iters_sum and ticks_ok are those of the untraced call bit for bit;
 * trace entry r is what (r + 1) stride calls of wbcqp_tick / wbcqp_tick_mixed leave for that tick (q_next, v_next, x, tau, status, iters,
 * objective) and its cost row is wbcqp_task_costs on that tick's record.  The solve and the integration of a recorded tick write straight
 * into the trace (a recorded last tick is copied there from io).  Refused with WBCQP_ERR_INVALID before anything is launched, besides
 * what the untraced call refuses: stride < 1, a cost without a tau (a stack with a torque task, trace->tau and io->out.tau NULL). */
int wbcqp_rollout_traced(wbcqp_handle* handle, int slot, int batch, int n_ticks, const wbcqp_rollout_io* io, const wbcqp_trace* trace,
                         void* stream);
int wbcqp_rollout_mixed_traced(wbcqp_handle* handle, const wbcqp_mix* mix, int batch, int n_ticks, const int32_t* schedule,
                               const wbcqp_rollout_io* io, const wbcqp_trace* trace, void* stream);

/* ---- Where the robots are: centre of mass and frame poses from (q, v) ----
 * What the reference's controller exposes one robot at a time as com() and model_frame_pos(name) (controller.hpp:110,141-146) and its drivers log every
 * tick as com, lf, rh, ... beside cost_<task>.  One wavefront per instance (observe_kernel, csrc/wbcqp_observe.hpp): the rows kernel's kinematics in the
 * true world frame.  Per instance, each output optional:
 *     com       [3]            sum_i m_i (p_i + R_i c_i) / sum_i m_i
 *     vcom      [3]            its velocity (= the first three entries of wbcqp_state.momentum over the total mass)
 *     placement [n_frames][12] world placement of every observed frame: rotation row-major (9), translation (3) -- the layout of wbcqp_model.placement
 *                              (pinocchio's oMf)
 *     velocity  [n_frames][6]  linear (3), angular (3) velocity of the frame in ITS OWN axes (tsid RobotWrapper::frameVelocity)
 * No atomics, a fixed order of summation, and an instance's result depends on its own (q, v) row alone: the same bits from run to run and at whatever
 * index or batch size the row arrives (F32 handles read float, compute in double, write float).
 * A trace needs no entry point of its own: wbcqp_trace.q and wbcqp_trace.v are [n_rec][batch][.] arrays, so one call with batch = n_rec * batch on those
 * pointers observes every recorded tick (bit for bit n_rec calls, one per tick).  Likewise a mixed fleet: the observables depend on the tree alone, which
 * every slot of a mix shares, so any slot of the mix serves (each slot keeps its own selection of frames). */
#define WBCQP_MAX_OBSERVED 64
typedef struct {
    void* com;       /* [batch][3] */
    void* vcom;      /* [batch][3] */
    void* placement; /* [batch][n_frames][12] */
    void* velocity;  /* [batch][n_frames][6] */
} wbcqp_observables; /* each may be NULL: not computed */
/* Which frames of the slot's model are observed: indices into wbcqp_model's frame tables (frames: HOST [n_frames], repeats allowed, n_frames 0 .. 64),
 * uploaded once.  The slot needs a model; a later wbcqp_set_structure or wbcqp_set_model on the slot drops the selection, as it drops the model.
 * WBCQP_ERR_INVALID for a slot without a model, n_frames outside 0 .. WBCQP_MAX_OBSERVED, a frame index outside the model. */
int wbcqp_set_observed_frames(wbcqp_handle* handle, int slot, int n_frames, const int32_t* frames);
/* q [batch][nq], v [batch][nv] and the outputs are DEVICE pointers of the handle's dtype; nothing is copied from the host.  v may be NULL when vcom and
 * velocity are.  Asynchronous on `stream`, ordered like wbcqp_task_costs.  Refused with WBCQP_ERR_INVALID before anything is launched: a slot without a
 * model, batch < 0, placement or velocity given while no frames are selected, vcom or velocity given with v == NULL.  batch == 0: WBCQP_OK, nothing
 * launched. */
int wbcqp_observe(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, void* stream);
/* Same with HOST pointers: stages through device buffers owned by the handle, blocks until done. */
int wbcqp_observe_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out);
/* wbcqp_observe with one more output, acom [batch][3]: the acceleration of the CoM with zero joint accelerations and no gravity, in the world's axes --
 * sum_i m_i a_ci / sum_i m_i, what tsid keeps as data.acom[0] and the CoM task subtracts as its drift; the stabiliser's model ZMP needs it (below).  The
 * same launch of the same kernel: the acceleration sweep sits behind a wave-uniform branch, and the outputs of `out` have the bits wbcqp_observe gives
 * them.  (A call of its own and not a fifth member: wbcqp_observables keeps its size for callers built against it.)  `out` may be NULL (acom alone); acom
 * needs v (refused with v == NULL); acom == NULL is wbcqp_observe.  The _host twin takes HOST pointers. */
int wbcqp_observe_acom(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, void* acom, void* stream);
int wbcqp_observe_acom_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const wbcqp_observables* out, void* acom);

/* ---- Does a robot's sphere model touch itself ----
 * The reference's CollisionCheck::is_colliding (src/safety/collision_check.cpp:27-87), which its controller runs on the solver's own model after every
 * solve (controller.cpp:309-312): every link carries a few spheres, the links are grouped into MEMBERS (arm_left, torso, ...), and the robot collides
 * with itself when two spheres of DIFFERENT members overlap.  One wavefront per instance (collide_kernel, csrc/wbcqp_collide.hpp) on the kinematics of
 * wbcqp_observe.  To the letter of the reference:
 *     world centre   R_body centre + p_body, with the true-world placement of the body's joint frame (oMi[frame.parent] there)
 *     a hit          |c_a - c_b| < (double)(d_a * 0.5f + d_b * 0.5f): the threshold is ONE float addition, the comparison strict and in double
 *     first_pair     the pair the reference's loops meet first.  It walks members in std::map order (sorted by name) a, then b != a, then i over a's
 *                    spheres, then j over b's, so the first hit has the smallest (a, b, i, j) with a < b -- NOT the smallest pair of table indices:
 *                    member b ranks before sphere i.  Sorting the members by name before numbering them is the caller's job.
 * Per instance, each output optional:
 *     colliding  1 / 0          first_pair  [2] table indices of that pair, -1 -1 without a hit
 *     n_pairs    unordered cross-member pairs in collision
 *     clearance  min over cross-member pairs of distance - threshold (negative: penetration depth of the worst pair); +inf with fewer than two members
 *     centres    [n_spheres][3] world centres (the reference's spherical_members())
 * Integer sums and minima and one double minimum, no atomics: the same bits from run to run and at whatever index or batch size a row arrives (F32
 * handles read q as float, compute in double, write clearance and centres as float).  Like wbcqp_observe the call takes any [rows][nq] array: on a
 * trace's q array (batch = n_rec * batch) it checks every recorded tick in one launch, and any slot of a mix serves. */
#define WBCQP_MAX_SPHERES 256
#define WBCQP_MAX_MEMBERS 16
typedef struct {
    int32_t n_spheres;       /* 0 .. WBCQP_MAX_SPHERES; 0 drops the table */
    const int32_t* body;     /* [n_spheres] body (joint) whose joint frame carries the sphere: oMi[frame.parent] in the reference */
    const int32_t* member;   /* [n_spheres] 0 .. WBCQP_MAX_MEMBERS-1, NON-DECREASING: spheres sorted by member, file order inside a member */
    const double* centre;    /* [n_spheres][3] in the body's joint frame */
    const float* diameter;   /* [n_spheres] -- a DIAMETER, and a float, as the reference reads it */
} wbcqp_sphere_model;        /* HOST arrays, copied by wbcqp_set_collision_spheres */
typedef struct {
    int32_t* colliding;  /* [batch]    1 / 0 */
    int32_t* first_pair; /* [batch][2] table indices of the pair the reference's loops meet first, -1 -1 without a hit */
    int32_t* n_pairs;    /* [batch]    unordered cross-member pairs in collision */
    void* clearance;     /* [batch]    min over cross-member pairs of dist - threshold (handle's dtype); +inf with < 2 members */
    void* centres;       /* [batch][n_spheres][3] world centres (handle's dtype) */
} wbcqp_collisions;      /* each may be NULL: not computed */
/* The slot's sphere table, uploaded once.  The slot needs a model; a later wbcqp_set_structure or wbcqp_set_model on the slot drops the table, as it
 * drops the model.  WBCQP_ERR_INVALID (and the table before stays) for a slot without a model, n_spheres outside 0 .. WBCQP_MAX_SPHERES, a body outside
 * the tree, a member outside 0 .. WBCQP_MAX_MEMBERS-1, a decreasing member array, a non-finite centre, a diameter that is non-finite or <= 0. */
int wbcqp_set_collision_spheres(wbcqp_handle* handle, int slot, const wbcqp_sphere_model* spheres);
/* q [batch][nq] and the outputs are DEVICE pointers (q, clearance, centres of the handle's dtype); nothing is copied from the host.  Asynchronous on
 * `stream`, ordered like wbcqp_observe.  Refused with WBCQP_ERR_INVALID before anything is launched: a slot without a model, a slot without a sphere
 * table, batch < 0.  batch == 0: WBCQP_OK, nothing launched. */
int wbcqp_check_collisions(wbcqp_handle* handle, int slot, int batch, const void* q, const wbcqp_collisions* out, void* stream);
/* Same with HOST pointers: stages through device buffers owned by the handle, blocks until done. */
int wbcqp_check_collisions_host(wbcqp_handle* handle, int slot, int batch, const void* q, const wbcqp_collisions* out);

/* ---- Which joint torques a motion needs, under wrenches at frames ----
 * The reference's inria_wbc::utils::RobotModel (src/utils/robot_model.cpp): update() followed by pinocchio::rnea, nonLinearEffects,
 * computeGeneralizedGravity, and compute_rnea_double_support (:138-229), the model-side torque that measured joint torques are compared with.
 * One wavefront per instance (rnea_kernel, csrc/wbcqp_rnea.hpp): a recursive Newton-Euler pass in the rows kernel's frame, world-aligned with its origin
 * at the floating base -- the base's translation q[0..2] is never read, so the result does not lose digits far from the world's origin.
 *     tau [batch][nv] = M(q) a + nle(q, v) - sum_k J_k(q)' w_k      (all nv rows: a floating base's six come first, in pinocchio's convention)
 *       q [batch][nq]; v [batch][nv] or NULL (zero); a: row i at a + i * lda, nv entries, or NULL (zero); lda >= nv
 *       wrench [batch][n_frames][6] or NULL (none): linear (3), angular (3) in the frame's OWN axes -- pinocchio::Force against the LOCAL frame
 *       Jacobian J_k of the k-th selected frame (wbcqp_set_wrench_frames)
 * v == NULL and a == NULL: generalized gravity; a == NULL alone: nonLinearEffects.  lda exists so that the x of a tick or of a trace (rows ldx long, dv
 * first) is passed as `a` without a copy.  No atomics, every sum in a fixed order, and an instance's result depends on its own rows alone: the same bits
 * from run to run and at whatever index or batch size the rows arrive (F32 handles read float, compute in double, write float).  Two frames on one body
 * are subtracted in the order of the selection.
 * Like wbcqp_observe the call takes any arrays of rows: with batch = n_rec * batch on a trace's arrays one call covers every recorded tick.  Mind that
 * wbcqp_trace.q and .v are the state AFTER the recorded tick while .x (and .tau) belong to the state BEFORE it: auditing a trace pairs entry r's x
 * with entry r - 1's q, v (entry 0's with the roll-out's initial state).  For a solved tick, inverse dynamics of (q, v, dv = x[..nv], w_c = T_c f_c at the
 * contact frames, T_c the structure's force generator) is zero on a floating base's six rows and the decoded tau on the actuated rows, up to the
 * solver's equality residual. */
#define WBCQP_MAX_WRENCH_FRAMES 8
/* Where the wrenches of wbcqp_inverse_dynamics act: indices into wbcqp_model's frame tables (frames: HOST [n_frames], 0 .. 8, repeats allowed), uploaded
 * once.  The slot needs a model; a later wbcqp_set_structure or wbcqp_set_model on the slot drops the selection, as it drops the observed frames.
 * WBCQP_ERR_INVALID (and the selection before stays) for a slot without a model, n_frames outside 0 .. WBCQP_MAX_WRENCH_FRAMES, a frame index outside
 * the model. */
int wbcqp_set_wrench_frames(wbcqp_handle* handle, int slot, int n_frames, const int32_t* frames);
/* DEVICE pointers of the handle's dtype, asynchronous on `stream`, ordered like wbcqp_observe; nothing is copied from the host.  Refused with
 * WBCQP_ERR_INVALID before anything is launched: a slot without a model, batch < 0, q or tau NULL, lda < nv with a given, wrench given while no frames
 * are selected.  batch == 0: WBCQP_OK, nothing launched. */
int wbcqp_inverse_dynamics(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench,
                           void* tau, void* stream);
/* Same with HOST pointers: stages through device buffers owned by the handle, blocks until done.  `a` is read up to its last row's nv-th entry. */
int wbcqp_inverse_dynamics_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const void* a, int lda, const void* wrench,
                                void* tau);

/* ---- Which accelerations joint torques produce: M(q), forward dynamics, stable-PD commands ----
 * The reference's RobotModel::inertia_matrix() (include/inria_wbc/utils/robot_model.hpp:41) and inria_wbc::robot_dart::compute_spd
 * (include/inria_wbc/robot_dart/cmd.hpp:10-38), the law by which its drivers turn the controller's position targets into torque commands
 * (--actuators spd).  One wavefront per instance (fdyn_kernel, csrc/wbcqp_fdyn.hpp): the composite-rigid-body algorithm in rnea_kernel's frame, a
 * Cholesky factorisation of M + diag(damping) in wave-private LDS and two triangular solves.  The slot needs a model (nb <= 64, nv <= 64: what
 * wbcqp_inverse_dynamics admits).  No atomics, every sum in a fixed order, an instance's result depends on its own rows alone: the same bits from run
 * to run and at whatever index or batch size the rows arrive.
 *
 * wbcqp_mass_matrix:       M [batch][nv][nv], both triangles (the same bits in both), exact zeros between unrelated branches; a floating base's six
 *                          rows and columns come first, in the base's own axes (pinocchio's convention, as everywhere in this header).
 * wbcqp_forward_dynamics:  (M(q) + diag(damping)) a = tau - nle(q, v) + sum_k J_k(q)' w_k
 *       q [batch][nq]; v [batch][nv] or NULL (zero); tau: row i at tau + i * ldt, ALL nv entries (a floating base's six first), or NULL (zero);
 *       ldt >= nv.  A tick's decoded tau ([batch][na], the actuated joints alone) is not such a row on a floating base: the caller zero-pads it to nv
 *       (six zeros in front).  Passing pointer - 6 elements with ldt = na is NOT admitted (ldt < nv is refused, and the six entries read in front of
 *       row 0 would not be the caller's).
 *       wrench [batch][n_frames][6] or NULL: as for wbcqp_inverse_dynamics -- the frames of wbcqp_set_wrench_frames, linear then angular, in each
 *       frame's own axes.  damping: HOST [nv] or NULL (zero), finite and >= 0, copied into the kernel's arguments by the call.
 *       a [batch][nv]; info [batch] or NULL: 0, or k + 1 when the k-th pivot of the factorisation was not > 0 (LAPACK's potrf convention; a NaN in
 *       q ends here with info = 1): that instance's row of a is all NaN, and no other instance notices.
 *       The bias nle(q, v) - sum_k J_k' w_k is formed by rnea_kernel INTO the row of a and read back from it: on an F32 handle it passes through
 *       a float.
 * wbcqp_spd_commands:      compute_spd.  p = -kp (q + v dt - target), d = -kd v on every dof but a floating base's six (zero there: the
 *       reference's default floating_base = true), qddot = (M + diag(kd) dt)^-1 (p + d - nle(q, v) + sum_k J_k' w_k), commands = p + d - kd qddot dt.
 *       target: row i at target + i * ldtarget, na entries (the actuated joints); a q array serves as pointer + 7 elements with ldtarget = nq on a
 *       floating base.  The reference's robot->constraint_forces() are the `wrench` argument here (the contact wrenches at the selected frames).
 *       commands [batch][nv]; qddot [batch][nv] or NULL; info as above (a failed instance: both rows NaN).
 *       The reference's gains are float(10000 / (dt * 1000)) and float(100 / (dt * 1000)).
 * The output rows (a; commands, qddot) must not overlap any input of the call (q, v, tau, target, wrench) nor each other: the bias is written
 * into the output row BEFORE tau, v and target are read, so a == tau (in place) or commands over target gives wrong results without a word.
 * Refused with WBCQP_ERR_INVALID before anything is launched: a slot without a model, batch < 0, q or the required output (M, a, commands) NULL,
 * ldt < nv with tau given, target NULL or ldtarget < na, wrench given while no frames are selected, a non-finite or negative damping, law NULL,
 * dt not finite or <= 0, a non-finite kp or kd.  batch == 0: WBCQP_OK, nothing launched. */
typedef struct {
    double dt, kp, kd;
} wbcqp_spd;
/* DEVICE pointers of the handle's dtype (info: int32), asynchronous on `stream`, ordered like wbcqp_observe. */
int wbcqp_mass_matrix(wbcqp_handle* handle, int slot, int batch, const void* q, void* M, void* stream);
int wbcqp_forward_dynamics(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const void* tau, int ldt, const void* wrench,
                           const double* damping, void* a, int32_t* info, void* stream);
int wbcqp_spd_commands(wbcqp_handle* handle, int slot, int batch, const wbcqp_spd* law, const void* q, const void* v, const void* target, int ldtarget,
                       const void* wrench, void* commands, void* qddot, int32_t* info, void* stream);
/* Same with HOST pointers: stage through device buffers owned by the handle, block until done.  tau / target are read up to their last row's
 * nv-th / na-th entry. */
int wbcqp_mass_matrix_host(wbcqp_handle* handle, int slot, int batch, const void* q, void* M);
int wbcqp_forward_dynamics_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const void* tau, int ldt, const void* wrench,
                                const double* damping, void* a, int32_t* info);
int wbcqp_spd_commands_host(wbcqp_handle* handle, int slot, int batch, const wbcqp_spd* law, const void* q, const void* v, const void* target,
                            int ldtarget, const void* wrench, void* commands, void* qddot, int32_t* info);

/* ---- Where a fleet's frames move for a given v: frame Jacobians, the CoM Jacobian, the centroidal momentum matrix ----
 * What the reference's RobotModel::update(..., update_jacobians = true) fills one robot at a time (include/inria_wbc/utils/robot_model.hpp;
 * src/utils/robot_model.cpp:92-98, 115-126: computeJointJacobians, jacobianCenterOfMass, RobotModel::jacobian(name, reference_frame)) and the
 * matrix its controller and tsid's TaskMomentumEquality read as momentumJacobian (controller.cpp:245, task-momentum-equality.cpp:151), for a
 * whole fleet.  One wavefront per instance (jacobian_kernel, csrc/wbcqp_jacobians.hpp), no atomics, every sum in a fixed order, an instance's
 * result depends on its own rows alone: the same bits from run to run and at whatever index or batch size the rows arrive.  The slot needs a
 * model (nb <= 64, nv <= 64: what wbcqp_inverse_dynamics admits).
 *
 * reference_frame: pinocchio's values and meanings.  WORLD: the spatial Jacobian about the TRUE world origin in the world's axes (the base
 * translation is kept, as in wbcqp_observe); LOCAL: at the frame's origin in the frame's own axes; LOCAL_WORLD_ALIGNED: at the frame's origin in
 * the world's axes.  J_world = Ad(oMf) J_local with wbcqp_observe's placement oMf.
 *
 * Each member of wbcqp_jacobian_outputs may be NULL; what is given is written, nothing else:
 *   J     [batch][n_frames][6][nv]  the frames of wbcqp_set_jacobian_frames, in the order selected (repeats allowed).  Rows: linear (3), angular (3).
 *                                   Columns in v's order; a floating base's six columns are in the base's own axes, as v is.  The column of a dof
 *                                   that does not move the frame's body is an exact +0.0.
 *   Jcom  [batch][3][nv]            the CoM Jacobian, world axes: vcom = Jcom v.
 *   Ag    [batch][6][nv]            the centroidal momentum matrix: linear, then angular about the CoM, world axes -- the convention of
 *                                   wbcqp_state.momentum (momentum = Ag v).  Jcom = Ag's linear rows over the total mass.
 *   drift [batch][n_frames][6]      the frame's classical acceleration with zero joint accelerations and no gravity (what tsid's SE(3) task uses
 *                                   as Jdot v), in LOCAL or LOCAL_WORLD_ALIGNED axes.  Needs v; not defined for WBCQP_RF_WORLD.
 *   dAgv  [batch][6]                d(Ag)/dt v: the rate of the centroidal momentum with zero joint accelerations.  Needs v.
 * q [batch][nq]; v [batch][nv], or NULL when neither drift nor dAgv is asked for (v is not read then).  The arrays of a trace
 * (wbcqp_trace.q / .v, [n_rec][batch][...]) pass as they are with batch = n_rec * batch: one call answers every recorded tick.
 * Refused with WBCQP_ERR_INVALID before anything is launched (nothing is written): a slot without a model, batch < 0, outputs NULL or every
 * member NULL, an unknown reference_frame, J or drift while no frames are selected, drift or dAgv without v, drift with WBCQP_RF_WORLD, q NULL
 * (batch > 0).  batch == 0: WBCQP_OK, nothing launched. */
typedef enum { WBCQP_RF_WORLD = 0, WBCQP_RF_LOCAL = 1, WBCQP_RF_LOCAL_WORLD_ALIGNED = 2 } wbcqp_reference_frame;
#define WBCQP_MAX_JACOBIAN_FRAMES 64
typedef struct {
    void *J, *Jcom, *Ag, *drift, *dAgv;
} wbcqp_jacobian_outputs;
/* Chooses the frames of J and drift by their indices in the model's frame table: a selection of its own, independent of
 * wbcqp_set_observed_frames and wbcqp_set_wrench_frames.  n_frames == 0 drops it; wbcqp_set_structure / wbcqp_set_model on the slot drop it with
 * the model.  WBCQP_ERR_INVALID (and the selection before stays) for a slot without a model, n_frames outside 0 .. WBCQP_MAX_JACOBIAN_FRAMES, a
 * frame index outside the model. */
int wbcqp_set_jacobian_frames(wbcqp_handle* handle, int slot, int n_frames, const int32_t* frames);
/* DEVICE pointers of the handle's dtype, asynchronous on `stream`, ordered like wbcqp_observe.  reference_frame: a wbcqp_reference_frame. */
int wbcqp_jacobians(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, int reference_frame, const wbcqp_jacobian_outputs* out,
                    void* stream);
/* Same with HOST pointers: stage through device buffers owned by the handle, block until done. */
int wbcqp_jacobians_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, int reference_frame,
                         const wbcqp_jacobian_outputs* out);

/* ---- How a fleet's frame Jacobians change: kinematic Hessians dJ/dq and the Jacobians' time variation ----
 * What the reference's RobotModel::update(..., update_jacobians = true) fills with computeJointKinematicHessians and hands out as
 * RobotModel::hessian(name, reference_frame) (include/inria_wbc/utils/robot_model.hpp:61; src/utils/robot_model.cpp:92-98, 128-135), and
 * pinocchio's getFrameJacobianTimeVariation, for a whole fleet.  One wavefront per instance (hessian_kernel, csrc/wbcqp_hessians.hpp), no
 * atomics, every sum in a fixed order, an instance's result depends on its own rows alone: the same bits from run to run and at whatever index
 * or batch size the rows arrive.  The slot needs a model and a selection of frames (wbcqp_set_jacobian_frames: the frames of wbcqp_jacobians' J,
 * no selection of its own).
 *
 * For a selected frame f in the convention reference_frame, J is exactly what wbcqp_jacobians returns (rows linear then angular, a floating
 * base's six columns in the base's own axes).  Each member of wbcqp_hessian_outputs may be NULL; what is given is written whole, nothing else:
 *   H   [batch][n_frames][6][nv][nv]  H[b][f][r][j][k] = d J[b][f][r][j] / d q_k, k fastest: pinocchio's Tensor3x (6, nv, nv).  d/dq_k is the
 *                                     derivative along dof k in the tangent space, d/de at e = 0 of J(q (+) e e_k) with the SE(3) integration
 *                                     of wbcqp_integrate; that fixes the free-flyer's own 6 x 6 block.
 *   dJ  [batch][n_frames][6][nv]      dJ[b][f][r][j] = sum_k H[b][f][r][j][k] v_k: dJ/dt along v, pinocchio's getFrameJacobianTimeVariation.
 *                                     Needs v.  Formed from the bodies' velocities, not from H: asking for dJ alone costs no H.
 * With "k <= j" for "dof k's body is dof j's body or one of its ancestors" (two dofs of the free-flyer are each <= the other), J_j = (l_j, w_j)
 * column j of J and x_m the motion cross product (l1, w1) x_m (l2, w2) = (w1 x l2 + l1 x w2, w1 x w2), H[.][.][.][j][k] is, where both j and k
 * move the frame's body,
 *   WBCQP_RF_WORLD                k <= j: J_k x_m J_j                 otherwise: +0.0
 *   WBCQP_RF_LOCAL                k <= j: +0.0                        otherwise: J_j x_m J_k
 *   WBCQP_RF_LOCAL_WORLD_ALIGNED  k <= j: (w_k x l_j, w_k x w_j)      otherwise: (w_j x l_k, +0.0)
 * and +0.0 everywhere else.  Every such +0.0, and the entries k = j that are a vector's product with itself, are +0.0 bit for bit; so are the
 * free-flyer's translation and rotation along one axis of the base (dofs i and i + 3) against one another, the same vector twice: all six rows in
 * WBCQP_RF_WORLD, the linear rows in WBCQP_RF_LOCAL_WORLD_ALIGNED (the base's axis does not move when the base turns about it).
 * dJ v is the frame's spatial acceleration at zero joint accelerations: in LOCAL_WORLD_ALIGNED it equals wbcqp_jacobians' drift, in LOCAL
 * drift = dJ v + (w_f x l_f, 0) with (l_f, w_f) = J v.
 * q [batch][nq]; v [batch][nv], or NULL when dJ is not asked for (v is not read then, and H has the bits of the call with v).  The arrays of a
 * trace (wbcqp_trace.q / .v, [n_rec][batch][...]) pass as they are with batch = n_rec * batch.  H is large (6 nv^2 numbers per frame and robot:
 * 120 KB for the Talos-like model, nv = 50): offsets are 64-bit, a call may write more than 4 GB.
 * Refused with WBCQP_ERR_INVALID before anything is launched (nothing is written): a slot without a model, batch < 0, outputs NULL or both
 * members NULL, an unknown reference_frame, no frames selected, dJ without v, q NULL (batch > 0).  batch == 0: WBCQP_OK, nothing launched. */
typedef struct {
    void *H, *dJ;
} wbcqp_hessian_outputs;
/* DEVICE pointers of the handle's dtype, asynchronous on `stream`, ordered like wbcqp_observe.  reference_frame: a wbcqp_reference_frame. */
int wbcqp_kinematic_hessians(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, int reference_frame,
                             const wbcqp_hessian_outputs* out, void* stream);
/* Same with HOST pointers: stage through device buffers owned by the handle, block until done. */
int wbcqp_kinematic_hessians_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, int reference_frame,
                                  const wbcqp_hessian_outputs* out);

/* ---- How a fleet's joint torques change with the state: the derivatives of the inverse dynamics, dtau/dq and dtau/dv ----
 * The linearisation of tau = M(q) a + nle(q, v) - sum_k J_k(q)' w_k (wbcqp_inverse_dynamics) in q and in v -- pinocchio's
 * computeRNEADerivatives -- for a whole fleet: what MPC, DDP or iLQR on a recorded roll-out, a gain or stability analysis of the stable-PD law, the
 * sensitivity of the torque-collision detector's model torque to encoder error and the gravity stiffness dg/dq (v = a = NULL) need; with
 * wbcqp_mass_matrix, the forward dynamics' derivatives da/dq = -M^-1 dtau/dq.  One wavefront per instance (id_derivatives_kernel,
 * csrc/wbcqp_idderiv.hpp), no atomics, every sum in a fixed order, an instance's result depends on its own rows alone: the same bits from run to
 * run and at whatever index or batch size the rows arrive.  The slot needs a model.
 *
 * The inputs are exactly those of wbcqp_inverse_dynamics: q [batch][nq]; v [batch][nv] or NULL (zero); a: rows lda >= nv apart, or NULL (zero), so
 * that a tick's or a trace's x passes as it lies; wrench [batch][n_frames][6] or NULL, acting at the frames of wbcqp_set_wrench_frames, linear
 * then angular in each frame's OWN axes -- and held fixed in those axes while q varies.  Each member of wbcqp_id_derivative_outputs may be NULL;
 * what is given is written whole, nothing else is touched, and asking for one costs none of the other's stores:
 *   dtau_dq  [batch][nv][nv]  dtau_dq[b][i][j] = d tau_i / d q_j, j fastest.  d/dq_j is the derivative along dof j in the tangent space, d/de at
 *                             e = 0 of tau(q (+) e e_j) with the SE(3) integration of wbcqp_integrate: the convention of wbcqp_kinematic_hessians.
 *   dtau_dv  [batch][nv][nv]  dtau_dv[b][i][j] = d tau_i / d v_j.  Needs v.
 * d tau / d a is M(q): wbcqp_mass_matrix gives it; it is no output here.
 * Exact +0.0, bit for bit: every entry whose two dofs lie on unrelated branches (M's pattern, in both matrices); columns 0..2 of dtau_dq on a
 * floating base (nothing depends on where the base is); and, with v NULL, every velocity term of dtau_dq (that sweep is not run).
 * The closed forms are at the head of csrc/wbcqp_idderiv.hpp and in DESIGN 4.22.  Offsets are 64-bit.  F32 handles read float, compute in double
 * and write float.
 * Refused with WBCQP_ERR_INVALID before anything is launched (nothing is written): a slot without a model, batch < 0, outputs NULL or both members
 * NULL, dtau_dv without v, lda < nv with a given, wrench given while no frames are selected, q NULL (batch > 0).  batch == 0: WBCQP_OK, nothing
 * launched. */
typedef struct {
    void *dtau_dq, *dtau_dv;
} wbcqp_id_derivative_outputs;
/* DEVICE pointers of the handle's dtype, asynchronous on `stream`, ordered like wbcqp_observe. */
int wbcqp_inverse_dynamics_derivatives(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const void* a, int lda,
                                       const void* wrench, const wbcqp_id_derivative_outputs* out, void* stream);
/* Same with HOST pointers: stage through device buffers owned by the handle, block until done. */
int wbcqp_inverse_dynamics_derivatives_host(wbcqp_handle* handle, int slot, int batch, const void* q, const void* v, const void* a, int lda,
                                            const void* wrench, const wbcqp_id_derivative_outputs* out);

/* ---- Did a robot hit something: model torques against measured torques over a stream of ticks ----
 * The reference's inria_wbc::safety::TorqueCollisionDetection (src/safety/torque_collision_detection.cpp) with the filters of
 * include/inria_wbc/estimators/filtering.hpp, as its controller wires them (src/controllers/talos_pos_tracker.cpp:62-158), for a whole fleet and
 * n_ticks ticks in one call.  One wavefront per instance (torque_monitor_kernel, csrc/wbcqp_monitor.hpp), one lane per monitored joint; the wave walks
 * its instance's ticks in order.  No slot and no model: this is signal processing on arrays the other calls produce.  Per instance and tick:
 *   1. filter the sensors' samples over a window (Filter::filter): while fewer than `window` samples have been seen the window is the samples so far,
 *      afterwards the last `window` samples.  MEAN: the window summed oldest first, one division by the count.  MEDIAN: the middle element of the
 *      sorted window, the mean of the two middle ones for an even count (a NaN sorts above every number).  NONE: the sample itself.
 *   2. filtered += offset, when given
 *   3. discrepancy = tau_model[joint[j]] - filtered[j]; RAW validity is |discrepancy| < threshold, strict
 *   4. with K = max_invalid + 1, joint j is INVALID iff in each of the last K ticks it was raw-invalid with the same non-zero sign of the discrepancy
 *   5. detected = any joint invalid (the reference's check returns false)
 * A NaN discrepancy is raw-invalid but has no sign, so by itself it never makes a joint invalid (the reference casts the sign of a NaN to int, which is
 * undefined; this is the reading its ring of signs gives when that cast yields 0).  The same holds for a discrepancy of exactly zero under a threshold <= 0.
 * Arrays (tau_model, tau_sensor, discrepancy, filtered of the handle's dtype):
 *   tau_model   row (t, i) at tau_model + (t * batch + i) * ldt: a trace's tau with ldt = na as it lies; the output of inverse dynamics passed as pointer
 *               + 6 elements with ldt = nv.  Read at the columns `joint` alone.
 *   tau_sensor  [n_ticks][batch][n_joints]
 *   state       [batch][state_bytes], in and out, always double whatever the dtype: the window and the K-step memory of every joint.  All-zero bytes
 *               are a freshly reset detector (the reference's reset is a memset); NULL: a fresh detector for this call, discarded afterwards.
 *               A state belongs to the monitor's n_joints, filter, window and max_invalid; thresholds, offsets and columns may change between calls.
 * A stream cut into calls at any tick, the state carried along, gives the bits of one call.  Only additions, one division and one subtraction: no
 * atomics, nothing to fuse, an instance's results depend on its own rows alone (F32 handles read float, compute in double, write float). */
#define WBCQP_MAX_MONITORED 64 /* one lane per monitored joint */
#define WBCQP_MAX_FILTER_WINDOW 64
#define WBCQP_MAX_INVALID 31
enum { WBCQP_FILTER_NONE = 0, WBCQP_FILTER_MEAN = 1, WBCQP_FILTER_MEDIAN = 2 };
typedef struct {
    int32_t n_joints;        /* 1 .. WBCQP_MAX_MONITORED */
    const int32_t* joint;    /* [n_joints] column of a tau_model row; repeats allowed */
    const double* threshold; /* [n_joints]; +-inf and negative values allowed (the reference's file uses 1e10 as "off"), NaN refused */
    const double* offset;    /* [n_joints] or NULL (set_offset / remove_offset); finite */
    int32_t filter, window;  /* WBCQP_FILTER_*; 1 .. WBCQP_MAX_FILTER_WINDOW (ignored for NONE) */
    int32_t max_invalid;     /* 0 .. WBCQP_MAX_INVALID: set_max_consecutive_invalid */
} wbcqp_torque_monitor;      /* HOST; copied into the kernel's arguments each call (about 1.3 KB): no device table, nothing to drop */
typedef struct {
    int32_t* detected;   /* [n_ticks][batch] 1 where the reference's check returned false */
    uint64_t* invalid;   /* [n_ticks][batch] bit j: monitored joint j invalid (get_invalid_ids) */
    void* discrepancy;   /* [n_ticks][batch][n_joints] handle's dtype (get_discrepancy) */
    void* filtered;      /* [n_ticks][batch][n_joints] handle's dtype (get_filtered_sensors, offset included) */
    int32_t* first_tick; /* [batch] first tick of THIS call with detected, -1 if none */
    int32_t* n_detected; /* [batch] ticks of this call with detected */
} wbcqp_torque_checks;   /* each may be NULL: not written */
/* Bytes of one instance's state for this monitor: 8 + 8 n_joints + 8 window n_joints (no window for NONE).  Pure host code; 0 for a monitor the calls
 * below refuse (NULL, n_joints / filter / window / max_invalid out of range, a NULL or negative joint, a NaN threshold, a non-finite offset). */
int64_t wbcqp_torque_monitor_state_bytes(const wbcqp_torque_monitor* monitor);
/* DEVICE pointers (state included), asynchronous on `stream`, ordered like wbcqp_observe; the monitor itself is read on the host before the call returns.
 * Refused with WBCQP_ERR_INVALID before anything is launched: a monitor as above, a joint outside [0, ldt), batch < 0, n_ticks < 0, tau_model, tau_sensor
 * or out NULL.  WBCQP_OK with nothing launched: batch == 0, n_ticks == 0, or every output NULL and state NULL.  Every output NULL with a state given
 * still runs and advances the state. */
int wbcqp_detect_torque_collisions(wbcqp_handle* handle, const wbcqp_torque_monitor* monitor, int batch, int n_ticks, const void* tau_model, int ldt,
                                   const void* tau_sensor, void* state, const wbcqp_torque_checks* out, void* stream);
/* Same with HOST pointers, state included (staged both ways): through device buffers owned by the handle, blocks until done.  tau_model is read up to
 * its last row's highest monitored column. */
int wbcqp_detect_torque_collisions_host(wbcqp_handle* handle, const wbcqp_torque_monitor* monitor, int batch, int n_ticks, const void* tau_model, int ldt,
                                        const void* tau_sensor, void* state, const wbcqp_torque_checks* out);

/* ---- Keep a fleet on its feet: CoP estimator and admittance laws on a tick's references ----
 * The stabiliser of the reference's humanoid controllers (src/controllers/humanoid_pos_tracker.cpp:134-302, src/stabilizers/stabilizer.cpp,
 * src/estimators/cop.cpp, include/inria_wbc/estimators/filtering.hpp), one tick of it for every robot of a fleet.  Only a tick's references change, never
 * the QP's structure: one wavefront per instance (stabilize_kernel, csrc/wbcqp_stabilize.hpp) reads the reference row, the feet's force/torque samples,
 * the model's CoM, its acceleration and the feet's positions, and writes the row that wbcqp_problem_data / wbcqp_tick / wbcqp_tick_mixed consume
 * unchanged.  The caller keeps `ref` and passes ref_out to the tick: that is the reference's "put the references back".  Per instance and tick, in double
 * (w = window, FMIN = 30):
 *   filters   every filter is a moving average: the samples so far while fewer than w have been pushed, afterwards the last w; summed oldest first, one
 *             division by the count.  READY: at least w samples since the start or the last reset.
 *   CoP       left foot, when lf_force.z > FMIN: raw = foot.xy + ((-torque.y - foot.z force.x) / force.z, (torque.x - foot.z force.y) / force.z), pushed
 *             into the left CoP filter; otherwise that filter is RESET.  The right foot alike.  With both raw CoPs: Kajita's weighted combination
 *             (cop.cpp:71-83, in its order of operations) pushed into the combined filter; with a foot missing the combined filter is neither pushed nor
 *             reset, so its stale samples are averaged after touch-down.  A filtered CoP is VALID this tick iff its raw value existed this tick, its
 *             filter is ready and neither coordinate is NaN.  valid_cop: the first valid one of (combined, left, right).
 *   forces    when |lf_force| > FMIN (sqrt(x^2 + y^2 + z^2)), lf_force.z is pushed into the left force filter; otherwise the filtered force of this tick
 *             is zero and the filter is left alone.  The right foot alike.
 *   CoM       with a valid_cop: zmp = com.xy - com.z / 9.81 * acom.xy, cor = zmp - valid_cop; on the xy entries of the CoM reference
 *             pos -= p[0:2] cor, vel -= p[2:4] cor / dt, acc -= p[4:6] cor / (dt dt)                                       (p = com_gains)
 *   ankles    per foot with a valid CoP and an active contact: pitch = p[0] (cop.x - foot.x), roll = p[1] (cop.y - foot.y); (e0, e1, e2) = Eigen's
 *             eulerAngles(0, 1, 2) of the foot task's reference rotation; R' = Rx(e0 + roll) Ry(e1 + pitch) Rz(e2); vel[4] += p[2] pitch / dt,
 *             vel[3] += p[3] roll / dt, acc[4] += p[4] pitch / (dt dt), acc[3] += p[5] roll / (dt dt)                      (p = ankle_gains)
 *             The foot task's reference becomes (its translation, R', these vel / acc); the contact's (ITS translation, R', the FOOT TASK's vel / acc).
 *             Eigen's first angle lies in [0, pi]: for a rotation whose atan2(R(1,2), R(2,2)) > 0 the added pitch acts with the opposite sign.
 *   torso     with x_prev, both force columns and both force filters ready: n_l, n_r = sum over the contact's four point forces of normal . f_i in
 *             x_prev; zctrl = |n_l - n_r| - |lf_filtered.z - rf_filtered.z|; roll = g[0] zctrl; the torso reference's e0 += roll,
 *             vel[3] += g[1] roll / dt, acc[3] += g[2] roll / (dt dt)                                                      (g = ffda_gains)
 *   guards    where the reference throws -- a CoP handed to a law with |x| >= 10 AND |y| >= 10 (WBCQP_STAB_ERR_COP); otherwise, inside the torso law,
 *             |lf_filtered.z + rf_filtered.z| > 10 mass 9.81 (WBCQP_STAB_ERR_FORCE) -- the instance's ref_out is its ref, no law's bit is set, and its
 *             state has advanced as usual (the reference throws after its filters are updated).  No other instance is affected.
 * com, acom and the feet's positions are arrays of the caller's: wbcqp_observe_acom's com, acom and placement as they lie (lf_pos = 12 f + 9 for observed
 * frame f).  The reference reads them from the state the PREVIOUS tick's rows were formed at.
 * Every product, sum and quotient rounds once, in the reference's association; rotations go through atan2 / sin / cos and are the only entries that depend
 * on the device's libm.  No atomics, an instance's results depend on its own rows alone (F32 handles read float, compute in double, write float).
 * Not here: the momentum / IMU admittances and direct_zmp_distributor_admittance (the reference's controller never calls them), the torso-roll clamp
 * of TalosPosTracker, a roll-out form (a stabilised tick needs that tick's sensors).  The ZMP force distributor (use_zmp) is wbcqp_stabilize_zmp below.
 * A mixed fleet: one call per contact set on that set's rows. */
#define WBCQP_MAX_STAB_WINDOW 64
enum {
    WBCQP_STAB_COP = 1, WBCQP_STAB_LCOP = 2, WBCQP_STAB_RCOP = 4,                               /* the combined / left / right filtered CoP is valid */
    WBCQP_STAB_COM = 8, WBCQP_STAB_LANKLE = 16, WBCQP_STAB_RANKLE = 32, WBCQP_STAB_FFDA = 64, /* the law was applied */
    WBCQP_STAB_ERR_COP = 128, WBCQP_STAB_ERR_FORCE = 256,
    WBCQP_STAB_ZMP = 512,      /* wbcqp_stabilize_zmp: the ZMP force distributor ran (the force references were formed) */
    WBCQP_STAB_ERR_ZMP = 1024  /* ... or met the reference's "this case should not exists" */
};
typedef struct {
    int32_t window;                              /* filter_size, 1 .. WBCQP_MAX_STAB_WINDOW */
    double dt, mass;                             /* CONTROLLER.dt; total model mass (Mg = mass * 9.81) */
    double com_gains[6], ankle_gains[6], ffda_gains[3];
    int32_t nref;
    int32_t com_ref, lf_ref, rf_ref, torso_ref;  /* offsets in a reference row (wbcqp_task.ref); all required */
    int32_t lf_contact_ref, rf_contact_ref;      /* wbcqp_taskmap.contact_ref of the foot's contact; -1: contact not active */
    int32_t lf_force_col, rf_force_col;          /* first of the contact's 12 force variables in a row of x; -1: not active */
    double normal[3];                            /* contact normal (tasks.yaml `normal`) */
    int32_t lf_pos, rf_pos;                      /* element offset of the foot's translation inside a row of `placement` */
} wbcqp_stabilizer;                              /* HOST, read before the call returns */
typedef struct {
    const void* ref;       /* [batch][nref] */
    const void* wrench;    /* [batch][12]: lf_force, lf_torque, rf_force, rf_torque (the sensor_data keys) */
    const void* com;       /* [batch][3] */
    const void* acom;      /* [batch][3] */
    const void* placement; /* row i at placement + i * ldp: wbcqp_observables.placement as it lies */
    int32_t ldp;
    const void* x_prev;    /* row i at x_prev + i * ldx: the previous tick's x, or NULL (first tick: no torso law) */
    int32_t ldx;
} wbcqp_stab_inputs;
typedef struct {
    void* ref_out;  /* [batch][nref]; may equal ref exactly (in place) */
    int32_t* flags; /* [batch] WBCQP_STAB_* */
    void* cop;      /* [batch][3][2] filtered CoP: combined, left, right; NaN where not valid */
} wbcqp_stab_outputs; /* each may be NULL (and so may the struct) */
/* Bytes of one instance's state: 40 + 64 window.  Layout (always double, whatever the dtype): [5]{int32 count, int32 head} of the filters combined, left,
 * right CoP, left, right force z; then [window][8] samples, channels combined x, y, left x, y, right x, y, left fz, right fz.  All-zero bytes are a
 * fresh stabiliser.  A state belongs to its window.  The block is read and written as 8-byte words: `state` must be 8-byte aligned (the size is a
 * multiple of 8, so every instance's block then is).  Pure host code; 0 for a stabiliser the calls below refuse. */
int64_t wbcqp_stabilizer_state_bytes(const wbcqp_stabilizer* stabilizer);
/* DEVICE pointers (state included; state NULL: a fresh stabiliser for this call, discarded afterwards), asynchronous on `stream`, ordered like
 * wbcqp_observe.  Refused with WBCQP_ERR_INVALID before anything is launched: a NULL stabiliser, inputs, ref, wrench, com, acom or placement; window out
 * of range; dt or mass not finite or not > 0; a gain or the normal not finite; a required offset negative (an optional one below -1), an offset whose
 * block (CoM 9, others 24) runs past nref, two blocks that overlap; ldp < max(lf_pos, rf_pos) + 3; with x_prev, ldx < an active force column + 12; batch < 0.
 * WBCQP_OK with nothing launched: batch == 0; every output NULL and state NULL. */
int wbcqp_stabilize(wbcqp_handle* handle, const wbcqp_stabilizer* stabilizer, int batch, const wbcqp_stab_inputs* in, void* state,
                    const wbcqp_stab_outputs* out, void* stream);
/* Same with HOST pointers, state included (staged both ways): through device buffers owned by the handle, blocks until done. */
int wbcqp_stabilize_host(wbcqp_handle* handle, const wbcqp_stabilizer* stabilizer, int batch, const wbcqp_stab_inputs* in, void* state,
                         const wbcqp_stab_outputs* out);

/* ---- The stabiliser's ZMP force distributor (use_zmp: true in the reference's Talos support files) ----
 * stabilizer.cpp:277-311, 340-440 and humanoid_pos_tracker.cpp:212-224 there: the robot's weight is split between the feet by where the ZMP lies between
 * them, the split becomes a 6-D force reference per foot, and the contacts' force-regularisation weights become zmp_w.  wbcqp_stabilize_zmp is
 * wbcqp_stabilize with that law compiled in (a second instantiation of stabilize_kernel: same state, same layout, same
 * wbcqp_stabilizer_state_bytes); zmp == NULL IS wbcqp_stabilize, bit for bit.
 *   distribute(z), both contacts active (PL, PR: the xy of the left / right CONTACT reference's translation as it lies in `ref`; all at height 0):
 *             u = PR - PL, e = u / |u| (u itself where u.u is not > 0: Eigen's normalized()), proj = PR + e ((z - PR) . e),
 *             L = |PR - PL|, a1 = |proj - PL|, a2 = |PR - proj|;  alpha = a1 / L if |(L - a1) - a2| < 1e-10, else 0 if a1 < a2, else 1 if a1 > a2,
 *             else the reference throws (only non-finite inputs get there).  Coincident feet: alpha = 0 / 0 = NaN and no throw.
 *             only the right contact active: alpha = 1, PL = (0, 0); only the left: alpha = 0, PR = (0, 0)
 *             f_r = ((-alpha) mass) 9.81, f_l = ((-(1 - alpha)) mass) 9.81, tau0 = (-(PR - z)) f_r - (PL - z) f_l  (per coordinate),
 *             tauR.y = alpha tau0.y, tauL.y = (1 - alpha) tau0.y; tau0.x < 0: tauR.x = tau0.x, tauL.x = 0, otherwise tauR.x = 0, tauL.x = tau0.x
 *             left = (0, 0, f_l, tauL.y, -tauL.x, 0), right = (0, 0, f_r, tauR.y, -tauR.x, 0); signed zeros as the arithmetic leaves them
 *   ZMP law   exactly when the CoM law runs (a valid_cop, no guard tripped), after it and before the ankles: t = distribute(zmp) with the CoM law's
 *             zmp = com.xy - com.z / 9.81 * acom.xy, s = distribute(valid_cop); per foot and entry e = t - s, fref = (t - p e) - (d e) / dt.
 *             fref of the left / right foot is written at lf_force_ref / rf_force_ref of ref_out (an offset -1: not written), whether or not that
 *             foot's contact is active, and WBCQP_STAB_ZMP is set.  On a tick where the law does not run the two blocks pass through from `ref`
 *             (the caller's base row holds zeros there: the reference's "put the force references back").
 *   guards    far CoP (the CoM law's own, the same valid_cop), then the throw above in either distribute (WBCQP_STAB_ERR_ZMP), then the torso law's
 *             force guard: the first that trips ends the tick as the guards of wbcqp_stabilize do (ref_out is ref, no law's bit, filters advanced).
 * Additions, products, quotients and one square root, each rounded once: the force references have no libm tolerance.
 * The latch.  The reference sets zmp_w on BOTH contact objects the first time the law runs for a robot and never sets it back.  A slot's forcereg_mat is
 * diag(w_f) T, so the caller keeps two slots per contact set -- one made with the default w_f, one with forcereg_mat = diag(zmp_w) T -- both with
 * wbcqp_set_force_references, and ticks the fleet through wbcqp_tick_mixed: from the first tick whose flags carry WBCQP_STAB_ZMP robot i is ticked in
 * the zmp_w slot, for good (three contact sets x two weightings: 6 of the 8 slots). */
typedef struct {
    double p[6], d[6];                  /* zmp_p, zmp_d */
    int32_t lf_force_ref, rf_force_ref; /* offsets of the feet's 6-number force references in a reference row, -1: not written */
} wbcqp_zmp_distributor;                /* HOST, read before the call returns */
/* wbcqp_stabilize with the distributor.  alpha (DEVICE, the handle's dtype) [batch][2] or NULL: alpha of the model's ZMP, of the measured one; NaN where
 * the law did not run.  Refused with WBCQP_ERR_INVALID before anything is launched: everything wbcqp_stabilize refuses; with zmp, a p or d that is not
 * finite, a force reference offset below -1, a block [offset, offset + 6) that runs past nref or overlaps one of the stabiliser's six blocks or the other
 * force reference, lf_contact_ref < 0 && rf_contact_ref < 0 (the reference's "is talos jumping ?").  An alpha alone counts as an output. */
int wbcqp_stabilize_zmp(wbcqp_handle* handle, const wbcqp_stabilizer* stabilizer, const wbcqp_zmp_distributor* zmp, int batch, const wbcqp_stab_inputs* in,
                        void* state, const wbcqp_stab_outputs* out, void* alpha, void* stream);
/* Same with HOST pointers (state and alpha included), blocks until done; the same refusals. */
int wbcqp_stabilize_zmp_host(wbcqp_handle* handle, const wbcqp_stabilizer* stabilizer, const wbcqp_zmp_distributor* zmp, int batch,
                             const wbcqp_stab_inputs* in, void* state, const wbcqp_stab_outputs* out, void* alpha);

/* ---- References generated on the device from a reference program ----
 * wbcqp_rollout and its companions read the references of n_ticks ticks as one array [n_ticks][batch][nref] (2.44 KB per Talos instance and tick) that the
 * caller plans on the host and copies up.  Every behaviour of the reference precomputes its references as streams of consecutive min-jerk moves and holds
 * and plays one sample per tick (include/inria_wbc/trajs/trajectory_generator.hpp:23-156, src/behaviors/humanoid/move_com.cpp:22-60,
 * src/behaviors/generic/cartesian.cpp:28-61, src/behaviors/humanoid/walk_on_spot.cpp:40-184); a fleet differs between its robots only in WHEN each starts.
 * A wbcqp_program is that stream as data -- a few dozen numbers and one start tick per instance -- and refgen_kernel (csrc/wbcqp_refgen.hpp) expands it on the
 * device, a chunk of ticks per launch, into a ring of two chunks that the rows kernel reads: a roll-out of any length needs neither a host plan nor a
 * reference array sized by n_ticks.
 *
 * Timeline: n_intro ticks played once, then n_cycle ticks repeated (n_cycle = 0: the last sample is held).  Instance i is at behaviour tick
 * tau = tick0 + t - offset[i] on tick t of a call; the sample played is number 0 for tau < 0, tau for tau < n_intro, else
 * n_intro + (tau - n_intro) % n_cycle (n_cycle = 0: min(tau, n_intro - 1)).  Every track's segments tile the n_intro + n_cycle samples of the timeline.
 * Sample i of a segment (T, x0, xf, R0, axis, angle) is the reference's closed form at t = dt i, td = t / T:
 *     s = 6 td^5 - 15 td^4 + 10 td^3,  pos = x0 + (xf - x0) s,  vel = (xf - x0)(30 td^4 - 60 td^3 + 30 td^2) / T,  acc = (xf - x0)(120 td^3 - 180 td^2 + 60 td) / T^2
 *     R = R0 Rot(axis, angle s), angular velocity / acceleration R0 (angle s' axis), R0 (angle s'' axis)          (trajectory_generator.hpp:41-59, 80-147)
 * computed in double whatever the handle's dtype.  A hold is a segment with xf = x0 (angle = 0): it comes out as x0 (R0) bit for bit.  The caller makes
 * n_steps = floor(T / dt) and (axis, angle) from R0' R1 (Eigen::AngleAxisd(Matrix3d)); the library takes them as given.  The result is a pure function of
 * (program, offset[i], tick): the same bits whichever chunk, call or sub-batch a tick falls in. */
#define WBCQP_MAX_TRACKS 16
typedef enum {
    WBCQP_TRACK_VEC = 0, /* dim 3: pos 3 | vel 3 | acc 3 at the destination (a CoM task's reference, wbcqp_task.ref); dim 1: one number (a posture entry) */
    WBCQP_TRACK_SE3 = 1  /* placement 12 (translation, rotation column-major) | velocity 6 | acceleration 6 (an SE3 task's or a contact's reference) */
} wbcqp_track_kind;
#define WBCQP_TRACK_POSE_ONLY 1 /* velocity and acceleration are written as zeros (what set_se3_ref(SE3, name) / set_com_ref(Vector3d) leave) */
#define WBCQP_TRACK_RELATIVE 2  /* translations are added to the position `base` row i holds at dst[0]; an SE3 track's rotation becomes R_base(i) R(t) and
                                   its angular parts are rotated by R_base(i) (`absolute: false` of move_com.cpp, cartesian.cpp's relative targets) */
typedef struct {
    int32_t n_steps;   /* ticks of the segment, >= 1 */
    double T;          /* its duration, > 0 */
    double x0[3], xf[3]; /* VEC of dim 1: entry 0 */
    double R0[9];      /* SE3: rotation at the start, row-major */
    double axis[3];    /* SE3: unit axis of R0' R1 */
    double angle;      /* SE3: its angle */
} wbcqp_segment;

typedef struct {
    int32_t kind;      /* wbcqp_track_kind */
    int32_t dim;       /* VEC: 1 or 3 */
    int32_t flags;     /* WBCQP_TRACK_* */
    int32_t dst[2];    /* offsets into the reference row; dst[1] < 0: one destination (a foot's stream feeds the foot task AND its contact's reference) */
    int32_t n_segments;
    const wbcqp_segment* segments; /* HOST [n_segments], consecutive on the timeline */
} wbcqp_track;

typedef struct {
    int32_t nref;          /* length of a reference row = the slot's (the mix's) nref */
    int32_t base_stride;   /* 1: base is [batch][nref]; 0: [1][nref], one row for every instance */
    const void* base;      /* DEVICE, the handle's dtype: every entry no track writes, and the origin of the RELATIVE tracks */
    const int32_t* offset; /* HOST [batch]: the call tick at which instance i starts the behaviour */
    int32_t n_intro, n_cycle;
    double dt;             /* sample i of a segment is at t = dt i */
    int32_t n_tracks;      /* <= WBCQP_MAX_TRACKS */
    const wbcqp_track* tracks; /* HOST [n_tracks] */
    const int32_t* set_of; /* HOST [n_intro + n_cycle] or NULL: contact set (index into wbcqp_mix.slots) of every sample; read by wbcqp_rollout_mixed_program only */
} wbcqp_program;

/* Pure host, no device (like wbcqp_check_model); error text through wbcqp_last_error(NULL).  WBCQP_ERR_INVALID for: more than WBCQP_MAX_TRACKS tracks, an
 * empty timeline, a track whose segments do not sum to n_intro + n_cycle, n_steps < 1 or T <= 0, a destination whose extent leaves [0, nref), two extents
 * that overlap, dim outside {1, 3}, a non-unit axis, a set_of entry outside [0, n_slots) (n_slots <= 0: set_of is not looked at). */
int wbcqp_check_program(const wbcqp_program* prog, int batch, int n_slots);
/* The expansion alone: ref_out (DEVICE, the handle's dtype) [n_ticks][batch][nref] = the references of call ticks [0, n_ticks) of a call at tick0.
 * Asynchronous on `stream`.  The tables and offsets go up through a ring of four page-locked buffers (a call waits for the one four calls ago). */
int wbcqp_reference_samples(wbcqp_handle* handle, const wbcqp_program* prog, int batch, int tick0, int n_ticks, void* ref_out, void* stream);
/* wbcqp_rollout_traced with the references generated on the device: io->state.ref is not read and may be NULL, trace may be NULL.  The rows are made
 * WBCQP_REFPROG_CHUNK ticks per launch (environment, read at wbcqp_create; default 32) on the stream of the sub-batch that reads them.  Bit for bit
 * wbcqp_rollout_traced on the output of wbcqp_reference_samples.  Refusals: those of wbcqp_rollout_traced, then wbcqp_check_program's, then nref. */
int wbcqp_rollout_program(wbcqp_handle* handle, int slot, int batch, int tick0, int n_ticks, const wbcqp_rollout_io* io, const wbcqp_program* prog,
                          const wbcqp_trace* trace, void* stream);
/* wbcqp_rollout_mixed_traced likewise; the schedule is made on the host from set_of (required), offset and tick0. */
int wbcqp_rollout_mixed_program(wbcqp_handle* handle, const wbcqp_mix* mix, int batch, int tick0, int n_ticks, const wbcqp_rollout_io* io,
                                const wbcqp_program* prog, const wbcqp_trace* trace, void* stream);

/* The same sequence captured once into a HIP graph and replayed: one graph launch per tick instead of four kernel
 * launches (what matters when the batch is small -- one robot at 1 kHz is the reference's own use case).  The graph is
 * bound to the pointers of `io`; the caller changes the CONTENT of those buffers between ticks (new references, or
 * q_next / v_next copied back into state.q / state.v), not the pointers.  wbcqp_tick_graph_create runs one ordinary tick
 * first (so nothing is allocated inside the capture) and blocks until it is done. */
typedef struct wbcqp_graph wbcqp_graph;
int wbcqp_tick_graph_create(wbcqp_handle* handle, int slot, int batch, const wbcqp_tick_io* io, wbcqp_graph** out);
int wbcqp_tick_graph_launch(wbcqp_handle* handle, wbcqp_graph* graph, void* stream);
int wbcqp_tick_graph_destroy(wbcqp_handle* handle, wbcqp_graph* graph);

int wbcqp_sync(wbcqp_handle* handle, void* stream);

/* Diagnostics: the launch order the next solve of the last launch's shape will use (what the schedule kernels left),
   copied to host memory after a device synchronisation.  Returns the number of entries written (0: no order yet, the next
   launch runs in index order), or a negative wbcqp_error.  *packed (may be NULL): 1 if this is the bin-packed order,
   0 if plain longest-first.  Nothing in the reference corresponds to it; tests compare it with a host model. */
int wbcqp_launch_order(wbcqp_handle* handle, int32_t* order, int32_t capacity, int32_t* packed);

#ifdef __cplusplus
}
#endif
#endif /* WBCQP_H */
