// Batched stand-in for inria_wbc::controllers::Controller (/root/reference/include/inria_wbc/controllers/controller.hpp:46-233,
// /root/reference/src/controllers/controller.cpp:161-313): same method names and tick contract, but every getter
// returns one row per robot instance.  The per-tick hot path -- computeProblemData's assembly + solver_->solve +
// decode (controller.cpp:244-251) -- goes through the C ABI of libwbcqp (include/wbcqp.h) in ONE call for all
// B instances.  What the reference gets from pinocchio and from each task's compute() (the step before the path)
// is supplied by a ProblemSource.
#ifndef IWBC_HIP_CONTROLLER_HPP
#define IWBC_HIP_CONTROLLER_HPP

#include <array>
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include <inria_wbc/controllers/task_stack.hpp>
#include <inria_wbc/exceptions.hpp>
#include <inria_wbc/utils/factory.hpp>
#include <inria_wbc/utils/yaml_lite.hpp>

#include "wbcqp.h"

namespace inria_wbc {
    namespace controllers {

        // dense row-major matrix: [rows = instances][cols]
        struct MatrixXd {
            int rows = 0, cols = 0;
            std::vector<double> data;
            MatrixXd() = default;
            MatrixXd(int r, int c, double v = 0.0) : rows(r), cols(c), data((size_t)r * c, v) {}
            double& operator()(int r, int c) { return data[(size_t)r * cols + c]; }
            double operator()(int r, int c) const { return data[(size_t)r * cols + c]; }
            double* row(int r) { return data.data() + (size_t)r * cols; }
            const double* row(int r) const { return data.data() + (size_t)r * cols; }
        };
        using VectorXi = std::vector<int>;

        // same keys as the reference (controller.cpp:165-187): "positions", "joint_velocities", "floating_base_position", ...
        using SensorData = std::unordered_map<std::string, MatrixXd>;

        struct behavior_types {
            static constexpr const char* FIXED_BASE = "FIXED_BASE";
            static constexpr const char* SINGLE_SUPPORT = "SINGLE_SUPPORT";
            static constexpr const char* DOUBLE_SUPPORT = "DOUBLE_SUPPORT";
        };

        // Per-tick inputs of the path for B instances, laid out exactly as wbcqp_inputs wants them ([B][len], row-major).
        struct TickInputs {
            int batch = 0;
            std::vector<double> M, h, A, b1, Ac, bc, blb, bub, tlb, tub, w, Acop;
            // sizes the arrays for B instances; contents are left alone when nothing changed (every tick overwrites what it uses)
            void resize(int B, const wbcqp_layout& L)
            {
                batch = B;
                auto fit = [B](std::vector<double>& a, int len) {
                    if (a.size() != (size_t)B * len) a.assign((size_t)B * len, 0.0);
                };
                fit(M, L.len_M); fit(h, L.len_h); fit(A, L.len_A); fit(b1, L.len_b1); fit(Ac, L.len_Ac); fit(bc, L.len_bc);
                fit(blb, L.len_blb); fit(bub, L.len_bub); fit(tlb, L.len_tlb); fit(tub, L.len_tub); fit(w, L.len_w); fit(Acop, L.len_Acop);
            }
        };

        // TrajectorySample of tsid: value / first / second derivative
        struct TrajectorySample {
            std::vector<double> pos, vel, acc;
            explicit TrajectorySample(int n = 0) : pos(n, 0.0), vel(n, 0.0), acc(n, 0.0) {}
        };

        // "The step before the path": rigid-body terms and task rows for every instance at time t (pinocchio computeAllTerms +
        // each task's compute() in the reference, controller.cpp:244 upstream half).  Two kinds: FileSource replays rows
        // computed elsewhere and leaves the reference-driven right-hand sides to the controller; ModelSource
        // (model_source.hpp) computes everything on the device from the robot state (wbcqp_problem_data) and therefore
        // owns the task references too.
        // the active stabiliser file (filter_size, com, ankle, ffda) with the controller's dt and the contacts' normal
        struct StabilizerParams {
            int window = 1;
            double dt = 0.001;
            std::array<double, 6> com{}, ankle{};
            std::array<double, 3> ffda{}, normal{{0.0, 0.0, 1.0}};
        };

        class ProblemSource {
        public:
            virtual ~ProblemSource() {}
            virtual int batch() const = 0;
            // fills every array of `in` except the reference-driven parts the controller adds afterwards
            virtual void compute(double t, const MatrixXd& q, const MatrixXd& v, const tasks::TaskStack& stack, const wbcqp_layout& L, TickInputs& in) = 0;
            // current CoM position / velocity per instance (3 columns) for the CoM task's PD law
            virtual void com(MatrixXd& pos, MatrixXd& vel) const = 0;
            // sources that evaluate the task laws themselves
            virtual bool handles_references() const { return false; }
            virtual void bind(wbcqp_handle*, int, const tasks::TaskStack&, double) {}
            virtual void set_com_ref(const TrajectorySample&) {}
            virtual void set_se3_ref(const std::string&, const TrajectorySample&) {}
            virtual void set_posture_ref(const std::vector<double>&) {}
            virtual std::vector<double> get_se3_ref(const std::string&) const { return {}; } // 12 numbers, SE3ToVector order
            virtual void set_contact_se3_ref(const std::string&, const std::vector<double>&) {}  // 12 numbers, or 24 with derivatives
            virtual const double* reference_data() const { return nullptr; }                   // [batch][nref] for wbcqp_tick_host
            virtual void fill_limits(const wbcqp_layout&, TickInputs&) const {}                // constant tlb / tub
            // What a source without a model answers to a question only a model can answer: `who` is the asker with its verb.  The askers that
            // Controller refuses itself as well (before it looks at an argument) are named here, so that each is spelled once
            static constexpr const char *RNEA = "rnea_double_support needs", *INERTIA = "inertia_matrix needs", *FDYN = "forward_dynamics needs",
                                        *SPD = "compute_spd needs", *JACOBIAN = "jacobian needs"; // (the Hessians ask in the Jacobians' name)
            static std::string no_model(const char* who)
            {
                return detail::cat("this problem source has no model: ", who, " a model-driven source (CONTROLLER.model)");
            }
            // where the robots are at the states (q, v): CoM and its velocity (B x 3 each), world placement (B x 12 n: rotation row-major, translation)
            // and local velocity (B x 6 n: linear, angular) of the n named model frames -- wbcqp_observe_host.  Only a source that holds a model can tell
            virtual void observe(const MatrixXd&, const MatrixXd&, const std::vector<std::string>&, MatrixXd&, MatrixXd&, MatrixXd&, MatrixXd&)
            { IWBC_ERROR(no_model("com_now / model_frame_pos / model_frame_vel need")); }
            // tau (B x nv) = M(q) a + nle(q, v) - sum_k J_k' w_k for the n named model frames, wrenches B x 6 n (linear, angular in each frame's own
            // axes; n <= 8) -- wbcqp_inverse_dynamics_host.  Only a source that holds a model can tell
            virtual void inverse_dynamics(const MatrixXd&, const MatrixXd&, const MatrixXd&, const std::vector<std::string>&, const MatrixXd&, MatrixXd&)
            { IWBC_ERROR(no_model(RNEA)); }
            // dtau/dq and dtau/dv of the inverse dynamics at (q, v, a), each B x nv*nv (row-major per instance: [i][j] = d tau_i / d q_j, d tau_i /
            // d v_j; d/dq_j in the tangent space), for the n named model frames and their wrenches as for inverse_dynamics --
            // wbcqp_inverse_dynamics_derivatives_host.  Only a source that holds a model can tell
            virtual void inverse_dynamics_derivatives(const MatrixXd&, const MatrixXd&, const MatrixXd&, const std::vector<std::string>&, const MatrixXd&,
                                                      MatrixXd&, MatrixXd&)
            { IWBC_ERROR(no_model(RNEA)); }
            // M(q), B x nv*nv (row-major per instance, both triangles) -- wbcqp_mass_matrix_host.  Only a source that holds a model can tell
            virtual void mass_matrix(const MatrixXd&, MatrixXd&)
            { IWBC_ERROR(no_model(INERTIA)); }
            // a (B x nv) with (M(q) + diag(damping)) a = tau - nle(q, v) + sum_k J_k' w_k: tau B x nv (all dofs), the n named frames and their
            // wrenches as for inverse_dynamics, damping nv entries or none; info (B): 0, or k + 1 for a pivot that is not > 0 --
            // wbcqp_forward_dynamics_host.  Only a source that holds a model can tell
            virtual void forward_dynamics(const MatrixXd&, const MatrixXd&, const MatrixXd&, const std::vector<std::string>&, const MatrixXd&,
                                          const std::vector<double>&, MatrixXd&, VectorXi&)
            { IWBC_ERROR(no_model(FDYN)); }
            // the reference's compute_spd (robot_dart/cmd.hpp:10-38) for every instance: commands B x nv from q, dq, the targets of the actuated
            // joints (the last na columns of targetpos), dt, kp, kd -- wbcqp_spd_commands_host.  Only a source that holds a model can tell
            virtual void spd_commands(const MatrixXd&, const MatrixXd&, const MatrixXd&, double, double, double, MatrixXd&)
            { IWBC_ERROR(no_model(SPD)); }
            // Frame Jacobians, the CoM Jacobian and the centroidal momentum matrix at the states q -- wbcqp_jacobians_host.  J (null: not asked for):
            // B x n*6*nv for the n named frames in the convention reference_frame (pinocchio's values: 0 WORLD, 1 LOCAL, 2 LOCAL_WORLD_ALIGNED),
            // each frame's 6 x nv block row-major; Jcom: B x 3*nv; Ag: B x 6*nv.  Only a source that holds a model can tell
            virtual void jacobians(const MatrixXd&, const std::vector<std::string>&, int, MatrixXd*, MatrixXd&, MatrixXd&)
            { IWBC_ERROR(no_model(JACOBIAN)); }
            // The kinematic Hessians dJ/dq and the Jacobians' time variation at the states q (and v, for dJ) -- wbcqp_kinematic_hessians_host.  H (null:
            // not asked for): B x n*6*nv*nv for the n named frames in the convention reference_frame, each frame's [6][nv][nv] block as it is; dJ
            // (null: not asked for; needs v): B x n*6*nv.  Only a source that holds a model can tell
            virtual void hessians(const MatrixXd&, const MatrixXd*, const std::vector<std::string>&, int, MatrixXd*, MatrixXd*)
            { IWBC_ERROR(no_model(JACOBIAN)); }
            // the foot's own mass added to a measured wrench (robot_model.cpp:171-186 of the reference), per instance, at the states q: force -= m g
            // with m the mass of the body that carries ft_frame, torque += (ankle - sole) x force with the world positions of that body's joint
            // frame and of sole_frame.  Only a source that holds a model can tell
            virtual void add_foot_mass(const MatrixXd&, const std::string&, const std::string&, MatrixXd&, MatrixXd&) const
            { IWBC_ERROR(no_model(RNEA)); }
            // One tick of the stabiliser (wbcqp_stabilize_host) on the source's stored references: com, acom and the two ankle frames are observed at
            // (q, v); wrench is B x 12 (lf_force, lf_torque, rf_force, rf_torque); feet_forces_prev: B x 24, the previous solution's point forces of
            // contact_lfoot then contact_rfoot, or null.  state: [B][wbcqp_stabilizer_state_bytes] bytes, sized and zeroed here when it does not fit.
            // ref_out [B][nref] is what the tick reads instead of the stored references, which are not touched.  Only a source with a model can
            virtual void stabilize(const StabilizerParams&, const MatrixXd&, const MatrixXd&, const MatrixXd&, const double*, std::vector<unsigned char>&,
                                   std::vector<double>&, VectorXi&, MatrixXd&)
            { IWBC_ERROR(no_model("the stabilizer needs")); }
            // whether the source holds a kinematic model (what observe() and check_collisions() need)
            virtual bool has_model() const { return false; }
            // self-collision of the sphere model in the collision file `file` (the reference's members: {member: {link: [[x, y, z, d], ...]}}) at
            // the states q: colliding (B: 1 / 0), first_pair (2 B: table indices of the pair the reference's loops meet first, -1 -1 without a hit)
            // and, per table entry, its (member, place inside the member) -- wbcqp_check_collisions_host.  Only a source that holds a model can tell
            virtual void check_collisions(const MatrixXd&, const std::string&, VectorXi&, VectorXi&, std::vector<std::pair<std::string, int>>&)
            { IWBC_ERROR(no_model("check_model_collisions needs")); }
        };

        // "computed at this (source, q, v)": an answer a controller keeps WITH the state and the source it was made for, so whatever moves the
        // state or replaces the source makes the next question fetch again (v null: the answer does not depend on it)
        struct ComputedAt {
            const ProblemSource* source = nullptr; // null: nothing kept
            MatrixXd q, v;
            bool current(const ProblemSource* s, const MatrixXd& qn, const MatrixXd* vn) const
            {
                return source && source == s && q.rows == qn.rows && q.data == qn.data && (!vn || v.data == vn->data);
            }
            void set(const ProblemSource* s, const MatrixXd& qn, const MatrixXd* vn) { source = s; q = qn; if (vn) v = *vn; }
        };

        // The model frames a controller has been asked about so far, in the order they joined: what goes to the source with every fetch
        struct FrameSelection {
            std::vector<std::string> names;
            // fetch(joined) runs with `frame` in the selection -- joined: it was asked for the first time and has just been appended -- and a
            // frame whose fetch throws (the model does not have it) does not stay.  Returns the frame's place
            template <typename Fetch>
            int with(const std::string& frame, Fetch&& fetch)
            {
                const int at = (int)std::distance(names.begin(), std::find(names.begin(), names.end(), frame));
                const bool joined = at == (int)names.size();
                if (joined) names.push_back(frame);
                try {
                    fetch(joined);
                }
                catch (...) {
                    if (joined) names.pop_back();
                    throw;
                }
                return at;
            }
        };

        class Controller {
        public:
            explicit Controller(const yaml::Node& config)
            {
                yaml::Node c = IWBC_CHECK(config["CONTROLLER"]);
                base_path_ = c["base_path"] ? c["base_path"].as<std::string>() : std::string(".");
                dt_ = IWBC_CHECK(c["dt"].as<double>());
                floating_base_ = IWBC_CHECK(c["floating_base"].as<bool>());
                verbose_ = c["verbose"] ? c["verbose"].as<bool>() : false;
                // controller.cpp:63,72 (the reference requires both keys; here they default to what a model without mimic joints has)
                fb_joint_name_ = c["floating_base_joint_name"] ? c["floating_base_joint_name"].as<std::string>() : std::string("root_joint");
                if (c["mimic_dof_names"]) mimic_dof_names_ = c["mimic_dof_names"].as<std::vector<std::string>>();
                // check collisions in the solver's own model (controller.cpp:89-99; the reference requires the key, here absent means false)
                check_model_collisions_ = c["check_model_collisions"] ? c["check_model_collisions"].as<bool>() : false;
                if (check_model_collisions_) {
                    auto collision_path = IWBC_CHECK(c["collision_path"].as<std::string>());
                    collision_file_ = collision_path.size() && collision_path[0] == '/' ? collision_path : base_path_ + "/" + collision_path;
                }
                t_ = 0.0;
            }
            Controller(const Controller&) = delete;
            Controller& operator=(const Controller&) = delete;
            virtual ~Controller()
            {
                if (handle_) wbcqp_destroy(handle_);
            }

            const std::string& base_path() const { return base_path_; }
            // Controller::update (controller.cpp:161-205): open loop integrates the controller's own state; closed loop REQUIRES
            // the sensor keys the reference requires and builds q = [floating_base_position, positions],
            // dq = [floating_base_velocity, joint_velocities] per instance (one row per instance instead of one vector)
            virtual void update(const SensorData& sensor_data = {})
            {
                if (!closed_loop_) {
                    _solve();
                    return;
                }
                auto qi = sensor_data.find("positions"), vi = sensor_data.find("joint_velocities");
                IWBC_ASSERT(qi != sensor_data.end(), "we need the joint positions in closed loop mode!");
                IWBC_ASSERT(vi != sensor_data.end(), "we need the joint velocities in closed loop mode!");
                const MatrixXd &pos = qi->second, &vel = vi->second;
                IWBC_ASSERT(pos.rows == batch_ && vel.rows == batch_, "closed loop: one sensor row per instance (", batch_, ")");
                if (!floating_base_) {
                    IWBC_ASSERT(vel.cols == v_tsid_.cols, "Joint velocities do not have the correct size:", vel.cols, " vs (expected)", v_tsid_.cols);
                    IWBC_ASSERT(pos.cols == q_tsid_.cols, "Joint positions do not have the correct size:", pos.cols, " vs (expected)", q_tsid_.cols);
                    _solve(pos, vel);
                    return;
                }
                auto fqi = sensor_data.find("floating_base_position"), fvi = sensor_data.find("floating_base_velocity");
                IWBC_ASSERT(fqi != sensor_data.end(), "we need the floating base position in closed loop mode!");
                IWBC_ASSERT(fvi != sensor_data.end(), "we need the floating base velocity in closed loop mode!");
                const MatrixXd &fb_pos = fqi->second, &fb_vel = fvi->second;
                IWBC_ASSERT(fb_pos.rows == batch_ && fb_vel.rows == batch_, "closed loop: one floating-base row per instance (", batch_, ")");
                IWBC_ASSERT(vel.cols + fb_vel.cols == v_tsid_.cols, "Joint velocities do not have the correct size:", vel.cols + fb_vel.cols,
                            " vs (expected)", v_tsid_.cols);
                IWBC_ASSERT(pos.cols + fb_pos.cols == q_tsid_.cols, "Joint positions do not have the correct size:", pos.cols + fb_pos.cols,
                            " vs (expected)", q_tsid_.cols);
                MatrixXd q(batch_, q_tsid_.cols), dq(batch_, v_tsid_.cols);
                for (int i = 0; i < batch_; ++i) {
                    std::copy(fb_pos.row(i), fb_pos.row(i) + fb_pos.cols, q.row(i));
                    std::copy(pos.row(i), pos.row(i) + pos.cols, q.row(i) + fb_pos.cols);
                    std::copy(fb_vel.row(i), fb_vel.row(i) + fb_vel.cols, dq.row(i));
                    std::copy(vel.row(i), vel.row(i) + vel.cols, dq.row(i) + fb_vel.cols);
                }
                _solve(q, dq);
            }

            int batch_size() const { return batch_; }
            double t() const { return t_; }
            double dt() const { return dt_; }
            bool verbose() const { return verbose_; }
            void set_verbose(bool b) { verbose_ = b; }
            virtual void set_behavior_type(const std::string& bt) { behavior_type_ = bt; }
            const std::string& behavior_type() const { return behavior_type_; }

            // one row per instance (the reference returns one Eigen::VectorXd), in the reference's "DART" format
            // (controller.cpp:262-281): ndofs = nv entries; a floating base is [position(3), angle * axis(3)] in q and six
            // leading zeros in tau.  filter_mimics (default true, as in the reference, controller.cpp:369-397) drops the columns of
            // the joints named in CONTROLLER.mimic_dof_names: slice_vec(x, non_mimic_indexes_) per instance.
            // With check_model_collisions these four are the COMMANDS: the rows of an instance whose model has collided stay at the last values
            // sent, while q_solver() and q_tsid() keep following the solver (controller.cpp:263-282); without it they are the solver's state.
            MatrixXd tau(bool filter_mimics = true) const { return _cmd(_latched() ? tau_sent_ : tau_dart_, filter_mimics); }
            MatrixXd ddq(bool filter_mimics = true) const { return _cmd(_latched() ? ddq_sent_ : a_tsid_, filter_mimics); }
            MatrixXd dq(bool filter_mimics = true) const { return _cmd(_latched() ? dq_sent_ : v_tsid_, filter_mimics); }
            MatrixXd q(bool filter_mimics = true) const { return _cmd(_latched() ? q_sent_ : q_solver_, filter_mimics); }
            MatrixXd q_solver(bool filter_mimics = true) const { return filter_mimics ? filter_cmd(q_solver_) : q_solver_; }
            // controller.cpp:245: momentum_ = momentumJacobian(data).bottomRows(3) * dq -- the angular momentum about the CoM of the
            // state the last tick was solved at, one row per instance (zero until a tick has run on a model-driven source)
            const MatrixXd& momentum() const { return momentum_; }
            // controller.hpp:60-64,114-115 of the reference
            const std::vector<std::string>& mimic_names() const { return mimic_dof_names_; }
            const std::vector<int>& non_mimic_indexes() const { return non_mimic_indexes_; }
            MatrixXd filter_cmd(const MatrixXd& cmd) const
            {
                if (non_mimic_indexes_.empty() || (int)non_mimic_indexes_.size() == cmd.cols) return cmd;
                MatrixXd out(cmd.rows, (int)non_mimic_indexes_.size());
                for (int i = 0; i < cmd.rows; ++i)
                    for (size_t j = 0; j < non_mimic_indexes_.size(); ++j) out(i, (int)j) = cmd(i, non_mimic_indexes_[j]);
                return out;
            }
            // Removes the universe and root (floating base) joint names (controller.cpp:316-331)
            std::vector<std::string> controllable_dofs(bool filter_mimics = true) const
            {
                std::vector<std::string> out;
                for (const auto& n : joint_names_)
                    if (!filter_mimics || std::find(mimic_dof_names_.begin(), mimic_dof_names_.end(), n) == mimic_dof_names_.end()) out.push_back(n);
                return out;
            }
            // Order of the floating base in q_ according to dart naming convention (controller.cpp:333-363)
            std::vector<std::string> floating_base_dofs() const
            {
                if (!floating_base_) return {};
                const std::string b = (fb_joint_name_ == "root_joint") ? std::string("rootJoint") : fb_joint_name_;
                return {b + "_pos_x", b + "_pos_y", b + "_pos_z", b + "_rot_x", b + "_rot_y", b + "_rot_z"};
            }
            std::vector<std::string> all_dofs(bool filter_mimics = true) const
            {
                std::vector<std::string> all = floating_base_dofs(), ctl = controllable_dofs(filter_mimics);
                all.insert(all.end(), ctl.begin(), ctl.end());
                return all;
            }
            // controller.cpp:445-450 / controller.hpp:170-171: back to the state the last tick started from (the reference also
            // restores pinocchio's data; here every tick recomputes the rigid-body terms from (q, dq) on the device)
            void qp_step_back(const MatrixXd& q, const MatrixXd& dq)
            {
                IWBC_ASSERT(q.rows == batch_ && dq.rows == batch_ && q.cols == q_tsid_.cols && dq.cols == v_tsid_.cols, "qp_step_back: wrong size");
                q_tsid_ = q;
                v_tsid_ = dq;
            }
            void qp_step_back()
            {
                if (q_tsid_prev_.rows == batch_ && batch_ > 0) qp_step_back(q_tsid_prev_, v_tsid_prev_);
            }
            // tsid's own forms: q with the base quaternion (nq = nv + 1 entries), tau of the actuated joints only (na entries)
            const MatrixXd& q_tsid() const { return q_tsid_; }
            const MatrixXd& tau_tsid() const { return tau_; }
            const std::vector<std::string>& activated_contacts() const { return activated_contacts_; }
            // 12 force components per activated contact and instance (tsid getContactForces, controller.cpp:258-261)
            const std::unordered_map<std::string, MatrixXd>& activated_contacts_forces() const { return activated_contacts_forces_; }
            const VectorXi& qp_status() const { return status_; }
            const VectorXi& qp_iterations() const { return iters_; }
            virtual double cost(const std::string& task_name) const = 0;

            // the CoM as the problem source reports it (a model-driven source: the CoM at q0, filled once; com_now() below is the live one)
            void com(MatrixXd& pos, MatrixXd& vel) const
            {
                _source().com(pos, vel);
            }
            // Where the robots are NOW -- at the controller's current state (q_tsid(), dq(): after the last tick's integration), computed on the
            // device by wbcqp_observe_host when somebody asks and kept until the next tick: the batched counterparts of the reference's com() and
            // model_frame_pos(name) (controller.hpp:110,141-146).  com() of this facade keeps returning the CoM at q0.
            void com_now(MatrixXd& pos, MatrixXd& vel) const
            {
                _ensure_observed(nullptr);
                pos = obs_com_;
                vel = obs_vcom_;
            }
            // B x 12: rotation row-major (9), translation (3) of the model frame in the world (pinocchio's oMf)
            MatrixXd model_frame_pos(const std::string& frame) const { return _observed_block(obs_place_, _ensure_observed(&frame), 12); }
            // B x 6: linear (3), angular (3) velocity of the frame in its own axes (tsid RobotWrapper::frameVelocity)
            MatrixXd model_frame_vel(const std::string& frame) const { return _observed_block(obs_vel_, _ensure_observed(&frame), 6); }

            // The model-side torques of the current motion under measured foot wrenches, B x nv (a floating base's six rows first): the reference's
            // RobotModel::compute_rnea_double_support (robot_model.cpp:138-229), per instance, for the controller's current q_tsid(), dq(false) and
            // the last tick's ddq -- rnea(q, v, a) - J_left' w_left - J_right' w_right with the LOCAL Jacobians of the two frames, computed on the
            // device (wbcqp_inverse_dynamics_host).  sensor_data holds lf_force, rf_force, lf_torque, rf_torque: B x 3 each, or three numbers
            // for every instance alike.  add_foot_mass: the wrench is first corrected by the foot's own weight and applied at the sole frame.
            MatrixXd rnea_double_support(const SensorData& sensor_data, bool add_foot_mass, const std::string& left_ft_frame, const std::string& right_ft_frame,
                                         const std::string& left_sole_frame, const std::string& right_sole_frame) const
            {
                ProblemSource& source = _model_source(ProblemSource::RNEA);
                if ((sensor_data.find("lf_force") == sensor_data.end()) || (sensor_data.find("rf_force") == sensor_data.end()) ||
                    (sensor_data.find("lf_torque") == sensor_data.end()) || (sensor_data.find("rf_torque") == sensor_data.end()))
                    throw IWBC_EXCEPTION("when FT is missing in fext_map"); // robot_model.cpp:161-163
                const int B = batch_, nv = v_tsid_.cols;
                auto per_instance = [&](const std::string& key) {
                    const MatrixXd& m = sensor_data.at(key);
                    IWBC_ASSERT((m.rows == B && m.cols == 3) || m.data.size() == 3, key, " holds three numbers, or B x 3");
                    MatrixXd o(B, 3);
                    for (int i = 0; i < B; ++i)
                        for (int d = 0; d < 3; ++d) o(i, d) = m.data.size() == 3 ? m.data[d] : m(i, d);
                    return o;
                };
                MatrixXd force[2] = {per_instance("lf_force"), per_instance("rf_force")}, torque[2] = {per_instance("lf_torque"), per_instance("rf_torque")};
                std::vector<std::string> frames = {left_ft_frame, right_ft_frame};
                if (add_foot_mass) {
                    source.add_foot_mass(q_tsid_, left_ft_frame, left_sole_frame, force[0], torque[0]);
                    source.add_foot_mass(q_tsid_, right_ft_frame, right_sole_frame, force[1], torque[1]);
                    frames = {left_sole_frame, right_sole_frame};
                }
                MatrixXd w(B, 12), a(B, nv), tau;
                for (int i = 0; i < B; ++i)
                    for (int k = 0; k < 2; ++k)
                        for (int d = 0; d < 3; ++d) {
                            w(i, 6 * k + d) = force[k](i, d);
                            w(i, 6 * k + 3 + d) = torque[k](i, d);
                        }
                if (a_tsid_.rows == B && a_tsid_.cols == nv) a = a_tsid_; // (before the first tick: no acceleration yet)
                source.inverse_dynamics(q_tsid_, v_tsid_, a, frames, w, tau);
                return tau;
            }

            // The reference's RobotModel::inertia_matrix() (utils/robot_model.hpp:41) for every instance: M(q_tsid()), B x nv*nv (instance i's
            // matrix row-major in row i, both triangles), computed on the device (wbcqp_mass_matrix_host) when somebody asks and kept with the
            // state like com_now(): a tick, qp_step_back() or a new problem source makes the next call fetch again.
            const MatrixXd& inertia_matrix() const
            {
                ProblemSource& source = _model_source(ProblemSource::INERTIA);
                _keep(mass_at_, nullptr, [&] { source.mass_matrix(q_tsid_, mass_); });
                return mass_;
            }
            // The accelerations joint torques produce at the controller's current q_tsid(), dq(false): tau B x nv (all dofs; a floating base's six
            // first), no wrenches, no damping -- wbcqp_forward_dynamics_host.  info (B): 0, or k + 1 where the k-th pivot was not > 0.
            MatrixXd forward_dynamics(const MatrixXd& tau, VectorXi* info = nullptr) const
            {
                MatrixXd a;
                VectorXi flags;
                _model_source(ProblemSource::FDYN).forward_dynamics(q_tsid_, v_tsid_, tau, {}, MatrixXd(), {}, a, flags);
                if (info) *info = flags;
                return a;
            }
            // The linearisation of the inverse dynamics tau = M(q) a + nle(q, v) (pinocchio's computeRNEADerivatives) for every instance at the
            // controller's current q_tsid(), dq(false) and the accelerations a (B x nv, or wider: the first nv columns), no wrenches: dtau_dq and
            // dtau_dv, each B x nv*nv with instance i's matrix row-major in row i ([r][c] = d tau_r / d q_c along dof c in the tangent space,
            // d tau_r / d v_c); d tau / d a is inertia_matrix().  Computed on the device (wbcqp_inverse_dynamics_derivatives_host) when somebody
            // asks and kept with the state and with `a` like inertia_matrix(): the same question again costs no second call.
            struct IdDerivatives {
                MatrixXd dtau_dq, dtau_dv;
            };
            const IdDerivatives& inverse_dynamics_derivatives(const MatrixXd& a) const
            {
                ProblemSource& source = _model_source(ProblemSource::RNEA);
                if (idd_a_.rows != a.rows || idd_a_.data != a.data) idd_at_ = ComputedAt{}; // (another a: another answer)
                _keep(idd_at_, &v_tsid_, [&] {
                    source.inverse_dynamics_derivatives(q_tsid_, v_tsid_, a, {}, MatrixXd(), idd_.dtau_dq, idd_.dtau_dv);
                    idd_a_ = a;
                });
                return idd_;
            }
            // compute_spd of inria_wbc/robots/cmd.hpp goes through here: the states are the caller's (a simulator's), not the controller's
            MatrixXd spd_commands(const MatrixXd& q, const MatrixXd& dq, const MatrixXd& targetpos, double dt, double kp, double kd) const
            {
                MatrixXd commands;
                _model_source(ProblemSource::SPD).spd_commands(q, dq, targetpos, dt, kp, kd, commands);
                return commands;
            }

            // The reference's RobotModel::jacobian(name, reference_frame), jacobianCenterOfMass and the momentumJacobian its controller reads
            // (src/utils/robot_model.cpp:92-98, 115-126; controller.cpp:245) for every instance at q_tsid(): B x 6*nv, B x 3*nv and B x 6*nv
            // (instance i's matrix row-major in row i; rows linear then angular, a floating base's six columns in the base's own axes; Ag's
            // angular rows about the CoM), computed on the device (wbcqp_jacobians_host) when somebody asks and kept with the state like
            // inertia_matrix().  A frame asked for the first time joins the selection and costs one more call.
            enum ReferenceFrame { WORLD = 0, LOCAL = 1, LOCAL_WORLD_ALIGNED = 2 }; // pinocchio's values
            MatrixXd jacobian(const std::string& frame, ReferenceFrame rf = WORLD) const
            {
                const int at = _ensure_jacobians(&frame, rf);
                return _observed_block(jac_J_[rf], at, 6 * v_tsid_.cols);
            }
            const MatrixXd& jacobian_com() const
            {
                _ensure_jacobians(nullptr, LOCAL);
                return jac_com_;
            }
            const MatrixXd& momentum_matrix() const
            {
                _ensure_jacobians(nullptr, LOCAL);
                return jac_ag_;
            }

            // The reference's RobotModel::hessian(name, reference_frame) (src/utils/robot_model.cpp:128-135: pinocchio's getJointKinematicHessian)
            // and the Jacobian's time variation (getFrameJacobianTimeVariation) for every instance at q_tsid() and the velocity beside it (dq(false) of an instance that is not latched): B x 6*nv*nv with
            // instance i's tensor in row i as [6][nv][nv] (H[r][j][k] = d J[r][j] / d q_k, k fastest), and B x 6*nv with sum_k H[r][j][k] v_k
            // row-major in row i.  Computed on the device (wbcqp_kinematic_hessians_host) when somebody asks and kept with the state like
            // jacobian(); the frames are jacobian()'s selection, and a frame asked for the first time joins it.
            MatrixXd hessian(const std::string& frame, ReferenceFrame rf = WORLD) const
            {
                const int at = _ensure_hessians(frame, rf, false);
                return _observed_block(hes_H_[rf], at, 6 * v_tsid_.cols * v_tsid_.cols);
            }
            MatrixXd jacobian_time_variation(const std::string& frame, ReferenceFrame rf = WORLD) const
            {
                const int at = _ensure_hessians(frame, rf, true);
                return _observed_block(hes_dJ_[rf], at, 6 * v_tsid_.cols);
            }

            // The reference's self-collision check of the solver's own model (CONTROLLER.check_model_collisions, collision_path;
            // controller.hpp:148-150, collision_check.cpp), per instance, for the controller's CURRENT state: computed on the device
            // (wbcqp_check_collisions_host) and kept with the state like the observables above, so a tick or qp_step_back() refreshes it.
            // Without check_model_collisions nothing collides.
            bool check_model_collisions() const { return check_model_collisions_; }
            const VectorXi& is_model_colliding() const
            {
                _ensure_collisions();
                return col_flags_;
            }
            // ((member, i), (member, j)) of the pair the reference's loops meet first; two empty names and -1 for an instance without a hit
            using CollisionIndex = std::pair<std::pair<std::string, int>, std::pair<std::string, int>>;
            std::vector<CollisionIndex> collision_index() const
            {
                _ensure_collisions();
                std::vector<CollisionIndex> out(col_flags_.size(), CollisionIndex{{std::string(), -1}, {std::string(), -1}});
                for (size_t i = 0; i < out.size(); ++i)
                    if (col_flags_[i]) out[i] = {col_names_[col_pairs_[2 * i]], col_names_[col_pairs_[2 * i + 1]]};
                return out;
            }
            // 1 while an instance's commands are sent, 0 once its model has collided (the reference's send_cmd_); all 1 without the check
            std::vector<int> send_cmd() const { return send_cmd_.empty() ? std::vector<int>(batch_, 1) : send_cmd_; }

            void set_problem_source(const std::shared_ptr<ProblemSource>& src)
            {
                IWBC_ASSERT(src, "Invalid problem source");
                if (check_model_collisions_ && !src->has_model())
                    IWBC_ERROR("check_model_collisions is set, but ", ProblemSource::no_model("the check needs"));
                send_cmd_.clear();
                col_at_ = ComputedAt{};
                source_ = src;
                batch_ = src->batch();
                _reset();
            }

        protected:
            virtual void _reset() {}
            // builds this tick's inputs (source + references) -- implemented by PosTracker
            virtual void _build_inputs(const MatrixXd& q, const MatrixXd& v) = 0;
            virtual const tasks::TaskStack& _stack() const = 0;
            virtual int _slot() const = 0;
            virtual const wbcqp_layout& _layout() const = 0;

            void _solve() { _solve(MatrixXd(q_tsid_), MatrixXd(v_tsid_)); }

            // tsid_joint_names_ = all_dofs(false), non_mimic_indexes_ = get_non_mimics_indexes() (controller.cpp:157-158,208-229):
            // called by the derived controller once the model's joint names are known (without a model: no names, no mimic joints)
            void _set_joint_names(const std::vector<std::string>& actuated_joint_names)
            {
                joint_names_ = actuated_joint_names;
                const std::vector<std::string> tsid_joint_names = all_dofs(false);
                std::vector<int> mimic_indexes;
                for (const auto& m : mimic_dof_names_) {
                    auto it = std::find(tsid_joint_names.begin(), tsid_joint_names.end(), m);
                    IWBC_ASSERT(it != tsid_joint_names.end(), " joint ", m, " not found");
                    mimic_indexes.push_back((int)std::distance(tsid_joint_names.begin(), it));
                }
                non_mimic_indexes_.clear();
                for (int i = 0; i < (int)tsid_joint_names.size(); ++i)
                    if (std::find(mimic_indexes.begin(), mimic_indexes.end(), i) == mimic_indexes.end()) non_mimic_indexes_.push_back(i);
            }

            // Controller::_solve (controller.cpp:231-313) for B instances
            void _solve(const MatrixXd& q, const MatrixXd& dq)
            {
                IWBC_ASSERT(handle_, "no solver: the controller was not fully constructed");
                IWBC_ASSERT(source_, "no problem source set (set_problem_source)");
                const tasks::TaskStack& st = _stack();
                const wbcqp_layout& L = _layout();
                _build_inputs(q, dq);
                const int B = batch_, n = L.n, na = st.na(), nv = st.nv();
                x_.assign((size_t)B * n, 0.0);
                tau_ = MatrixXd(B, na);
                status_.assign(B, WBCQP_HQP_UNKNOWN);
                iters_.assign(B, 0);
                objective_.assign(B, 0.0);
                wbcqp_inputs in = {in_.M.data(), in_.h.data(), in_.A.data(), in_.b1.data(), in_.Ac.data(), in_.bc.data(),
                                   in_.blb.data(), in_.bub.data(), in_.tlb.data(), in_.tub.data(), in_.w.data(), in_.Acop.data()};
                wbcqp_outputs out = {x_.data(), tau_.data.data(), status_.data(), iters_.data(), objective_.data(), nullptr};
                IWBC_ASSERT(q.cols == (floating_base_ ? nv + 1 : nv), "q must hold ", floating_base_ ? nv + 1 : nv, " entries per instance");
                q_tsid_prev_ = q; // controller.cpp:237-241 (the reference keeps them when send_cmd_ is set; qp_step_back() returns here)
                v_tsid_prev_ = dq;
                momentum_ = MatrixXd(B, 3);
                std::vector<double> mom6((size_t)B * 6, 0.0);
                MatrixXd vnew(B, nv);
                MatrixXd qnew(B, q.cols);
                MatrixXd qsol(B, nv);
                const bool whole_tick = source_->handles_references();
                if (whole_tick) {
                    // rows, QP and integration in one trip to the device: only the state and the references go up, the solution
                    // and the integrated state come back.  The rows stay on the device; cost() fetches them when somebody asks.
                    wbcqp_tick_io io{};
                    io.state = {q.data.data(), dq.data.data(), tick_references_ ? tick_references_ : source_->reference_data(), mom6.data()};
                    io.rows = in;
                    io.rows.M = io.rows.h = io.rows.A = io.rows.b1 = io.rows.Ac = io.rows.bc = io.rows.blb = io.rows.bub = io.rows.Acop = nullptr;
                    last_q_ = q;
                    last_v_ = dq;
                    rows_valid_ = false;
                    io.out = out;
                    io.q_next = qnew.data.data();
                    io.v_next = vnew.data.data();
                    io.q_solver = qsol.data.data();
                    io.dt = dt_;
                    if (wbcqp_tick_host(handle_, _slot(), B, &io) != WBCQP_OK) IWBC_ERROR("wbcqp_tick_host failed: ", wbcqp_last_error(handle_));
                    for (int i = 0; i < B; ++i)
                        for (int k = 0; k < 3; ++k) momentum_(i, k) = mom6[(size_t)i * 6 + 3 + k];
                }
                else {
                    int rc = wbcqp_solve_batch_host(handle_, _slot(), B, &in, &out);
                    if (rc != WBCQP_OK) IWBC_ERROR("wbcqp_solve_batch_host failed: ", wbcqp_last_error(handle_));
                    rows_valid_ = true;
                }
                for (int i = 0; i < B; ++i) {
                    if (status_[i] != WBCQP_HQP_OPTIMAL) {
                        // same text as controller.cpp:285-307, with the instance appended
                        std::string error = "Controller failed, can't solve problem. ";
                        error += "Status : " + std::to_string(status_[i]);
                        switch (status_[i]) {
                        case -1: error += " => Unknown"; break;
                        case 1: error += " => Infeasible "; break;
                        case 2: error += " => Unbounded "; break;
                        case 3: error += " => Max iter reached "; break;
                        case 4: error += " => Error "; break;
                        default: error += " => Uknown status";
                        }
                        error += " (t=" + std::to_string(t_) + ")";
                        error += " [instance " + std::to_string(i) + "]";
                        throw IWBC_EXCEPTION(error);
                    }
                }
                // a_tsid = dv ; v_tsid = dq + dt dv ; q = integrate(q, dt v)  (controller.cpp:250-256): on the device
                a_tsid_ = MatrixXd(B, nv);
                for (int i = 0; i < B; ++i)
                    for (int j = 0; j < nv; ++j) a_tsid_(i, j) = x_[(size_t)i * n + j];
                if (!whole_tick &&
                    wbcqp_integrate_host(handle_, B, nv, floating_base_ ? 1 : 0, dt_, q.data.data(), dq.data.data(), x_.data(), n,
                                         status_.data(), qnew.data.data(), vnew.data.data(), qsol.data.data()) != WBCQP_OK)
                    IWBC_ERROR(wbcqp_last_error(handle_));
                v_tsid_ = vnew;
                q_tsid_ = qnew;
                q_solver_ = qsol;
                // tau_ << 0, 0, 0, 0, 0, 0, tau_tsid_ for a floating base (controller.cpp:269); tau_tsid_ itself otherwise
                tau_dart_ = MatrixXd(B, nv);
                for (int i = 0; i < B; ++i)
                    for (int j = 0; j < na; ++j) tau_dart_(i, nv - na + j) = tau_(i, j);
                t_ += dt_;
                activated_contacts_forces_.clear();
                for (size_t c = 0; c < st.contacts().size(); ++c) {
                    MatrixXd f(B, 12);
                    for (int i = 0; i < B; ++i)
                        for (int m = 0; m < 12; ++m) f(i, m) = x_[(size_t)i * n + nv + 12 * c + m];
                    activated_contacts_forces_[st.contacts()[c].name] = f;
                }
                if (check_model_collisions_) _latch();
            }

            // controller.cpp:263-282,309-312 per instance: the commands follow the solver while send_cmd_ holds; then the new state is checked, and
            // an instance that collides while its q_ is not all zero (within 1e-3, Eigen's isZero) stops sending from the next tick on
            void _latch()
            {
                const int B = batch_;
                if ((int)send_cmd_.size() != B) {
                    send_cmd_.assign(B, 1);
                    q_sent_ = MatrixXd(B, q_solver_.cols);
                    dq_sent_ = MatrixXd(B, v_tsid_.cols);
                    ddq_sent_ = MatrixXd(B, a_tsid_.cols);
                    tau_sent_ = MatrixXd(B, tau_dart_.cols);
                }
                for (int i = 0; i < B; ++i) {
                    if (!send_cmd_[i]) continue;
                    std::copy(q_solver_.row(i), q_solver_.row(i) + q_solver_.cols, q_sent_.row(i));
                    std::copy(v_tsid_.row(i), v_tsid_.row(i) + v_tsid_.cols, dq_sent_.row(i));
                    std::copy(a_tsid_.row(i), a_tsid_.row(i) + a_tsid_.cols, ddq_sent_.row(i));
                    std::copy(tau_dart_.row(i), tau_dart_.row(i) + tau_dart_.cols, tau_sent_.row(i));
                }
                _ensure_collisions();
                for (int i = 0; i < B; ++i) {
                    if (!col_flags_[i]) continue;
                    bool zero = true;
                    for (int j = 0; j < q_sent_.cols; ++j) zero = zero && std::fabs(q_sent_(i, j)) <= 1e-3;
                    if (!zero) send_cmd_[i] = 0;
                }
            }
            MatrixXd _cmd(const MatrixXd& m, bool filter_mimics) const { return filter_mimics ? filter_cmd(m) : m; }
            bool _latched() const { return check_model_collisions_ && !send_cmd_.empty(); } // (before the first tick: the solver's state, as without the check)

            // the source, or the words for there being none; with `who` asking (ProblemSource::no_model): a source that holds a model
            ProblemSource& _source() const
            {
                IWBC_ASSERT(source_, "no problem source set (set_problem_source)");
                return *source_;
            }
            ProblemSource& _model_source(const char* who) const
            {
                if (!_source().has_model()) IWBC_ERROR(ProblemSource::no_model(who));
                return *source_;
            }
            // The rule of ComputedAt, once: an answer that is not current for (source_, q_tsid_, v) is fetched and marked.  The mark is cleared
            // before the fetch, so a fetch that throws leaves nothing kept.  What is kept this way is mutable: the accessors that ask are const
            template <typename Fetch>
            void _keep(ComputedAt& kept, const MatrixXd* v, Fetch&& fetch) const
            {
                if (kept.current(source_.get(), q_tsid_, v)) return;
                kept = ComputedAt{};
                fetch();
                kept.set(source_.get(), q_tsid_, v);
            }

            // the collision answer of the current state
            void _ensure_collisions() const
            {
                if (!check_model_collisions_) {
                    col_flags_.assign(batch_, 0);
                    return;
                }
                ProblemSource& source = _source();
                _keep(col_at_, nullptr, [&] { source.check_collisions(q_tsid_, collision_file_, col_flags_, col_pairs_, col_names_); });
            }
            bool check_model_collisions_ = false;
            std::string collision_file_;
            std::vector<int> send_cmd_; // per instance; empty until the first tick with the check on
            MatrixXd q_sent_, dq_sent_, ddq_sent_, tau_sent_;
            mutable VectorXi col_flags_, col_pairs_;
            mutable std::vector<std::pair<std::string, int>> col_names_;
            mutable ComputedAt col_at_; // the state (q alone) and the source the answer above was made for

            bool verbose_ = false;
            double t_ = 0.0, dt_ = 0.001;
            bool floating_base_ = true;
            bool closed_loop_ = false;
            int solver_max_iter_ = 1000; // eiquadprog-fast DEFAULT_MAX_ITER
            std::string base_path_, behavior_type_, solver_to_use_;
            int batch_ = 0;

            MatrixXd q_tsid_, v_tsid_, a_tsid_, tau_, tau_dart_, q_solver_, momentum_, q_tsid_prev_, v_tsid_prev_;
            std::string fb_joint_name_;
            std::vector<std::string> mimic_dof_names_, joint_names_; // joint_names_: the 1-dof joints in model order (no universe, no root)
            std::vector<int> non_mimic_indexes_;
            std::vector<double> x_, objective_;
            VectorXi status_, iters_;
            std::vector<std::string> activated_contacts_, all_contacts_;
            std::unordered_map<std::string, MatrixXd> activated_contacts_forces_;

            // the rows of the last tick on the host, for cost(): fetched on demand when the tick computed them on the device
            void _ensure_rows() const
            {
                if (rows_valid_ || !source_ || in_.batch == 0) return;
                source_->compute(t_ - dt_, last_q_, last_v_, _stack(), _layout(), in_);
                rows_valid_ = true;
            }

            // the observables of the current state, fetched on demand like the rows above: one wbcqp_observe_host per tick at the most (a frame
            // asked for the first time joins the selection and costs one more).  The answer is kept WITH the state and the source it was made
            // for, so whatever moves q_tsid_ / v_tsid_ (a tick, qp_step_back, _reset) or replaces the source makes the next call fetch again.
            // Returns the frame's place in the selection (-1: none asked)
            int _ensure_observed(const std::string* frame) const
            {
                ProblemSource& source = _source();
                auto fetch = [&](bool joined) {
                    if (joined) obs_at_ = ComputedAt{};
                    _keep(obs_at_, &v_tsid_, [&] { source.observe(q_tsid_, v_tsid_, obs_names_.names, obs_com_, obs_vcom_, obs_place_, obs_vel_); });
                };
                if (frame) return obs_names_.with(*frame, fetch);
                fetch(false);
                return -1;
            }
            static MatrixXd _observed_block(const MatrixXd& all, int at, int width)
            {
                MatrixXd out(all.rows, width);
                for (int i = 0; i < all.rows; ++i) std::copy(all.row(i) + (size_t)at * width, all.row(i) + (size_t)(at + 1) * width, out.row(i));
                return out;
            }
            mutable FrameSelection obs_names_;
            mutable MatrixXd obs_com_, obs_vcom_, obs_place_, obs_vel_;
            mutable ComputedAt obs_at_; // the state and the source the four above were made for
            mutable MatrixXd mass_;
            mutable ComputedAt mass_at_; // the state (q alone) and the source mass_ was made for
            mutable IdDerivatives idd_;
            mutable MatrixXd idd_a_;
            mutable ComputedAt idd_at_; // the state and the source idd_ was made for; idd_a_: the accelerations

            // who answers for Jacobians and Hessians in the convention rf
            ProblemSource& _jacobian_source(int rf) const
            {
                ProblemSource& source = _model_source(ProblemSource::JACOBIAN);
                IWBC_ASSERT(rf == WORLD || rf == LOCAL || rf == LOCAL_WORLD_ALIGNED, "unknown reference frame ", rf);
                return source;
            }
            // the Jacobians of the current state, fetched on demand on the pattern of _ensure_observed: J per convention for the frames asked for
            // so far, Jcom and Ag with whichever call comes first at a state.  Returns the frame's place in the selection (-1: none asked)
            int _ensure_jacobians(const std::string* frame, int rf) const
            {
                ProblemSource& source = _jacobian_source(rf);
                auto fetch = [&](bool joined) {
                    if (joined) _jacobian_selection_grew();
                    _keep(frame ? jac_at_[rf] : jac_com_at_, nullptr, [&] {
                        jac_com_at_ = ComputedAt{};
                        source.jacobians(q_tsid_, jac_names_.names, rf, frame ? &jac_J_[rf] : nullptr, jac_com_, jac_ag_);
                        jac_com_at_.set(source_.get(), q_tsid_, nullptr); // (Jcom and Ag come with every call)
                    });
                };
                if (frame) return jac_names_.with(*frame, fetch);
                fetch(false);
                return -1;
            }
            mutable FrameSelection jac_names_;
            mutable MatrixXd jac_J_[3], jac_com_, jac_ag_; // J: per convention
            mutable ComputedAt jac_at_[3], jac_com_at_;    // the state (q alone) and the source they were made for
            // (the selection grew: what is kept of every convention, Jacobians and Hessians alike, is the old selection's)
            void _jacobian_selection_grew() const
            {
                for (auto& c : jac_at_) c = ComputedAt{};
                for (auto& c : hes_H_at_) c = ComputedAt{};
                for (auto& c : hes_dJ_at_) c = ComputedAt{};
            }

            // the kinematic Hessians (time: false) or the Jacobians' time variation (time: true) of the current state for the frames of the
            // Jacobians' selection, fetched on demand on the pattern of _ensure_jacobians.  Returns the frame's place in the selection
            int _ensure_hessians(const std::string& frame, int rf, bool time) const
            {
                ProblemSource& source = _jacobian_source(rf);
                const MatrixXd* v = time ? &v_tsid_ : nullptr;
                return jac_names_.with(frame, [&](bool joined) {
                    if (joined) _jacobian_selection_grew();
                    _keep(time ? hes_dJ_at_[rf] : hes_H_at_[rf], v, [&] {
                        source.hessians(q_tsid_, v, jac_names_.names, rf, time ? nullptr : &hes_H_[rf], time ? &hes_dJ_[rf] : nullptr);
                    });
                });
            }
            mutable MatrixXd hes_H_[3], hes_dJ_[3];          // per convention
            mutable ComputedAt hes_H_at_[3], hes_dJ_at_[3];  // the state (H: q alone) and the source they were made for

            std::shared_ptr<ProblemSource> source_;
            const double* tick_references_ = nullptr; // [batch][nref] read by the next tick instead of the source's stored references (the stabiliser's ref_out)
            mutable TickInputs in_; // (mutable with rows_valid_: _ensure_rows() fetches the rows for a const cost())
            MatrixXd last_q_, last_v_;
            mutable bool rows_valid_ = false;
            wbcqp_handle* handle_ = nullptr; // the reference's solver_ (controller.hpp:224)
        };

        using Factory = utils::Factory<Controller, yaml::Node>;
        template <typename T>
        using Register = Factory::AutoRegister<T>;
    } // namespace controllers
} // namespace inria_wbc
#endif
