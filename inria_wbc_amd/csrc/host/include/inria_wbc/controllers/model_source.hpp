// ModelSource: the step before the path on the device.  Holds what the reference's task objects hold after construction
// (/root/reference/src/controllers/tasks.cpp:38-404: tracked frame, mask, gains, reference per task) and turns the robot
// state of every instance into the rows of the QP with wbcqp_problem_data -- the batched counterpart of
// tsid_->computeProblemData(t, q, dq) at /root/reference/src/controllers/controller.cpp:244.
#ifndef IWBC_HIP_MODEL_SOURCE_HPP
#define IWBC_HIP_MODEL_SOURCE_HPP

#include <map>
#include <memory>

#include <inria_wbc/controllers/controller.hpp>
#include <inria_wbc/robots/robot_wrapper.hpp>

namespace inria_wbc {
    namespace controllers {
        class ModelSource : public ProblemSource {
            // what one (slot, task stack) pair needs: the task table handed to wbcqp_set_model and the reference vector laid out
            // for it.  One per slot: a controller that switches between contact sets keeps them all and only re-points.
            struct Bound {
                int nref_ = 0, posture_ref_ = 0;
                double posture_kp_ = 0.0, posture_kd_ = 0.0;
                bool joint_bounds_ = false;
                std::string posture_ref_name_;
                std::vector<double> ref_; // [batch][nref_]
                std::vector<wbcqp_task> tasks_;
                std::vector<std::string> names_, contact_names_;
                std::vector<int32_t> avoided_frames_, contact_frame_, contact_ref_;
                std::vector<double> avoided_r0_, contact_kp_, contact_kd_;
                // the place of the task `name` of kind `kind` in the table (-1: the stack has none)
                int task(const std::string& name, int kind) const
                {
                    for (size_t i = 0; i < tasks_.size(); ++i)
                        if (names_[i] == name && tasks_[i].kind == kind) return (int)i;
                    return -1;
                }
                // the reference r goes to every instance's row, at offset off
                template <typename Range>
                void put(int off, const Range& r)
                {
                    for (size_t row = 0; row < ref_.size(); row += nref_) std::copy(r.begin(), r.end(), ref_.begin() + row + off);
                }
            };

        public:
            // q0: the configuration the task references are initialised at (the controller's ref_config, pos_tracker.cpp:60-67)
            ModelSource(const std::shared_ptr<robots::RobotWrapper>& robot, int batch, const std::vector<double>& q0)
                : robot_(robot), batch_(batch), q0_(q0)
            {
                IWBC_ASSERT(robot_, "Invalid robot");
                IWBC_ASSERT(batch_ > 0, "batch must be positive");
                IWBC_ASSERT((int)q0_.size() == robot_->nq(), "q0 must hold nq entries");
            }
            int batch() const override { return batch_; }
            bool handles_references() const override { return true; }
            bool has_model() const override { return true; }

            void bind(wbcqp_handle* h, int slot, const tasks::TaskStack& stack, double dt) override
            {
                handle_ = h;
                slot_ = slot;
                const bool known = bounds_.count(slot) == 1;
                cur_ = &bounds_[slot];
                if (known) {
                    refresh(*cur_);
                    return;
                }
                read_tasks(*cur_, stack);
                initial_references(*cur_, stack);
                upload(*cur_, dt);
            }

            // the controller re-set the structure of a slot (wbcqp_set_structure drops the model): build again on the next bind
            void forget(int slot)
            {
                if (cur_ && bounds_.count(slot) && cur_ == &bounds_[slot]) cur_ = nullptr;
                bounds_.erase(slot);
                drop_query_tables(slot);
            }

            // wbcqp_check_collisions_host on the slot in use.  The table is built from the collision file when the slot has none for that file:
            // members sorted by name (the reference's std::map), links in file order, numbers read as float; a link is looked up in the model's
            // frames (the sphere rides on the frame's parent joint), a name X_link the frames do not hold is the link joint X_joint moves, and a
            // name that resolves to nothing is skipped, as the reference's loop over model.frames skips it (collision_check.cpp:58-87)
            void check_collisions(const MatrixXd& q, const std::string& file, VectorXi& colliding, VectorXi& first_pair,
                                  std::vector<std::pair<std::string, int>>& names) override
            {
                bound(q);
                auto known = spheres_.find(slot_);
                if (known == spheres_.end() || known->second.first != file) {
                    yaml::Node members = IWBC_CHECK(yaml::LoadFile(file)["members"]);
                    std::vector<std::string> order;
                    for (const auto& m : members) order.push_back(m.first);
                    std::sort(order.begin(), order.end());
                    IWBC_ASSERT((int)order.size() <= WBCQP_MAX_MEMBERS, "collisions yaml : at most ", WBCQP_MAX_MEMBERS, " members");
                    const wbcqp_model md = robot_->c_model();
                    const auto& joints = robot_->joint_names();
                    std::vector<int32_t> body, member;
                    std::vector<double> centre;
                    std::vector<float> diameter;
                    std::vector<std::pair<std::string, int>> table;
                    for (size_t k = 0; k < order.size(); ++k) {
                        int place = 0;
                        for (const auto& link : members[order[k]]) {
                            int b = -1;
                            if (robot_->existFrame(link.first))
                                b = md.frame_body[robot_->getFrameId(link.first)];
                            else if (link.first.size() > 5 && link.first.compare(link.first.size() - 5, 5, "_link") == 0) {
                                auto it = std::find(joints.begin(), joints.end(), link.first.substr(0, link.first.size() - 5) + "_joint");
                                if (it != joints.end()) b = (int)std::distance(joints.begin(), it);
                            }
                            if (b < 0) continue;
                            for (const auto& sphere : link.second.as<std::vector<std::vector<float>>>()) {
                                if (sphere.size() != 4) IWBC_ERROR("collisions yaml : sphere data should be an float array of dim 4");
                                body.push_back(b);
                                member.push_back((int32_t)k);
                                for (int d = 0; d < 3; ++d) centre.push_back((double)sphere[d]);
                                diameter.push_back(sphere[3]);
                                table.emplace_back(order[k], place++);
                            }
                        }
                    }
                    IWBC_ASSERT(!body.empty() && (int)body.size() <= WBCQP_MAX_SPHERES, "collisions yaml : ", body.size(), " spheres on this model, 1 .. ",
                                WBCQP_MAX_SPHERES, " are possible");
                    wbcqp_sphere_model sm = {(int32_t)body.size(), body.data(), member.data(), centre.data(), diameter.data()};
                    check(wbcqp_set_collision_spheres(handle_, slot_, &sm), "wbcqp_set_collision_spheres");
                    spheres_[slot_] = std::make_pair(file, table);
                    known = spheres_.find(slot_);
                }
                names = known->second.second;
                colliding.assign(batch_, 0);
                first_pair.assign((size_t)2 * batch_, -1);
                wbcqp_collisions out = {colliding.data(), first_pair.data(), nullptr, nullptr, nullptr};
                check(wbcqp_check_collisions_host(handle_, slot_, batch_, q.data.data(), &out), "wbcqp_check_collisions_host");
            }

            // wbcqp_observe_host on the slot in use; the selection of frames goes to the device when it changes, not per call
            void observe(const MatrixXd& q, const MatrixXd& v, const std::vector<std::string>& frames, MatrixXd& com, MatrixXd& vcom, MatrixXd& place,
                         MatrixXd& vel) override
            {
                bound(q, &v);
                IWBC_ASSERT((int)frames.size() <= WBCQP_MAX_OBSERVED, "at most ", WBCQP_MAX_OBSERVED, " frames can be observed");
                select_frames(observed_, frames, wbcqp_set_observed_frames, "wbcqp_set_observed_frames");
                const int n = (int)frames.size();
                com = MatrixXd(batch_, 3);
                vcom = MatrixXd(batch_, 3);
                place = MatrixXd(batch_, 12 * n);
                vel = MatrixXd(batch_, 6 * n);
                wbcqp_observables out = {com.data.data(), vcom.data.data(), n ? place.data.data() : nullptr, n ? vel.data.data() : nullptr};
                check(wbcqp_observe_host(handle_, slot_, batch_, q.data.data(), v.data.data(), &out), "wbcqp_observe_host");
            }

            // wbcqp_observe_acom_host (com, acom, the two ankle frames) and wbcqp_stabilize_host on the slot in use.  "The ankle" is the frame the
            // foot's contact tracks (humanoid_pos_tracker.cpp:163-166), also while that contact is removed; the offsets are found by the reference's
            // task names com, lf, rf, torso, contact_lfoot, contact_rfoot
            void stabilize(const StabilizerParams& p, const MatrixXd& q, const MatrixXd& v, const MatrixXd& wrench, const double* feet_forces_prev,
                           std::vector<unsigned char>& state, std::vector<double>& ref_out, VectorXi& flags, MatrixXd& cop) override
            {
                const Bound& b = bound(q, &v);
                IWBC_ASSERT(wrench.rows == batch_ && wrench.cols == 12, "one row of 12 sensor values per instance");
                wbcqp_stabilizer s{};
                s.window = p.window;
                s.dt = p.dt;
                const wbcqp_model md = robot_->c_model();
                for (int k = 0; k < md.nbody; ++k) s.mass += md.inertia[10 * k];
                std::copy(p.com.begin(), p.com.end(), s.com_gains);
                std::copy(p.ankle.begin(), p.ankle.end(), s.ankle_gains);
                std::copy(p.ffda.begin(), p.ffda.end(), s.ffda_gains);
                std::copy(p.normal.begin(), p.normal.end(), s.normal);
                s.nref = b.nref_;
                s.com_ref = s.lf_ref = s.rf_ref = s.torso_ref = -1;
                int lf_frame = -1, rf_frame = -1;
                for (size_t i = 0; i < b.tasks_.size(); ++i) {
                    const wbcqp_task& t = b.tasks_[i];
                    if (t.kind == WBCQP_T_COM) s.com_ref = t.ref;
                    if (t.kind != WBCQP_T_SE3) continue;
                    if (b.names_[i] == "lf") { s.lf_ref = t.ref; lf_frame = t.frame; }
                    if (b.names_[i] == "rf") { s.rf_ref = t.ref; rf_frame = t.frame; }
                    if (b.names_[i] == "torso") s.torso_ref = t.ref;
                }
                IWBC_ASSERT(s.com_ref >= 0 && s.lf_ref >= 0 && s.rf_ref >= 0 && s.torso_ref >= 0, "the stabilizer needs the tasks com, lf, rf and torso");
                s.lf_contact_ref = s.rf_contact_ref = -1;
                for (size_t c = 0; c < b.contact_names_.size(); ++c) {
                    ankle_frame_[b.contact_names_[c]] = b.contact_frame_[c];
                    if (b.contact_names_[c] == "contact_lfoot") s.lf_contact_ref = b.contact_ref_[c];
                    if (b.contact_names_[c] == "contact_rfoot") s.rf_contact_ref = b.contact_ref_[c];
                }
                if (ankle_frame_.count("contact_lfoot")) lf_frame = ankle_frame_["contact_lfoot"];
                if (ankle_frame_.count("contact_rfoot")) rf_frame = ankle_frame_["contact_rfoot"];
                s.lf_force_col = 0; // (feet_forces_prev is laid out here: left then right, whatever the previous tick's contact set was)
                s.rf_force_col = 12;
                s.lf_pos = 9;
                s.rf_pos = 21;
                const size_t bytes = (size_t)wbcqp_stabilizer_state_bytes(&s);
                IWBC_ASSERT(bytes > 0, "stabilizer: filter_size must be in [1, ", WBCQP_MAX_STAB_WINDOW, "] and every gain finite");
                if (state.size() != bytes * batch_) state.assign(bytes * batch_, 0); // (fresh filters, also after a change of filter_size)
                select_frames(observed_, {robot_->frame_names()[lf_frame], robot_->frame_names()[rf_frame]}, wbcqp_set_observed_frames, "wbcqp_set_observed_frames");
                MatrixXd com(batch_, 3), acom(batch_, 3), place(batch_, 24);
                const wbcqp_observables obs = {com.data.data(), nullptr, place.data.data(), nullptr};
                check(wbcqp_observe_acom_host(handle_, slot_, batch_, q.data.data(), v.data.data(), &obs, acom.data.data()), "wbcqp_observe_acom_host");
                ref_out.assign(b.ref_.size(), 0.0);
                flags.assign(batch_, 0);
                cop = MatrixXd(batch_, 6);
                const wbcqp_stab_inputs in = {b.ref_.data(), wrench.data.data(), com.data.data(), acom.data.data(), place.data.data(), 24, feet_forces_prev, 24};
                const wbcqp_stab_outputs out = {ref_out.data(), flags.data(), cop.data.data()};
                check(wbcqp_stabilize_host(handle_, &s, batch_, &in, state.data(), &out), "wbcqp_stabilize_host");
            }

            // wbcqp_inverse_dynamics_host on the slot in use; the selection of frames goes to the device when it changes, not per call
            void inverse_dynamics(const MatrixXd& q, const MatrixXd& v, const MatrixXd& a, const std::vector<std::string>& frames, const MatrixXd& wrenches,
                                  MatrixXd& tau) override
            {
                bound(q, &v, &a);
                const double* w = select_wrenches(frames, wrenches);
                tau = MatrixXd(batch_, robot_->nv());
                check(wbcqp_inverse_dynamics_host(handle_, slot_, batch_, q.data.data(), v.data.data(), a.data.data(), a.cols, w, tau.data.data()),
                      "wbcqp_inverse_dynamics_host");
            }
            // wbcqp_inverse_dynamics_derivatives_host on the slot in use; the wrench frames are inverse_dynamics' selection
            void inverse_dynamics_derivatives(const MatrixXd& q, const MatrixXd& v, const MatrixXd& a, const std::vector<std::string>& frames,
                                              const MatrixXd& wrenches, MatrixXd& dtau_dq, MatrixXd& dtau_dv) override
            {
                bound(q, &v, &a);
                const double* w = select_wrenches(frames, wrenches);
                const int nv = robot_->nv();
                dtau_dq = MatrixXd(batch_, nv * nv);
                dtau_dv = MatrixXd(batch_, nv * nv);
                const wbcqp_id_derivative_outputs out = {dtau_dq.data.data(), dtau_dv.data.data()};
                check(wbcqp_inverse_dynamics_derivatives_host(handle_, slot_, batch_, q.data.data(), v.data.data(), a.data.data(), a.cols, w, &out),
                      "wbcqp_inverse_dynamics_derivatives_host");
            }
            // wbcqp_mass_matrix_host on the slot in use
            void mass_matrix(const MatrixXd& q, MatrixXd& M) override
            {
                bound(q);
                M = MatrixXd(batch_, robot_->nv() * robot_->nv());
                check(wbcqp_mass_matrix_host(handle_, slot_, batch_, q.data.data(), M.data.data()), "wbcqp_mass_matrix_host");
            }
            // wbcqp_forward_dynamics_host on the slot in use.  The wrench frames are inverse_dynamics' selection ON THE SLOT: a call with other
            // frames -- or none, as Controller::forward_dynamics makes it -- replaces (clears) it there; wrench_frames_ remembers, so the next
            // inverse_dynamics selects its own again
            void forward_dynamics(const MatrixXd& q, const MatrixXd& v, const MatrixXd& tau, const std::vector<std::string>& frames, const MatrixXd& wrenches,
                                  const std::vector<double>& damping, MatrixXd& a, VectorXi& info) override
            {
                bound(q, &v, &tau);
                const int nv = robot_->nv();
                IWBC_ASSERT(damping.empty() || (int)damping.size() == nv, "damping holds nv entries, or none");
                const double* w = select_wrenches(frames, wrenches);
                a = MatrixXd(batch_, nv);
                info.assign(batch_, 0);
                check(wbcqp_forward_dynamics_host(handle_, slot_, batch_, q.data.data(), v.data.data(), tau.data.data(), tau.cols, w,
                                                  damping.empty() ? nullptr : damping.data(), a.data.data(), info.data()),
                      "wbcqp_forward_dynamics_host");
            }
            // wbcqp_spd_commands_host on the slot in use, without constraint forces; targetpos: B x na, or B x nv with a floating base's six in front
            void spd_commands(const MatrixXd& q, const MatrixXd& dq, const MatrixXd& targetpos, double dt, double kp, double kd, MatrixXd& commands) override
            {
                bound(q, &dq);
                const int nv = robot_->nv(), na = robot_->na();
                IWBC_ASSERT(targetpos.rows == batch_ && (targetpos.cols == na || targetpos.cols == nv), "targetpos holds na or nv entries per instance");
                commands = MatrixXd(batch_, nv);
                const wbcqp_spd law = {dt, kp, kd};
                check(wbcqp_spd_commands_host(handle_, slot_, batch_, &law, q.data.data(), dq.data.data(), targetpos.data.data() + (targetpos.cols - na),
                                              targetpos.cols, nullptr, commands.data.data(), nullptr, nullptr),
                      "wbcqp_spd_commands_host");
            }
            // wbcqp_jacobians_host on the slot in use; the selection of frames goes to the device when it changes, not per call
            void jacobians(const MatrixXd& q, const std::vector<std::string>& frames, int reference_frame, MatrixXd* J, MatrixXd& Jcom, MatrixXd& Ag) override
            {
                bound(q);
                const int n = select_jacobian_frames(frames), nv = robot_->nv();
                if (J) *J = MatrixXd(batch_, 6 * nv * n);
                Jcom = MatrixXd(batch_, 3 * nv);
                Ag = MatrixXd(batch_, 6 * nv);
                const wbcqp_jacobian_outputs out = {(J && n) ? J->data.data() : nullptr, Jcom.data.data(), Ag.data.data(), nullptr, nullptr};
                check(wbcqp_jacobians_host(handle_, slot_, batch_, q.data.data(), nullptr, reference_frame, &out), "wbcqp_jacobians_host");
            }
            // wbcqp_kinematic_hessians_host on the slot in use, for the Jacobians' selection of frames
            void hessians(const MatrixXd& q, const MatrixXd* v, const std::vector<std::string>& frames, int reference_frame, MatrixXd* H, MatrixXd* dJ) override
            {
                bound(q);
                const int nv = robot_->nv();
                IWBC_ASSERT(!v || (v->rows == batch_ && v->cols == nv), "one velocity row per instance");
                const int n = select_jacobian_frames(frames);
                if (H) *H = MatrixXd(batch_, 6 * nv * nv * n);
                if (dJ) *dJ = MatrixXd(batch_, 6 * nv * n);
                const wbcqp_hessian_outputs out = {H ? H->data.data() : nullptr, dJ ? dJ->data.data() : nullptr};
                check(wbcqp_kinematic_hessians_host(handle_, slot_, batch_, q.data.data(), v ? v->data.data() : nullptr, reference_frame, &out),
                      "wbcqp_kinematic_hessians_host");
            }
            void add_foot_mass(const MatrixXd& q, const std::string& ft_frame, const std::string& sole_frame, MatrixXd& force, MatrixXd& torque) const override
            {
                if (!robot_->existFrame(ft_frame)) IWBC_ERROR("Frame name ", ft_frame, "is not in model"); // robot_model.cpp:173-176
                if (!robot_->existFrame(sole_frame)) IWBC_ERROR("Frame name ", sole_frame, "is not in model");
                const int ft = robot_->getFrameId(ft_frame), sole = robot_->getFrameId(sole_frame);
                const wbcqp_model md = robot_->c_model();
                const int body = md.frame_body[ft];
                const float mass_to_add = (float)md.inertia[10 * body]; // (a float there too)
                for (int i = 0; i < batch_; ++i) {
                    const auto ankle = robot_->bodyPlacements(q.row(i))[body].p;
                    const auto s = robot_->framePosition(q.row(i), sole).p;
                    for (int d = 0; d < 3; ++d) force(i, d) -= mass_to_add * md.gravity[d];
                    const double r[3] = {ankle[0] - s[0], ankle[1] - s[1], ankle[2] - s[2]};
                    torque(i, 0) += r[1] * force(i, 2) - r[2] * force(i, 1);
                    torque(i, 1) += r[2] * force(i, 0) - r[0] * force(i, 2);
                    torque(i, 2) += r[0] * force(i, 1) - r[1] * force(i, 0);
                }
            }

            void compute(double, const MatrixXd& q, const MatrixXd& v, const tasks::TaskStack& stack, const wbcqp_layout& L, TickInputs& in) override
            {
                wbcqp_state st = {q.data.data(), v.data.data(), bound(q, &v).ref_.data()};
                wbcqp_inputs rows{};
                rows.M = in.M.data(); rows.h = in.h.data(); rows.A = in.A.data(); rows.b1 = in.b1.data(); rows.Ac = in.Ac.data();
                rows.bc = in.bc.data(); rows.blb = in.blb.data(); rows.bub = in.bub.data(); rows.Acop = in.Acop.data();
                check(wbcqp_problem_data_host(handle_, slot_, batch_, &st, &rows), "wbcqp_problem_data_host");
                fill_limits(L, in);
                (void)stack;
            }
            // actuation bounds: -tau_max, tau_max (tasks.cpp:315-316)
            void fill_limits(const wbcqp_layout& L, TickInputs& in) const override
            {
                const auto& tmax = robot_->effortLimit();
                for (int i = 0; i < batch_; ++i)
                    for (int j = 0; j < L.len_tlb; ++j) {
                        in.tlb[(size_t)i * L.len_tlb + j] = -tmax[j];
                        in.tub[(size_t)i * L.len_tub + j] = tmax[j];
                    }
            }
            const double* reference_data() const override { return cur_ ? cur_->ref_.data() : nullptr; }
            void com(MatrixXd& pos, MatrixXd& vel) const override { pos = com_pos_; vel = com_vel_; }

            void set_com_ref(const TrajectorySample& s) override
            {
                const Bound& b = bound();
                for (size_t i = 0; i < b.tasks_.size(); ++i)
                    if (b.tasks_[i].kind == WBCQP_T_COM) {
                        std::vector<double> r(9);
                        for (int d = 0; d < 3; ++d) { r[d] = s.pos[d]; r[3 + d] = s.vel[d]; r[6 + d] = s.acc[d]; }
                        store(b.names_[i], b.tasks_[i].ref, r);
                    }
            }
            // sample.pos: 12 numbers (translation, rotation column-major), vel / acc: 6 each (PosTracker::set_se3_ref, pos_tracker.cpp:221-237)
            void set_se3_ref(const std::string& name, const TrajectorySample& s) override
            {
                const int i = bound().task(name, WBCQP_T_SE3);
                if (i < 0) IWBC_ERROR("Task [", name, "] not found");
                IWBC_ASSERT(s.pos.size() == 12 && s.vel.size() == 6 && s.acc.size() == 6, "an SE3 sample holds 12 + 6 + 6 numbers");
                std::vector<double> r(s.pos);
                r.insert(r.end(), s.vel.begin(), s.vel.end());
                r.insert(r.end(), s.acc.begin(), s.acc.end());
                store(name, cur_->tasks_[i].ref, r);
            }
            std::vector<double> get_se3_ref(const std::string& name) const override
            {
                const Bound& b = bound();
                const int i = b.task(name, WBCQP_T_SE3);
                if (i < 0) IWBC_ERROR("Task [", name, "] not found");
                return std::vector<double>(b.ref_.begin() + b.tasks_[i].ref, b.ref_.begin() + b.tasks_[i].ref + 12);
            }
            // PosTracker::set_contact_se3_ref (pos_tracker.cpp:227-232): kept for contacts that are currently removed too
            void set_contact_se3_ref(const std::string& name, const std::vector<double>& sample) override
            {
                Bound& b = bound();
                IWBC_ASSERT(sample.size() == 12 || sample.size() == 24, "a contact reference holds 12 numbers (placement) or 24 (with velocity and acceleration)");
                std::vector<double> pose(sample);
                pose.resize(24, 0.0); // to_sample(SE3): zero derivatives (pos_tracker.cpp:227-232)
                named_[name] = pose;
                for (size_t c = 0; c < b.contact_names_.size(); ++c)
                    if (b.contact_names_[c] == name) b.put(b.contact_ref_[c], pose);
            }
            void set_posture_ref(const std::vector<double>& q_actuated) override
            {
                Bound& b = bound();
                IWBC_ASSERT((int)q_actuated.size() == robot_->na(), "the posture reference holds na entries");
                posture_user_ = q_actuated;
                b.put(b.posture_ref_, q_actuated);
            }
            const std::vector<double>& references() const { return cur_->ref_; }
            int nref() const { return cur_ ? cur_->nref_ : 0; }

        private:
            using FrameNames = std::map<int, std::vector<std::string>>; // slot -> the frames selected on it
            // the selection of frames goes to the slot in use when it differs from the one the slot holds
            void select_frames(FrameNames& held, const std::vector<std::string>& frames, int (*setter)(wbcqp_handle*, int, int, const int32_t*), const char* setter_name)
            {
                auto known = held.find(slot_);
                if (known != held.end() && known->second == frames) return;
                std::vector<int32_t> ids;
                for (const auto& f : frames) ids.push_back(robot_->getFrameId(f));
                check(setter(handle_, slot_, (int)ids.size(), ids.data()), setter_name);
                held[slot_] = frames;
            }
            // the library drops the selections of frames and the sphere table with the model
            void drop_query_tables(int slot)
            {
                observed_.erase(slot);
                spheres_.erase(slot);
                wrench_frames_.erase(slot);
                jacobian_frames_.erase(slot);
            }

            // Every device call starts here: the source is bound to a solver and, given states, holds one row per instance -- q, v (null: the
            // call takes none) and `wide` (null: none), the accelerations or torques that may carry columns behind the first nv
            Bound& bound() const
            {
                IWBC_ASSERT(cur_ && handle_, "ModelSource is not bound to a solver");
                return *cur_;
            }
            Bound& bound(const MatrixXd& q, const MatrixXd* v = nullptr, const MatrixXd* wide = nullptr) const
            {
                const int nv = robot_->nv();
                IWBC_ASSERT(q.rows == batch_ && q.cols == robot_->nq() && (!v || (v->rows == batch_ && v->cols == nv)) &&
                                (!wide || (wide->rows == batch_ && wide->cols >= nv)),
                            "one state row per instance");
                return bound();
            }
            // ... and ends here
            void check(int rc, const char* call) const
            {
                if (rc != WBCQP_OK) IWBC_ERROR(call, " failed: ", wbcqp_last_error(handle_));
            }
            // the wrench frames of inverse and forward dynamics go to the slot; returns the wrenches for the call (null: no frames)
            const double* select_wrenches(const std::vector<std::string>& frames, const MatrixXd& wrenches)
            {
                const int n = (int)frames.size();
                IWBC_ASSERT(n <= WBCQP_MAX_WRENCH_FRAMES, "at most ", WBCQP_MAX_WRENCH_FRAMES, " wrench frames");
                IWBC_ASSERT(n == 0 || (wrenches.rows == batch_ && wrenches.cols == 6 * n), "six numbers per frame and instance");
                select_frames(wrench_frames_, frames, wbcqp_set_wrench_frames, "wbcqp_set_wrench_frames");
                return n ? wrenches.data.data() : nullptr;
            }
            // the frames of the Jacobians and Hessians go to the slot; returns how many they are
            int select_jacobian_frames(const std::vector<std::string>& frames)
            {
                const int n = (int)frames.size();
                IWBC_ASSERT(n <= WBCQP_MAX_JACOBIAN_FRAMES, "at most ", WBCQP_MAX_JACOBIAN_FRAMES, " frames can have a Jacobian");
                select_frames(jacobian_frames_, frames, wbcqp_set_jacobian_frames, "wbcqp_set_jacobian_frames");
                return n;
            }

            void store(const std::string& name, int off, const std::vector<double>& r)
            {
                named_[name] = r;
                bound().put(off, r);
            }

            // bind, step 1: the task file becomes the task table, and every reference gets its offset in an instance's row
            void read_tasks(Bound& b, const tasks::TaskStack& stack)
            {
                const int na = robot_->na();
                IWBC_ASSERT(stack.nv() == robot_->nv() && stack.na() == na, "task stack and robot disagree on nv / na");
                std::vector<size_t> av_begin;
                int off = 0;
                for (const auto& kv : stack.source()) {
                    const yaml::Node& node = kv.second;
                    const auto type = IWBC_CHECK(node["type"].as<std::string>());
                    wbcqp_task t{};
                    const size_t begin = b.avoided_frames_.size();
                    auto mask_bits = [](const std::string& m) { int bits = 0; for (size_t i = 0; i < m.size(); ++i) if (m[i] != '0') bits |= 1 << i; return bits; };
                    if (type == "se3" || type == "com" || type == "momentum") {
                        const double kp = IWBC_CHECK(node["kp"].as<double>());
                        t.kind = type == "se3" ? WBCQP_T_SE3 : (type == "com" ? WBCQP_T_COM : WBCQP_T_MOMENTUM);
                        t.frame = type == "se3" ? robot_->getFrameId(IWBC_CHECK(node["tracked"].as<std::string>())) : 0;
                        t.mask = mask_bits(IWBC_CHECK(node["mask"].as<std::string>()));
                        t.kp = kp;
                        t.kd = 2.0 * std::sqrt(kp); // tasks.cpp:57,107,140
                        t.ref = off;
                        off += type == "se3" ? 24 : (type == "com" ? 9 : 12);
                    }
                    else if (type == "self-collision") {
                        t.kind = WBCQP_T_SELFCOLLISION;
                        t.frame = robot_->getFrameId(IWBC_CHECK(node["tracked"].as<std::string>()));
                        t.mask = 1;
                        t.kp = IWBC_CHECK(node["kp"].as<double>());
                        t.kd = IWBC_CHECK(node["kd"].as<double>());
                        t.radius = IWBC_CHECK(node["radius"].as<double>());
                        t.margin = IWBC_CHECK(node["margin"].as<double>());
                        t.m = IWBC_CHECK(node["m"].as<double>());
                        for (const auto& a : IWBC_CHECK(node["avoided"])) {
                            IWBC_ASSERT(robot_->existFrame(a.first), "Frame ", a.first, " in ", kv.first, " does not exists."); // tasks.cpp:388
                            b.avoided_frames_.push_back(robot_->getFrameId(a.first));
                            b.avoided_r0_.push_back(a.second.as<double>());
                            ++t.n_avoided;
                        }
                    }
                    else if (type == "posture") {
                        b.posture_kp_ = IWBC_CHECK(node["kp"].as<double>());
                        b.posture_kd_ = 2.0 * std::sqrt(b.posture_kp_);
                        b.posture_ref_name_ = IWBC_CHECK(node["ref"].as<std::string>());
                        continue;
                    }
                    else if (type == "contact") {
                        const auto joint = IWBC_CHECK(node["joint"].as<std::string>());
                        IWBC_ASSERT(robot_->existFrame(joint), joint, " does not exist!"); // tasks.cpp:349
                        const double kp = IWBC_CHECK(node["kp"].as<double>());
                        b.contact_names_.push_back(kv.first);
                        b.contact_frame_.push_back(robot_->getFrameId(joint));
                        b.contact_kp_.push_back(kp);
                        b.contact_kd_.push_back(2.0 * std::sqrt(kp)); // tasks.cpp:360
                        continue;
                    }
                    else if (type == "bounds") { b.joint_bounds_ = true; continue; }
                    else continue; // actuation-bounds: constant limits; torque / cop: the rows are the structure's (task_stack.hpp), the
                                   // cop rows come out of the rows kernel with the contact frames, the torque reference is zero (tasks.cpp:263)
                    av_begin.push_back(begin);
                    b.tasks_.push_back(t);
                    b.names_.push_back(kv.first);
                }
                for (size_t i = 0; i < b.tasks_.size(); ++i)
                    if (b.tasks_[i].kind == WBCQP_T_SELFCOLLISION) {
                        b.tasks_[i].avoided_frame = b.avoided_frames_.data() + av_begin[i];
                        b.tasks_[i].avoided_r0 = b.avoided_r0_.data() + av_begin[i];
                    }
                b.posture_ref_ = off;
                if (stack.n_sel() > 0) off += na;
                for (size_t c = 0; c < b.contact_names_.size(); ++c) {
                    b.contact_ref_.push_back(off);
                    off += 24; // a full sample, like an SE3 task
                }
                b.nref_ = off;
            }
            // bind, step 2: the references of a freshly constructed controller -- every frame where it is at q0 (tasks.cpp:64-80,361), the CoM
            // where it is (tasks.cpp:109), zero momentum (tasks.cpp:144-145), the named posture (tasks.cpp:194-217) -- under what was set since
            void initial_references(Bound& b, const tasks::TaskStack& stack)
            {
                b.ref_.assign((size_t)batch_ * b.nref_, 0.0);
                for (const wbcqp_task& t : b.tasks_) {
                    if (t.kind == WBCQP_T_SE3) b.put(t.ref, robot_->framePosition(q0_.data(), t.frame).to_vector());
                    if (t.kind == WBCQP_T_COM) b.put(t.ref, robot_->com(q0_.data()));
                }
                if (stack.n_sel() > 0) {
                    const auto& refs = robot_->referenceConfigurations();
                    IWBC_ASSERT(refs.count(b.posture_ref_name_) == 1, "Reference name ", b.posture_ref_name_, " not found"); // tasks.cpp:194
                    const auto& rq = refs.at(b.posture_ref_name_);
                    b.put(b.posture_ref_, std::vector<double>(rq.end() - robot_->na(), rq.end()));
                }
                for (size_t c = 0; c < b.contact_frame_.size(); ++c) b.put(b.contact_ref_[c], robot_->framePosition(q0_.data(), b.contact_frame_[c]).to_vector());
                refresh(b);
            }
            // bind, step 3: the model and the task table go to the slot (which drops the slot's selections of frames and sphere table)
            void upload(Bound& b, double dt)
            {
                wbcqp_model md = robot_->c_model();
                wbcqp_taskmap tm{};
                tm.n_task = (int)b.tasks_.size();
                tm.task = b.tasks_.data();
                tm.posture_kp = b.posture_kp_; tm.posture_kd = b.posture_kd_; tm.posture_ref = b.posture_ref_;
                tm.n_contact = (int)b.contact_frame_.size();
                tm.contact_frame = b.contact_frame_.data(); tm.contact_kp = b.contact_kp_.data(); tm.contact_kd = b.contact_kd_.data();
                tm.contact_ref = b.contact_ref_.data();
                tm.bounds = b.joint_bounds_ ? 1 : 0;
                tm.dt = dt;
                tm.nref = b.nref_;
                check(wbcqp_set_model(handle_, slot_, &md, &tm), "wbcqp_set_model");
                drop_query_tables(slot_);
                auto c0 = robot_->com(q0_.data());
                com_pos_ = MatrixXd(batch_, 3);
                com_vel_ = MatrixXd(batch_, 3);
                for (int i = 0; i < batch_; ++i)
                    for (int d = 0; d < 3; ++d) com_pos_(i, d) = c0[d];
            }

            // a slot seen before: nothing goes to the device, the references set meanwhile are laid out for this stack
            void refresh(Bound& b)
            {
                for (size_t i = 0; i < b.tasks_.size(); ++i) {
                    auto it = named_.find(b.names_[i]);
                    if (it != named_.end() && b.tasks_[i].kind != WBCQP_T_SELFCOLLISION) b.put(b.tasks_[i].ref, it->second);
                }
                for (size_t c = 0; c < b.contact_names_.size(); ++c) {
                    auto it = named_.find(b.contact_names_[c]);
                    if (it != named_.end()) b.put(b.contact_ref_[c], it->second);
                }
                if (!posture_user_.empty()) b.put(b.posture_ref_, posture_user_);
            }

            std::shared_ptr<robots::RobotWrapper> robot_;
            int batch_ = 0, slot_ = 0;
            std::vector<double> q0_, posture_user_;
            wbcqp_handle* handle_ = nullptr;
            std::map<int, Bound> bounds_;
            FrameNames observed_, wrench_frames_, jacobian_frames_; // wbcqp_set_observed_frames, wbcqp_set_wrench_frames, wbcqp_set_jacobian_frames
            // slot -> the collision file whose table it holds (wbcqp_set_collision_spheres) and every table entry's (member, place in the member)
            std::map<int, std::pair<std::string, std::vector<std::pair<std::string, int>>>> spheres_;
            Bound* cur_ = nullptr;
            std::map<std::string, std::vector<double>> named_;
            std::map<std::string, int> ankle_frame_; // contact name -> the frame it tracks, kept while the contact is removed
            MatrixXd com_pos_, com_vel_;
        };
    } // namespace controllers
} // namespace inria_wbc
#endif
