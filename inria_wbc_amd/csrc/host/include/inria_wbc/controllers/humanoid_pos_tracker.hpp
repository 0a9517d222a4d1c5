// "humanoid-pos-tracker" and "talos-pos-tracker" (/root/reference/src/controllers/humanoid_pos_tracker.cpp:35,
// /root/reference/src/controllers/talos_pos_tracker.cpp:35): the reference's two humanoid controllers, under their registration names and with
// their constructor signature, for B instances.
//
// HumanoidPosTracker adds the STABILISER around the tick (humanoid_pos_tracker.cpp:41-131 parse, :134-302 update): with
// CONTROLLER.stabilizer.activated it reads params_fixed_base / params_ss / params_ds (files relative to base_path: filter_size, com, ankle,
// ffda, use_zmp), and update(sensor_data) requires lf_force, rf_force, lf_torque, rf_torque and imu_vel (B x 3 each, or three numbers for all
// instances), runs wbcqp_stabilize_host on the controller's stored references with com, acom and the two ankle frames observed at the state the
// PREVIOUS tick's rows were formed at (the reference's tsid data lags by one tick; on the first tick: the constructor's state) and with the
// previous solution's contact forces, and ticks on the stabilised references.  The stored references are never touched, which is the
// reference's restore step.  An instance whose CoP or ground force fails the reference's sanity checks raises the reference's message with
// the instance appended, before the solve and after every filter has advanced.  cop() is the valid CoP per instance (NaN where none),
// stabilizer_flags() the WBCQP_STAB_* bits.  set_behavior_type selects the file; a change of filter_size starts fresh filters (the
// reference resizes its buffers in place).
// NOT built (include/wbcqp.h): the ZMP force distributor -- `use_zmp: true` in the ACTIVE file is refused, set use_zmp:
// false; the momentum / IMU admittances (use_momentum is read by nobody in the reference's update either; imu_vel is required and unused, as
// there); default gains -- activated: true without the three params_* keys is refused.
//
// TalosPosTracker adds the torque-collision safety (talos_pos_tracker.cpp:62-158) for every instance of the batch: before a tick's solve the
// measured joint torques are compared with tau() as the previous tick left it, through wbcqp_detect_torque_collisions_host (a moving average
// over filter_size samples, max_invalid + 1 consecutive same-signed violations).  The torso-roll clamp of its constructor is not built.
#ifndef IWBC_HIP_HUMANOID_POS_TRACKER_HPP
#define IWBC_HIP_HUMANOID_POS_TRACKER_HPP

#include <cmath>
#include <limits>
#include <map>
#include <inria_wbc/controllers/pos_tracker.hpp>

namespace inria_wbc {
    namespace controllers {
        class HumanoidPosTracker : public PosTracker {
        public:
            explicit HumanoidPosTracker(const yaml::Node& config) : PosTracker(config)
            {
                behavior_type_ = behavior_types::FIXED_BASE; // humanoid_pos_tracker.cpp:39
                parse_stabilizer(IWBC_CHECK(config["CONTROLLER"]));
                if (verbose_) std::cout << "Humanoid pos tracker initialized (stabilizer: " << _use_stabilizer << ")" << std::endl;
            }
            // the reference accepts FIXED_BASE / SINGLE_SUPPORT / DOUBLE_SUPPORT only (humanoid_pos_tracker.cpp:116-131)
            void set_behavior_type(const std::string& bt) override
            {
                if (bt != behavior_types::FIXED_BASE && bt != behavior_types::SINGLE_SUPPORT && bt != behavior_types::DOUBLE_SUPPORT)
                    IWBC_ERROR("_stabilizer_configs does not have ", bt);
                if (_use_stabilizer) _check_active(bt);
                Controller::set_behavior_type(bt);
            }

            void update(const SensorData& sensor_data = {}) override
            {
                if (!_use_stabilizer) {
                    PosTracker::update(sensor_data);
                    return;
                }
                const StabilizerConfig& cfg = _check_active(behavior_type_);
                const int B = batch_size();
                MatrixXd wrench(B, 12);
                _sensor(sensor_data, "lf_force", "the stabilizer needs the LF force", wrench, 0);
                _sensor(sensor_data, "rf_force", "the stabilizer needs the RF force", wrench, 6);
                _sensor(sensor_data, "lf_torque", "the stabilizer needs the LF torque", wrench, 3);
                _sensor(sensor_data, "rf_torque", "the stabilizer needs the RF torque", wrench, 9);
                IWBC_ASSERT(sensor_data.find("imu_vel") != sensor_data.end(), "the stabilizer imu needs angular velocity");
                StabilizerParams p;
                p.window = cfg.filter_size;
                p.dt = dt_;
                p.com = cfg.com;
                p.ankle = cfg.ankle;
                p.ffda = cfg.ffda;
                if (!_stack().contacts().empty()) p.normal = _stack().contacts()[0].normal;
                // the model state the reference's stabiliser sees: the one the previous tick's rows were formed at
                const bool lagged = q_tsid_prev_.rows == B && B > 0;
                const MatrixXd& q = lagged ? q_tsid_prev_ : q_tsid_;
                const MatrixXd& v = lagged ? v_tsid_prev_ : v_tsid_;
                // the previous solution's forces of both feet, when both were in contact then
                MatrixXd feet;
                auto lf = activated_contacts_forces_.find("contact_lfoot"), rf = activated_contacts_forces_.find("contact_rfoot");
                if (lf != activated_contacts_forces_.end() && rf != activated_contacts_forces_.end() && lf->second.rows == B && rf->second.rows == B) {
                    feet = MatrixXd(B, 24);
                    for (int i = 0; i < B; ++i) {
                        std::copy(lf->second.row(i), lf->second.row(i) + 12, feet.row(i));
                        std::copy(rf->second.row(i), rf->second.row(i) + 12, feet.row(i) + 12);
                    }
                }
                if (cfg.filter_size != _stab_window) _stab_state.clear(); // fresh filters
                _stab_window = cfg.filter_size;
                MatrixXd cops;
                IWBC_ASSERT(source_, "no problem source set (set_problem_source)");
                source_->stabilize(p, q, v, wrench, feet.rows ? feet.data.data() : nullptr, _stab_state, _stab_ref, _stab_flags, cops);
                _cop = MatrixXd(B, 2, std::numeric_limits<double>::quiet_NaN());
                for (int i = 0; i < B; ++i) {
                    const int f = _stab_flags[i];
                    const int which = (f & WBCQP_STAB_COP) ? 0 : (f & WBCQP_STAB_LCOP) ? 1 : (f & WBCQP_STAB_RCOP) ? 2 : -1;
                    if (which >= 0) { _cop(i, 0) = cops(i, 2 * which); _cop(i, 1) = cops(i, 2 * which + 1); }
                }
                for (int i = 0; i < B; ++i) {
                    if (_stab_flags[i] & WBCQP_STAB_ERR_COP)
                        IWBC_ERROR("com_admittance : something is wrong with input cop_filtered, check sensor measurment: ", std::fabs(_cop(i, 0)), " ",
                                   std::fabs(_cop(i, 1)), " [instance ", i, "]");
                    if (_stab_flags[i] & WBCQP_STAB_ERR_FORCE)
                        IWBC_ERROR("zmp_distributor_admittance : ground force is more than 10*M*g , check sensor measurment [instance ", i, "]");
                }
                tick_references_ = _stab_ref.data();
                try {
                    PosTracker::update(sensor_data);
                }
                catch (...) {
                    tick_references_ = nullptr;
                    throw;
                }
                tick_references_ = nullptr;
            }

            bool stabilizer_activated() const { return _use_stabilizer; }
            // the valid CoP of the last update per instance (combined, else left, else right), NaN where none is valid: B x 2
            const MatrixXd& cop() const { return _cop; }
            // WBCQP_STAB_* of the last update, one per instance
            const VectorXi& stabilizer_flags() const { return _stab_flags; }
            // the references the last stabilised tick read: B x nref (empty before the first one)
            const std::vector<double>& stabilized_references() const { return _stab_ref; }

        protected:
            struct StabilizerConfig {
                int filter_size = 1;
                std::array<double, 6> com{}, ankle{};
                std::array<double, 3> ffda{};
                bool use_zmp = false;
            };
            // humanoid_pos_tracker.cpp:41-114
            void parse_stabilizer(const yaml::Node& c)
            {
                yaml::Node st = c["stabilizer"];
                if (!st || !st["activated"] || !st["activated"].as<bool>()) return;
                if (!st["params_fixed_base"] || !st["params_ss"] || !st["params_ds"])
                    IWBC_ERROR("humanoid-pos-tracker: stabilizer.activated is true, but stabilizer.params_fixed_base / params_ss / params_ds are missing; "
                               "default stabilizer gains are not part of this build");
                _stabilizer_configs[behavior_types::FIXED_BASE] = _parse_file(st["params_fixed_base"].as<std::string>());
                _stabilizer_configs[behavior_types::SINGLE_SUPPORT] = _parse_file(st["params_ss"].as<std::string>());
                _stabilizer_configs[behavior_types::DOUBLE_SUPPORT] = _parse_file(st["params_ds"].as<std::string>());
                _use_stabilizer = true;
                _check_active(behavior_type_);
            }
            StabilizerConfig _parse_file(const std::string& file) const
            {
                const std::string path = file.size() && file[0] == '/' ? file : base_path() + "/" + file;
                yaml::Node n = IWBC_CHECK(yaml::LoadFile(path));
                StabilizerConfig cfg;
                cfg.filter_size = IWBC_CHECK(n["filter_size"].as<int>());
                IWBC_ASSERT(cfg.filter_size >= 1 && cfg.filter_size <= WBCQP_MAX_STAB_WINDOW, path, ": filter_size must be in [1, ", WBCQP_MAX_STAB_WINDOW, "]");
                auto vec = [&](const char* key, size_t len, double* out) {
                    auto v = IWBC_CHECK(n[key].as<std::vector<double>>());
                    IWBC_ASSERT(v.size() == len, path, ": you need ", len, " coefficients in ", key);
                    std::copy(v.begin(), v.end(), out);
                };
                vec("com", 6, cfg.com.data());
                vec("ankle", 6, cfg.ankle.data());
                vec("ffda", 3, cfg.ffda.data());
                cfg.use_zmp = n["use_zmp"] ? n["use_zmp"].as<bool>() : false;
                return cfg;
            }
            const StabilizerConfig& _check_active(const std::string& bt) const
            {
                auto it = _stabilizer_configs.find(bt);
                if (it == _stabilizer_configs.end()) IWBC_ERROR("_stabilizer_configs does not have ", bt);
                if (it->second.use_zmp)
                    IWBC_ERROR("humanoid-pos-tracker: use_zmp is true in the stabilizer file of ", bt, ", but the ZMP force distributor is not part of this "
                               "build; set use_zmp: false");
                return it->second;
            }
            // a sensor of the stabiliser into three columns of the wrench rows: B x 3, or three numbers for every instance
            void _sensor(const SensorData& sd, const char* key, const char* missing, MatrixXd& wrench, int at) const
            {
                auto it = sd.find(key);
                IWBC_ASSERT(it != sd.end(), missing);
                const MatrixXd& s = it->second;
                const bool one = (int)s.data.size() == 3;
                IWBC_ASSERT(one || (s.rows == wrench.rows && s.cols == 3), key, ": 3 numbers per instance (", wrench.rows, " x 3), or 3 numbers for all");
                for (int i = 0; i < wrench.rows; ++i)
                    for (int k = 0; k < 3; ++k) wrench(i, at + k) = one ? s.data[k] : s(i, k);
            }

            bool _use_stabilizer = false;
            std::map<std::string, StabilizerConfig> _stabilizer_configs;
            int _stab_window = 0;
            std::vector<unsigned char> _stab_state; // [batch][state bytes]: empty or all-zero = fresh filters
            std::vector<double> _stab_ref;
            VectorXi _stab_flags;
            MatrixXd _cop;
        };

        class TalosPosTracker : public HumanoidPosTracker {
        public:
            explicit TalosPosTracker(const yaml::Node& config) : HumanoidPosTracker(config)
            {
                parse_torque_safety(IWBC_CHECK(config["CONTROLLER"]));
                if (verbose_)
                    std::cout << "Talos pos tracker initialized (torque collision detection: " << _use_torque_collision_detection
                              << "; no torso roll clamp in this build)" << std::endl;
            }

            // talos_pos_tracker.cpp:125-158: the check comes BEFORE the tick's solve, so the torques compared are tau() as the previous tick
            // left it (zero before the first tick).  joints_torque: B x 22, or 22 numbers for every instance alike
            void update(const SensorData& sensor_data = {}) override
            {
                if (_use_torque_collision_detection) {
                    IWBC_ASSERT(sensor_data.find("joints_torque") != sensor_data.end(), "torque collision detection requires torque sensor data");
                    const MatrixXd& s = sensor_data.at("joints_torque");
                    const int B = batch_size(), n = (int)_torque_collision_joints.size();
                    IWBC_ASSERT((s.rows == B && s.cols == n) || (s.rows * s.cols == n && (int)s.data.size() == n),
                                "torque sensor data has a wrong size. call torque_sensor_joints() for needed values");
                    MatrixXd sensors(B, n);
                    for (int i = 0; i < B; ++i)
                        for (int j = 0; j < n; ++j) sensors(i, j) = (int)s.data.size() == n ? s.data[j] : s(i, j);
                    MatrixXd model = this->tau(); // slice_vec(tau(), ids) is the kernel's read of the columns `joint`
                    const int ldt = (int)all_dofs(true).size();
                    if (model.rows != B || model.cols != ldt) model = MatrixXd(B, ldt);
                    const wbcqp_torque_monitor mon = _torque_monitor();
                    const size_t bytes = (size_t)wbcqp_torque_monitor_state_bytes(&mon);
                    IWBC_ASSERT(bytes > 0, "torque collision detection: filter_size must be in [1, 64] and max_invalid in [0, 31]");
                    if (_torque_collision_state.size() != bytes * B) _torque_collision_state.assign(bytes * B, 0);
                    _collision_detected.assign(B, 0);
                    _torque_collision_invalid.assign(B, 0);
                    const wbcqp_torque_checks out = {_collision_detected.data(), _torque_collision_invalid.data(), nullptr, nullptr, nullptr, nullptr};
                    if (wbcqp_detect_torque_collisions_host(handle_, &mon, B, 1, model.data.data(), ldt, sensors.data.data(), _torque_collision_state.data(),
                                                            &out) != WBCQP_OK)
                        IWBC_ERROR("wbcqp_detect_torque_collisions_host failed: ", wbcqp_last_error(handle_));
                }
                HumanoidPosTracker::update(sensor_data);
            }

            // one flag per instance (the reference: one bool): the last check() returned false
            const VectorXi& collision_detected() const { return _collision_detected; }
            bool torque_collision_detection_activated() const { return _use_torque_collision_detection; }
            const std::vector<std::string>& torque_sensor_joints() const { return _torque_collision_joints; }
            const std::vector<int>& torque_collision_joints_ids() const { return _torque_collision_joints_ids; }
            const std::vector<double>& torque_collision_threshold() const { return _torque_collision_threshold; }
            // get_invalid_ids() of instance i's detector: positions in torque_sensor_joints()
            std::vector<int> torque_collision_invalid_ids(int i) const
            {
                std::vector<int> ids;
                if (i >= 0 && i < (int)_torque_collision_invalid.size())
                    for (int j = 0; j < (int)_torque_collision_joints.size(); ++j)
                        if ((_torque_collision_invalid[i] >> j) & 1) ids.push_back(j);
                return ids;
            }
            // talos_pos_tracker.cpp:153-158: detector and filter of every instance start afresh (all-zero state), the flags are lowered.
            // qp_step_back() does NOT rewind the detector: like the reference's, it has seen the samples it has seen.
            void clear_collision_detection()
            {
                std::fill(_torque_collision_state.begin(), _torque_collision_state.end(), 0);
                std::fill(_collision_detected.begin(), _collision_detected.end(), 0);
                std::fill(_torque_collision_invalid.begin(), _torque_collision_invalid.end(), 0);
            }

        protected:
            // talos_pos_tracker.cpp:62-123.  The reference requires the collision_detection block; here a missing block (or activated: false)
            // leaves a plain tick, as before
            void parse_torque_safety(const yaml::Node& config)
            {
                yaml::Node c = config["collision_detection"];
                if (!c || !c["activated"] || !c["activated"].as<bool>()) return;
                _torque_collision_filter_size = IWBC_CHECK(c["filter_size"].as<int>());
                _torque_collision_max_invalid = IWBC_CHECK(c["max_invalid"].as<int>());
                _torque_collision_joints = {
                    "leg_left_1_joint", "leg_left_2_joint", "leg_left_3_joint", "leg_left_4_joint", "leg_left_5_joint", "leg_left_6_joint",
                    "leg_right_1_joint", "leg_right_2_joint", "leg_right_3_joint", "leg_right_4_joint", "leg_right_5_joint", "leg_right_6_joint",
                    "torso_1_joint", "torso_2_joint",
                    "arm_left_1_joint", "arm_left_2_joint", "arm_left_3_joint", "arm_left_4_joint",
                    "arm_right_1_joint", "arm_right_2_joint", "arm_right_3_joint", "arm_right_4_joint"};
                const auto filtered_dof_names = this->all_dofs(true); // filter out mimics
                for (const auto& joint : _torque_collision_joints) {
                    auto it = std::find(filtered_dof_names.begin(), filtered_dof_names.end(), joint);
                    // (the reference takes the distance to end() for a joint it does not find; a model without the joint is refused here)
                    IWBC_ASSERT(it != filtered_dof_names.end(), "torque collision detection: the model has no joint ", joint, " (CONTROLLER.model)");
                    _torque_collision_joints_ids.push_back((int)std::distance(filtered_dof_names.begin(), it));
                }
                _torque_collision_threshold = {3.5e+05, 3.9e+05, 2.9e+05, 4.4e+05, 5.7e+05, 2.4e+05,
                                               3.5e+05, 3.9e+05, 2.9e+05, 4.4e+05, 5.7e+05, 2.4e+05,
                                               1e+01, 1e+01,
                                               1e+01, 1e+01, 1e+01, 1e+01,
                                               1e+01, 1e+01, 1e+01, 1e+01};
                // update thresholds from file (if any)
                if (c["thresholds"]) {
                    const auto file = c["thresholds"].as<std::string>();
                    parse_collision_thresholds(file.size() && file[0] == '/' ? file : base_path() + "/" + file);
                }
                const wbcqp_torque_monitor mon = _torque_monitor();
                IWBC_ASSERT(wbcqp_torque_monitor_state_bytes(&mon) > 0,
                            "torque collision detection: filter_size must be in [1, 64], max_invalid in [0, 31] and no threshold NaN");
                _use_torque_collision_detection = true;
            }
            void parse_collision_thresholds(const std::string& config_path)
            {
                yaml::Node config = IWBC_CHECK(yaml::LoadFile(config_path));
                for (size_t jid = 0; jid < _torque_collision_joints.size(); ++jid)
                    if (config[_torque_collision_joints[jid]]) _torque_collision_threshold[jid] = IWBC_CHECK(config[_torque_collision_joints[jid]].as<double>());
            }
            wbcqp_torque_monitor _torque_monitor() const
            {
                return wbcqp_torque_monitor{(int32_t)_torque_collision_joints.size(), _torque_collision_joints_ids.data(), _torque_collision_threshold.data(),
                                            nullptr, WBCQP_FILTER_MEAN, _torque_collision_filter_size, _torque_collision_max_invalid};
            }

            bool _use_torque_collision_detection = false;
            int _torque_collision_filter_size = 1, _torque_collision_max_invalid = 0;
            std::vector<std::string> _torque_collision_joints;
            std::vector<int> _torque_collision_joints_ids;
            std::vector<double> _torque_collision_threshold;
            std::vector<unsigned char> _torque_collision_state; // [batch][state bytes]: all-zero = a fresh detector
            VectorXi _collision_detected;
            std::vector<uint64_t> _torque_collision_invalid;
        };
    } // namespace controllers
} // namespace inria_wbc
#endif
