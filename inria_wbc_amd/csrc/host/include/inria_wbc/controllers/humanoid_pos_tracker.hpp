// "humanoid-pos-tracker" and "talos-pos-tracker" (/root/reference/src/controllers/humanoid_pos_tracker.cpp:35,
// /root/reference/src/controllers/talos_pos_tracker.cpp:35): the registration names and constructor signature of the
// reference's two humanoid controllers, so that a configuration file that names them loads here.  HumanoidPosTracker's
// update() is the plain PosTracker tick: what the reference adds around it -- the stabiliser (CoM / ankle / ZMP admittance on
// force-torque and IMU data, humanoid_pos_tracker.cpp:133-260), the CoP estimator and its filters -- is host-side signal
// processing outside the hot path (OUT OF SCOPE) and is NOT built; a configuration that switches the
// stabiliser on is refused with a message that says so.  TalosPosTracker adds the torque-collision safety
// (talos_pos_tracker.cpp:62-158) for every instance of the batch: before a tick's solve the measured joint torques are
// compared with tau() as the previous tick left it, through wbcqp_detect_torque_collisions_host (a moving average over
// filter_size samples, max_invalid + 1 consecutive same-signed violations).  The torso-roll clamp of its constructor is not built.
#ifndef IWBC_HIP_HUMANOID_POS_TRACKER_HPP
#define IWBC_HIP_HUMANOID_POS_TRACKER_HPP

#include <inria_wbc/controllers/pos_tracker.hpp>

namespace inria_wbc {
    namespace controllers {
        class HumanoidPosTracker : public PosTracker {
        public:
            explicit HumanoidPosTracker(const yaml::Node& config) : PosTracker(config)
            {
                behavior_type_ = behavior_types::FIXED_BASE; // humanoid_pos_tracker.cpp:39
                yaml::Node c = IWBC_CHECK(config["CONTROLLER"]);
                if (c["stabilizer"] && c["stabilizer"]["activated"] && c["stabilizer"]["activated"].as<bool>())
                    IWBC_ERROR("humanoid-pos-tracker: stabilizer.activated is true, but the stabilizer (CoM / ankle / ZMP admittance, CoP "
                               "estimator, sensor filters) is outside the batched hot path and is not part of this build; set "
                               "stabilizer.activated: false");
                if (verbose_) std::cout << "Humanoid pos tracker initialized (plain tick: no stabilizer in this build)" << std::endl;
            }
            // the reference accepts FIXED_BASE / SINGLE_SUPPORT / DOUBLE_SUPPORT only (humanoid_pos_tracker.cpp:116-131)
            void set_behavior_type(const std::string& bt) override
            {
                if (bt != behavior_types::FIXED_BASE && bt != behavior_types::SINGLE_SUPPORT && bt != behavior_types::DOUBLE_SUPPORT)
                    IWBC_ERROR("_stabilizer_configs does not have ", bt);
                Controller::set_behavior_type(bt);
            }
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
