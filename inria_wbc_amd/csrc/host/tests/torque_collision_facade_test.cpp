// Talos' torque-collision safety through the facade: TalosPosTracker with CONTROLLER.collision_detection.activated (the reference's
// talos_pos_tracker.cpp:62-158), wbcqp_detect_torque_collisions_host behind update().
//   torque_collision_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <thresholds.yaml> <n_ticks> <batch> <streams.txt>
//       runs n_ticks of the behavior on two controllers of `batch` instances: one with collision_detection on (filter_size 5, max_invalid 2, the
//       thresholds file), one without the block.  The sensors are the controller's own sliced tau(), except that instance kBad's arm_left_4_joint
//       reads kPush N m more from tick kFrom on; at tick kClear the detector is cleared.  Prints per tick the flags and invalid ids, how many
//       command rows of the other instances differ between the two controllers, and how the missing / mis-sized sensor is refused; writes the
//       two streams (model, sensors: one line per tick and instance, %.17g) for the test to run the reference's detector on.
//       Before the counted ticks one warm-up tick runs and the detector is cleared: tau() is zero before the first solve, as the reference's is,
//       so a window that starts there holds a zero beside the robot's real torques for filter_size - 1 ticks -- a mean off by up to tau / 2,
//       which latches every robot whose arm carries more than twice its threshold (Talos' arm_left_2_joint: 7 N m against 1 N m).
#include "model_query_facade.hpp"

#include <cstdio>
#include <cstring>

#include <inria_wbc/controllers/humanoid_pos_tracker.hpp>

static const int kBad = 5, kFrom = 20, kClear = 40;
static const double kPush = 3.0;

static std::shared_ptr<controllers::Controller> make_talos(const std::string& path, int batch, const std::string& thresholds, const char* activated)
{
    yaml::Node c_config = IWBC_CHECK(yaml::LoadFile(path));
    c_config["CONTROLLER"].set("base_path", path.substr(0, path.find_last_of('/')));
    c_config["CONTROLLER"].set("batch", std::to_string(batch));
    if (activated) {
        yaml::Node cd = yaml::Node::MakeMap();
        cd.set("activated", activated);
        cd.set("filter_size", "5");
        cd.set("max_invalid", "2");
        cd.set("thresholds", thresholds); // (absolute: taken as it is)
        c_config["CONTROLLER"].set("collision_detection", cd);
    }
    return controllers::Factory::instance().create("talos-pos-tracker", c_config);
}

static int rows_that_differ(const MatrixXd& a, const MatrixXd& b, int skip)
{
    if (a.rows != b.rows || a.cols != b.cols) return -1;
    int n = 0;
    for (int i = 0; i < a.rows; ++i)
        if (i != skip && std::memcmp(a.row(i), b.row(i), sizeof(double) * a.cols) != 0) ++n;
    return n;
}

template <typename F>
static std::string message_of(F&& f)
{
    try { f(); }
    catch (std::exception& e) { return e.what(); }
    return "(not refused)";
}

int main(int argc, char** argv)
{
    try {
        if (argc != 7) {
            std::cerr << "usage: " << argv[0] << " <controller.yaml> <behavior.yaml> <thresholds.yaml> <n_ticks> <batch> <streams.txt>" << std::endl;
            return 2;
        }
        const int n_ticks = std::atoi(argv[4]), batch = std::atoi(argv[5]);
        auto with = make_talos(argv[1], batch, argv[3], "true"), without = make_talos(argv[1], batch, argv[3], nullptr),
             off = make_talos(argv[1], batch, argv[3], "false");
        auto talos = std::dynamic_pointer_cast<controllers::TalosPosTracker>(with);
        IWBC_ASSERT(talos && talos->torque_collision_detection_activated(), "a talos-pos-tracker with the detection on");
        IWBC_ASSERT(!std::dynamic_pointer_cast<controllers::TalosPosTracker>(off)->torque_collision_detection_activated(), "activated: false");
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        const auto b_name = IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>());
        auto b_with = behaviors::Factory::instance().create(b_name, with, b_config), b_without = behaviors::Factory::instance().create(b_name, without, b_config),
             b_off = behaviors::Factory::instance().create(b_name, off, b_config);

        const auto& joints = talos->torque_sensor_joints();
        const auto& ids = talos->torque_collision_joints_ids();
        const int n = (int)joints.size(), B = with->batch_size();
        const auto dofs = with->all_dofs(true);
        std::cout << "instances: " << B << std::endl << "joints: " << n << std::endl << "ids:";
        bool ids_name_their_joints = true;
        for (int j = 0; j < n; ++j) {
            std::cout << " " << ids[j];
            ids_name_their_joints = ids_name_their_joints && dofs[ids[j]] == joints[j];
        }
        std::cout << std::endl << "ids name their joints: " << ids_name_their_joints << std::endl << "thresholds:";
        for (double t : talos->torque_collision_threshold()) std::cout << " " << t;
        std::cout << std::endl;
        const int arm4 = (int)std::distance(joints.begin(), std::find(joints.begin(), joints.end(), "arm_left_4_joint"));
        std::cout << "pushed: instance " << kBad << " joint " << arm4 << " by " << kPush << " from tick " << kFrom << ", cleared at tick " << kClear << std::endl;

        // refusals, before any tick: in the reference's words
        std::cout << "missing: " << message_of([&] { with->update(controllers::SensorData{}); }) << std::endl;
        controllers::SensorData wrong;
        wrong["joints_torque"] = MatrixXd(B, n + 1);
        std::cout << "mis-sized: " << message_of([&] { with->update(wrong); }) << std::endl;
        wrong["joints_torque"] = MatrixXd(1, n - 1);
        std::cout << "mis-sized: " << message_of([&] { with->update(wrong); }) << std::endl;

        // the warm-up tick (tau() is zero before it: so are its sensors), then every detector afresh
        {
            controllers::SensorData zero;
            zero["joints_torque"] = MatrixXd(1, n);
            b_with->update(zero);
            b_without->update(controllers::SensorData{});
            b_off->update(controllers::SensorData{});
            talos->clear_collision_detection();
        }
        FILE* streams = std::fopen(argv[6], "w");
        IWBC_ASSERT(streams, "cannot write ", argv[6]);
        int differing = 0;
        double tmax = 0.0;
        for (int it = 0; it < n_ticks; ++it) {
            if (it == kClear) {
                int before = 0, after = 0;
                for (int f : talos->collision_detected()) before += f;
                talos->clear_collision_detection();
                for (int f : talos->collision_detected()) after += f;
                std::cout << "cleared: " << before << " flags up before, " << after << " after" << std::endl;
            }
            // the sensors: tau() as the previous tick left it, sliced the reference's way
            const MatrixXd tau = with->tau();
            IWBC_ASSERT(tau.rows == B && tau.cols == (int)dofs.size(), "tau() is B x the non-mimic dofs");
            controllers::SensorData sensors;
            MatrixXd s(B, n);
            for (int i = 0; i < B; ++i) {
                for (int j = 0; j < n; ++j) {
                    s(i, j) = tau(i, ids[j]) + ((i == kBad && j == arm4 && it >= kFrom) ? kPush : 0.0);
                    tmax = std::max(tmax, std::fabs(tau(i, ids[j])));
                }
                std::fprintf(streams, "m");
                for (int j = 0; j < n; ++j) std::fprintf(streams, " %.17g", tau(i, ids[j]));
                std::fprintf(streams, "\ns");
                for (int j = 0; j < n; ++j) std::fprintf(streams, " %.17g", s(i, j));
                std::fprintf(streams, "\n");
            }
            sensors["joints_torque"] = s;
            b_with->update(sensors);
            b_without->update(controllers::SensorData{});
            if (it < 3) b_off->update(controllers::SensorData{}); // activated: false stays a plain tick: no sensors asked for
            std::cout << "tick " << it << " detected:";
            for (int f : talos->collision_detected()) std::cout << " " << f;
            std::cout << " invalid of " << kBad << ":";
            for (int j : talos->torque_collision_invalid_ids(kBad)) std::cout << " " << j;
            std::cout << std::endl;
            differing += std::abs(rows_that_differ(with->q(), without->q(), kBad)) + std::abs(rows_that_differ(with->tau(), without->tau(), kBad)) +
                         std::abs(rows_that_differ(with->dq(), without->dq(), kBad)) + std::abs(rows_that_differ(with->ddq(), without->ddq(), kBad));
            if (it == 2) differing += std::abs(rows_that_differ(off->q(), without->q(), -1)) + std::abs(rows_that_differ(off->tau(), without->tau(), -1));
        }
        std::fclose(streams);
        // 22 numbers for every instance alike are accepted
        controllers::SensorData alike;
        alike["joints_torque"] = MatrixXd(1, n);
        std::cout << "one row for all: " << message_of([&] { with->update(alike); }) << std::endl;
        std::cout << "max |tau| monitored: " << tmax << std::endl;
        std::cout << "command rows of the other instances that differ: " << differing << std::endl;
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
