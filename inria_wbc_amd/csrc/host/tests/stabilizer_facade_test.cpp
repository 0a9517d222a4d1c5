// The stabiliser through the facade: HumanoidPosTracker with CONTROLLER.stabilizer.activated (the reference's humanoid_pos_tracker.cpp:41-302),
// wbcqp_observe_acom_host and wbcqp_stabilize_host behind update().
//   stabilizer_facade_test <pos_tracker_stab.yaml> <behavior.yaml> <n_ticks> <batch> <dump.txt>
//       runs n_ticks of the behavior in DOUBLE_SUPPORT on two controllers of `batch` instances, one with the stabiliser and one with
//       stabilizer.activated: false, each on a model source of the program's own (so that the stored references can be read).  The sensors are
//       synthetic and differ per instance and tick.  Per tick and instance the dump holds what the test needs to run the transcription of the
//       reference on the same inputs: the state the stabiliser must have observed (the one the PREVIOUS tick started from; on the first tick the
//       constructor's), the sensors, the previous solution's foot forces, the stored references, the references the tick read, the flags and cop().
//       Prints how the missing sensors are refused, that three numbers serve every instance, that the stored references equal the unstabilised
//       controller's in every bit, and the message raised for the one instance whose ground force is absurd.
//   n_ticks == 0: only constructs the controller and sets DOUBLE_SUPPORT (a refused configuration ends with its message and status 1).
#include "model_query_facade.hpp"

#include <cstdio>
#include <cstring>

#include <inria_wbc/controllers/humanoid_pos_tracker.hpp>

static const int kHeavy = 2; // the instance whose ground force fails the reference's check at the end

static std::shared_ptr<controllers::Controller> make_humanoid(const std::string& path, int batch, bool stabilised)
{
    yaml::Node c_config = IWBC_CHECK(yaml::LoadFile(path));
    c_config["CONTROLLER"].set("base_path", path.substr(0, path.find_last_of('/')));
    c_config["CONTROLLER"].set("batch", std::to_string(batch));
    if (!stabilised) {
        yaml::Node off = yaml::Node::MakeMap();
        off.set("activated", "false");
        c_config["CONTROLLER"].set("stabilizer", off);
    }
    return controllers::Factory::instance().create("humanoid-pos-tracker", c_config);
}

template <typename F>
static std::string message_of(F&& f)
{
    try { f(); }
    catch (std::exception& e) { return e.what(); }
    return "(not refused)";
}

static void put(FILE* f, const char* tag, const double* p, int n)
{
    std::fprintf(f, "%s", tag);
    for (int k = 0; k < n; ++k) std::fprintf(f, " %.17g", p[k]);
    std::fprintf(f, "\n");
}

// lf_force, rf_force, lf_torque, rf_torque (B x 3) of tick t: both feet loaded, each instance's CoP somewhere else and drifting
static controllers::SensorData sensors_of(int B, int t)
{
    controllers::SensorData s;
    MatrixXd lf(B, 3), rf(B, 3), lt(B, 3), rt(B, 3);
    for (int i = 0; i < B; ++i) {
        lf(i, 0) = 3.0 + i; lf(i, 1) = -2.0; lf(i, 2) = 450.0 + 10.0 * i + 0.5 * t;
        rf(i, 0) = -4.0; rf(i, 1) = 1.0 + 0.5 * i; rf(i, 2) = 430.0 - 5.0 * i;
        lt(i, 0) = 2.0 + 0.5 * i; lt(i, 1) = -3.0 + 0.2 * t; lt(i, 2) = 0.1;
        rt(i, 0) = -1.0; rt(i, 1) = 1.5 + 0.1 * i - 0.1 * t; rt(i, 2) = 0.0;
    }
    s["lf_force"] = lf; s["rf_force"] = rf; s["lf_torque"] = lt; s["rf_torque"] = rt;
    s["imu_vel"] = MatrixXd(1, 3);
    return s;
}

int main(int argc, char** argv)
{
    try {
        if (argc != 6) {
            std::cerr << "usage: " << argv[0] << " <pos_tracker_stab.yaml> <behavior.yaml> <n_ticks> <batch> <dump.txt>" << std::endl;
            return 2;
        }
        const int n_ticks = std::atoi(argv[3]), batch = std::atoi(argv[4]);
        auto with = make_humanoid(argv[1], batch, true);
        auto hum = std::dynamic_pointer_cast<controllers::HumanoidPosTracker>(with);
        IWBC_ASSERT(hum && hum->stabilizer_activated(), "a humanoid-pos-tracker with the stabiliser on");
        with->set_behavior_type(controllers::behavior_types::DOUBLE_SUPPORT);
        if (n_ticks == 0) {
            std::cout << "constructed" << std::endl;
            return 0;
        }
        auto without = make_humanoid(argv[1], batch, false);
        IWBC_ASSERT(!std::dynamic_pointer_cast<controllers::HumanoidPosTracker>(without)->stabilizer_activated(), "activated: false");
        auto src_with = make_source<controllers::ModelSource>(*hum, argv[1]);
        auto src_without = make_source<controllers::ModelSource>(*std::dynamic_pointer_cast<controllers::PosTracker>(without), argv[1]);
        with->set_problem_source(src_with);
        without->set_problem_source(src_without);
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        const auto b_name = IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>());
        auto b_with = behaviors::Factory::instance().create(b_name, with, b_config), b_without = behaviors::Factory::instance().create(b_name, without, b_config);
        with->set_behavior_type(controllers::behavior_types::DOUBLE_SUPPORT);
        without->set_behavior_type(controllers::behavior_types::DOUBLE_SUPPORT);
        const int B = with->batch_size(), nref = src_with->nref();
        std::cout << "instances: " << B << std::endl << "nref: " << nref << std::endl;

        // refusals, before any tick: in the reference's words
        for (const char* key : {"lf_force", "rf_force", "lf_torque", "rf_torque", "imu_vel"}) {
            auto s = sensors_of(B, 0);
            s.erase(key);
            std::cout << "missing " << key << ": " << message_of([&] { with->update(s); }) << std::endl;
        }
        {
            auto s = sensors_of(B, 0);
            s["lf_force"] = MatrixXd(B + 1, 3);
            std::cout << "mis-sized: " << message_of([&] { with->update(s); }) << std::endl;
        }
        std::cout << "cop before the first tick: " << hum->cop().rows << " rows" << std::endl;

        FILE* dump = std::fopen(argv[5], "w");
        IWBC_ASSERT(dump, "cannot write ", argv[5]);
        MatrixXd q_lag = with->q_tsid(), v_lag = with->dq(false); // the constructor's state
        long moved = 0;
        for (int it = 0; it < n_ticks; ++it) {
            const MatrixXd q_now = with->q_tsid(), v_now = with->dq(false);
            const auto forces = with->activated_contacts_forces();
            const auto s = sensors_of(B, it);
            b_with->update(s);
            b_without->update(controllers::SensorData{}); // a plain tick: no sensors asked for
            const auto& stored = src_with->references();
            const auto& plain = src_without->references();
            moved += std::memcmp(stored.data(), plain.data(), sizeof(double) * stored.size()) != 0;
            for (int i = 0; i < B; ++i) {
                put(dump, "q", q_lag.row(i), q_lag.cols);
                put(dump, "v", v_lag.row(i), v_lag.cols);
                double w[12];
                for (int k = 0; k < 3; ++k) {
                    w[k] = s.at("lf_force")(i, k); w[3 + k] = s.at("lf_torque")(i, k);
                    w[6 + k] = s.at("rf_force")(i, k); w[9 + k] = s.at("rf_torque")(i, k);
                }
                put(dump, "w", w, 12);
                if (forces.count("contact_lfoot") && forces.count("contact_rfoot")) {
                    double x[24];
                    std::copy(forces.at("contact_lfoot").row(i), forces.at("contact_lfoot").row(i) + 12, x);
                    std::copy(forces.at("contact_rfoot").row(i), forces.at("contact_rfoot").row(i) + 12, x + 12);
                    put(dump, "x", x, 24);
                }
                else
                    put(dump, "x", nullptr, 0);
                put(dump, "s", stored.data() + (size_t)i * nref, nref);
                put(dump, "r", hum->stabilized_references().data() + (size_t)i * nref, nref);
                const double f[3] = {(double)hum->stabilizer_flags()[i], hum->cop()(i, 0), hum->cop()(i, 1)};
                put(dump, "f", f, 3);
            }
            q_lag = q_now; // what this tick started from is what the next tick's stabiliser observes
            v_lag = v_now;
        }
        std::fclose(dump);
        std::cout << "ticks where the stored references differ from the unstabilised controller's: " << moved << std::endl;
        int differ = 0;
        const MatrixXd qa = with->q(), qb = without->q();
        for (int i = 0; i < B; ++i) differ += std::memcmp(qa.row(i), qb.row(i), sizeof(double) * qa.cols) != 0;
        std::cout << "instances whose commands differ from the unstabilised controller's: " << differ << std::endl;

        // three numbers serve every instance
        {
            auto s = sensors_of(B, n_ticks);
            for (const char* key : {"lf_force", "rf_force", "lf_torque", "rf_torque"}) {
                MatrixXd one(1, 3);
                std::copy(s[key].row(0), s[key].row(0) + 3, one.row(0));
                s[key] = one;
            }
            std::cout << "three numbers for all: " << message_of([&] { with->update(s); }) << std::endl;
            int same = 0;
            for (int i = 1; i < B; ++i) same += hum->stabilizer_flags()[i] == hum->stabilizer_flags()[0];
            std::cout << "instances with instance 0's flags: " << same + 1 << std::endl;
        }
        // an absurd ground force on one instance: the reference's message with the instance; the tick is not solved, the filters have advanced
        {
            const double t_before = with->t();
            std::string msg;
            for (int k = 0; k < 10 && msg.empty(); ++k) { // (the force filter averages: a window's worth of samples at the most)
                auto s = sensors_of(B, n_ticks + 1 + k);
                s["lf_force"](kHeavy, 2) = 1e6;
                const std::string m = message_of([&] { with->update(s); });
                if (m != "(not refused)") msg = m;
            }
            std::cout << "absurd force: " << msg << std::endl;
            std::cout << "error bits:";
            for (int f : hum->stabilizer_flags()) std::cout << " " << ((f & WBCQP_STAB_ERR_FORCE) ? 1 : 0);
            std::cout << std::endl << "ticks solved meanwhile: " << (int)std::lround((with->t() - t_before) / with->dt()) << " of the calls before the raise" << std::endl;
        }
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
