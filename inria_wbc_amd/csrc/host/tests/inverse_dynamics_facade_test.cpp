// The model-side torques through the facade: Controller::rnea_double_support (wbcqp_inverse_dynamics_host behind a model-driven problem source).
//   inverse_dynamics_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <n_ticks> <batch>
//       runs n_ticks of the behavior on `batch` instances, steps back to the state the last tick started from (its ddq and contact forces belong
//       to that state), and feeds the QP's own contact wrenches T_c f_c back as the foot sensors: the answer must be zero on the base rows and
//       tau() on the actuated rows.  Then the foot-mass correction against the same correction made here from RobotWrapper::framePosition, and
//       a sensor map with a key missing.  Prints the deviations.
//   inverse_dynamics_facade_test --file-source <controller.yaml> <batch.bin>
//       a controller on a FileSource must refuse (it has no model)
#include "model_query_facade.hpp"

static const char* kLeft = "leg_left_6_joint";
static const char* kRight = "leg_right_6_joint";
static const char* kLeftSole = "left_sole_under_test";
static const char* kRightSole = "right_sole_under_test";

static controllers::SensorData zero_sensors()
{
    controllers::SensorData s;
    for (const char* k : {"lf_force", "rf_force", "lf_torque", "rf_torque"}) s[k] = MatrixXd(1, 3);
    return s;
}

static int file_source_mode(char** argv)
{
    auto controller = make_controller(argv[2], 0);
    controller->set_problem_source(std::make_shared<controllers::FileSource>(argv[3]));
    const int refused = refused_without_model([&] { controller->rnea_double_support(zero_sensors(), false, kLeft, kRight, kLeftSole, kRightSole); }) +
                        refused_without_model([&] { controller->rnea_double_support(zero_sensors(), true, kLeft, kRight, kLeftSole, kRightSole); });
    std::cout << "refused: " << refused << " of 2" << std::endl;
    return refused == 2 ? 0 : 1;
}

static double max_abs_diff(const MatrixXd& a, const MatrixXd& b)
{
    double d = 0.0;
    for (size_t i = 0; i < a.data.size(); ++i) d = std::max(d, std::fabs(a.data[i] - b.data[i]));
    return a.data.size() == b.data.size() ? d : 1e300;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 4 && std::string(argv[1]) == "--file-source") return file_source_mode(argv);
        if (argc != 5) {
            std::cerr << "usage: " << argv[0] << " <controller.yaml> <behavior.yaml> <n_ticks> <batch>" << std::endl;
            return 2;
        }
        auto controller = make_controller(argv[1], std::atoi(argv[4]));
        auto pt = std::dynamic_pointer_cast<controllers::PosTracker>(controller);
        IWBC_ASSERT(pt && pt->robot(), "the controller must be a PosTracker with a model");
        // two sole frames under the ankles (the reference's robots carry them in their URDF), then a source that uploads the model with them
        pt->robot()->addFrame(kLeftSole, kLeft, {{0.01, 0.0, -0.107}});
        pt->robot()->addFrame(kRightSole, kRight, {{0.01, 0.0, -0.107}});
        auto source = make_source<controllers::ModelSource>(*pt, argv[1]);
        controller->set_problem_source(source);
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        auto behavior = behaviors::Factory::instance().create(IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>()), controller, b_config);
        const int n_ticks = std::atoi(argv[3]);
        for (int it = 0; it < n_ticks; ++it) behavior->update(controllers::SensorData{});
        controller->qp_step_back(); // the last tick's ddq, tau and contact forces belong to the state it started from

        const auto& robot = *pt->robot();
        const int B = controller->batch_size(), nv = robot.nv(), na = robot.na();
        // the QP's own contact wrenches as the sensors: w_c = T_c f_c, in the contact frame's own axes, linear first
        const auto& stack = pt->stack();
        const wbcqp_structure cs = stack.c_struct();
        controllers::SensorData sensors;
        double wmax = 0.0;
        for (size_t c = 0; c < stack.contacts().size(); ++c) {
            const auto& spec = stack.contacts()[c];
            const bool left = spec.joint == kLeft;
            IWBC_ASSERT(left || spec.joint == kRight, "a contact on neither foot: ", spec.joint);
            const MatrixXd& f = controller->activated_contacts_forces().at(spec.name);
            MatrixXd force(B, 3), torque(B, 3);
            for (int i = 0; i < B; ++i)
                for (int r = 0; r < 6; ++r) {
                    double s = 0.0;
                    for (int k = 0; k < 12; ++k) s += cs.force_gen[(c * 6 + r) * 12 + k] * f(i, k);
                    (r < 3 ? force(i, r) : torque(i, r - 3)) = s;
                    wmax = std::max(wmax, std::fabs(s));
                }
            sensors[left ? "lf_force" : "rf_force"] = force;
            sensors[left ? "lf_torque" : "rf_torque"] = torque;
        }
        const MatrixXd tau_id = controller->rnea_double_support(sensors, false, kLeft, kRight, kLeftSole, kRightSole);
        const MatrixXd tau = controller->tau(false);
        IWBC_ASSERT(tau_id.rows == B && tau_id.cols == nv && tau.rows == B && tau.cols == nv, "B x nv torques");
        double base = 0.0, act = 0.0, tmax = 0.0;
        for (int i = 0; i < B; ++i)
            for (int j = 0; j < nv; ++j) {
                if (j < nv - na) base = std::max(base, std::fabs(tau_id(i, j)));
                else act = std::max(act, std::fabs(tau_id(i, j) - tau(i, j)));
                tmax = std::max(tmax, std::fabs(tau(i, j)));
            }
        // without the wrenches the base rows carry the robot's weight: the sensors count
        const MatrixXd bare = controller->rnea_double_support(zero_sensors(), false, kLeft, kRight, kLeftSole, kRightSole);
        double bare_base = 0.0;
        for (int i = 0; i < B; ++i)
            for (int j = 0; j < nv - na; ++j) bare_base = std::max(bare_base, std::fabs(bare(i, j)));

        // add_foot_mass = true against the same correction made here, applied at the sole frames with add_foot_mass = false
        const MatrixXd with_mass = controller->rnea_double_support(sensors, true, kLeft, kRight, kLeftSole, kRightSole);
        controllers::SensorData adjusted = sensors;
        const wbcqp_model md = robot.c_model();
        const auto& q = controller->q_tsid();
        for (int side = 0; side < 2; ++side) {
            const int ft = robot.getFrameId(side ? kRight : kLeft), sole = robot.getFrameId(side ? kRightSole : kLeftSole);
            const float mass = (float)md.inertia[10 * md.frame_body[ft]];
            MatrixXd& F = adjusted[side ? "rf_force" : "lf_force"];
            MatrixXd& T = adjusted[side ? "rf_torque" : "lf_torque"];
            for (int i = 0; i < B; ++i) {
                const auto ankle = robot.framePosition(q.row(i), ft).p; // (the joint's own frame: its placement on the body is the identity)
                const auto s = robot.framePosition(q.row(i), sole).p;
                for (int d = 0; d < 3; ++d) F(i, d) -= mass * md.gravity[d];
                const double r[3] = {ankle[0] - s[0], ankle[1] - s[1], ankle[2] - s[2]};
                T(i, 0) += r[1] * F(i, 2) - r[2] * F(i, 1);
                T(i, 1) += r[2] * F(i, 0) - r[0] * F(i, 2);
                T(i, 2) += r[0] * F(i, 1) - r[1] * F(i, 0);
            }
        }
        const MatrixXd by_hand = controller->rnea_double_support(adjusted, false, kLeftSole, kRightSole, kLeftSole, kRightSole);
        const double dmass = max_abs_diff(with_mass, by_hand), mass_counts = max_abs_diff(with_mass, tau_id);

        // a sensor key missing: refused in the reference's words
        controllers::SensorData three = sensors;
        three.erase("rf_torque");
        bool missing_refused = false;
        try { controller->rnea_double_support(three, false, kLeft, kRight, kLeftSole, kRightSole); }
        catch (std::exception& e) { missing_refused = std::string(e.what()).find("when FT is missing in fext_map") != std::string::npos; }
        bool unknown_refused = false;
        try { controller->rnea_double_support(sensors, true, "no_such_frame", kRight, kLeftSole, kRightSole); }
        catch (std::exception&) { unknown_refused = true; }

        std::cout.precision(4);
        std::cout << "instances: " << B << std::endl;
        std::cout << "max |contact wrench|: " << wmax << std::endl;
        std::cout << "max |tau|: " << tmax << std::endl;
        std::cout << "max |rnea_double_support| on the base rows: " << base << std::endl;
        std::cout << "max |rnea_double_support - tau()| on the actuated rows: " << act << std::endl;
        std::cout << "max |base rows| without the wrenches: " << bare_base << std::endl;
        std::cout << "max |add_foot_mass - the correction by hand at the sole frames|: " << dmass << std::endl;
        std::cout << "max |add_foot_mass - without|: " << mass_counts << std::endl;
        std::cout << "missing key refused: " << missing_refused << " unknown frame refused: " << unknown_refused << std::endl;
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
