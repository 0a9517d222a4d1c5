// M(q), forward dynamics and the stable-PD commands through the facade: Controller::inertia_matrix, Controller::forward_dynamics and
// robots::compute_spd (wbcqp_mass_matrix_host, wbcqp_forward_dynamics_host, wbcqp_spd_commands_host behind a model-driven problem source).
//   forward_dynamics_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <n_ticks> <batch> <out.bin>
//       runs n_ticks of the behavior on `batch` instances, then writes q_tsid, dq, inertia_matrix(), a target, compute_spd's commands for it,
//       tau() and forward_dynamics(tau()) to out.bin (raw doubles, in this order) and prints what it checked on the way.
//   forward_dynamics_facade_test --file-source <controller.yaml> <batch.bin>
//       a controller on a FileSource must refuse (it has no model)
#include "model_query_facade.hpp"

#include <inria_wbc/robots/cmd.hpp>

static int file_source_mode(char** argv)
{
    auto controller = make_controller(argv[2], 0);
    controller->set_problem_source(std::make_shared<controllers::FileSource>(argv[3]));
    const int B = controller->batch_size();
    const MatrixXd q(B, 1), dq(B, 1); // (a source without a model refuses before it looks at a shape)
    const int refused = refused_without_model([&] { controller->inertia_matrix(); }) +
                        refused_without_model([&] { controller->forward_dynamics(dq); }) +
                        refused_without_model([&] { robots::compute_spd(controller, q, dq, dq, 0.001); });
    std::cout << "refused: " << refused << " of 3" << std::endl;
    return refused == 3 ? 0 : 1;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 4 && std::string(argv[1]) == "--file-source") return file_source_mode(argv);
        if (argc != 6) {
            std::cerr << "usage: " << argv[0] << " <controller.yaml> <behavior.yaml> <n_ticks> <batch> <out.bin>" << std::endl;
            return 2;
        }
        auto controller = make_controller(argv[1], std::atoi(argv[4]));
        auto pt = std::dynamic_pointer_cast<controllers::PosTracker>(controller);
        IWBC_ASSERT(pt && pt->robot(), "the controller must be a PosTracker with a model");
        auto counting = count_device_calls(controller, argv[1]);
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        auto behavior = behaviors::Factory::instance().create(IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>()), controller, b_config);
        const int n_ticks = std::atoi(argv[3]);
        for (int it = 0; it < n_ticks; ++it) behavior->update(controllers::SensorData{});

        const auto& robot = *pt->robot();
        const int B = controller->batch_size(), nq = robot.nq(), nv = robot.nv(), na = robot.na();
        const MatrixXd q = controller->q_tsid(), dq = controller->dq(false);
        IWBC_ASSERT(q.rows == B && q.cols == nq && dq.rows == B && dq.cols == nv, "B states");
        // asked twice at one state: one matrix, kept; after a step back: the matrix of the restored state
        const MatrixXd& M1 = controller->inertia_matrix();
        const MatrixXd M = M1;
        const bool kept = &controller->inertia_matrix() == &M1 && controller->inertia_matrix().data == M.data;
        IWBC_ASSERT(M.rows == B && M.cols == nv * nv, "B x nv*nv");
        double asym = 0.0, diag_min = 1e300;
        for (int i = 0; i < B; ++i)
            for (int r = 0; r < nv; ++r) {
                diag_min = std::min(diag_min, M(i, r * nv + r));
                for (int c = 0; c < nv; ++c) asym = std::max(asym, std::fabs(M(i, r * nv + c) - M(i, c * nv + r)));
            }
        // a target a little away from where the joints are; the reference's layout (nv entries, the base's six in front) and the short one
        MatrixXd target(B, na), target_nv(B, nv);
        for (int i = 0; i < B; ++i)
            for (int j = 0; j < na; ++j) target_nv(i, nv - na + j) = target(i, j) = q(i, nq - na + j) + 0.01 * ((i + j) % 7 - 3);
        const double dt = 0.001;
        const MatrixXd cmd = robots::compute_spd(controller, q, dq, target, dt), cmd_nv = robots::compute_spd(controller, q, dq, target_nv, dt);
        IWBC_ASSERT(cmd.rows == B && cmd.cols == nv, "B x nv commands");
        double base = 0.0, cmax = 0.0;
        for (int i = 0; i < B; ++i)
            for (int j = 0; j < nv; ++j) (j < nv - na ? base : cmax) = std::max(j < nv - na ? base : cmax, std::fabs(cmd(i, j)));
        const MatrixXd vel = robots::compute_velocities(target, target, dt);
        double vmax = 0.0;
        for (double x : vel.data) vmax = std::max(vmax, std::fabs(x));
        const MatrixXd tau = controller->tau(false);
        controllers::VectorXi info;
        const MatrixXd a = controller->forward_dynamics(tau, &info);
        int bad = 0;
        for (int f : info) bad += f != 0;

        controller->qp_step_back();
        const bool refreshed = controller->inertia_matrix().data != M.data;

        std::ofstream f(argv[5], std::ios::binary);
        auto put = [&](const MatrixXd& m) { f.write(reinterpret_cast<const char*>(m.data.data()), (std::streamsize)(m.data.size() * sizeof(double))); };
        put(q); put(dq); put(M); put(target); put(cmd); put(tau); put(a);
        std::cout.precision(4);
        std::cout << "instances: " << B << std::endl;
        std::cout << "device calls: " << counting->calls() << std::endl;
        std::cout << "kept: " << kept << " refreshed after qp_step_back: " << refreshed << std::endl;
        std::cout << "max |M - M'|: " << asym << std::endl;
        std::cout << "min M(j, j): " << diag_min << std::endl;
        std::cout << "max |commands| on the base rows: " << base << std::endl;
        std::cout << "max |commands| on the actuated rows: " << cmax << std::endl;
        std::cout << "commands for nv-wide targets equal: " << (cmd.data == cmd_nv.data) << std::endl;
        std::cout << "max |compute_velocities(target, target)|: " << vmax << std::endl;
        std::cout << "forward dynamics failed instances: " << bad << std::endl;
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
