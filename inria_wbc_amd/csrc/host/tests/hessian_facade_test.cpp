// The kinematic Hessians and the Jacobians' time variation through the facade: Controller::hessian and Controller::jacobian_time_variation
// (wbcqp_set_jacobian_frames and wbcqp_kinematic_hessians_host behind a model-driven problem source).
//   hessian_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <n_ticks> <batch> <out.bin> <frame> <frame>
//       runs n_ticks of the behavior on `batch` instances, then writes q_tsid, dq(false), hessian(first frame) in WORLD, LOCAL and
//       LOCAL_WORLD_ALIGNED, hessian(second frame, LOCAL), jacobian_time_variation(first frame) in the three conventions and
//       jacobian_time_variation(second frame, LOCAL) to out.bin (raw doubles, in this order) and prints what it checked on the way.
//   hessian_facade_test --file-source <controller.yaml> <batch.bin>
//       a controller on a FileSource must refuse (it has no model)
#include "model_query_facade.hpp"

using controllers::Controller;

static int file_source_mode(char** argv)
{
    auto controller = make_controller(argv[2], 0);
    controller->set_problem_source(std::make_shared<controllers::FileSource>(argv[3]));
    const int refused = refused_without_model([&] { controller->hessian("base_link"); }, true) +
                        refused_without_model([&] { controller->hessian("base_link", Controller::LOCAL); }) +
                        refused_without_model([&] { controller->jacobian_time_variation("base_link"); }) +
                        refused_without_model([&] { controller->jacobian_time_variation("base_link", Controller::LOCAL_WORLD_ALIGNED); });
    std::cout << "refused: " << refused << " of 4" << std::endl;
    return refused == 4 ? 0 : 1;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 4 && std::string(argv[1]) == "--file-source") return file_source_mode(argv);
        if (argc != 8) {
            std::cerr << "usage: " << argv[0] << " <controller.yaml> <behavior.yaml> <n_ticks> <batch> <out.bin> <frame> <frame>" << std::endl;
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
        const int B = controller->batch_size(), nq = robot.nq(), nv = robot.nv();
        const std::string first = argv[6], second = argv[7];
        const MatrixXd q = controller->q_tsid(), v = controller->dq(false);
        IWBC_ASSERT(q.rows == B && q.cols == nq && v.rows == B && v.cols == nv, "B states");
        // the default convention is WORLD, as the reference's RobotModel::hessian has it
        const MatrixXd Hw = controller->hessian(first), Hl = controller->hessian(first, Controller::LOCAL),
                       Ha = controller->hessian(first, Controller::LOCAL_WORLD_ALIGNED);
        const bool world_is_default = Hw.data == controller->hessian(first, Controller::WORLD).data;
        const MatrixXd Dw = controller->jacobian_time_variation(first), Dl = controller->jacobian_time_variation(first, Controller::LOCAL),
                       Da = controller->jacobian_time_variation(first, Controller::LOCAL_WORLD_ALIGNED);
        // a second frame joins the selection (the Jacobians' own); the first one's answers stay what they were, the Jacobian's too
        const MatrixXd Jl = controller->jacobian(first, Controller::LOCAL);
        const MatrixXd H2 = controller->hessian(second, Controller::LOCAL), D2 = controller->jacobian_time_variation(second, Controller::LOCAL);
        const bool first_stays = controller->hessian(first, Controller::LOCAL).data == Hl.data && controller->hessian(first).data == Hw.data &&
                                 controller->jacobian_time_variation(first).data == Dw.data && controller->jacobian(first, Controller::LOCAL).data == Jl.data;
        IWBC_ASSERT(Hw.rows == B && Hw.cols == 6 * nv * nv && H2.cols == 6 * nv * nv && Dw.rows == B && Dw.cols == 6 * nv && D2.cols == 6 * nv,
                    "B x 6*nv*nv, B x 6*nv");
        // dJ is H contracted with v: [6][nv][nv] against the row of v
        double gap = 0.0, big = 0.0;
        for (int i = 0; i < B; ++i)
            for (int rj = 0; rj < 6 * nv; ++rj) {
                double s = 0.0;
                for (int k = 0; k < nv; ++k) s += Hl(i, rj * nv + k) * v(i, k);
                gap = std::max(gap, std::fabs(s - Dl(i, rj)));
                big = std::max(big, std::fabs(Dl(i, rj)));
            }
        bool unknown_refused = false;
        try { controller->hessian("no_such_frame"); }
        catch (std::exception&) { unknown_refused = controller->hessian(first).data == Hw.data; } // (and the selection is what it was)

        controller->qp_step_back();
        const bool refreshed = controller->hessian(first).data != Hw.data && controller->jacobian_time_variation(first).data != Dw.data;

        std::ofstream f(argv[5], std::ios::binary);
        auto put = [&](const MatrixXd& m) { f.write(reinterpret_cast<const char*>(m.data.data()), (std::streamsize)(m.data.size() * sizeof(double))); };
        put(q); put(v); put(Hw); put(Hl); put(Ha); put(H2); put(Dw); put(Dl); put(Da); put(D2);
        std::cout.precision(6);
        std::cout << "instances: " << B << std::endl;
        std::cout << "device calls: " << counting->calls() << std::endl;
        std::cout << "world is the default: " << world_is_default << std::endl;
        std::cout << "refreshed after qp_step_back: " << refreshed << std::endl;
        std::cout << "a second frame leaves the first: " << first_stays << std::endl;
        std::cout << "an unknown frame is refused: " << unknown_refused << std::endl;
        std::cout << "max |H v - dJ|: " << gap << std::endl;
        std::cout << "max |dJ|: " << big << std::endl;
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
