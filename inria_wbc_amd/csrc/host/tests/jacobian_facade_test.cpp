// Frame Jacobians, the CoM Jacobian and the centroidal momentum matrix through the facade: Controller::jacobian, Controller::jacobian_com and
// Controller::momentum_matrix (wbcqp_set_jacobian_frames and wbcqp_jacobians_host behind a model-driven problem source).
//   jacobian_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <n_ticks> <batch> <out.bin> <frame> <frame>
//       runs n_ticks of the behavior on `batch` instances, then writes q_tsid, jacobian(first frame) in WORLD, LOCAL and LOCAL_WORLD_ALIGNED,
//       jacobian(second frame, LOCAL), jacobian_com() and momentum_matrix() to out.bin (raw doubles, in this order) and prints what it checked
//       on the way.
//   jacobian_facade_test --file-source <controller.yaml> <batch.bin>
//       a controller on a FileSource must refuse (it has no model)
#include "model_query_facade.hpp"

using controllers::Controller;

static int file_source_mode(char** argv)
{
    auto controller = make_controller(argv[2], 0);
    controller->set_problem_source(std::make_shared<controllers::FileSource>(argv[3]));
    const int refused = refused_without_model([&] { controller->jacobian("base_link"); }, true) +
                        refused_without_model([&] { controller->jacobian("base_link", Controller::LOCAL); }) +
                        refused_without_model([&] { controller->jacobian_com(); }) + refused_without_model([&] { controller->momentum_matrix(); });
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
        const MatrixXd q = controller->q_tsid();
        IWBC_ASSERT(q.rows == B && q.cols == nq, "B states");
        // the default convention is WORLD, as the reference's RobotModel::jacobian has it
        const MatrixXd Jw = controller->jacobian(first), Jl = controller->jacobian(first, Controller::LOCAL),
                       Ja = controller->jacobian(first, Controller::LOCAL_WORLD_ALIGNED);
        const bool world_is_default = Jw.data == controller->jacobian(first, Controller::WORLD).data;
        // asked twice at one state: one matrix, kept
        const MatrixXd& Jcom1 = controller->jacobian_com();
        const MatrixXd Jcom = Jcom1, Ag = controller->momentum_matrix();
        const bool kept = &controller->jacobian_com() == &Jcom1 && controller->jacobian_com().data == Jcom.data && controller->momentum_matrix().data == Ag.data;
        // a second frame joins the selection; the first one's answer stays what it was
        const MatrixXd J2 = controller->jacobian(second, Controller::LOCAL);
        const bool first_stays = controller->jacobian(first, Controller::LOCAL).data == Jl.data && controller->jacobian(first).data == Jw.data;
        IWBC_ASSERT(Jw.rows == B && Jw.cols == 6 * nv && J2.cols == 6 * nv && Jcom.rows == B && Jcom.cols == 3 * nv && Ag.rows == B && Ag.cols == 6 * nv,
                    "B x 6*nv, B x 3*nv, B x 6*nv");
        // the angular rows of LOCAL_WORLD_ALIGNED are WORLD's; Jcom is Ag's linear rows over the mass: the same ratio everywhere
        double ang = 0.0, lo = 1e300, hi = 0.0;
        for (int i = 0; i < B; ++i) {
            for (int e = 3 * nv; e < 6 * nv; ++e) ang = std::max(ang, std::fabs(Ja(i, e) - Jw(i, e)));
            for (int e = 0; e < 3 * nv; ++e)
                if (std::fabs(Jcom(i, e)) > 1e-3) {
                    lo = std::min(lo, Ag(i, e) / Jcom(i, e));
                    hi = std::max(hi, Ag(i, e) / Jcom(i, e));
                }
        }
        bool unknown_refused = false;
        try { controller->jacobian("no_such_frame"); }
        catch (std::exception&) { unknown_refused = controller->jacobian(first).data == Jw.data; } // (and the selection is what it was)

        controller->qp_step_back();
        const bool refreshed = controller->jacobian(first).data != Jw.data && controller->momentum_matrix().data != Ag.data;

        std::ofstream f(argv[5], std::ios::binary);
        auto put = [&](const MatrixXd& m) { f.write(reinterpret_cast<const char*>(m.data.data()), (std::streamsize)(m.data.size() * sizeof(double))); };
        put(q); put(Jw); put(Jl); put(Ja); put(J2); put(Jcom); put(Ag);
        std::cout.precision(6);
        std::cout << "instances: " << B << std::endl;
        std::cout << "device calls: " << counting->calls() << std::endl;
        std::cout << "world is the default: " << world_is_default << std::endl;
        std::cout << "kept: " << kept << " refreshed after qp_step_back: " << refreshed << std::endl;
        std::cout << "a second frame leaves the first: " << first_stays << std::endl;
        std::cout << "an unknown frame is refused: " << unknown_refused << std::endl;
        std::cout << "max |angular rows, aligned - world|: " << ang << std::endl;
        std::cout << "Ag / Jcom between: " << lo << " " << hi << std::endl;
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
