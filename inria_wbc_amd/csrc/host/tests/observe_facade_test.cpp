// Where the robots are, through the facade: Controller::com_now / model_frame_pos / model_frame_vel (wbcqp_observe_host behind a model-driven
// problem source) against the host's own forward kinematics (robots::RobotWrapper), after a few ticks of a behavior.
//   observe_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <n_ticks> <batch> <out.bin> <frame> [frame ...]
//       runs n_ticks of the behavior on `batch` instances, prints the largest deviations and writes, as doubles: q (B x nq), dq (B x nv),
//       com_now pos and vel (B x 3 each), then per frame model_frame_pos (B x 12) and model_frame_vel (B x 6)
//   observe_facade_test --file-source <controller.yaml> <batch.bin>
//       a controller on a FileSource must refuse the three accessors (it has no model)
#include "model_query_facade.hpp"

static int file_source_mode(char** argv)
{
    auto controller = make_controller(argv[2], 0);
    controller->set_problem_source(std::make_shared<controllers::FileSource>(argv[3]));
    controllers::MatrixXd a, b;
    const int refused = refused_without_model([&] { controller->com_now(a, b); }) + refused_without_model([&] { controller->model_frame_pos("leg_left_6_joint"); }) +
                        refused_without_model([&] { controller->model_frame_vel("leg_left_6_joint"); });
    std::cout << "refused: " << refused << " of 3" << std::endl;
    return refused == 3 ? 0 : 1;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 4 && std::string(argv[1]) == "--file-source") return file_source_mode(argv);
        if (argc < 7) {
            std::cerr << "usage: " << argv[0] << " <controller.yaml> <behavior.yaml> <n_ticks> <batch> <out.bin> <frame> [frame ...]" << std::endl;
            return 2;
        }
        auto controller = make_controller(argv[1], std::atoi(argv[4]));
        auto pt = std::dynamic_pointer_cast<controllers::PosTracker>(controller);
        IWBC_ASSERT(pt && pt->robot(), "the controller must be a PosTracker with a model");
        auto counting = make_source<CountingSource>(*pt, argv[1]);
        controller->set_problem_source(counting);
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        auto behavior = behaviors::Factory::instance().create(IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>()), controller, b_config);
        const int n_ticks = std::atoi(argv[3]);
        for (int it = 0; it < n_ticks; ++it) behavior->update(controllers::SensorData{});

        const auto& robot = *pt->robot();
        const auto& q = controller->q_tsid();
        const auto dq = controller->dq(false);
        const int B = controller->batch_size();
        controllers::MatrixXd c0, v0, cn, vn;
        controller->com(c0, v0);
        controller->com_now(cn, vn);
        double moved = 0.0, dcom = 0.0, dpos = 0.0;
        for (int i = 0; i < B; ++i) {
            const auto want = robot.com(q.row(i));
            for (int d = 0; d < 3; ++d) {
                moved = std::max(moved, std::fabs(cn(i, d) - c0(i, d)));
                dcom = std::max(dcom, std::fabs(cn(i, d) - want[d]));
            }
        }
        std::ofstream f(argv[5], std::ios::binary);
        auto put = [&](const controllers::MatrixXd& m) { f.write(reinterpret_cast<const char*>(m.data.data()), (std::streamsize)(m.data.size() * sizeof(double))); };
        put(q); put(dq); put(cn); put(vn);
        for (int a = 6; a < argc; ++a) {
            const auto P = controller->model_frame_pos(argv[a]);
            const auto V = controller->model_frame_vel(argv[a]);
            IWBC_ASSERT(P.rows == B && P.cols == 12 && V.rows == B && V.cols == 6, "one row of 12 / 6 numbers per instance");
            const int id = robot.getFrameId(argv[a]);
            for (int i = 0; i < B; ++i) {
                const auto want = robot.framePosition(q.row(i), id);
                for (int k = 0; k < 9; ++k) dpos = std::max(dpos, std::fabs(P(i, k) - want.R[k]));
                for (int k = 0; k < 3; ++k) dpos = std::max(dpos, std::fabs(P(i, 9 + k) - want.p[k]));
            }
            put(P); put(V);
        }
        // asked again within the tick: no further trip to the device (so far: com_now, then one per frame that joined the selection); a
        // frame the model does not have is refused without spoiling the selection
        const int n_frames = argc - 6, calls_first = counting->observe_calls;
        controllers::MatrixXd cn2, vn2;
        controller->com_now(cn2, vn2);
        for (int a = 6; a < argc; ++a) { controller->model_frame_pos(argv[a]); controller->model_frame_vel(argv[a]); }
        const bool cached = calls_first == 1 + n_frames && counting->observe_calls == calls_first && cn2.data == cn.data;
        bool unknown_refused = false;
        try { controller->model_frame_pos("no_such_frame"); } catch (std::exception&) { unknown_refused = true; }
        const bool still_works = controller->model_frame_pos(argv[6]).cols == 12;
        // one more tick, then qp_step_back(): the accessors follow the state back (the reference restores pinocchio's data there)
        behavior->update(controllers::SensorData{});
        controllers::MatrixXd c_after, v_after, c_back, v_back;
        controller->com_now(c_after, v_after);
        const int calls_tick = counting->observe_calls;
        controller->qp_step_back();
        controller->com_now(c_back, v_back);
        const auto P_back = controller->model_frame_pos(argv[6]);
        double dback = 0.0, stepped = 0.0;
        const int id0 = robot.getFrameId(argv[6]);
        for (int i = 0; i < B; ++i) {
            const auto want = robot.com(controller->q_tsid().row(i));
            const auto wantP = robot.framePosition(controller->q_tsid().row(i), id0);
            for (int d = 0; d < 3; ++d) {
                dback = std::max(dback, std::fabs(c_back(i, d) - want[d]));
                dback = std::max(dback, std::fabs(P_back(i, 9 + d) - wantP.p[d]));
                stepped = std::max(stepped, std::fabs(c_back(i, d) - c_after(i, d)));
            }
        }
        const bool refetched = counting->observe_calls == calls_tick + 1;
        // a controller put back to its start (a new problem source: _reset) answers for q0 again
        auto fresh = make_source<CountingSource>(*pt, argv[1]);
        controller->set_problem_source(fresh);
        controllers::MatrixXd c_reset, v_reset;
        controller->com_now(c_reset, v_reset);
        double dreset = 0.0;
        for (int i = 0; i < B; ++i)
            for (int d = 0; d < 3; ++d) dreset = std::max(dreset, std::fabs(c_reset(i, d) - c0(i, d)));
        const bool same = cached && refetched && fresh->observe_calls == 1;
        std::cout.precision(3);
        std::cout << "instances: " << B << std::endl;
        std::cout << "max |com_now - com()|: " << moved << std::endl;
        std::cout << "max |com_now - RobotWrapper::com(q)|: " << dcom << std::endl;
        std::cout << "max |model_frame_pos - RobotWrapper::framePosition(q)|: " << dpos << std::endl;
        std::cout << "max |com_now, model_frame_pos after qp_step_back - RobotWrapper at the restored q|: " << dback << std::endl;
        std::cout << "max |com_now after qp_step_back - com_now before it|: " << stepped << std::endl;
        std::cout << "max |com_now after a new problem source - com()|: " << dreset << std::endl;
        std::cout << "device calls: " << calls_first << " for com_now and " << n_frames << " new frames, " << counting->observe_calls - calls_tick
                  << " after the step back, " << fresh->observe_calls << " on the new source" << std::endl;
        std::cout << "cached: " << same << " unknown frame refused: " << unknown_refused << " then still answering: " << still_works << std::endl;
        return (moved > 1e-9 && dcom <= 1e-10 && dpos <= 1e-10 && dback <= 1e-10 && stepped > 1e-9 && dreset <= 1e-10 && same && unknown_refused && still_works) ? 0 : 1;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
