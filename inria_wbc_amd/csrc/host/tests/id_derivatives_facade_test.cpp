// The derivatives of the inverse dynamics through the facade: Controller::inverse_dynamics_derivatives (wbcqp_inverse_dynamics_derivatives_host
// behind a model-driven problem source).
//   id_derivatives_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <n_ticks> <batch> <out.bin>
//       runs n_ticks of the behavior on `batch` instances, then writes q_tsid, dq(false), the accelerations a it asks with, dtau_dq and dtau_dv to
//       out.bin (raw doubles, in this order) and prints what it checked on the way.
//   id_derivatives_facade_test --file-source <controller.yaml> <batch.bin>
//       a controller on a FileSource must refuse (it has no model)
#include "model_query_facade.hpp"

// CountingSource, and the new query counted beside it (what CountingSource::calls() returns is what the other programs print)
struct DerivativeCountingSource : CountingSource {
    using CountingSource::CountingSource;
    int id_derivative_calls = 0;
    void inverse_dynamics_derivatives(const MatrixXd& q, const MatrixXd& v, const MatrixXd& a, const std::vector<std::string>& frames,
                                      const MatrixXd& wrenches, MatrixXd& dtau_dq, MatrixXd& dtau_dv) override
    {
        ++id_derivative_calls;
        controllers::ModelSource::inverse_dynamics_derivatives(q, v, a, frames, wrenches, dtau_dq, dtau_dv);
    }
};

static int file_source_mode(char** argv)
{
    auto controller = make_controller(argv[2], 0);
    controller->set_problem_source(std::make_shared<controllers::FileSource>(argv[3]));
    const MatrixXd a(controller->batch_size(), 1); // (a source without a model refuses before it looks at a shape)
    const int refused = refused_without_model([&] { controller->inverse_dynamics_derivatives(a); }, true);
    std::cout << "refused: " << refused << " of 1" << std::endl;
    return refused == 1 ? 0 : 1;
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
        auto counting = make_source<DerivativeCountingSource>(*pt, argv[1]);
        controller->set_problem_source(counting);
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        auto behavior = behaviors::Factory::instance().create(IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>()), controller, b_config);
        const int n_ticks = std::atoi(argv[3]);
        for (int it = 0; it < n_ticks; ++it) behavior->update(controllers::SensorData{});

        const auto& robot = *pt->robot();
        const int B = controller->batch_size(), nq = robot.nq(), nv = robot.nv();
        const MatrixXd q = controller->q_tsid(), v = controller->dq(false);
        IWBC_ASSERT(q.rows == B && q.cols == nq && v.rows == B && v.cols == nv, "B states");
        // accelerations of the program's own making, of order 1
        MatrixXd a(B, nv);
        for (int i = 0; i < B; ++i)
            for (int j = 0; j < nv; ++j) a(i, j) = 0.1 * ((3 * i + 7 * j) % 11 - 5);
        // asked twice at one state with one a: one answer, kept, one trip to the device; another a: another answer
        const auto& first = controller->inverse_dynamics_derivatives(a);
        const MatrixXd dq = first.dtau_dq, dv = first.dtau_dv;
        const int after_first = counting->id_derivative_calls;
        const auto& again = controller->inverse_dynamics_derivatives(a);
        const bool kept = &again == &first && again.dtau_dq.data == dq.data && counting->id_derivative_calls == after_first && after_first == 1;
        IWBC_ASSERT(dq.rows == B && dq.cols == nv * nv && dv.rows == B && dv.cols == nv * nv, "B x nv*nv");
        MatrixXd a2 = a;
        a2(0, nv - 1) += 1.0;
        const MatrixXd dq2 = controller->inverse_dynamics_derivatives(a2).dtau_dq;
        const bool another_a = dq2.data != dq.data && counting->id_derivative_calls == 2;
        const bool back = controller->inverse_dynamics_derivatives(a).dtau_dq.data == dq.data && counting->id_derivative_calls == 3;

        controller->qp_step_back();
        const bool refreshed = controller->inverse_dynamics_derivatives(a).dtau_dq.data != dq.data && counting->id_derivative_calls == 4;

        std::ofstream f(argv[5], std::ios::binary);
        auto put = [&](const MatrixXd& m) { f.write(reinterpret_cast<const char*>(m.data.data()), (std::streamsize)(m.data.size() * sizeof(double))); };
        put(q); put(v); put(a); put(dq); put(dv);
        std::cout << "instances: " << B << std::endl;
        std::cout << "device calls: " << counting->calls() << std::endl;
        std::cout << "inverse dynamics derivative calls: " << counting->id_derivative_calls << std::endl;
        std::cout << "kept: " << kept << std::endl;
        std::cout << "another a, another answer: " << another_a << std::endl;
        std::cout << "and back: " << back << std::endl;
        std::cout << "refreshed after qp_step_back: " << refreshed << std::endl;
        return 0;
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
