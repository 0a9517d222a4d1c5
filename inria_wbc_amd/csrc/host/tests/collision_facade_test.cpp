// The reference's self-collision check through the facade: CONTROLLER.check_model_collisions / collision_path, Controller::is_model_colliding,
// collision_index and the latch that stops an instance's commands (controller.cpp:263-282,309-312) -- wbcqp_check_collisions_host behind a
// model-driven problem source.
//   collision_facade_test <controller.yaml with CONTROLLER.model> <behavior.yaml> <collisions.yaml> <n_ticks> <batch> <k> <roll> <out.bin>
//       two controllers on `batch` instances, one with the check and one without, both started with instance k's shoulders rolled inwards by
//       `roll` rad (arm_left_2_joint, arm_right_2_joint: the arms meet the legs, then each other), then n_ticks of the behavior on each.  Prints what the latch did and
//       writes, as doubles: the checked controller's final q_tsid (B x nq) and its is_model_colliding (B)
//   collision_facade_test --file-source <controller.yaml> <collisions.yaml> <batch.bin>
//       check_model_collisions on a source without a model must be refused, in words that say so
#include "model_query_facade.hpp"

static int file_source_mode(char** argv)
{
    const bool refused = refused_without_model([&] { make_controller(argv[2], 0, argv[3])->set_problem_source(std::make_shared<controllers::FileSource>(argv[4])); }, true);
    std::cout << "refused: " << refused << std::endl;
    return refused ? 0 : 1;
}

static bool same_row(const MatrixXd& a, const MatrixXd& b, int i)
{
    return a.cols == b.cols && std::equal(a.row(i), a.row(i) + a.cols, b.row(i)); // (no NaN is expected: == on doubles is bit equality here)
}

// the controller's state with instance k's shoulders rolled inwards
static MatrixXd driven(const controllers::PosTracker& pt, const MatrixXd& q0, int k, double roll)
{
    const auto& jn = pt.robot()->joint_names();
    auto col = [&](const std::string& n) { return 7 + (int)std::distance(jn.begin(), std::find(jn.begin(), jn.end(), n)) - 1; };
    MatrixXd q = q0;
    q(k, col("arm_left_2_joint")) -= roll;
    q(k, col("arm_right_2_joint")) += roll;
    return q;
}

struct Tick {
    MatrixXd q, dq, ddq, tau, q_solver;
};

int main(int argc, char** argv)
{
    try {
        if (argc == 5 && std::string(argv[1]) == "--file-source") return file_source_mode(argv);
        if (argc != 9) {
            std::cerr << "usage: " << argv[0] << " <controller.yaml> <behavior.yaml> <collisions.yaml> <n_ticks> <batch> <k> <roll> <out.bin>" << std::endl;
            return 2;
        }
        const int n_ticks = std::atoi(argv[4]), B = std::atoi(argv[5]), k = std::atoi(argv[6]);
        const double roll = std::atof(argv[7]);
        yaml::Node b_config = IWBC_CHECK(yaml::LoadFile(argv[2]));
        std::shared_ptr<controllers::Controller> ctl[2] = {make_controller(argv[1], B, argv[3]), make_controller(argv[1], B)};
        std::shared_ptr<CountingSource> counting[2];
        std::vector<Tick> rec[2];
        std::vector<std::vector<int>> flags;
        MatrixXd q_start, zero_v;
        for (int c = 0; c < 2; ++c) {
            auto pt = std::dynamic_pointer_cast<controllers::PosTracker>(ctl[c]);
            IWBC_ASSERT(pt && pt->robot(), "the controller must be a PosTracker with a model");
            IWBC_ASSERT(ctl[c]->check_model_collisions() == (c == 0), "CONTROLLER.check_model_collisions was not read");
            counting[c] = count_device_calls(ctl[c], argv[1]);
            auto behavior = behaviors::Factory::instance().create(IWBC_CHECK(b_config["BEHAVIOR"]["name"].as<std::string>()), ctl[c], b_config);
            q_start = ctl[c]->q_tsid();
            zero_v = MatrixXd(B, ctl[c]->dq(false).cols);
            ctl[c]->qp_step_back(driven(*pt, q_start, k, roll), zero_v);
            for (int it = 0; it < n_ticks; ++it) {
                behavior->update(controllers::SensorData{});
                rec[c].push_back(Tick{ctl[c]->q(false), ctl[c]->dq(false), ctl[c]->ddq(false), ctl[c]->tau(false), ctl[c]->q_solver(false)});
                if (c == 0) flags.push_back(ctl[c]->is_model_colliding());
            }
        }
        // when instance k was first seen colliding, and whether anybody else ever was
        int hit = -1;
        bool others_free = true;
        for (int t = 0; t < n_ticks; ++t)
            for (int i = 0; i < B; ++i) {
                if (i == k && flags[t][i] && hit < 0) hit = t + 1;
                if (i != k && flags[t][i]) others_free = false;
            }
        // from the tick after the hit instance k's commands stand still while the solver's own state goes on -- as it does without the check
        bool frozen = hit > 0 && hit < n_ticks, advancing = frozen, solver_equal = true, others_equal = true, off_is_solver = true;
        for (int t = 0; t < n_ticks; ++t) {
            const Tick &a = rec[0][t], &b = rec[1][t];
            if (hit > 0 && t + 1 > hit) {
                const Tick& h = rec[0][hit - 1];
                frozen = frozen && same_row(a.q, h.q, k) && same_row(a.dq, h.dq, k) && same_row(a.ddq, h.ddq, k) && same_row(a.tau, h.tau, k);
                advancing = advancing && !same_row(a.q_solver, h.q_solver, k);
            }
            else if (hit > 0) // up to and including the tick of the hit the commands are the solver's
                frozen = frozen && same_row(a.q, a.q_solver, k);
            solver_equal = solver_equal && same_row(a.q_solver, b.q_solver, k);
            for (int i = 0; i < B; ++i) {
                off_is_solver = off_is_solver && same_row(b.q, b.q_solver, i);
                if (i != k)
                    others_equal = others_equal && same_row(a.q, b.q, i) && same_row(a.dq, b.dq, i) && same_row(a.ddq, b.ddq, i) &&
                                   same_row(a.tau, b.tau, i) && same_row(a.q_solver, b.q_solver, i);
            }
        }
        const auto send = ctl[0]->send_cmd();
        bool latch_only_k = true;
        for (int i = 0; i < B; ++i) latch_only_k = latch_only_k && send[i] == (i == k ? 0 : 1);
        const auto index = ctl[0]->collision_index();
        const MatrixXd q_end = ctl[0]->q_tsid();
        const std::vector<int> flags_end = ctl[0]->is_model_colliding();
        // a step back refreshes the answer: everybody to the start (free), then ANOTHER instance driven together
        auto pt0 = std::dynamic_pointer_cast<controllers::PosTracker>(ctl[0]);
        ctl[0]->qp_step_back(q_start, zero_v);
        bool all_free = true;
        for (int f : ctl[0]->is_model_colliding()) all_free = all_free && f == 0;
        const int j = (k + 1) % B;
        ctl[0]->qp_step_back(driven(*pt0, q_start, j, roll), zero_v);
        const auto fj = ctl[0]->is_model_colliding();
        bool only_j = true;
        for (int i = 0; i < B; ++i) only_j = only_j && fj[i] == (i == j ? 1 : 0);
        const auto index_j = ctl[0]->collision_index();
        bool never_off = true;
        for (int f : ctl[1]->is_model_colliding()) never_off = never_off && f == 0;

        std::ofstream f(argv[8], std::ios::binary);
        f.write(reinterpret_cast<const char*>(q_end.data.data()), (std::streamsize)(q_end.data.size() * sizeof(double)));
        for (int i = 0; i < B; ++i) {
            const double v = flags_end[i];
            f.write(reinterpret_cast<const char*>(&v), sizeof(double));
        }
        std::cout << "instances: " << B << std::endl;
        std::cout << "device calls: " << counting[0]->calls() << std::endl;
        std::cout << "device calls without the check: " << counting[1]->calls() << std::endl;
        std::cout << "hit seen after tick: " << hit << std::endl;
        std::cout << "others never collide: " << others_free << std::endl;
        std::cout << "commands frozen from the tick after the hit: " << frozen << std::endl;
        std::cout << "solver state keeps advancing: " << advancing << std::endl;
        std::cout << "solver state equals the run without the check: " << solver_equal << std::endl;
        std::cout << "other instances bit-equal to the run without the check: " << others_equal << std::endl;
        std::cout << "without the check q() is q_solver() and nothing collides: " << (off_is_solver && never_off) << std::endl;
        std::cout << "send_cmd is 0 for k alone: " << latch_only_k << std::endl;
        std::cout << "collision_index: " << index[k].first.first << " " << index[k].first.second << " " << index[k].second.first << " "
                  << index[k].second.second << std::endl;
        std::cout << "collision_index of a free instance: [" << index[j].first.first << "] " << index[j].first.second << std::endl;
        std::cout << "step back to the start frees everybody: " << all_free << std::endl;
        std::cout << "step back with another instance driven names it alone: " << only_j << std::endl;
        std::cout << "collision_index after that step back: " << index_j[j].first.first << " " << index_j[j].first.second << " " << index_j[j].second.first
                  << " " << index_j[j].second.second << std::endl;
        return 0; // (tests/test_collision_facade.py judges the lines)
    }
    catch (std::exception& e) {
        std::cerr << "Exception:" << e.what() << std::endl;
        return 1;
    }
}
