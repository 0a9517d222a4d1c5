// What the model-query facade programs (observe_, collision_, inverse_dynamics_facade_test, ...) share: the controller of a yaml file, the
// model-driven source it would make for itself (and one that counts its trips to the device), and the --file-source mode's "a source without
// a model must refuse, in words that say so".
#ifndef IWBC_HIP_TESTS_MODEL_QUERY_FACADE_HPP
#define IWBC_HIP_TESTS_MODEL_QUERY_FACADE_HPP
#include <cmath>
#include <fstream>
#include <iostream>

#include <inria_wbc/behaviors/humanoid/move_com.hpp>
#include <inria_wbc/controllers/file_source.hpp>
#include <inria_wbc/controllers/model_source.hpp>
#include <inria_wbc/controllers/pos_tracker.hpp>

using namespace inria_wbc;
using controllers::MatrixXd;

// batch 0: the file's own; collisions: CONTROLLER.check_model_collisions with this collision file
static std::shared_ptr<controllers::Controller> make_controller(const std::string& path, int batch, const std::string& collisions = "")
{
    yaml::Node c_config = IWBC_CHECK(yaml::LoadFile(path));
    c_config["CONTROLLER"].set("base_path", path.substr(0, path.find_last_of('/')));
    if (batch > 0) c_config["CONTROLLER"].set("batch", std::to_string(batch));
    if (!collisions.empty()) {
        c_config["CONTROLLER"].set("check_model_collisions", "true");
        c_config["CONTROLLER"].set("collision_path", collisions);
    }
    return controllers::Factory::instance().create(IWBC_CHECK(c_config["CONTROLLER"]["name"].as<std::string>()), c_config);
}

// a source of the controller's own kind (Source: ModelSource or a class derived from it) at the reference configuration its yaml file names
template <typename Source>
static std::shared_ptr<Source> make_source(const controllers::PosTracker& pt, const std::string& controller_yaml)
{
    yaml::Node cc = IWBC_CHECK(yaml::LoadFile(controller_yaml));
    return std::make_shared<Source>(pt.robot(), pt.batch_size(), pt.robot()->referenceConfigurations().at(IWBC_CHECK(cc["CONTROLLER"]["ref_config"].as<std::string>())));
}

// the controller's own kind of source, counting per query the trips to the device the controller's kept answers cause (a call that ends in a
// refusal counts: it was made)
struct CountingSource : controllers::ModelSource {
    using controllers::ModelSource::ModelSource;
    using VectorXi = controllers::VectorXi;
    int observe_calls = 0, collision_calls = 0, mass_matrix_calls = 0, jacobian_calls = 0, hessian_calls = 0;
    void observe(const MatrixXd& q, const MatrixXd& v, const std::vector<std::string>& frames, MatrixXd& com, MatrixXd& vcom, MatrixXd& place,
                 MatrixXd& vel) override
    {
        ++observe_calls;
        controllers::ModelSource::observe(q, v, frames, com, vcom, place, vel);
    }
    void check_collisions(const MatrixXd& q, const std::string& file, VectorXi& colliding, VectorXi& first_pair,
                          std::vector<std::pair<std::string, int>>& names) override
    {
        ++collision_calls;
        controllers::ModelSource::check_collisions(q, file, colliding, first_pair, names);
    }
    void mass_matrix(const MatrixXd& q, MatrixXd& M) override
    {
        ++mass_matrix_calls;
        controllers::ModelSource::mass_matrix(q, M);
    }
    void jacobians(const MatrixXd& q, const std::vector<std::string>& frames, int reference_frame, MatrixXd* J, MatrixXd& Jcom, MatrixXd& Ag) override
    {
        ++jacobian_calls;
        controllers::ModelSource::jacobians(q, frames, reference_frame, J, Jcom, Ag);
    }
    void hessians(const MatrixXd& q, const MatrixXd* v, const std::vector<std::string>& frames, int reference_frame, MatrixXd* H, MatrixXd* dJ) override
    {
        ++hessian_calls;
        controllers::ModelSource::hessians(q, v, frames, reference_frame, H, dJ);
    }
    // what follows "device calls: " in a program's output
    std::string calls() const
    {
        return "observe " + std::to_string(observe_calls) + ", check_collisions " + std::to_string(collision_calls) + ", mass_matrix " +
               std::to_string(mass_matrix_calls) + ", jacobians " + std::to_string(jacobian_calls) + ", hessians " + std::to_string(hessian_calls);
    }
};

// puts a counting source of the controller's own kind in the place of the one it made for itself (before anything is asked of it)
static std::shared_ptr<CountingSource> count_device_calls(const std::shared_ptr<controllers::Controller>& controller, const std::string& controller_yaml)
{
    auto pt = std::dynamic_pointer_cast<controllers::PosTracker>(controller);
    IWBC_ASSERT(pt && pt->robot(), "the controller must be a PosTracker with a model");
    auto counting = make_source<CountingSource>(*pt, controller_yaml);
    controller->set_problem_source(counting);
    return counting;
}

// 1 when f() is refused in words that say the source has no model
template <typename F>
static int refused_without_model(F&& f, bool print = false)
{
    try { f(); }
    catch (std::exception& e) {
        if (print) std::cout << "message: " << e.what() << std::endl;
        return std::string(e.what()).find("no model") != std::string::npos;
    }
    return 0;
}
#endif
