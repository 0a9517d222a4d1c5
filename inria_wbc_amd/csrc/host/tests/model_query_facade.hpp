// What the three model-query facade programs (observe_, collision_, inverse_dynamics_facade_test) share: the controller of a yaml file, the
// model-driven source it would make for itself, and the --file-source mode's "a source without a model must refuse, in words that say so".
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
