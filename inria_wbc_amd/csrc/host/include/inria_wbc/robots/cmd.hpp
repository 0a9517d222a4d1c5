// compute_spd and compute_velocities of the reference's inria_wbc/robot_dart/cmd.hpp, for a whole fleet: how a driver turns the controller's
// position targets into torque (--actuators spd) or velocity commands.  The reference asks a simulated robot for q, dq, M, the Coriolis and
// gravity forces; here the states are the caller's, one row per instance, and M and the bias come from the controller's model on the device
// (wbcqp_spd_commands_host behind a model-driven problem source).  A B-row matrix stands where the reference has a vector.
#ifndef IWBC_HIP_ROBOTS_CMD_HPP
#define IWBC_HIP_ROBOTS_CMD_HPP

#include <memory>

#include <inria_wbc/controllers/controller.hpp>

namespace inria_wbc {
    namespace robots {
        // compute torques from positions.  q: B x nq (tsid's form, the base quaternion included), dq: B x nv, targetpos: B x nv (the reference's
        // layout: a floating base's six entries in front, where the gains are zero) or B x na (the actuated joints alone).  Returns B x nv.
        inline controllers::MatrixXd compute_spd(const std::shared_ptr<controllers::Controller>& controller, const controllers::MatrixXd& q,
                                                 const controllers::MatrixXd& dq, const controllers::MatrixXd& targetpos, double dt)
        {
            IWBC_ASSERT(controller, "Invalid controller");
            float stiffness = 10000 / (dt * 1000); // tuned for 1000hz and then scaled for other freq (cmd.hpp:15-16: floats there too)
            float damping = 100 / (dt * 1000);
            return controller->spd_commands(q, dq, targetpos, dt, stiffness, damping);
        }

        // compute velocities from positions: (targetpos - q) / dt, entry by entry; q and targetpos of one shape
        inline controllers::MatrixXd compute_velocities(const controllers::MatrixXd& q, const controllers::MatrixXd& targetpos, double dt)
        {
            IWBC_ASSERT(q.rows == targetpos.rows && q.cols == targetpos.cols, "q and targetpos must have one shape");
            controllers::MatrixXd vel(q.rows, q.cols);
            for (size_t i = 0; i < q.data.size(); ++i) vel.data[i] = (targetpos.data[i] - q.data[i]) / dt;
            return vel;
        }
    } // namespace robots
} // namespace inria_wbc
#endif
