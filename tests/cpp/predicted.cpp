// The C++ surface of the predicted trajectories (include/mppi_amd.hpp, mppi_amd_logging.hpp):
//  - without arguments: the row layout's constants, both entry points refusing null arguments, and
//    logger::MPPI::Configuration::log_predicted's default; prints {"cpu": "ok"} (no GPU touched);
//  - "log <folder> <0|1>": the run of trajectory_demo's logger test (64 rollouts, 0.16 s horizon, three
//    updates, device Philox) with logger::MPPI writing into <folder>, log_predicted as given; then
//    one JSON line with get_predicted_optimal's and get_predicted_rollouts' sizes and first values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mppi_amd.hpp"
#include "mppi_amd_logging.hpp"

static int fail(const char *what)
{
    std::fprintf(stderr, "predicted: %s\n", what);
    return 1;
}

// the methods instantiate against a const Trajectory (get_predicted_optimal is what the logger calls)
static std::size_t surface(const mppi::Trajectory &t)
{
    return t.get_predicted_optimal().size() + t.get_predicted_rollouts({0, 1}).size();
}

int main(int argc, char **argv)
{
    static_assert(MPPI_PRED_Q == 0 && MPPI_PRED_QD == 12 && MPPI_PRED_ENERGY == 24 && MPPI_PRED_EE == 25 &&
                      MPPI_PRED_ARM_MOUNT == 28 && MPPI_PRED_LINKS == 31 && MPPI_PRED_N == 31 + 3 * MPPI_LINK_N,
                  "row layout");
    double row[MPPI_PRED_N];
    const int64_t index = 0;
    if (mppi_predicted_optimal(nullptr, row) != MPPI_ERR_INVALID) return fail("mppi_predicted_optimal(null handle)");
    if (mppi_predicted_rollouts(nullptr, &index, 1, row) != MPPI_ERR_INVALID) return fail("mppi_predicted_rollouts(null handle)");
    if (logger::MPPI::Configuration{}.log_predicted) return fail("log_predicted default");
    if (argc < 2) {
        (void)&surface;
        std::printf("{\"cpu\": \"ok\"}\n");
        return 0;
    }
    if (std::strcmp(argv[1], "log") != 0 || argc < 4) return fail("usage: predicted [log <folder> <0|1>]");

    mppi::Configuration c;   // trajectory_demo's configuration
    c.initial_state.assign(MPPI_FR_STATE, 0.0);
    mppi_frankaridgeback_huddled(c.initial_state.data());
    c.rollouts = 64;
    c.keep_best_rollouts = 20;
    c.time_step = 0.01;
    c.horison = 0.16;
    c.gradient_step = 2.0;
    c.cost_scale = 10.0;
    c.cost_discount_factor = 1.0;
    c.covariance.assign(144, 0.0);
    for (int i = 0; i < 12; i++) c.covariance[13 * i] = MPPI_FR_DEFAULT_VARIANCE[i];
    c.control_bound = true;
    c.control_min.assign(MPPI_FR_DEFAULT_CONTROL_MIN, MPPI_FR_DEFAULT_CONTROL_MIN + 12);
    c.control_max.assign(MPPI_FR_DEFAULT_CONTROL_MAX, MPPI_FR_DEFAULT_CONTROL_MAX + 12);
    c.control_default = std::vector<double>(12, 0.0);
    c.threads = 36;
    auto traj = mppi::Trajectory::create(c, std::make_unique<FrankaRidgeback::PinocchioDynamics>(),
                                         std::make_unique<FrankaRidgeback::AssistedManipulation>());
    if (!traj) return fail("Trajectory::create");
    if (mppi_predicted_optimal(traj->handle(), nullptr) != MPPI_ERR_INVALID) return fail("mppi_predicted_optimal(null out)");
    if (mppi_predicted_rollouts(traj->handle(), nullptr, 1, row) != MPPI_ERR_INVALID) return fail("mppi_predicted_rollouts(null indices)");
    logger::MPPI::Configuration lc;
    lc.folder = argv[2];
    lc.state_dof = MPPI_FR_STATE;
    lc.control_dof = MPPI_FR_CONTROL;
    lc.rollouts = traj->get_rollout_count();
    lc.log_predicted = std::atoi(argv[3]) != 0;
    auto log = logger::MPPI::create(lc);
    if (!log) return fail("logger::MPPI::create");
    traj->set_noise_source(MPPI_NOISE_DEVICE_PHILOX, 0x5EED);
    std::vector<double> forecast(6 * traj->get_step_count(), 0.0);
    for (unsigned k = 0; k < traj->get_step_count(); k++) forecast[6 * k] = 20.0;
    traj->set_forecast(forecast);
    for (int j = 0; j < 3; j++) {
        traj->update(c.initial_state, 0.05 * j);
        log->log(*traj);
        log->log(*traj);   // same update time: skipped
    }
    const std::vector<double> opt = traj->get_predicted_optimal(), two = traj->get_predicted_rollouts({5, 0});
    std::printf("{\"optimal\": %zu, \"rollouts\": %zu, \"surface\": %zu, \"q3\": %.17g, \"r0_q3\": %.17g, \"r5_ee_x\": %.17g}\n",
                opt.size(), two.size(), surface(*traj), opt[MPPI_PRED_Q + 3],
                two[(std::size_t)traj->get_step_count() * MPPI_PRED_N + MPPI_PRED_Q + 3], two[MPPI_PRED_EE]);
    return 0;
}
