// The C++ surface of target tracking (include/mppi_amd.hpp):
//  - without arguments: the structs' layout and the default configuration; prints {"cpu": "ok"}
//    (no GPU touched);
//  - with "gpu": Trajectory::set_target_tracking / set_target_path / get_optimal_target_cost around
//    three updates (Philox, seed 0x5EED: the numbers the Python API writes for the same inputs), the
//    refusals (an AssistedManipulation trajectory, orientation in the zero link mode, after the first
//    update), and PinocchioDynamics::target_cost against the C call.  One JSON line per check.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "mppi_amd.hpp"

using FrankaRidgeback::PinocchioDynamics;

static int fail(const char *what)
{
    std::fprintf(stderr, "target_path: %s\n", what);
    return 1;
}

static std::unique_ptr<mppi::Trajectory> trajectory(bool link_positions, bool track_point)
{
    mppi::Configuration c;   // trajectory_demo.cpp's, at 64 rollouts over 16 steps
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
    PinocchioDynamics::Configuration dc;
    dc.link_positions = link_positions;
    std::unique_ptr<mppi::Cost> cost;
    if (track_point) cost = FrankaRidgeback::TrackPoint::create(FrankaRidgeback::TrackPoint::DEFAULT_CONFIGURATION);
    else cost = std::make_unique<FrankaRidgeback::AssistedManipulation>();
    auto t = mppi::Trajectory::create(c, PinocchioDynamics::create(dc), std::move(cost));
    if (t) t->set_noise_source(MPPI_NOISE_DEVICE_PHILOX, 0x5EED);
    return t;
}

static mppi_target_path path()
{
    mppi_target_path p{};
    p.count = 3;
    p.has_orientation = 1;
    const double times[3] = {0.015, 0.085, 0.145};
    const double pos[3][3] = {{0.88, 0.86, 0.90}, {0.80, 0.95, 0.95}, {0.75, 0.80, 1.00}};
    const double quat[3][4] = {{0.1, 0.0, 0.0, 1.0}, {0.2, 0.1, -0.1, 0.9}, {-0.3, -0.3, 0.2, -0.7}};
    for (int i = 0; i < 3; i++) {
        p.waypoints[i].time = times[i];
        for (int k = 0; k < 3; k++) p.waypoints[i].position[k] = pos[i][k];
        for (int k = 0; k < 4; k++) p.waypoints[i].quaternion[k] = quat[i][k];
    }
    return p;
}

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    static_assert(sizeof(mppi_target_tracking_config) == 16 && offsetof(mppi_target_tracking_config, track_orientation) == 8,
                  "mppi_target_tracking_config layout");
    static_assert(sizeof(mppi_target_waypoint) == 64 && offsetof(mppi_target_waypoint, position) == 8 &&
                      offsetof(mppi_target_waypoint, quaternion) == 32,
                  "mppi_target_waypoint layout");
    static_assert(sizeof(mppi_target_path) == 8 + 64 * MPPI_TARGET_WAYPOINTS_MAX && offsetof(mppi_target_path, waypoints) == 8,
                  "mppi_target_path layout");
    static_assert(MPPI_TARGET_WAYPOINTS_MAX == 32, "constants");
    mppi_target_tracking_config def;
    mppi_default_target_tracking_config(&def);
    if (def.orientation_weight != 10.0 || def.track_orientation != 0) return fail("default configuration");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    const mppi_target_path p = path();
    mppi_target_tracking_config pose = def;
    pose.orientation_weight = 4.0;
    pose.track_orientation = 1;
    {   // the refusals
        auto a = trajectory(true, false);
        auto z = trajectory(false, true);
        if (!a || !z) return fail("Trajectory::create");
        const bool am_on = a->set_target_tracking();
        const bool zero_pose = z->set_target_tracking(&pose);
        const bool zero_position = z->set_target_tracking();
        std::printf("{\"assisted_manipulation\": %s, \"zero_mode_orientation\": %s, \"zero_mode_position\": %s, \"path_without_tracking\": %s}\n",
                    am_on ? "true" : "false", zero_pose ? "true" : "false", zero_position ? "true" : "false",
                    a->set_target_path(&p) ? "true" : "false");
    }
    auto t = trajectory(true, true);
    if (!t) return fail("Trajectory::create");
    if (t->target_tracking()) return fail("tracking reported before it was enabled");
    if (!t->set_target_tracking(&pose)) return fail("set_target_tracking");
    mppi_target_tracking_config back{};
    const bool on = t->target_tracking(&back);
    std::printf("{\"enabled\": %s, \"weight\": %.17g, \"orientation\": %d}\n", on ? "true" : "false", back.orientation_weight,
                back.track_orientation);
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    for (int j = 0; j < 3; j++) {
        if (j == 1 && !t->set_target_path(&p)) return fail("set_target_path");
        if (j == 2 && !t->set_target_path(nullptr)) return fail("clearing the path");
        t->update(x, 0.03 * j);
        const auto c = t->get_optimal_target_cost();
        std::printf("{\"update\": %d, \"optimal_cost\": %.17g, \"position\": %.17g, \"orientation\": %.17g}\n", j,
                    t->get_optimal_total_cost(), c[0], c[1]);
    }
    std::printf("{\"late_enable\": %s}\n", t->set_target_tracking() ? "true" : "false");

    // the dynamics object: the class's call against the C call, after a step
    PinocchioDynamics::Configuration dc;
    auto d = PinocchioDynamics::create(dc);
    mppi::VectorXd u(MPPI_FR_CONTROL);
    d->set_state(x, 0.0);
    for (int i = 0; i < MPPI_FR_CONTROL; i++) u[i] = (i >= 3 && i < 10) ? 5.0 - i : 0.1;
    d->step(u, 0.01);
    const auto a = d->target_cost(p.waypoints[1].position, p.waypoints[1].quaternion, &pose);
    double b[2] = {0.0, 0.0};
    if (mppi_dynamics_target_cost(d->object(), p.waypoints[1].position, p.waypoints[1].quaternion, &pose, b) != MPPI_OK)
        return fail("mppi_dynamics_target_cost");
    std::printf("{\"object_position\": %.17g, \"object_orientation\": %.17g, \"same\": %s}\n", a[0], a[1],
                (a[0] == b[0] && a[1] == b[1]) ? "true" : "false");
    return 0;
}
