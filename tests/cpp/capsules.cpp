// The C++ surface of obstacle avoidance with capsules (include/mppi_amd.hpp):
//  - without arguments: the struct's layout, the constants and the default radii; prints {"cpu": "ok"}
//    (no GPU touched);
//  - with "gpu": Trajectory::set_obstacle_capsules / obstacle_capsules around two updates with a capsule
//    set, the refusals (before avoidance is enabled, the capsule kind without capsules, after the first
//    update), and PinocchioDynamics::capsule_cost against the C call.  One JSON line per check.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "mppi_amd.hpp"

using FrankaRidgeback::PinocchioDynamics;

static int fail(const char *what)
{
    std::fprintf(stderr, "capsules: %s\n", what);
    return 1;
}

static std::unique_ptr<mppi::Trajectory> trajectory()
{
    mppi::Configuration c;
    c.initial_state.assign(MPPI_FR_STATE, 0.0);
    mppi_frankaridgeback_huddled(c.initial_state.data());
    c.rollouts = 17;
    c.keep_best_rollouts = 5;
    c.time_step = 0.01;
    c.horison = 0.045;
    c.gradient_step = 2.0;
    c.cost_scale = 10.0;
    c.cost_discount_factor = 1.0;
    const double var[12] = {0.1, 0.1, 0.2, 7.5, 7.5, 7.5, 7.5, 7.5, 7.5, 7.5, 0.0, 0.0};
    const double lim[12] = {0.5, 0.5, 1.0, 100, 100, 100, 100, 100, 100, 100, 0.05, 0.05};
    c.covariance.assign(144, 0.0);
    for (int i = 0; i < 12; i++) {
        c.covariance[13 * i] = var[i];
        c.control_min.push_back(-lim[i]);
        c.control_max.push_back(lim[i]);
    }
    c.control_bound = true;
    c.threads = 1;
    PinocchioDynamics::Configuration dc;
    dc.link_positions = true;
    FrankaRidgeback::AssistedManipulation::Configuration ac;
    mppi_assisted_manipulation_default(&ac);
    return mppi::Trajectory::create(c, PinocchioDynamics::create(dc), FrankaRidgeback::AssistedManipulation::create(ac));
}

static mppi_obstacle post(double vx)
{
    mppi_obstacle o{};
    o.kind = MPPI_OBSTACLE_CAPSULE;
    o.mask = MPPI_OBSTACLE_MASK_ALL | MPPI_OBSTACLE_MASK_SEGMENTS;
    o.position[0] = 2.0, o.position[1] = 2.0;
    o.normal[2] = 2.0;   // the axis
    o.velocity[0] = vx;
    o.radius = 0.05;
    return o;
}

static mppi_obstacle ball_in_the_forearm()
{
    mppi_obstacle o{};
    o.kind = MPPI_OBSTACLE_SPHERE;
    o.mask = MPPI_OBSTACLE_MASK_SEGMENTS & ~MPPI_OBSTACLE_MASK_SEGMENT(0);   // the arm's segments
    o.position[0] = 0.7106, o.position[1] = 0.7176, o.position[2] = 1.1857;
    o.radius = 0.03;
    return o;
}

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    static_assert(sizeof(mppi_capsule_config) == 64 && offsetof(mppi_capsule_config, segment_radii) == 0, "mppi_capsule_config layout");
    static_assert(sizeof(mppi_obstacle) == 88, "mppi_obstacle keeps its layout");
    static_assert(MPPI_OBSTACLE_SEGMENTS == 8 && MPPI_OBSTACLE_CAPSULE == 2 && MPPI_OBSTACLE_MASK_ALL == 0x1FFu &&
                      MPPI_OBSTACLE_MASK_SEGMENTS == 0xFF0000u && MPPI_OBSTACLE_MASK_SEGMENT(3) == 0x80000u && MPPI_AMD_ABI_VERSION == 5,
                  "constants");
    mppi_capsule_config def;
    mppi_default_capsule_config(&def);
    for (int s = 0; s < MPPI_OBSTACLE_SEGMENTS; s++)
        if (def.segment_radii[s] != 0.1) return fail("default radii");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    const std::vector<mppi_obstacle> set = {post(-0.5), ball_in_the_forearm()};
    auto t = trajectory();
    if (!t) return fail("Trajectory::create");
    {   // capsules need avoidance
        const bool on = t->set_obstacle_capsules();
        std::printf("{\"before_avoidance\": %s, \"reports\": %s}\n", on ? "true" : "false", t->obstacle_capsules() ? "true" : "false");
    }
    if (!t->set_obstacle_avoidance()) return fail("set_obstacle_avoidance");
    const bool refused = !t->set_obstacles(set, 0.0);   // the capsule kind, without capsules
    mppi_capsule_config conf = def;
    for (int s = 1; s < 7; s++) conf.segment_radii[s] = 0.06;
    conf.segment_radii[7] = 0.03;
    if (!t->set_obstacle_capsules(&conf)) return fail("set_obstacle_capsules");
    mppi_capsule_config back{};
    const bool on = t->obstacle_capsules(&back);
    std::printf("{\"enabled\": %s, \"radius7\": %.17g, \"capsule_refused_without\": %s}\n", on ? "true" : "false", back.segment_radii[7],
                refused ? "true" : "false");
    if (!t->set_obstacles(set, -0.25)) return fail("set_obstacles");
    const auto got = t->obstacles();
    std::printf("{\"count\": %d, \"kind0\": %d, \"mask1\": %u, \"axis_z\": %.17g}\n", (int)got.size(), got.empty() ? -1 : got[0].kind,
                got.size() > 1 ? got[1].mask : 0u, got.empty() ? 0.0 : got[0].normal[2]);
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    t->update(x, 0.0);
    const double with_set = t->get_optimal_obstacle_cost();
    if (!t->set_obstacles({}, 0.0)) return fail("clearing the set");
    t->update(x, 0.01);
    const double cleared = t->get_optimal_obstacle_cost();
    std::printf("{\"with_set\": %.17g, \"cleared\": %.17g, \"late_enable\": %s}\n", with_set, cleared,
                t->set_obstacle_capsules() ? "true" : "false");

    // the dynamics object: the class's call against the C call, after a step
    PinocchioDynamics::Configuration dc;
    dc.link_positions = true;
    auto d = PinocchioDynamics::create(dc);
    mppi::VectorXd u(MPPI_FR_CONTROL);
    d->set_state(x, 0.0);
    for (int i = 0; i < MPPI_FR_CONTROL; i++) u[i] = (i >= 3 && i < 10) ? 5.0 - i : 0.1;
    d->step(u, 0.01);
    const double a = d->capsule_cost(set, 0.3, nullptr, &conf);
    double b = 0.0;
    if (mppi_dynamics_capsule_cost(d->object(), nullptr, &conf, set.data(), (int32_t)set.size(), 0.3, &b) != MPPI_OK)
        return fail("mppi_dynamics_capsule_cost");
    std::printf("{\"object_cost\": %.17g, \"same\": %s}\n", a, a == b ? "true" : "false");
    return 0;
}
