// The C++ surface of obstacle avoidance (include/mppi_amd.hpp):
//  - without arguments: the structs' layout and the default configuration; prints {"cpu": "ok"}
//    (no GPU touched);
//  - with "gpu": Trajectory::set_obstacle_avoidance / set_obstacles / obstacles /
//    get_optimal_obstacle_cost around two updates, the refusals (zero link mode, after the first
//    update), and PinocchioDynamics::obstacle_cost against the C call.  One JSON line per check.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "mppi_amd.hpp"

using FrankaRidgeback::PinocchioDynamics;

static int fail(const char *what)
{
    std::fprintf(stderr, "obstacles: %s\n", what);
    return 1;
}

static std::unique_ptr<mppi::Trajectory> trajectory(bool link_positions)
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
    dc.link_positions = link_positions;
    FrankaRidgeback::AssistedManipulation::Configuration ac;
    mppi_assisted_manipulation_default(&ac);
    return mppi::Trajectory::create(c, PinocchioDynamics::create(dc), FrankaRidgeback::AssistedManipulation::create(ac));
}

static mppi_obstacle sphere(double x, double y, double z, double r, double vx, uint32_t mask)
{
    mppi_obstacle o{};
    o.kind = MPPI_OBSTACLE_SPHERE;
    o.mask = mask;
    o.position[0] = x, o.position[1] = y, o.position[2] = z;
    o.velocity[0] = vx;
    o.radius = r;
    return o;
}

static mppi_obstacle floor_plane(double z)
{
    mppi_obstacle o{};
    o.kind = MPPI_OBSTACLE_HALF_SPACE;
    o.mask = MPPI_OBSTACLE_MASK_ALL & ~1u;   // not the base sphere
    o.position[2] = z;
    o.normal[2] = 1.0;
    return o;
}

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    static_assert(sizeof(mppi_obstacle) == 88 && offsetof(mppi_obstacle, position) == 8 && offsetof(mppi_obstacle, radius) == 80,
                  "mppi_obstacle layout");
    static_assert(sizeof(mppi_obstacle_config) == 96 && offsetof(mppi_obstacle_config, radii) == 24, "mppi_obstacle_config layout");
    static_assert(MPPI_MAX_OBSTACLES == 16 && MPPI_OBSTACLE_POINTS == 9 && MPPI_AMD_ABI_VERSION == 5, "constants");
    mppi_obstacle_config def;
    mppi_default_obstacle_config(&def);
    if (def.limit.bound != 0.0 || def.limit.scale != 1.0 || def.limit.maximum_cost != 1e10) return fail("default limit");
    if (def.radii[0] != 0.75) return fail("default base radius");
    for (int i = 1; i < MPPI_OBSTACLE_POINTS; i++)
        if (def.radii[i] != 0.1) return fail("default radii");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    const std::vector<mppi_obstacle> set = {sphere(2.2, 0.9, 1.0, 0.3, -0.5, MPPI_OBSTACLE_MASK_ALL), floor_plane(-0.3)};
    {   // the zero link mode refuses
        auto t = trajectory(false);
        if (!t) return fail("Trajectory::create");
        const bool on = t->set_obstacle_avoidance();
        std::printf("{\"zero_mode_enabled\": %s, \"reports\": %s, \"set_obstacles\": %s}\n", on ? "true" : "false",
                    t->obstacle_avoidance() ? "true" : "false", t->set_obstacles(set, 0.0) ? "true" : "false");
    }
    auto t = trajectory(true);
    if (!t) return fail("Trajectory::create");
    mppi_obstacle_config conf = def;
    conf.radii[8] = 0.12;
    if (!t->set_obstacle_avoidance(&conf)) return fail("set_obstacle_avoidance");
    mppi_obstacle_config back{};
    const bool on = t->obstacle_avoidance(&back);
    std::printf("{\"enabled\": %s, \"ee_radius\": %.17g, \"empty\": %d}\n", on ? "true" : "false", back.radii[8], (int)t->obstacles().size());
    if (!t->set_obstacles(set, -0.25)) return fail("set_obstacles");
    double tref = 0.0;
    const auto got = t->obstacles(&tref);
    std::printf("{\"count\": %d, \"time\": %.17g, \"kind1\": %d, \"vx0\": %.17g}\n", (int)got.size(), tref, got.size() > 1 ? got[1].kind : -1,
                got.empty() ? 0.0 : got[0].velocity[0]);
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    t->update(x, 0.0);
    const double with_set = t->get_optimal_obstacle_cost();
    if (!t->set_obstacles({}, 0.0)) return fail("clearing the set");
    t->update(x, 0.01);
    const double cleared = t->get_optimal_obstacle_cost();
    std::printf("{\"with_set\": %.17g, \"cleared\": %.17g, \"late_enable\": %s}\n", with_set, cleared,
                t->set_obstacle_avoidance() ? "true" : "false");

    // the dynamics object: the class's call against the C call, after a step
    PinocchioDynamics::Configuration dc;
    dc.link_positions = true;
    auto d = PinocchioDynamics::create(dc);
    mppi::VectorXd u(MPPI_FR_CONTROL);
    d->set_state(x, 0.0);
    for (int i = 0; i < MPPI_FR_CONTROL; i++) u[i] = (i >= 3 && i < 10) ? 5.0 - i : 0.1;
    d->step(u, 0.01);
    const double a = d->obstacle_cost(set, 0.3, &conf);
    double b = 0.0;
    if (mppi_dynamics_obstacle_cost(d->object(), &conf, set.data(), (int32_t)set.size(), 0.3, &b) != MPPI_OK)
        return fail("mppi_dynamics_obstacle_cost");
    std::printf("{\"object_cost\": %.17g, \"same\": %s}\n", a, a == b ? "true" : "false");
    return 0;
}
