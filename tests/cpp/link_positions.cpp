// The C++ surface of the kinematic link-position model (include/mppi_amd.hpp):
//  - without arguments: the Link enum against the C-ABI's MPPI_LINK_* and mppi_link_name, the
//    Configuration flag's default; prints {"cpu": "ok"} (no GPU touched);
//  - with "gpu": PinocchioDynamics::get_link_position against mppi_dynamics_link_positions' rows in
//    both models after a set_state and a step, and Configuration::link_positions reaching the handle
//    of a Trajectory created on the dynamics.  One JSON line per check.
#include <cstdio>
#include <cstring>
#include <string>

#include "mppi_amd.hpp"

using FrankaRidgeback::Link;
using FrankaRidgeback::PinocchioDynamics;

static int fail(const char *what)
{
    std::fprintf(stderr, "link_positions: %s\n", what);
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

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    static_assert((int)Link::OMNI_BASE_ROOT_LINK == 0 && (int)Link::PIVOT == MPPI_LINK_PIVOT &&
                      (int)Link::PANDA_LINK7 == MPPI_LINK_PANDA_LINK7 && (int)Link::_SIZE == MPPI_LINK_N,
                  "Link enum");
    if (std::string(mppi_link_name((int)Link::PANDA_LINK5)) != "panda_link5") return fail("mppi_link_name");
    if (mppi_link_name(MPPI_LINK_N) != nullptr || mppi_link_name(-1) != nullptr) return fail("mppi_link_name out of range");
    if (PinocchioDynamics::Configuration{}.link_positions) return fail("Configuration::link_positions default");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    for (int mode = 0; mode < 2; mode++) {
        PinocchioDynamics::Configuration dc;
        dc.link_positions = mode == 1;
        auto d = PinocchioDynamics::create(dc);
        mppi::VectorXd x(MPPI_FR_STATE), u(MPPI_FR_CONTROL);
        mppi_frankaridgeback_huddled(x.data());
        d->set_state(x, 0.0);
        for (int i = 0; i < MPPI_FR_CONTROL; i++) u[i] = (i >= 3 && i < 10) ? 5.0 - i : 0.1;
        d->step(u, 0.01);
        double rows[3 * MPPI_LINK_N];
        if (mppi_dynamics_link_positions(d->object(), rows) != MPPI_OK) return fail("mppi_dynamics_link_positions");
        bool same = true, zero = true;
        for (int l = 0; l < MPPI_LINK_N; l++) {
            const auto p = d->get_link_position((Link)l);
            for (int k = 0; k < 3; k++) {
                same = same && p[k] == rows[3 * l + k];
                zero = zero && p[k] == 0.0;
            }
        }
        const auto ee = d->get_link_position(Link::PANDA_LINK7);
        std::printf("{\"mode\": %d, \"same\": %s, \"zero\": %s, \"panda_link7\": [%.17g, %.17g, %.17g]}\n", mode,
                    same ? "true" : "false", zero ? "true" : "false", ee[0], ee[1], ee[2]);
    }
    for (int mode = 0; mode < 2; mode++) {
        auto t = trajectory(mode == 1);
        if (!t) return fail("Trajectory::create");
        std::printf("{\"configured\": %d, \"handle\": %d}\n", mode, t->link_positions() ? 1 : 0);
    }
    return 0;
}
