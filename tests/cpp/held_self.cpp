// The C++ surface of the held object against the robot's own segments (include/mppi_amd.hpp):
//  - without arguments: the struct's layout, the constants, the defaults and HeldSelf's round trip through
//    the C struct; prints {"cpu": "ok"} (no GPU touched);
//  - with "gpu": Trajectory::set_held_self_avoidance / set_held_self / get_held_self /
//    get_optimal_held_self_cost around three updates (a beam under a configuration, the configuration
//    cleared, the defaults), the refusals (before held-object avoidance is enabled, a units bit above 6,
//    after the first update), and PinocchioDynamics::held_self_cost against the C call.
//    One JSON line per check.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mppi_amd.hpp"

using FrankaRidgeback::PinocchioDynamics;

static int fail(const char *what)
{
    std::fprintf(stderr, "held_self: %s\n", what);
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

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    static_assert(sizeof(mppi_held_self) == 72 && offsetof(mppi_held_self, segments) == 4 && offsetof(mppi_held_self, radii) == 8,
                  "mppi_held_self layout");
    static_assert(MPPI_HELD_SELF_UNITS == 0x7Fu && MPPI_HELD_SELF_SEGMENTS == 8 && MPPI_HELD_SELF_UNIT_POINT(3) == 0x8u &&
                      MPPI_HELD_SELF_UNIT_SEGMENT(0) == 0x10u && MPPI_HELD_SELF_UNIT_SEGMENT(2) == 0x40u && MPPI_AMD_ABI_VERSION == 5,
                  "constants");
    mppi_held_self def{};
    mppi_default_held_self(&def);
    const mppi::HeldSelf cxx_def;
    if (def.units != 0x7Fu || def.segments != 0x1Fu || cxx_def.units != def.units || cxx_def.segments != def.segments)
        return fail("the defaults");
    for (int s = 0; s < MPPI_HELD_SELF_SEGMENTS; s++)
        if (def.radii[s] != 0.1 || cxx_def.radii[(size_t)s] != 0.1) return fail("the default radii");
    mppi::HeldSelf wrist;
    wrist.units = 0x13u;
    wrist.segments = 0xE1u;
    wrist.radii = {{0.05, 0.0, 0.0, 0.0, 0.0, 0.1, 0.12, 0.01}};
    const mppi_held_self wc = wrist.to_c();
    if (wc.units != 0x13u || wc.segments != 0xE1u || wc.radii[6] != 0.12 || wc.radii[0] != 0.05) return fail("HeldSelf::to_c");
    const mppi::HeldSelf back = mppi::HeldSelf::from_c(wc);
    if (back.units != wrist.units || back.segments != wrist.segments || back.radii != wrist.radii) return fail("HeldSelf::from_c");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    auto t = trajectory();
    if (!t) return fail("Trajectory::create");
    if (!t->set_obstacle_avoidance() || !t->set_obstacle_capsules() || !t->set_distance_field_avoidance())
        return fail("set_obstacle_avoidance / capsules / field");
    const bool early = t->set_held_self_avoidance();     // needs held-object avoidance
    if (!t->set_held_object_avoidance()) return fail("set_held_object_avoidance");
    const bool unset = t->set_held_self(wrist);          // needs held-self avoidance
    if (t->held_self_avoidance()) return fail("held_self_avoidance before it is set");
    if (!t->set_held_self_avoidance() || !t->held_self_avoidance()) return fail("set_held_self_avoidance");
    std::printf("{\"before_held\": %s, \"config_before_avoidance\": %s}\n", early ? "true" : "false", unset ? "true" : "false");
    if (t->get_held_self()) return fail("a configuration before one is set");
    mppi::HeldSelf bit7 = wrist;
    bit7.units = 0x80u;
    const bool units7 = t->set_held_self(bit7);
    if (!t->set_held_self(wrist)) return fail("set_held_self");
    const auto got = t->get_held_self();
    if (!got || got->units != wrist.units || got->segments != wrist.segments || got->radii != wrist.radii) return fail("get_held_self");

    mppi::HeldObject beam;
    beam.centres = {{0.0, -0.3, 0.05}, {0.0, 0.3, 0.05}};
    beam.radii = {0.03, 0.035};
    beam.segment_radii = {0.025};
    if (!t->set_held_object(beam)) return fail("set_held_object");
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    t->update(x, 0.0);
    const double with_wrist = t->get_optimal_held_self_cost(), total = t->get_optimal_obstacle_cost();
    if (!t->set_held_self(nullptr)) return fail("clearing the configuration");
    t->update(x, 0.01);
    const double cleared = t->get_optimal_held_self_cost();
    if (!t->set_held_self(cxx_def)) return fail("set_held_self (defaults)");
    t->update(x, 0.02);
    const double with_defaults = t->get_optimal_held_self_cost();
    std::printf("{\"with_wrist\": %.17g, \"obstacle_cost\": %.17g, \"cleared\": %.17g, \"with_defaults\": %.17g, \"units7\": %s, "
                "\"late_enable\": %s}\n",
                with_wrist, total, cleared, with_defaults, units7 ? "true" : "false", t->set_held_self_avoidance() ? "true" : "false");

    // the dynamics object: the class's call against the C call
    PinocchioDynamics::Configuration dc;
    dc.link_positions = true;
    auto d = PinocchioDynamics::create(dc);
    d->set_state(x, 0.0);
    const double a = d->held_self_cost(beam, wrist);
    const mppi_held_object bc = beam.to_c();
    double b = 0.0;
    if (mppi_dynamics_held_self_cost(d->object(), nullptr, &bc, &wc, &b) != MPPI_OK) return fail("mppi_dynamics_held_self_cost");
    std::printf("{\"object_cost\": %.17g, \"same\": %s}\n", a, a == b ? "true" : "false");
    return 0;
}
