// The C++ surface of obstacle avoidance with a held object (include/mppi_amd.hpp):
//  - without arguments: the struct's layout, the constants and HeldObject's round trip through the C
//    struct; prints {"cpu": "ok"} (no GPU touched);
//  - with "gpu": Trajectory::set_held_object_avoidance / set_held_object / held_object /
//    get_optimal_held_cost / get_predicted_held_optimal around three updates (a beam against a sphere on
//    one of its ends, the beam put down, a tool tip), the refusals (before field avoidance is enabled,
//    a count of 5, after the first update), and PinocchioDynamics::held_object_cost against the C call.
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
    std::fprintf(stderr, "held_object: %s\n", what);
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
    static_assert(sizeof(mppi_held_object) == 160 && offsetof(mppi_held_object, centres) == 8 && offsetof(mppi_held_object, radii) == 104 &&
                      offsetof(mppi_held_object, segment_radii) == 136,
                  "mppi_held_object layout");
    static_assert(MPPI_HELD_POINTS == 4 && MPPI_HELD_SEGMENTS == 3 && MPPI_OBSTACLE_MASK_HELD == 0x07001E00u &&
                      MPPI_OBSTACLE_MASK_HELD_POINT(0) == 0x200u && MPPI_OBSTACLE_MASK_HELD_POINT(3) == 0x1000u &&
                      MPPI_OBSTACLE_MASK_HELD_SEGMENT(0) == 0x1000000u && MPPI_OBSTACLE_MASK_HELD_SEGMENT(2) == 0x4000000u &&
                      (MPPI_OBSTACLE_MASK_HELD & (MPPI_OBSTACLE_MASK_ALL | MPPI_OBSTACLE_MASK_SEGMENTS)) == 0u &&
                      MPPI_OBSTACLE_MASK_ALL == 0x1FFu && MPPI_OBSTACLE_MASK_SEGMENTS == 0xFF0000u && MPPI_AMD_ABI_VERSION == 5,
                  "constants");
    mppi::HeldObject beam;
    beam.centres = {{0.0, -0.3, 0.05}, {0.0, 0.3, 0.05}};
    beam.radii = {0.03, 0.035};
    beam.segment_radii = {0.025};
    const mppi_held_object bc = beam.to_c();
    if (bc.count != 2 || bc.centres[1][1] != 0.3 || bc.radii[1] != 0.035 || bc.segment_radii[0] != 0.025 || bc.segment_radii[1] != 0.0 ||
        bc.radii[2] != 0.0)
        return fail("HeldObject::to_c");
    const mppi::HeldObject back = mppi::HeldObject::from_c(bc);
    if (back.centres != beam.centres || back.radii != beam.radii || back.segment_radii != beam.segment_radii) return fail("HeldObject::from_c");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    auto t = trajectory();
    if (!t) return fail("Trajectory::create");
    if (!t->set_obstacle_avoidance() || !t->set_obstacle_capsules()) return fail("set_obstacle_avoidance / capsules");
    const bool early = t->set_held_object_avoidance();   // needs field avoidance
    if (!t->set_distance_field_avoidance()) return fail("set_distance_field_avoidance");
    const bool unset = t->set_held_object(beam);         // needs held-object avoidance
    if (t->held_object_avoidance()) return fail("held_object_avoidance before it is set");
    if (!t->set_held_object_avoidance() || !t->held_object_avoidance()) return fail("set_held_object_avoidance");
    std::printf("{\"before_field\": %s, \"object_before_avoidance\": %s}\n", early ? "true" : "false", unset ? "true" : "false");
    if (t->held_object()) return fail("an object before one is set");
    mppi::HeldObject five;
    five.centres.assign(5, {0.0, 0.0, 0.0});
    five.radii.assign(5, 0.1);
    const bool count5 = t->set_held_object(five);
    if (!t->set_held_object(beam)) return fail("set_held_object");
    const auto got = t->held_object();
    if (!got || got->centres != beam.centres || got->radii != beam.radii || got->segment_radii != beam.segment_radii) return fail("held_object");

    // a sphere on the beam's second end at the huddled state, seen through the held bits only
    mppi_obstacle o{};
    o.kind = MPPI_OBSTACLE_SPHERE;
    o.mask = MPPI_OBSTACLE_MASK_HELD;
    o.position[0] = 1.08, o.position[1] = 0.66, o.position[2] = 0.84;
    o.radius = 0.05;
    if (!t->set_obstacles({o}, 0.0)) return fail("set_obstacles with held bits");
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    t->update(x, 0.0);
    const double with_beam = t->get_optimal_held_cost(), total = t->get_optimal_obstacle_cost();
    const std::vector<double> path = t->get_predicted_held_optimal();
    bool rows = path.size() == (size_t)t->get_step_count() * MPPI_HELD_POINTS * 3;
    for (int i = 0; rows && i < 12; i++) rows = i < 6 ? std::isfinite(path[(size_t)i]) : std::isnan(path[(size_t)i]);
    if (!t->set_held_object(nullptr)) return fail("putting the object down");
    t->update(x, 0.01);
    const double put_down = t->get_optimal_held_cost();
    mppi::HeldObject tip;
    tip.centres = {{0.0, 0.0, 0.15}};
    tip.radii = {0.02};
    if (!t->set_held_object(tip)) return fail("set_held_object (tip)");
    t->update(x, 0.02);
    const double with_tip = t->get_optimal_held_cost();
    std::printf("{\"with_beam\": %.17g, \"obstacle_cost\": %.17g, \"put_down\": %.17g, \"with_tip\": %.17g, \"rows\": %s, \"count5\": %s, "
                "\"late_enable\": %s}\n",
                with_beam, total, put_down, with_tip, rows ? "true" : "false", count5 ? "true" : "false",
                t->set_held_object_avoidance() ? "true" : "false");

    // the dynamics object: the class's call against the C call
    PinocchioDynamics::Configuration dc;
    dc.link_positions = true;
    auto d = PinocchioDynamics::create(dc);
    d->set_state(x, 0.0);
    const double a = d->held_object_cost(beam, {o}, 0.0);
    double b = 0.0;
    if (mppi_dynamics_held_object_cost(d->object(), nullptr, &o, 1, 0.0, nullptr, nullptr, &bc, &b) != MPPI_OK)
        return fail("mppi_dynamics_held_object_cost");
    std::printf("{\"object_cost\": %.17g, \"same\": %s}\n", a, a == b ? "true" : "false");
    return 0;
}
