// The C++ surface of the trajectory safety filter (include/mppi_amd.hpp):
//  - without arguments: the struct's layout, the default configuration, the filter class's
//    descriptor and the refusals that need no device; prints {"cpu": "ok"} (no GPU touched);
//  - with "gpu": Trajectory::create with a FrankaRidgeback::TrajectorySafetyFilter, two updates,
//    the unfiltered plan and the changed steps, and the host-callable filter() against
//    mppi_dynamics_safety_filter.  One JSON line per check.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "mppi_amd.hpp"

using FrankaRidgeback::PinocchioDynamics;
using FrankaRidgeback::TrajectorySafetyFilter;

static int fail(const char *what)
{
    std::fprintf(stderr, "safety_filter: %s\n", what);
    return 1;
}

// a filter the device cannot run: no descriptor
class HostOnlyFilter : public mppi::Filter {
public:
    mppi::VectorXd filter(mppi::Ref<mppi::VectorXd>, mppi::Ref<mppi::VectorXd> control, double) override
    {
        mppi::VectorXd out(control.size());
        for (std::ptrdiff_t i = 0; i < control.size(); i++) out[i] = control[i];
        return out;
    }
    void reset(mppi::Ref<mppi::VectorXd>, double) override {}
};

static mppi::Configuration configuration()
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
    return c;
}

static TrajectorySafetyFilter::Configuration tight()
{
    TrajectorySafetyFilter::Configuration f = TrajectorySafetyFilter::default_configuration();
    f.limit_velocity = true;
    f.limit_acceleration = true;
    for (int i = 0; i < MPPI_FR_JOINTS; i++) {
        f.velocity_minimum[i] = -0.05;
        f.velocity_maximum[i] = 0.05;
        f.acceleration_minimum[i] = -1.0;
        f.acceleration_maximum[i] = 1.0;
    }
    return f;
}

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    static_assert(sizeof(mppi_safety_filter_desc) == 608 && offsetof(mppi_safety_filter_desc, velocity_minimum) == 192 &&
                      offsetof(mppi_safety_filter_desc, reach_maximum) == 576 && offsetof(mppi_safety_filter_desc, limit_joints) == 592,
                  "mppi_safety_filter_desc layout");
    mppi_safety_filter_desc def;
    mppi_default_safety_filter(&def);
    if (def.limit_joints || def.limit_velocity || def.limit_acceleration || def.limit_reach) return fail("default switches");
    if (def.position_minimum[6] != -3.0718 || def.position_maximum[6] != 0.0698 || def.velocity_maximum[3] != 2.175 ||
        def.velocity_minimum[9] != -2.61 || def.velocity_maximum[0] != 1.0 || def.velocity_maximum[11] != 0.3)
        return fail("default limits");
    if (!std::isinf(def.acceleration_maximum[4]) || def.acceleration_minimum[4] > 0) return fail("default acceleration limits");
    if (def.reach_maximum != 0.8 || def.reach_minimum != 0.15) return fail("default reach");
    auto f = TrajectorySafetyFilter::create(tight());
    mppi_safety_filter_desc d;
    if (!f->describe(d) || !d.limit_velocity || d.limit_joints || d.velocity_maximum[5] != 0.05 || d.acceleration_minimum[2] != -1.0 ||
        d.position_maximum[8] != def.position_maximum[8])
        return fail("describe");
    const mppi::Filter *as_filter = f.get();   // the reference's interface
    if (!dynamic_cast<const mppi::DeviceFilter *>(as_filter)) return fail("DeviceFilter mixin");
    {   // a filter without a descriptor is refused before anything touches the device
        PinocchioDynamics::Configuration dc;
        FrankaRidgeback::AssistedManipulation::Configuration ac;
        mppi_assisted_manipulation_default(&ac);
        auto t = mppi::Trajectory::create(configuration(), PinocchioDynamics::create(dc),
                                          FrankaRidgeback::AssistedManipulation::create(ac), std::make_unique<HostOnlyFilter>());
        if (t) return fail("a filter without a descriptor was accepted");
    }
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    PinocchioDynamics::Configuration dc;
    FrankaRidgeback::AssistedManipulation::Configuration ac;
    mppi_assisted_manipulation_default(&ac);
    auto t = mppi::Trajectory::create(configuration(), PinocchioDynamics::create(dc), FrankaRidgeback::AssistedManipulation::create(ac),
                                      TrajectorySafetyFilter::create(tight()));
    if (!t) return fail("Trajectory::create with a safety filter");
    mppi_safety_filter_desc back{};
    const bool on = t->safety_filter(&back);
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    t->update(x, 0.0);
    t->update(x, 0.01);
    const auto U = t->get_optimal_rollout(), Uu = t->get_unfiltered_rollout();
    double diff = 0.0;
    for (size_t i = 0; i < U.size(); i++) diff = std::fmax(diff, std::fabs(U[i] - Uu[i]));
    std::printf("{\"enabled\": %s, \"vmax\": %.17g, \"changed_steps\": %lld, \"steps\": %d, \"max_change\": %.17g}\n", on ? "true" : "false",
                back.velocity_maximum[4], (long long)t->safety_filter_changed_steps(), (int)(U.size() / MPPI_FR_CONTROL), diff);
    const bool off = t->set_safety_filter(nullptr);
    t->update(x, 0.02);
    const auto U2 = t->get_optimal_rollout(), Uu2 = t->get_unfiltered_rollout();
    std::printf("{\"turned_off\": %s, \"reports\": %s, \"same\": %s}\n", off ? "true" : "false", t->safety_filter() ? "true" : "false",
                U2 == Uu2 ? "true" : "false");

    // the host-callable filter() against the C call on an object at the same state
    auto filt = TrajectorySafetyFilter::create(tight());
    mppi::VectorXd u(MPPI_FR_CONTROL), u_in(MPPI_FR_CONTROL);
    for (int i = 0; i < MPPI_FR_CONTROL; i++) u[i] = u_in[i] = (i >= 3 && i < 10) ? 40.0 - 5.0 * i : (i < 3 ? 0.4 : 0.0);
    const mppi::VectorXd out = filt->filter(x, u, 0.0);
    auto obj = PinocchioDynamics::create(dc);
    obj->set_state(x, 0.0);
    double c_out[MPPI_FR_CONTROL];
    filt->describe(d);
    if (mppi_dynamics_safety_filter(obj->object(), &d, u_in.data(), 0.01, c_out) != MPPI_OK) return fail("mppi_dynamics_safety_filter");
    bool same = true, in_place = true, moved = false;
    for (int i = 0; i < MPPI_FR_CONTROL; i++) {
        same = same && out[i] == c_out[i];
        in_place = in_place && u[i] == out[i];
        moved = moved || out[i] != u_in[i];
    }
    std::printf("{\"filter_same\": %s, \"in_place\": %s, \"moved\": %s, \"fingers\": %s}\n", same ? "true" : "false",
                in_place ? "true" : "false", moved ? "true" : "false", (out[10] == u_in[10] && out[11] == u_in[11]) ? "true" : "false");
    return 0;
}
