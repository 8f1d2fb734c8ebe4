// The C++ surface of obstacle avoidance with a distance field (include/mppi_amd.hpp):
//  - without arguments: the struct's layout and the constants; prints {"cpu": "ok"} (no GPU touched);
//  - with "gpu": Trajectory::set_distance_field_avoidance / set_distance_field / get_optimal_field_cost
//    around two updates (a ball on the forearm's axis, then no field), the refusals (before capsules
//    are enabled, after the first update), and PinocchioDynamics::distance_field_cost against the C
//    call.  One JSON line per check.
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
    std::fprintf(stderr, "distance_field: %s\n", what);
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
    static_assert(sizeof(mppi_distance_field) == 56 && offsetof(mppi_distance_field, segment_samples) == 12 &&
                      offsetof(mppi_distance_field, mask) == 16 && offsetof(mppi_distance_field, origin) == 24 &&
                      offsetof(mppi_distance_field, voxel) == 48,
                  "mppi_distance_field layout");
    static_assert(MPPI_DISTANCE_FIELD_MIN_DIM == 2 && MPPI_DISTANCE_FIELD_MAX_DIM == 512 && MPPI_DISTANCE_FIELD_MAX_VALUES == 16777216 &&
                      MPPI_DISTANCE_FIELD_MAX_SAMPLES == 8 && MPPI_AMD_ABI_VERSION == 5,
                  "constants");
    std::printf("{\"cpu\": \"ok\"}\n");
    if (!gpu) return 0;

    // a ball of 3 cm on the forearm's axis in a 0.05 m grid around the robot
    mppi_distance_field f{};
    f.dims[0] = 63, f.dims[1] = 61, f.dims[2] = 47;
    f.segment_samples = 3;
    f.mask = MPPI_OBSTACLE_MASK_SEGMENTS & ~MPPI_OBSTACLE_MASK_SEGMENT(0);
    f.origin[0] = -1.0, f.origin[1] = -1.0, f.origin[2] = -0.5;
    f.voxel = 0.05;
    std::vector<float> values((size_t)f.dims[0] * f.dims[1] * f.dims[2]);
    for (int i = 0; i < f.dims[0]; i++)
        for (int j = 0; j < f.dims[1]; j++)
            for (int k = 0; k < f.dims[2]; k++) {
                const double x = f.origin[0] + i * f.voxel - 0.7106, y = f.origin[1] + j * f.voxel - 0.7176, z = f.origin[2] + k * f.voxel - 1.1857;
                values[((size_t)i * f.dims[1] + j) * f.dims[2] + k] = (float)(std::sqrt(x * x + y * y + z * z) - 0.03);
            }

    auto t = trajectory();
    if (!t) return fail("Trajectory::create");
    if (!t->set_obstacle_avoidance()) return fail("set_obstacle_avoidance");
    const bool early = t->set_distance_field_avoidance();   // needs capsules
    if (!t->set_obstacle_capsules()) return fail("set_obstacle_capsules");
    const bool unset = t->set_distance_field(&f, values.data());   // needs field avoidance
    if (!t->set_distance_field_avoidance()) return fail("set_distance_field_avoidance");
    std::printf("{\"before_capsules\": %s, \"field_before_avoidance\": %s}\n", early ? "true" : "false", unset ? "true" : "false");
    if (!t->set_distance_field(&f, values.data())) return fail("set_distance_field");
    mppi::VectorXd x(MPPI_FR_STATE);
    mppi_frankaridgeback_huddled(x.data());
    t->update(x, 0.0);
    const double with_field = t->get_optimal_field_cost(), total = t->get_optimal_obstacle_cost();
    if (!t->set_distance_field(nullptr, nullptr)) return fail("clearing the field");
    t->update(x, 0.01);
    const double cleared = t->get_optimal_field_cost();
    std::printf("{\"with_field\": %.17g, \"obstacle_cost\": %.17g, \"cleared\": %.17g, \"late_enable\": %s}\n", with_field, total, cleared,
                t->set_distance_field_avoidance() ? "true" : "false");

    // the dynamics object: the class's call against the C call
    PinocchioDynamics::Configuration dc;
    dc.link_positions = true;
    auto d = PinocchioDynamics::create(dc);
    d->set_state(x, 0.0);
    const double a = d->distance_field_cost(f, values.data());
    double b = 0.0;
    if (mppi_dynamics_distance_field_cost(d->object(), nullptr, nullptr, &f, values.data(), &b) != MPPI_OK)
        return fail("mppi_dynamics_distance_field_cost");
    std::printf("{\"object_cost\": %.17g, \"same\": %s}\n", a, a == b ? "true" : "false");
    return 0;
}
