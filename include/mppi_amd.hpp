// mppi_amd.hpp — header-only C++ drop-in for the reference's src/controller/mppi.hpp, over the
// C-ABI of mppi_amd.h (link libmppi_amd.so).
//
// Same class names, member names, argument meaning and error behaviour as the reference:
//   mppi::Dynamics / Cost / Filter  mppi.hpp:30-176    the reference's pure virtuals, unchanged, so a
//                                                       plugin written against the reference compiles
//   mppi::DeviceDynamics / DeviceCost                   mixin: the device descriptor the kernels
//                                                       evaluate; create() refuses plugins without it
//                                                       (there is no CPU rollout path)
//   mppi::Configuration             mppi.hpp:181-249   (Eigen members -> std::vector, column-major)
//   mppi::Trajectory                mppi.hpp:267-658   (create returns nullptr + stderr on error;
//                                                       optimise()'s "all nan rollouts" throws)
//   FrankaRidgeback::PinocchioDynamics, AssistedManipulation, TrackPoint, DynamicsForecast: the
//   reference's plugins, their methods run on the device (mppi_dynamics_*, mppi_cost_evaluate).
// Vector types: Eigen's when <Eigen/Dense> is available (the reference's own signatures), else
// mppi::VectorXd / mppi::Ref below, which carry the data() / size() / operator[] the engine uses.
// Trajectory's update / get take anything with data() / size().
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <iostream>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "mppi_amd.h"
#include "mppi_amd_frankaridgeback.h"

#if __has_include(<Eigen/Dense>)
#include <Eigen/Dense>
namespace mppi {
using VectorXd = Eigen::VectorXd;
template <class T>
using Ref = Eigen::Ref<T>;
}  // namespace mppi
#else
namespace mppi {
// An owning dense vector of doubles (the part of Eigen::VectorXd the plugin surface needs).
class VectorXd {
public:
    VectorXd() = default;
    explicit VectorXd(std::ptrdiff_t n) : m_v((size_t)n, 0.0) {}
    VectorXd(std::initializer_list<double> l) : m_v(l) {}
    static VectorXd Zero(std::ptrdiff_t n) { return VectorXd(n); }
    double *data() { return m_v.data(); }
    const double *data() const { return m_v.data(); }
    std::ptrdiff_t size() const { return (std::ptrdiff_t)m_v.size(); }
    double &operator[](std::ptrdiff_t i) { return m_v[(size_t)i]; }
    double operator[](std::ptrdiff_t i) const { return m_v[(size_t)i]; }
    double &operator()(std::ptrdiff_t i) { return m_v[(size_t)i]; }
    double operator()(std::ptrdiff_t i) const { return m_v[(size_t)i]; }
    void resize(std::ptrdiff_t n) { m_v.assign((size_t)n, 0.0); }
    void setZero() { std::fill(m_v.begin(), m_v.end(), 0.0); }

private:
    std::vector<double> m_v;
};
// A non-owning view of a vector (Eigen::Ref<VectorXd>): what step() / get_state() return.
template <class T>
class Ref {
public:
    Ref(T &v) : m_p(v.data()), m_n(v.size()) {}
    Ref(double *p, std::ptrdiff_t n) : m_p(p), m_n(n) {}
    double *data() const { return m_p; }
    std::ptrdiff_t size() const { return m_n; }
    double &operator[](std::ptrdiff_t i) const { return m_p[i]; }
    double &operator()(std::ptrdiff_t i) const { return m_p[i]; }

private:
    double *m_p;
    std::ptrdiff_t m_n;
};
}  // namespace mppi
#endif

namespace mppi {

// mppi::Dynamics (mppi.hpp:30-85): the reference's pure virtuals.
class Dynamics {
public:
    virtual ~Dynamics() = default;
    virtual std::unique_ptr<Dynamics> copy() = 0;                             // :47
    virtual Ref<VectorXd> step(const VectorXd &control, double dt) = 0;      // :58
    virtual void set_state(const VectorXd &state, double time) = 0;          // :66
    virtual Ref<VectorXd> get_state() = 0;                                    // :72
    virtual int get_control_dof() = 0;                                        // :78
    virtual int get_state_dof() = 0;                                          // :84
};

// mppi::Cost (mppi.hpp:93-145).
class Cost {
public:
    virtual ~Cost() = default;
    virtual std::unique_ptr<Cost> copy() = 0;                                 // :110
    virtual void reset(double time) = 0;                                      // :115
    virtual double get_cost(const VectorXd &state, const VectorXd &control, Dynamics *dynamics,
                            double time) = 0;                                 // :127-132
    virtual int get_control_dof() = 0;                                        // :138
    virtual int get_state_dof() = 0;                                          // :144
};

// mppi::Filter (mppi.hpp:150-176).
class Filter {
public:
    virtual ~Filter() = default;
    virtual VectorXd filter(Ref<VectorXd> state, Ref<VectorXd> control, double time) = 0;   // :163-167
    virtual void reset(Ref<VectorXd> state, double time) = 0;                                // :175
};

// The device descriptors a plugin provides so the rollout kernels can evaluate it (the plugin's
// own step / get_cost are the host-callable methods; the rollouts never call back into the host).
class DeviceDynamics {
public:
    virtual ~DeviceDynamics() = default;
    virtual bool describe(mppi_dynamics_desc &out) const = 0;
    // the link-position model the rollouts of a trajectory on this dynamics use
    // (MPPI_LINK_POSITIONS_*), or -1: the handle's own (the stub, or what MPPI_LINK_POSITIONS says)
    virtual int link_positions() const { return -1; }
    // the simulated end-effector wrench of those rollouts (MPPI_SIMULATED_WRENCH_*), or -1: the
    // handle's own (off, or what MPPI_SIMULATED_WRENCH says)
    virtual int simulated_wrench() const { return -1; }
};
class DeviceCost {
public:
    virtual ~DeviceCost() = default;
    virtual bool describe(mppi_cost_desc &out) const = 0;
    // the optimal rollout's per-term totals after an update (mppi_optimal_terms), for plugins that
    // keep the reference's accumulators (AssistedManipulation); the default ignores them
    virtual void set_optimal_terms(const double *) {}
};

// A trajectory filter the device can run: it describes itself as the engine's safety filter
// (mppi_safety_filter_desc).  Its own filter() stays host-callable; updates never call back into it.
class DeviceFilter {
public:
    virtual ~DeviceFilter() = default;
    virtual bool describe(mppi_safety_filter_desc &out) const = 0;
};

struct Configuration {
    std::vector<double> initial_state;
    std::int64_t rollouts = 0;
    std::int64_t keep_best_rollouts = 0;
    double time_step = 0.01;
    double horison = 0.0;
    double gradient_step = 1.0;
    double cost_scale = 1.0;
    double cost_discount_factor = 1.0;
    std::vector<double> covariance;   // C x C, column-major (Eigen's default)
    bool control_bound = false;
    std::vector<double> control_min;
    std::vector<double> control_max;
    std::optional<std::vector<double>> control_default;
    struct Smoothing {
        unsigned int window;
        unsigned int order;
    };
    std::optional<Smoothing> smoothing;
    unsigned int threads = 1;
};

// What the gripper carries (mppi_set_held_object): up to MPPI_HELD_POINTS spheres with centres in the
// grasp frame, in metres, and the segments between consecutive ones.  segment_radii: one per segment
// (centres.size() - 1 of them; missing ones are 0).
struct HeldObject {
    std::vector<std::array<double, 3>> centres;
    std::vector<double> radii;
    std::vector<double> segment_radii;

    // the C struct; a size that does not fit reaches the engine's own check (count out of range)
    mppi_held_object to_c() const
    {
        mppi_held_object o{};
        o.count = (int32_t)centres.size();
        for (size_t i = 0; i < centres.size() && i < (size_t)MPPI_HELD_POINTS; i++) {
            for (int a = 0; a < 3; a++) o.centres[i][a] = centres[i][(size_t)a];
            o.radii[i] = i < radii.size() ? radii[i] : 0.0;
        }
        for (size_t s = 0; s + 1 < centres.size() && s < (size_t)MPPI_HELD_SEGMENTS; s++) o.segment_radii[s] = s < segment_radii.size() ? segment_radii[s] : 0.0;
        return o;
    }
    static HeldObject from_c(const mppi_held_object &o)
    {
        HeldObject h;
        for (int i = 0; i < o.count && i < MPPI_HELD_POINTS; i++) {
            h.centres.push_back({o.centres[i][0], o.centres[i][1], o.centres[i][2]});
            h.radii.push_back(o.radii[i]);
        }
        for (int s = 0; s + 1 < o.count && s < MPPI_HELD_SEGMENTS; s++) h.segment_radii.push_back(o.segment_radii[s]);
        return h;
    }
};

// The held object against the robot's own segments (mppi_set_held_self): units bit i held point i, bit
// 4 + s held segment s; segments bit s robot segment s with radii[s].  The defaults are mppi_default_held_self's.
struct HeldSelf {
    uint32_t units = MPPI_HELD_SELF_UNITS;
    uint32_t segments = 0x1Fu;
    std::array<double, MPPI_HELD_SELF_SEGMENTS> radii{{0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1}};

    mppi_held_self to_c() const
    {
        mppi_held_self c{};
        c.units = units;
        c.segments = segments;
        for (int s = 0; s < MPPI_HELD_SELF_SEGMENTS; s++) c.radii[s] = radii[(size_t)s];
        return c;
    }
    static HeldSelf from_c(const mppi_held_self &c)
    {
        HeldSelf h;
        h.units = c.units;
        h.segments = c.segments;
        for (int s = 0; s < MPPI_HELD_SELF_SEGMENTS; s++) h.radii[(size_t)s] = c.radii[s];
        return h;
    }
};

class Trajectory {
public:
    struct Rollout {
        std::vector<double> noise;   // C x H column-major
        double cost;
    };

    static std::unique_ptr<Trajectory> create(const Configuration &configuration, std::unique_ptr<Dynamics> &&dynamics,
                                              std::unique_ptr<Cost> &&cost, std::unique_ptr<Filter> &&filter = nullptr,
                                              int device = 0)
    {
        // the reference's Actor passes nullptr (actor.cpp:100).  A filter that describes itself
        // (mppi::DeviceFilter: FrankaRidgeback::TrajectorySafetyFilter) runs on the device; any other
        // would have to be called from the update and is refused.
        mppi_safety_filter_desc fd{};
        const DeviceFilter *fdev = dynamic_cast<const DeviceFilter *>(filter.get());
        if (filter && (!fdev || !fdev->describe(fd))) {
            std::cerr << "mppi_amd: trajectory filters are not supported on the device" << std::endl;
            return nullptr;
        }
        mppi_dynamics_desc dd{};
        mppi_cost_desc cd{};
        const DeviceDynamics *ddev = dynamic_cast<const DeviceDynamics *>(dynamics.get());
        const DeviceCost *cdev = dynamic_cast<const DeviceCost *>(cost.get());
        if (!ddev || !ddev->describe(dd) || !cdev || !cdev->describe(cd)) {
            std::cerr << "mppi_amd: dynamics and cost must provide a device descriptor (mppi::DeviceDynamics / "
                         "mppi::DeviceCost); there is no CPU rollout path" << std::endl;
            return nullptr;
        }
        mppi_config c{};
        c.initial_state = configuration.initial_state.data();
        c.state_dof = (int64_t)configuration.initial_state.size();
        c.control_dof = (int64_t)configuration.control_min.size();
        c.rollouts = configuration.rollouts;
        c.keep_best_rollouts = configuration.keep_best_rollouts;
        c.time_step = configuration.time_step;
        c.horison = configuration.horison;
        c.gradient_step = configuration.gradient_step;
        c.cost_scale = configuration.cost_scale;
        c.cost_discount_factor = configuration.cost_discount_factor;
        if (configuration.covariance.size() != (size_t)(c.control_dof * c.control_dof)) {
            std::cerr << "controller covariance matrix not square" << std::endl;
            return nullptr;
        }
        c.covariance = configuration.covariance.data();
        c.control_bound = configuration.control_bound;
        c.control_min = configuration.control_min.data();
        c.control_max = configuration.control_max.data();
        c.has_control_default = configuration.control_default.has_value();
        c.control_default = configuration.control_default ? configuration.control_default->data() : nullptr;
        c.has_smoothing = configuration.smoothing.has_value();
        c.smoothing_window = configuration.smoothing ? configuration.smoothing->window : 0;
        c.smoothing_order = configuration.smoothing ? configuration.smoothing->order : 0;
        c.threads = configuration.threads;
        mppi_handle *h = nullptr;
        if (mppi_create(&c, &dd, &cd, device, &h) != MPPI_OK) {
            std::cerr << mppi_last_error(nullptr) << std::endl;   // the reference prints and returns nullptr
            return nullptr;
        }
        if (ddev->link_positions() >= 0 && mppi_set_link_positions(h, ddev->link_positions()) != MPPI_OK) {
            std::cerr << mppi_last_error(nullptr) << std::endl;
            mppi_destroy(h);
            return nullptr;
        }
        if (ddev->simulated_wrench() >= 0 && mppi_set_simulated_wrench(h, ddev->simulated_wrench()) != MPPI_OK) {
            std::cerr << mppi_last_error(nullptr) << std::endl;
            mppi_destroy(h);
            return nullptr;
        }
        if (filter && mppi_set_safety_filter(h, &fd) != MPPI_OK) {
            std::cerr << mppi_last_error(h) << std::endl;
            mppi_destroy(h);
            return nullptr;
        }
        std::unique_ptr<Trajectory> t(new Trajectory(h, configuration, std::move(dynamics), std::move(cost)));
        t->m_filter = std::move(filter);
        return t;
    }

    ~Trajectory() { mppi_destroy(m_h); }
    // whether the rollouts use the kinematic link-position model (mppi_get_link_positions)
    bool link_positions() const
    {
        int mode = MPPI_LINK_POSITIONS_ZERO;
        return mppi_get_link_positions(m_h, &mode) == MPPI_OK && mode == MPPI_LINK_POSITIONS_KINEMATIC;
    }
    // the rollouts' simulated end-effector wrench (MPPI_SIMULATED_WRENCH_*): set before the first
    // update (mppi_set_simulated_wrench; false and a message on stderr otherwise)
    bool set_simulated_wrench(int mode)
    {
        if (mppi_set_simulated_wrench(m_h, mode) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    int simulated_wrench() const
    {
        int mode = MPPI_SIMULATED_WRENCH_OFF;
        return mppi_get_simulated_wrench(m_h, &mode) == MPPI_OK ? mode : MPPI_SIMULATED_WRENCH_OFF;
    }
    // The safety filter (mppi_set_safety_filter; nullptr: off), between any two updates; false and
    // a message on stderr when it is refused
    bool set_safety_filter(const mppi_safety_filter_desc *filter)
    {
        if (mppi_set_safety_filter(m_h, filter) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // whether one is set, and its configuration
    bool safety_filter(mppi_safety_filter_desc *out = nullptr) const
    {
        int on = 0;
        return mppi_get_safety_filter(m_h, &on, out) == MPPI_OK && on != 0;
    }
    // the plan as optimise() left it, before the safety filter (C x H column-major, like get_optimal_rollout)
    std::vector<double> get_unfiltered_rollout() const { return fetch(mppi_unfiltered_control, (size_t)(m_C * m_H)); }
    // the steps of the last update's plan the safety filter changed
    std::int64_t safety_filter_changed_steps() const
    {
        int64_t n = 0;
        (void)mppi_safety_filter_stats(m_h, &n, nullptr);
        return n;
    }
    // Obstacle avoidance (mppi_set_obstacle_avoidance; nullptr: the default configuration): sphere
    // and half-space obstacles in the rollouts' objective.  A FrankaRidgeback trajectory in the
    // kinematic link-position model, before the first update; false and a message on stderr otherwise.
    bool set_obstacle_avoidance(const mppi_obstacle_config *config = nullptr)
    {
        if (mppi_set_obstacle_avoidance(m_h, config) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // whether it is on, and the configuration it runs with
    bool obstacle_avoidance(mppi_obstacle_config *out = nullptr) const
    {
        int on = 0;
        return mppi_get_obstacle_avoidance(m_h, &on, out) == MPPI_OK && on != 0;
    }
    // Capsules (mppi_set_obstacle_capsules; nullptr: the default radii): the robot's eight segments and
    // capsule obstacles in the obstacle term.  After set_obstacle_avoidance, before the first update;
    // false and a message on stderr otherwise.
    bool set_obstacle_capsules(const mppi_capsule_config *config = nullptr)
    {
        if (mppi_set_obstacle_capsules(m_h, config) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // whether they are on, and the radii the handle runs with
    bool obstacle_capsules(mppi_capsule_config *out = nullptr) const
    {
        int on = 0;
        return mppi_get_obstacle_capsules(m_h, &on, out) == MPPI_OK && on != 0;
    }
    // A signed-distance grid of the sensed environment behind the capsule term
    // (mppi_set_distance_field_avoidance): after set_obstacle_capsules, before the first update; false
    // and a message on stderr otherwise.
    bool set_distance_field_avoidance()
    {
        if (mppi_set_distance_field_avoidance(m_h) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // the field (mppi_set_distance_field; nullptr: no field), replaced between any two updates
    bool set_distance_field(const mppi_distance_field *field, const float *values)
    {
        if (mppi_set_distance_field(m_h, field, values) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // the field term of the optimal rollout, summed over its steps (mppi_optimal_field_cost)
    double get_optimal_field_cost()
    {
        double c = 0.0;
        if (mppi_optimal_field_cost(m_h, &c) != MPPI_OK) throw std::runtime_error(mppi_last_error(m_h));
        return c;
    }
    // A held object behind the field term (mppi_set_held_object_avoidance): after
    // set_distance_field_avoidance, before the first update; false and a message on stderr otherwise.
    bool set_held_object_avoidance()
    {
        if (mppi_set_held_object_avoidance(m_h) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    bool held_object_avoidance() const
    {
        int on = 0;
        return mppi_get_held_object_avoidance(m_h, &on) == MPPI_OK && on != 0;
    }
    // the object (mppi_set_held_object; nullptr: it was put down), replaced between any two updates
    bool set_held_object(const HeldObject *object)
    {
        mppi_held_object o{};
        if (object) o = object->to_c();
        if (mppi_set_held_object(m_h, object ? &o : nullptr) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    bool set_held_object(const HeldObject &object) { return set_held_object(&object); }
    // the current object, or nothing
    std::optional<HeldObject> held_object() const
    {
        mppi_held_object o{};
        int on = 0;
        if (mppi_get_held_object(m_h, &o, &on) != MPPI_OK || !on) return std::nullopt;
        return HeldObject::from_c(o);
    }
    // the held term of the optimal rollout, summed over its steps (mppi_optimal_held_cost)
    double get_optimal_held_cost()
    {
        double c = 0.0;
        if (mppi_optimal_held_cost(m_h, &c) != MPPI_OK) throw std::runtime_error(mppi_last_error(m_h));
        return c;
    }
    // The held object against the robot's own segments (mppi_set_held_self_avoidance): after
    // set_held_object_avoidance, before the first update; false and a message on stderr otherwise.
    bool set_held_self_avoidance()
    {
        if (mppi_set_held_self_avoidance(m_h) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    bool held_self_avoidance() const
    {
        int on = 0;
        return mppi_get_held_self_avoidance(m_h, &on) == MPPI_OK && on != 0;
    }
    // the configuration (mppi_set_held_self; nullptr: none), replaced between any two updates
    bool set_held_self(const HeldSelf *config)
    {
        mppi_held_self c{};
        if (config) c = config->to_c();
        if (mppi_set_held_self(m_h, config ? &c : nullptr) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    bool set_held_self(const HeldSelf &config) { return set_held_self(&config); }
    // the current configuration, or nothing
    std::optional<HeldSelf> get_held_self() const
    {
        mppi_held_self c{};
        int on = 0;
        if (mppi_get_held_self(m_h, &c, &on) != MPPI_OK || !on) return std::nullopt;
        return HeldSelf::from_c(c);
    }
    // the held-self term of the optimal rollout, summed over its steps (mppi_optimal_held_self_cost)
    double get_optimal_held_self_cost()
    {
        double c = 0.0;
        if (mppi_optimal_held_self_cost(m_h, &c) != MPPI_OK) throw std::runtime_error(mppi_last_error(m_h));
        return c;
    }
    // the held points' world paths at q_k (mppi_predicted_held_optimal / _rollouts): MPPI_HELD_POINTS x 3
    // doubles a step, NaN rows for the points the object does not have; H steps, and n x H in the order of
    // `rollouts` (global indices)
    std::vector<double> get_predicted_held_optimal() const { return fetch(mppi_predicted_held_optimal, (size_t)(m_H * MPPI_HELD_POINTS * 3)); }
    std::vector<double> get_predicted_held_rollouts(const std::vector<int64_t> &rollouts) const
    {
        std::vector<double> v(rollouts.size() * (size_t)(m_H * MPPI_HELD_POINTS * 3));
        check(mppi_predicted_held_rollouts(m_h, rollouts.data(), (int64_t)rollouts.size(), v.data()));
        return v;
    }
    // the whole set, given at reference time `time` (mppi_set_obstacles): between any two updates
    bool set_obstacles(const std::vector<mppi_obstacle> &obstacles, double time)
    {
        if (mppi_set_obstacles(m_h, obstacles.data(), (int32_t)obstacles.size(), time) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    std::vector<mppi_obstacle> obstacles(double *time = nullptr) const
    {
        std::vector<mppi_obstacle> out(MPPI_MAX_OBSTACLES);
        int32_t n = 0;
        if (mppi_get_obstacles(m_h, out.data(), &n, time) != MPPI_OK) n = 0;
        out.resize((size_t)n);
        return out;
    }
    // the obstacle term of the optimal rollout, summed over its steps (mppi_optimal_obstacle_cost)
    double get_optimal_obstacle_cost()
    {
        double c = 0.0;
        if (mppi_optimal_obstacle_cost(m_h, &c) != MPPI_OK) throw std::runtime_error(mppi_last_error(m_h));
        return c;
    }
    // Target tracking (mppi_set_target_tracking; nullptr: the defaults, position only): TrackPoint
    // follows a timed pose path.  A FrankaRidgeback trajectory with the TrackPoint objective, before
    // the first update; false and a message on stderr otherwise.
    bool set_target_tracking(const mppi_target_tracking_config *config = nullptr)
    {
        if (mppi_set_target_tracking(m_h, config) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // whether it is on, and the configuration it runs with
    bool target_tracking(mppi_target_tracking_config *out = nullptr) const
    {
        int on = 0;
        return mppi_get_target_tracking(m_h, &on, out) == MPPI_OK && on != 0;
    }
    // the path (mppi_set_target_path; nullptr: none, the objective's point again): between any two updates
    bool set_target_path(const mppi_target_path *path)
    {
        if (mppi_set_target_path(m_h, path) == MPPI_OK) return true;
        std::cerr << mppi_last_error(m_h) << std::endl;
        return false;
    }
    // the position and orientation terms of the optimal rollout, each summed over its steps (mppi_optimal_target_cost)
    std::array<double, 2> get_optimal_target_cost()
    {
        std::array<double, 2> c = {0.0, 0.0};
        if (mppi_optimal_target_cost(m_h, c.data()) != MPPI_OK) throw std::runtime_error(mppi_last_error(m_h));
        return c;
    }
    Trajectory(const Trajectory &) = delete;
    Trajectory &operator=(const Trajectory &) = delete;

    // Trajectory::update (mppi.cpp:154-187).  Throws std::runtime_error("all nan rollouts") like
    // optimise(), and std::runtime_error for device / smoothing failures.
    template <class Vec>
    void update(const Vec &state, double time)
    {
        update_raw(state.data(), (size_t)state.size(), time);
    }

    void update_raw(const double *state, size_t n, double time)
    {
        if (n != (size_t)m_X) throw std::invalid_argument("state has the wrong dimension");
        check(mppi_update(m_h, state, time));
        m_rolled_out_state.assign(state, state + n);
        m_update_last = time;
        ++m_update_count;
    }

    // Trajectory::get (mppi.cpp:481-512): `control` is pre-sized (Eigen::Ref<VectorXd> in the
    // reference).
    template <class Vec>
    void get(Vec &&control, double time)
    {
        check(mppi_get(m_h, time, control.data()));
    }

    std::vector<double> operator()(double time)
    {
        std::vector<double> u((size_t)m_C);
        check(mppi_get(m_h, time, u.data()));
        return u;
    }

    unsigned int get_state_dof() const { return (unsigned int)m_X; }
    unsigned int get_control_dof() const { return (unsigned int)m_C; }
    double get_time_step() const { return m_configuration.time_step; }
    unsigned int get_step_count() const { return (unsigned int)m_H; }
    double get_update_duration() const
    {
        double d = 0;
        mppi_update_duration(m_h, &d);
        return d;
    }
    double get_update_last() const { return m_update_last; }
    std::size_t get_update_count() const { return m_update_count; }
    std::size_t get_rollout_count() const { return (std::size_t)m_R; }
    const std::vector<double> &get_rolled_out_state() const { return m_rolled_out_state; }

    std::vector<double> get_weights() const { return fetch(mppi_weights, (size_t)m_R); }
    std::vector<double> get_gradient() const { return fetch(mppi_gradient, (size_t)(m_C * m_H)); }
    std::vector<double> get_optimal_rollout() const { return fetch(mppi_optimal_control, (size_t)(m_C * m_H)); }
    std::vector<double> trajectory() const { return get_optimal_rollout(); }
    std::vector<double> get_costs() const { return fetch(mppi_costs, (size_t)m_R); }

    std::vector<Rollout> get_rollouts() const
    {
        std::vector<double> n = fetch(mppi_noise, (size_t)(m_R * m_C * m_H));
        std::vector<double> c = get_costs();
        std::vector<Rollout> out((size_t)m_R);
        for (int64_t r = 0; r < m_R; r++) {
            out[(size_t)r].noise.assign(n.begin() + r * m_C * m_H, n.begin() + (r + 1) * m_C * m_H);
            out[(size_t)r].cost = c[(size_t)r];
        }
        return out;
    }

    double get_optimal_total_cost() const
    {
        double c = 0;
        mppi_optimal_cost(m_h, &c);
        return c;
    }

    // Thread 0's cost after filter() (mppi.hpp:448-454): BaseTest downcasts it to read the per-term
    // totals (base.cpp:140-146), so a cost that keeps them gets the optimal rollout's here.
    const Cost &get_optimal_cost() const
    {
        if (DeviceCost *dc = dynamic_cast<DeviceCost *>(m_cost.get())) {
            double t[7];
            if (mppi_optimal_terms(m_h, t) == MPPI_OK) dc->set_optimal_terms(t);
        }
        return *m_cost;
    }
    const Dynamics &get_optimal_dynamics() const { return *m_dynamics; }

    // Where the robot goes under the published plan and under the last update's rollouts
    // (mppi_predicted_optimal / mppi_predicted_rollouts): rows of MPPI_PRED_N doubles, row k the
    // state x_k (MPPI_PRED_Q, _QD, _ENERGY) and the frame and link positions at q_k (MPPI_PRED_EE,
    // _ARM_MOUNT, _LINKS); H rows, and n x H rows in the order of `rollouts` (global indices).
    std::vector<double> get_predicted_optimal() const { return fetch(mppi_predicted_optimal, (size_t)(m_H * MPPI_PRED_N)); }
    std::vector<double> get_predicted_rollouts(const std::vector<int64_t> &rollouts) const
    {
        std::vector<double> v(rollouts.size() * (size_t)(m_H * MPPI_PRED_N));
        check(mppi_predicted_rollouts(m_h, rollouts.data(), (int64_t)rollouts.size(), v.data()));
        return v;
    }

    // Per-update inputs and parity hooks of the device engine.
    template <class Vec>
    void set_forecast(const Vec &wrench_Hx6) { check(mppi_set_forecast(m_h, wrench_Hx6.data())); }
    void set_noise_source(int source, uint64_t seed = 0x5EED) { check(mppi_set_noise_source(m_h, source, seed)); }
    // The wrench forecast on the device (DynamicsForecast::observe_wrench / observe_time and
    // Forecast::forecast, dynamics.hpp:221-278): every update samples it at t0 + k dt.
    void attach_forecast(const mppi_forecast_config *configuration) { check(mppi_forecast_attach(m_h, configuration)); }
    void observe_wrench(const double *wrench6, double time) { check(mppi_forecast_observe(m_h, wrench6, time)); }
    void observe_time(double time) { check(mppi_forecast_observe_time(m_h, time)); }
    void forecast(double time, double *wrench6) { check(mppi_forecast_get(m_h, time, wrench6)); }
    void forecast_table(double t0, double dt, int64_t steps, double *out) { check(mppi_forecast_table(m_h, t0, dt, steps, out)); }
    mppi_handle *handle() const { return m_h; }

private:
    Trajectory(mppi_handle *h, const Configuration &c, std::unique_ptr<Dynamics> &&d, std::unique_ptr<Cost> &&k)
        : m_h(h), m_configuration(c), m_dynamics(std::move(d)), m_cost(std::move(k))
    {
        mppi_dims(m_h, &m_R, &m_H, &m_C, &m_X);
        m_rolled_out_state.assign((size_t)m_X, 0.0);   // m_rollout_state.setZero() (mppi.cpp:121)
    }

    void check(mppi_status st) const
    {
        if (st == MPPI_OK) return;
        throw std::runtime_error(st == MPPI_ERR_ALL_NAN ? std::string("all nan rollouts") : std::string(mppi_last_error(m_h)));
    }

    template <class F>
    std::vector<double> fetch(F fn, size_t n) const
    {
        std::vector<double> v(n);
        check(fn(m_h, v.data()));
        return v;
    }

    mppi_handle *m_h;
    Configuration m_configuration;
    std::unique_ptr<Dynamics> m_dynamics;
    std::unique_ptr<Cost> m_cost;
    std::unique_ptr<Filter> m_filter;   // the described filter create() took (kept alive, never called)
    int64_t m_R = 0, m_H = 0, m_C = 0, m_X = 0;
    std::vector<double> m_rolled_out_state;
    double m_update_last = 0;
    std::size_t m_update_count = 0;
};

}  // namespace mppi

namespace FrankaRidgeback {

// A wrench (force, moment) as the reference passes it (dynamics.hpp: Vector6d).
#if __has_include(<Eigen/Dense>)
using Vector6d = Eigen::Matrix<double, 6, 1>;
#else
struct Vector6d {
    double v[6] = {0, 0, 0, 0, 0, 0};
    static Vector6d Zero() { return Vector6d{}; }
    double *data() { return v; }
    const double *data() const { return v; }
    double &operator[](std::ptrdiff_t i) { return v[i]; }
    double operator[](std::ptrdiff_t i) const { return v[i]; }
    double &operator()(std::ptrdiff_t i) { return v[i]; }
    double operator()(std::ptrdiff_t i) const { return v[i]; }
};
#endif

// EndEffectorState (dynamics.hpp:95-117); orientation as (x, y, z, w) and as a row-major matrix.
struct EndEffectorState {
    double position[3];
    double orientation[4];
    double rotation[9];
    double linear_velocity[3], angular_velocity[3];
    double linear_acceleration[3], angular_acceleration[3];
    double jacobian[72];   // 6 x 12 row-major, WORLD

    static EndEffectorState from_row(const double *r)
    {
        EndEffectorState s{};
        std::copy(r + MPPI_EE_POSITION, r + MPPI_EE_POSITION + 3, s.position);
        std::copy(r + MPPI_EE_QUATERNION, r + MPPI_EE_QUATERNION + 4, s.orientation);
        std::copy(r + MPPI_EE_ROTATION, r + MPPI_EE_ROTATION + 9, s.rotation);
        std::copy(r + MPPI_EE_LINEAR_VELOCITY, r + MPPI_EE_LINEAR_VELOCITY + 3, s.linear_velocity);
        std::copy(r + MPPI_EE_ANGULAR_VELOCITY, r + MPPI_EE_ANGULAR_VELOCITY + 3, s.angular_velocity);
        std::copy(r + MPPI_EE_LINEAR_ACCELERATION, r + MPPI_EE_LINEAR_ACCELERATION + 3, s.linear_acceleration);
        std::copy(r + MPPI_EE_ANGULAR_ACCELERATION, r + MPPI_EE_ANGULAR_ACCELERATION + 3, s.angular_acceleration);
        std::copy(r + MPPI_EE_JACOBIAN, r + MPPI_EE_JACOBIAN + 72, s.jacobian);
        return s;
    }
};

// FrankaRidgeback::Link (dynamics.hpp:65-80): the universe, then the model's bodies in order
enum class Link {
    OMNI_BASE_ROOT_LINK = MPPI_LINK_OMNI_BASE_ROOT_LINK,
    X_SLIDER,
    Y_SLIDER,
    PIVOT,
    PANDA_LINK1,
    PANDA_LINK2,
    PANDA_LINK3,
    PANDA_LINK4,
    PANDA_LINK5,
    PANDA_LINK6,
    PANDA_LINK7,
    PANDA_LEFTFINGER,
    PANDA_RIGHTFINGER,
    _SIZE
};
static_assert((int)Link::_SIZE == MPPI_LINK_N && (int)Link::PANDA_RIGHTFINGER == MPPI_LINK_PANDA_RIGHTFINGER, "Link enum");

// FrankaRidgeback::PinocchioDynamics (pinocchio_dynamics.hpp:30-427).  The rollouts evaluate the
// body table (describe(): generated from robot.urdf by default); the object itself, when its
// methods are called, is a device object (mppi_dynamics_*) created at the first call with the
// configuration's initial state (the constructor's set_state, pinocchio_dynamics.cpp:84-115).
class PinocchioDynamics : public mppi::Dynamics, public mppi::DeviceDynamics {
public:
    struct Configuration {
        std::vector<double> initial_state;   // State (31); HUDDLED when empty
        int device = 0;
        // the kinematic link-position model (mppi_set_link_positions): get_link_position answers
        // the links' body-frame positions of the last calculate(), here and in the rollouts of a
        // Trajectory created on this dynamics.  false: the handle's default (the reference's stub,
        // zeros, unless MPPI_LINK_POSITIONS=1)
        bool link_positions = false;
        // the simulated end-effector wrench (mppi_set_simulated_wrench) of the rollouts of a
        // Trajectory created on this dynamics, MPPI_SIMULATED_WRENCH_OFF / _STATE / _FORECAST; any
        // mode but OFF also makes this object's forecast apply its wrench rows.  -1: the handle's
        // default (off, unless MPPI_SIMULATED_WRENCH says otherwise)
        int simulated_wrench = -1;
    };
    // wrench forecast(time) of the dynamics' forecast handle (DynamicsForecast::Handle), or none
    using WrenchSource = std::function<bool(double time, double *wrench6)>;

    PinocchioDynamics() { mppi_frankaridgeback_model(&m_model); }
    explicit PinocchioDynamics(const mppi_frankaridgeback_desc &model) : m_model(model) {}
    PinocchioDynamics(const mppi_frankaridgeback_desc &model, const Configuration &c) : m_model(model), m_configuration(c) {}
    static std::unique_ptr<PinocchioDynamics> create(const Configuration &c)
    {
        mppi_frankaridgeback_desc m;
        mppi_frankaridgeback_model(&m);
        return std::make_unique<PinocchioDynamics>(m, c);
    }
    ~PinocchioDynamics() override { mppi_dynamics_destroy(m_obj); }

    std::unique_ptr<mppi::Dynamics> copy() override
    {
        auto d = std::make_unique<PinocchioDynamics>(m_model, m_configuration);
        d->m_forecast = m_forecast;
        return d;
    }
    mppi::Ref<mppi::VectorXd> step(const mppi::VectorXd &control, double dt) override
    {
        if (control.size() != MPPI_FR_CONTROL) throw std::invalid_argument("control has the wrong dimension");
        check(mppi_dynamics_step(object(), control.data(), dt, m_state.data()));
        return m_state;
    }
    void set_state(const mppi::VectorXd &state, double time) override
    {
        if (state.size() != MPPI_FR_STATE) throw std::invalid_argument("state has the wrong dimension");
        check(mppi_dynamics_set_state(object(), state.data(), time));
        check(mppi_dynamics_get_state(m_obj, m_state.data()));
    }
    mppi::Ref<mppi::VectorXd> get_state() override
    {
        check(mppi_dynamics_get_state(object(), m_state.data()));
        return m_state;
    }
    int get_control_dof() override { return MPPI_FR_CONTROL; }
    int get_state_dof() override { return MPPI_FR_STATE; }
    bool describe(mppi_dynamics_desc &out) const override
    {
        out = mppi_dynamics_desc{};
        out.kind = MPPI_DYNAMICS_FRANKARIDGEBACK;
        out.frankaridgeback = m_model;
        return true;
    }

    // FrankaRidgeback::Dynamics queries (dynamics.hpp:416-537)
    EndEffectorState get_end_effector_state()
    {
        double r[MPPI_EE_N];
        check(mppi_dynamics_end_effector(object(), r));
        return EndEffectorState::from_row(r);
    }
    // get_link_position (dynamics.hpp:464; the reference's plugin answers zeros, .hpp:181-192)
    std::array<double, 3> get_link_position(Link link)
    {
        double p[3 * MPPI_LINK_N];
        check(mppi_dynamics_link_positions(object(), p));
        const int l = (int)link;
        if (l < 0 || l >= MPPI_LINK_N) throw std::out_of_range("link");
        return {p[3 * l], p[3 * l + 1], p[3 * l + 2]};
    }
    int link_positions() const override { return m_configuration.link_positions ? MPPI_LINK_POSITIONS_KINEMATIC : -1; }
    // the obstacle term of mppi_set_obstacle_avoidance at the positions cached by the last call, with
    // the obstacles moved by `elapsed` seconds (mppi_dynamics_obstacle_cost; the kinematic model only)
    double obstacle_cost(const std::vector<mppi_obstacle> &obstacles, double elapsed, const mppi_obstacle_config *config = nullptr)
    {
        double c = 0.0;
        check(mppi_dynamics_obstacle_cost(object(), config, obstacles.data(), (int32_t)obstacles.size(), elapsed, &c));
        return c;
    }
    // the same with the robot's segments, capsule obstacles and segment mask bits (mppi_dynamics_capsule_cost)
    double capsule_cost(const std::vector<mppi_obstacle> &obstacles, double elapsed, const mppi_obstacle_config *config = nullptr,
                        const mppi_capsule_config *capsules = nullptr)
    {
        double c = 0.0;
        check(mppi_dynamics_capsule_cost(object(), config, capsules, obstacles.data(), (int32_t)obstacles.size(), elapsed, &c));
        return c;
    }
    // the distance field's term at the same positions (mppi_dynamics_distance_field_cost; the grid is uploaded on every call)
    double distance_field_cost(const mppi_distance_field &field, const float *values, const mppi_obstacle_config *config = nullptr,
                               const mppi_capsule_config *capsules = nullptr)
    {
        double c = 0.0;
        check(mppi_dynamics_distance_field_cost(object(), config, capsules, &field, values, &c));
        return c;
    }
    // the held term of `held` at the grasp frame's cached pose (mppi_dynamics_held_object_cost): against
    // `obstacles` moved by `elapsed` (their held mask bits) and, with `field`, against the field
    double held_object_cost(const mppi::HeldObject &held, const std::vector<mppi_obstacle> &obstacles, double elapsed,
                            const mppi_distance_field *field = nullptr, const float *values = nullptr,
                            const mppi_obstacle_config *config = nullptr)
    {
        double c = 0.0;
        const mppi_held_object o = held.to_c();
        check(mppi_dynamics_held_object_cost(object(), config, obstacles.data(), (int32_t)obstacles.size(), elapsed, field, values, &o, &c));
        return c;
    }
    // the held-self term of `held` under `self` at the cached link positions and grasp pose
    // (mppi_dynamics_held_self_cost)
    double held_self_cost(const mppi::HeldObject &held, const mppi::HeldSelf &self, const mppi_obstacle_config *config = nullptr)
    {
        double c = 0.0;
        const mppi_held_object o = held.to_c();
        const mppi_held_self s = self.to_c();
        check(mppi_dynamics_held_self_cost(object(), config, &o, &s, &c));
        return c;
    }
    // the target-tracking terms at the grasp frame's cached pose (mppi_dynamics_target_cost): position,
    // orientation (0 with quaternion nullptr; x, y, z, w)
    std::array<double, 2> target_cost(const double *point3, const double *quaternion4 = nullptr,
                                      const mppi_target_tracking_config *config = nullptr)
    {
        std::array<double, 2> c = {0.0, 0.0};
        check(mppi_dynamics_target_cost(object(), point3, quaternion4, config, c.data()));
        return c;
    }
    std::vector<double> get_joint_position() { return query(0, 12); }
    std::vector<double> get_joint_velocity() { return query(12, 12); }
    std::vector<double> get_joint_acceleration() { return query(24, 12); }
    double get_tank_energy() { return query(48, 1)[0]; }
    double get_joint_power() const { return 0.0; }       // pinocchio_dynamics.hpp:211-214
    double get_external_power() const { return 0.0; }    // :220-223
    // :247-276, the reference's todo: a force and a moment at the grasp frame's origin in world
    // axes, cumulative until the next step applies the sum (mppi_amd.h, the simulated wrench)
    void add_end_effector_simulated_wrench(Vector6d wrench)
    {
        check(mppi_dynamics_add_end_effector_simulated_wrench(object(), wrench.data()));
    }
    // the wrench the last step applied (zeros before any step); the object is created on first use,
    // like every query here, so the method is const in the reference's sense only
    Vector6d get_end_effector_simulated_wrench() const
    {
        Vector6d w = Vector6d::Zero();
        check(mppi_dynamics_get_end_effector_simulated_wrench(const_cast<PinocchioDynamics *>(this)->object(), w.data()));
        return w;
    }
    int simulated_wrench() const override { return m_configuration.simulated_wrench; }
    // the safety filter on one control at this object's joint position and velocity
    // (mppi_dynamics_safety_filter); a pending simulated wrench is included and not consumed
    mppi::VectorXd safety_filter(const mppi_safety_filter_desc &filter, const mppi::VectorXd &control, double dt)
    {
        if (control.size() != MPPI_FR_CONTROL) throw std::invalid_argument("control has the wrong dimension");
        mppi::VectorXd out(MPPI_FR_CONTROL);
        check(mppi_dynamics_safety_filter(object(), &filter, control.data(), dt, out.data()));
        return out;
    }
    void set_forecast(WrenchSource source) { m_forecast = std::move(source); }
    const WrenchSource &get_forecast() const { return m_forecast; }

    mppi_frankaridgeback_desc &model() { return m_model; }
    mppi_dynamics *object()
    {
        if (!m_obj) {
            std::vector<double> x0 = m_configuration.initial_state;
            if (x0.empty()) {
                x0.assign(MPPI_FR_STATE, 0.0);
                mppi_frankaridgeback_huddled(x0.data());
            }
            mppi_dynamics_desc d;
            describe(d);
            check(mppi_dynamics_create(&d, x0.data(), m_configuration.device, &m_obj));
            if (m_configuration.link_positions) check(mppi_dynamics_set_link_positions(m_obj, MPPI_LINK_POSITIONS_KINEMATIC));
            if (m_configuration.simulated_wrench >= 0)
                check(mppi_dynamics_set_simulated_wrench(m_obj, m_configuration.simulated_wrench != MPPI_SIMULATED_WRENCH_OFF
                                                                    ? MPPI_SIMULATED_WRENCH_ON : MPPI_SIMULATED_WRENCH_OFF));
        }
        return m_obj;
    }

private:
    std::vector<double> query(int off, int n)
    {
        double q[MPPI_DYNAMICS_QUERY_N];
        check(mppi_dynamics_query(object(), q));
        return std::vector<double>(q + off, q + off + n);
    }
    static void check(mppi_status st)
    {
        if (st != MPPI_OK) throw std::runtime_error(mppi_last_error(nullptr));
    }

    mppi_frankaridgeback_desc m_model;
    Configuration m_configuration;
    mppi_dynamics *m_obj = nullptr;
    mppi::VectorXd m_state = mppi::VectorXd(MPPI_FR_STATE);
    WrenchSource m_forecast;
};

// FrankaRidgeback::TrajectorySafetyFilter (frankaridgeback/safety.hpp:11-61), whose methods the
// reference leaves empty: joint position, velocity and acceleration limits on the plan (mppi_amd.h,
// mppi_safety_filter_desc).  Passed to mppi::Trajectory::create it runs on the device inside every
// update with the trajectory's own time step.  filter() is the same filter on one control, run
// through mppi_dynamics_safety_filter on a dynamics object this filter owns, with
// Configuration::time_step (a field the reference's Configuration does not have: the reference's
// filter() is not told the step).  The filter is stateless: reset() does nothing, the time is unused.
class TrajectorySafetyFilter : public mppi::Filter, public mppi::DeviceFilter {
public:
    struct Configuration {
        std::array<double, MPPI_FR_JOINTS> position_minimum, position_maximum;
        std::array<double, MPPI_FR_JOINTS> velocity_minimum, velocity_maximum;
        std::array<double, MPPI_FR_JOINTS> acceleration_minimum, acceleration_maximum;
        double reach_maximum = 0.8;
        double reach_minimum = 0.15;
        bool limit_joints = false;
        bool limit_velocity = false;
        bool limit_acceleration = false;
        bool limit_reach = false;
        double time_step = 0.01;   // of the host-callable filter() only
        int device = 0;
    };
    // robot.urdf's position and velocity limits, no acceleration limits, every switch off
    static Configuration default_configuration()
    {
        mppi_safety_filter_desc d;
        mppi_default_safety_filter(&d);
        Configuration c;
        for (int i = 0; i < MPPI_FR_JOINTS; i++) {
            c.position_minimum[i] = d.position_minimum[i];
            c.position_maximum[i] = d.position_maximum[i];
            c.velocity_minimum[i] = d.velocity_minimum[i];
            c.velocity_maximum[i] = d.velocity_maximum[i];
            c.acceleration_minimum[i] = d.acceleration_minimum[i];
            c.acceleration_maximum[i] = d.acceleration_maximum[i];
        }
        return c;
    }
    static std::unique_ptr<TrajectorySafetyFilter> create(Configuration &&configuration)
    {
        return std::unique_ptr<TrajectorySafetyFilter>(new TrajectorySafetyFilter(std::move(configuration)));
    }
    bool describe(mppi_safety_filter_desc &out) const override
    {
        out = mppi_safety_filter_desc{};
        for (int i = 0; i < MPPI_FR_JOINTS; i++) {
            out.position_minimum[i] = m_configuration.position_minimum[i];
            out.position_maximum[i] = m_configuration.position_maximum[i];
            out.velocity_minimum[i] = m_configuration.velocity_minimum[i];
            out.velocity_maximum[i] = m_configuration.velocity_maximum[i];
            out.acceleration_minimum[i] = m_configuration.acceleration_minimum[i];
            out.acceleration_maximum[i] = m_configuration.acceleration_maximum[i];
        }
        out.reach_maximum = m_configuration.reach_maximum;
        out.reach_minimum = m_configuration.reach_minimum;
        out.limit_joints = m_configuration.limit_joints;
        out.limit_velocity = m_configuration.limit_velocity;
        out.limit_acceleration = m_configuration.limit_acceleration;
        out.limit_reach = m_configuration.limit_reach;
        return true;
    }
    mppi::VectorXd filter(mppi::Ref<mppi::VectorXd> state, mppi::Ref<mppi::VectorXd> control, double time) override
    {
        if (state.size() != MPPI_FR_STATE) throw std::invalid_argument("state has the wrong dimension");
        if (control.size() != MPPI_FR_CONTROL) throw std::invalid_argument("control has the wrong dimension");
        if (!m_dynamics) {
            PinocchioDynamics::Configuration c;
            c.device = m_configuration.device;
            m_dynamics = PinocchioDynamics::create(c);
        }
        mppi::VectorXd x(MPPI_FR_STATE), u(MPPI_FR_CONTROL);
        for (int i = 0; i < MPPI_FR_STATE; i++) x[i] = state[i];
        for (int i = 0; i < MPPI_FR_CONTROL; i++) u[i] = control[i];
        m_dynamics->set_state(x, time);
        mppi_safety_filter_desc d;
        describe(d);
        mppi::VectorXd out = m_dynamics->safety_filter(d, u, m_configuration.time_step);
        for (int i = 0; i < MPPI_FR_CONTROL; i++) control[i] = out[i];   // in place, as Trajectory::filter() uses it
        return out;
    }
    void reset(mppi::Ref<mppi::VectorXd>, double) override {}
    const Configuration &configuration() const { return m_configuration; }

private:
    explicit TrajectorySafetyFilter(Configuration &&c) : m_configuration(std::move(c)) {}
    Configuration m_configuration;
    std::unique_ptr<PinocchioDynamics> m_dynamics;
};

// FrankaRidgeback::AssistedManipulation (objective/assisted_manipulation.hpp:16-398): Configuration
// is the POD mirror of AssistedManipulation::Configuration; DEFAULT_CONFIGURATION by default.
// get_cost against a PinocchioDynamics runs on the device (mppi_cost_evaluate) and accumulates the
// reference's per-term totals (m_joint_cost += ..., .cpp:74-319) that get_*_cost() return.
class AssistedManipulation : public mppi::Cost, public mppi::DeviceCost {
public:
    using Configuration = mppi_assisted_manipulation_desc;
    static Configuration default_configuration()
    {
        Configuration c;
        mppi_assisted_manipulation_default(&c);
        return c;
    }
    static std::unique_ptr<AssistedManipulation> create(const Configuration &c)
    {
        return std::make_unique<AssistedManipulation>(c);
    }
    AssistedManipulation() : m_configuration(default_configuration()) {}
    explicit AssistedManipulation(const Configuration &c) : m_configuration(c) {}
    std::unique_ptr<mppi::Cost> copy() override { return std::make_unique<AssistedManipulation>(m_configuration); }
    void reset(double time) override   // :24-35
    {
        m_initial_time = time;
        for (double &t : m_terms) t = 0.0;
        m_cost = 0.0;
    }
    double get_cost(const mppi::VectorXd &state, const mppi::VectorXd &control, mppi::Dynamics *dynamics,
                    double time) override
    {
        auto *d = dynamic_cast<PinocchioDynamics *>(dynamics);
        if (!d) throw std::invalid_argument("AssistedManipulation::get_cost needs FrankaRidgeback::PinocchioDynamics");
        double wrench[6], out[8];
        const bool have = d->get_forecast() && d->get_forecast()(time, wrench);
        mppi_cost_desc cd;
        describe(cd);
        const mppi_status st = mppi_cost_evaluate(&cd, d->object(), state.data(), control.data(), have ? wrench : nullptr, out);
        if (st != MPPI_OK) throw std::runtime_error(mppi_last_error(nullptr));
        for (int i = 0; i < 7; i++) m_terms[i] += out[1 + i];
        m_cost += out[0];
        return out[0];
    }
    int get_control_dof() override { return MPPI_FR_CONTROL; }
    int get_state_dof() override { return MPPI_FR_STATE; }
    bool describe(mppi_cost_desc &out) const override
    {
        out = mppi_cost_desc{};
        out.kind = MPPI_COST_ASSISTED_MANIPULATION;
        out.assisted_manipulation = m_configuration;
        return true;
    }
    void set_optimal_terms(const double *t) override
    {
        for (int i = 0; i < 7; i++) m_terms[i] = t[i];
    }
    // assisted_manipulation.hpp:232-258
    double get_joint_limit_cost() const { return m_terms[MPPI_TERM_JOINT_LIMIT]; }
    double get_self_collision_cost() const { return m_terms[MPPI_TERM_SELF_COLLISION]; }
    double get_workspace_cost() const { return m_terms[MPPI_TERM_WORKSPACE]; }
    double get_energy_tank_cost() const { return m_terms[MPPI_TERM_ENERGY_TANK]; }
    double get_joint_velocity_cost() const { return m_terms[MPPI_TERM_JOINT_VELOCITY]; }
    double get_trajectory_cost() const { return m_terms[MPPI_TERM_TRAJECTORY]; }
    double get_manipulability_cost() const { return m_terms[MPPI_TERM_MANIPULABILITY]; }
    const Configuration &get_configuration() const { return m_configuration; }

private:
    Configuration m_configuration;
    double m_terms[7] = {0, 0, 0, 0, 0, 0, 0};
    double m_initial_time = 0.0, m_cost = 0.0;
};

// FrankaRidgeback::TrackPoint (frankaridgeback/objective/track_point.hpp:16-215): the same
// create / copy surface; DEFAULT_CONFIGURATION is track_point.hpp:72-107.
class TrackPoint : public mppi::Cost, public mppi::DeviceCost {
public:
    using Configuration = mppi_track_point_desc;
    static Configuration default_configuration()
    {
        Configuration c;
        mppi_track_point_default(&c);
        return c;
    }
    static inline const Configuration DEFAULT_CONFIGURATION = default_configuration();
    static std::unique_ptr<TrackPoint> create(const Configuration &c) { return std::make_unique<TrackPoint>(c); }
    TrackPoint() : m_configuration(default_configuration()) {}
    explicit TrackPoint(const Configuration &c) : m_configuration(c) {}
    std::unique_ptr<mppi::Cost> copy() override { return std::make_unique<TrackPoint>(m_configuration); }
    void reset(double) override {}
    double get_cost(const mppi::VectorXd &state, const mppi::VectorXd &control, mppi::Dynamics *dynamics, double) override
    {
        auto *d = dynamic_cast<PinocchioDynamics *>(dynamics);
        if (!d) throw std::invalid_argument("TrackPoint::get_cost needs FrankaRidgeback::PinocchioDynamics");
        mppi_cost_desc cd;
        describe(cd);
        double out[8];
        const mppi_status st = mppi_cost_evaluate(&cd, d->object(), state.data(), control.data(), nullptr, out);
        if (st != MPPI_OK) throw std::runtime_error(mppi_last_error(nullptr));
        return out[0];
    }
    int get_control_dof() override { return MPPI_FR_CONTROL; }
    int get_state_dof() override { return MPPI_FR_STATE; }
    bool describe(mppi_cost_desc &out) const override
    {
        out = mppi_cost_desc{};
        out.kind = MPPI_COST_TRACK_POINT;
        out.track_point = m_configuration;
        return true;
    }

private:
    Configuration m_configuration;
};

// FrankaRidgeback::DynamicsForecast (dynamics.hpp:122-387, dynamics.cpp:57-138).  The wrench
// forecast it owns in the reference is the trajectory's device forecast here: create() attaches
// the configuration's Forecast::Configuration to `owner` (the trajectory whose rollouts read it,
// as the Actor shares one DynamicsForecast between both, actor.cpp:70-89).
class DynamicsForecast {
public:
    struct Configuration {
        double time_step;
        double horison;
        mppi_forecast_config end_effector_wrench_forecast;
    };

    static std::unique_ptr<DynamicsForecast> create(const Configuration &configuration,
                                                    std::unique_ptr<PinocchioDynamics> &&dynamics, mppi::Trajectory &owner)
    {
        const double s = std::ceil(configuration.horison / configuration.time_step);
        if (!(s > 0)) {
            std::cerr << "time horison is too small for time step" << std::endl;   // dynamics.cpp:70-74
            return nullptr;
        }
        if (mppi_forecast_attach(owner.handle(), &configuration.end_effector_wrench_forecast) != MPPI_OK) {
            std::cerr << "failed to create forecast for end effector wrench" << std::endl;   // :62-67
            return nullptr;
        }
        return std::unique_ptr<DynamicsForecast>(new DynamicsForecast(configuration, std::move(dynamics), owner, (unsigned)s));
    }

    void observe_wrench(const double *wrench6, double time) { m_owner.observe_wrench(wrench6, time); }
    void observe_time(double time) { m_owner.observe_time(time); }

    // dynamics.cpp:104-138: one device launch for the horison
    void forecast(const std::vector<double> &state, double time)
    {
        std::vector<double> wrench((size_t)m_steps * 6);
        m_owner.forecast_table(time, m_configuration.time_step, m_steps, wrench.data());
        m_rows.assign((size_t)m_steps * MPPI_DF_N, 0.0);
        const mppi_status st = mppi_dynamics_forecast(m_dynamics->object(), state.data(), time, m_configuration.time_step,
                                                      m_steps, wrench.data(), m_rows.data());
        if (st != MPPI_OK) throw std::runtime_error(mppi_last_error(nullptr));
        m_last_forecast = time;
    }
    double get_last_forecast_time() const { return m_last_forecast; }
    std::vector<double> get_joint_position(unsigned step) const { return row(step, MPPI_DF_JOINT_POSITION, 12); }
    EndEffectorState get_end_effector_state(double time) const
    {
        return EndEffectorState::from_row(m_rows.data() + (size_t)parameterise(time) * MPPI_DF_N + MPPI_DF_END_EFFECTOR);
    }
    std::vector<double> get_end_effector_wrench(double time)   // dynamics.hpp:275-278: the forecast itself
    {
        std::vector<double> w(6);
        m_owner.forecast(time, w.data());
        return w;
    }
    std::vector<double> get_wrench(unsigned step) const { return row(step, MPPI_DF_WRENCH, 6); }
    double get_energy(unsigned step) const { return m_rows[(size_t)step * MPPI_DF_N + MPPI_DF_ENERGY]; }
    double get_time_step() const { return m_configuration.time_step; }
    double get_horison() const { return m_configuration.horison; }
    unsigned get_steps() const { return m_steps; }
    // a wrench source for PinocchioDynamics::set_forecast (DynamicsForecast::Handle)
    PinocchioDynamics::WrenchSource handle()
    {
        return [this](double time, double *w) {
            m_owner.forecast(time, w);
            return true;
        };
    }

private:
    DynamicsForecast(const Configuration &c, std::unique_ptr<PinocchioDynamics> &&d, mppi::Trajectory &owner, unsigned steps)
        : m_configuration(c), m_dynamics(std::move(d)), m_owner(owner), m_steps(steps)
    {
    }
    std::int64_t parameterise(double time) const   // dynamics.hpp:344-359, literally
    {
        if (time < m_last_forecast) return 0;
        if (time >= m_configuration.horison) return m_steps - 1;
        return (std::int64_t)((time - m_last_forecast) / m_configuration.time_step);
    }
    std::vector<double> row(unsigned step, int off, int n) const
    {
        const double *r = m_rows.data() + (size_t)step * MPPI_DF_N + off;
        return std::vector<double>(r, r + n);
    }

    Configuration m_configuration;
    std::unique_ptr<PinocchioDynamics> m_dynamics;
    mppi::Trajectory &m_owner;
    unsigned m_steps;
    double m_last_forecast = 2.2250738585072014e-308;   // std::numeric_limits<double>::min()
    std::vector<double> m_rows;
};

}  // namespace FrankaRidgeback
