/*
 * mppi_amd.h — C-ABI of the MI355X-native MPPI trajectory engine.
 *
 * Drop-in boundary for the reference's `mppi::Trajectory` (src/controller/mppi.{hpp,cpp}
 * of LuigiVan01/AssistedManipulation).  Every entry point is `extern "C"`, takes plain
 * pointers and sizes, never throws, and returns an `mppi_status`.  The reference symbol each
 * entry point replaces is cited next to it (paths relative to the reference's src/).
 *
 * Layout conventions (identical to the reference, which stores everything column-major with
 * Eigen):
 *   - a control trajectory is C x H, column-major: element (c, k) at [k * C + c];
 *   - the per-rollout noise tensor handed across the ABI is R x (C x H): rollout r, element
 *     (c, k) at [(r * H + k) * C + c]   (mppi.hpp:281 `Rollout::noise`);
 *   - costs and weights are R-vectors indexed by rollout (R = rollouts + 2, mppi.hpp:306).
 * Inside HBM the engine keeps its own layout; the ABI copies convert.
 */
#ifndef MPPI_AMD_H
#define MPPI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPPI_AMD_ABI_VERSION 5   /* 5: mppi_device_costs_count, MPPI_INFO_GRAPH_*, MPPI_INFO_UPDATE_COUNT */

#define MPPI_MAX_BODIES 16
#define MPPI_MAX_CONTROL 16
#define MPPI_MAX_STATE 48
#define MPPI_FR_JOINTS 12       /* frankaridgeback/dof.hpp:36-61 DoF::JOINTS */
#define MPPI_FR_STATE 31        /* dof.hpp:63 DoF::STATE */
#define MPPI_FR_CONTROL 12      /* dof.hpp:70 DoF::CONTROL */

typedef enum mppi_status {
    MPPI_OK = 0,
    MPPI_ERR_INVALID = 1,        /* Trajectory::create returns nullptr (mppi.cpp:17-69) */
    MPPI_ERR_DEVICE = 2,         /* HIP runtime failure */
    MPPI_ERR_ALL_NAN = 3,        /* optimise() throws "all nan rollouts" (mppi.cpp:369-370) */
    MPPI_ERR_SMOOTHING = 4,      /* SavitzkyGolay window throws (filter.cpp:37-44, 73-82) */
    MPPI_ERR_TIME = 5,           /* get() asserts monotonic time (mppi.cpp:483) */
    MPPI_ERR_COMM = 6,           /* RCCL failure */
    MPPI_ERR_NOISE = 7,          /* injected noise stream too short for this update */
    MPPI_ERR_UNSUPPORTED = 8
} mppi_status;

/* ------------------------------------------------------------------------------------------
 * Configuration — POD mirror of mppi::Configuration (mppi.hpp:181-249), field for field.
 * Optional fields carry a has_* flag.  `threads` is validated (> 0) as the reference does
 * (mppi.cpp:66-69) and otherwise ignored by the device engine.
 * ---------------------------------------------------------------------------------------- */
typedef struct mppi_config {
    const double *initial_state;   /* X doubles */
    int64_t state_dof;             /* X (must match the dynamics) */
    int64_t control_dof;           /* C (must match the dynamics) */
    int64_t rollouts;              /* S */
    int64_t keep_best_rollouts;    /* K */
    double time_step;
    double horison;                /* H = ceil(horison / time_step) (mppi.cpp:85) */
    double gradient_step;
    double cost_scale;
    double cost_discount_factor;
    const double *covariance;      /* C x C, column-major */
    int32_t control_bound;
    const double *control_min;     /* C */
    const double *control_max;     /* C */
    int32_t has_control_default;
    const double *control_default; /* C, may be NULL when !has_control_default */
    int32_t has_smoothing;
    uint32_t smoothing_window;
    uint32_t smoothing_order;
    uint32_t threads;
} mppi_config;

/* ------------------------------------------------------------------------------------------
 * Dynamics descriptors (replace the mppi::Dynamics plugin object, mppi.hpp:30-85).
 * ---------------------------------------------------------------------------------------- */
typedef enum mppi_dynamics_kind {
    MPPI_DYNAMICS_FRANKARIDGEBACK = 1,  /* FrankaRidgeback::PinocchioDynamics (pinocchio_dynamics.cpp) */
    MPPI_DYNAMICS_POINT_MASS = 2        /* build-defined bring-up plugin */
} mppi_dynamics_kind;

typedef enum mppi_joint_type {
    MPPI_JOINT_REVOLUTE = 0,
    MPPI_JOINT_PRISMATIC = 1
} mppi_joint_type;

/* One moving joint + the rigid body it carries, after fixed-joint merging, in Pinocchio's
 * conventions.  Rotations are row-major 3x3. */
typedef struct mppi_body {
    int32_t parent;          /* parent body index, -1 = universe */
    int32_t type;            /* mppi_joint_type */
    double axis[3];          /* joint axis in the joint frame (unit) */
    double rotation[9];      /* joint placement in the parent joint frame */
    double translation[3];
    double mass;
    double lever[3];         /* centre of mass in the joint frame */
    double inertia[6];       /* rotational inertia about the com, joint frame:
                                xx, xy, yy, xz, yz, zz (Pinocchio Symmetric3 order) */
} mppi_body;

typedef struct mppi_frame {
    int32_t parent;          /* body index the frame is rigidly attached to */
    double rotation[9];      /* placement in that body's joint frame */
    double translation[3];
} mppi_frame;

typedef struct mppi_frankaridgeback_desc {
    int32_t nbodies;                         /* 12 */
    mppi_body bodies[MPPI_MAX_BODIES];
    mppi_frame end_effector;                 /* "panda_grasp_joint" (pinocchio_dynamics.hpp:58) */
    mppi_frame arm_mount;                    /* "arm_mount_joint" (dynamics.cpp:26) */
    double gravity[3];                       /* Pinocchio default (0, 0, -9.81) */
} mppi_frankaridgeback_desc;

typedef struct mppi_point_mass_desc {
    double mass;                             /* state (p[3], v[3]), control = force[3] */
} mppi_point_mass_desc;

typedef struct mppi_dynamics_desc {
    int32_t kind;                            /* mppi_dynamics_kind */
    mppi_frankaridgeback_desc frankaridgeback;
    mppi_point_mass_desc point_mass;
} mppi_dynamics_desc;

/* ------------------------------------------------------------------------------------------
 * Cost descriptors (replace the mppi::Cost plugin object, mppi.hpp:93-145).
 * ---------------------------------------------------------------------------------------- */
typedef enum mppi_cost_kind {
    MPPI_COST_ASSISTED_MANIPULATION = 1,     /* objective/assisted_manipulation.{hpp,cpp} */
    MPPI_COST_QUADRATIC = 2,                 /* point-mass bring-up cost */
    MPPI_COST_TRACK_POINT = 3                /* objective/track_point.{hpp,cpp} */
} mppi_cost_kind;

typedef struct mppi_quadratic {              /* QuadraticCost (controller/cost.hpp:10-37) */
    double constant_cost;
    double linear_cost;
    double quadratic_cost;
} mppi_quadratic;

typedef struct mppi_barrier {                /* Left/RightInverseBarrierFunction (cost.hpp:43-99) */
    double bound;                            /* lower_bound (left) or upper_bound (right) */
    double scale;
    double maximum_cost;                     /* default 1e10 */
} mppi_barrier;

/* AssistedManipulation::Configuration (assisted_manipulation.hpp:16-131), field for field. */
typedef struct mppi_assisted_manipulation_desc {
    int32_t enable_joint_limit;
    int32_t enable_self_collision_limit;
    int32_t enable_workspace_limit;
    int32_t enable_energy_limit;
    int32_t enable_velocity_cost;
    int32_t enable_trajectory_cost;
    int32_t enable_manipulability_cost;
    mppi_barrier lower_joint_limit[MPPI_FR_JOINTS];   /* left barriers */
    mppi_barrier upper_joint_limit[MPPI_FR_JOINTS];   /* right barriers */
    mppi_barrier self_collision_limit;                /* left */
    double self_collision_radii[8];
    mppi_barrier workspace_limit_above;               /* left */
    mppi_barrier workspace_limit_infront;             /* left */
    mppi_barrier workspace_limit_reach;               /* right */
    mppi_quadratic workspace_cost_yaw;
    mppi_barrier energy_limit_below;                  /* left */
    mppi_barrier energy_limit_above;                  /* right */
    mppi_quadratic velocity_cost[MPPI_FR_JOINTS];
    double trajectory_target_scale;
    double trajectory_target_maximum;
    mppi_quadratic trajectory_position_cost;
    double trajectory_position_threshold;
    mppi_quadratic trajectory_velocity_cost;
    double trajectory_velocity_minimum;
    double trajectory_velocity_maximum;
    double trajectory_velocity_dropoff;
    mppi_quadratic manipulability_cost;
    /* The reference's Actor hands the dynamics a DynamicsForecast handle (actor.cpp:85-89);
     * without one trajectory_cost() returns 0 (assisted_manipulation.cpp:239-240). */
    int32_t has_forecast;
} mppi_assisted_manipulation_desc;

/* TrackPoint::Configuration (frankaridgeback/objective/track_point.hpp:20-61), field for field.
 * get_cost (track_point.cpp:10-34) = 100 |p_EE - point|^2, + joint_limit_cost (hard-coded limits,
 * track_point.cpp:45-95; the configured joint barriers are not read), + self_collision_cost,
 * + reach_cost; enable_power_limit is never read. */
typedef struct mppi_track_point_desc {
    double point[3];
    int32_t enable_joint_limits;
    int32_t enable_self_collision_avoidance;
    int32_t enable_power_limit;
    int32_t enable_reach_limits;
    mppi_barrier lower_joint_limit[MPPI_FR_JOINTS];   /* left barriers (configuration only) */
    mppi_barrier upper_joint_limit[MPPI_FR_JOINTS];   /* right barriers (configuration only) */
    mppi_barrier self_collision_limit;                /* left */
    double self_collision_radii[8];
    mppi_barrier maximum_reach_limit;                 /* right */
} mppi_track_point_desc;

typedef struct mppi_quadratic_cost_desc {    /* sum_i q_i (p_i - target_i)^2 + r_i u_i^2 */
    double target[3];
    double q[3];
    double r[3];
} mppi_quadratic_cost_desc;

typedef struct mppi_cost_desc {
    int32_t kind;                            /* mppi_cost_kind */
    mppi_assisted_manipulation_desc assisted_manipulation;
    mppi_quadratic_cost_desc quadratic;
    mppi_track_point_desc track_point;
} mppi_cost_desc;

/* ------------------------------------------------------------------------------------------
 * Engine handle.
 * ---------------------------------------------------------------------------------------- */
typedef struct mppi_handle mppi_handle;

typedef enum mppi_noise_source {
    MPPI_NOISE_DEVICE_PHILOX = 0,   /* eps = T z, z ~ N(0,1) from Philox4x32-10 keyed by (seed, draw) */
    MPPI_NOISE_HOST_INJECTED = 1    /* eps columns supplied by mppi_inject_noise, consumed in
                                       the reference's draw order (mppi.cpp:242-262) */
} mppi_noise_source;

typedef enum mppi_index_semantics {
    MPPI_INDEX_WIDE = 0,            /* 64-bit rollout indices (documented deviation, R > 255) */
    MPPI_INDEX_COMPAT_UINT8 = 1     /* reference std::uint8_t indices (mppi.hpp:639,642); R <= 255 */
} mppi_index_semantics;

/* Library identity / build info. */
int mppi_abi_version(void);
const char *mppi_build_info(void);

/* Defaults: the FrankaRidgeback body table generated from robot.urdf
 * (include/mppi_amd_frankaridgeback.h) and AssistedManipulation::DEFAULT_CONFIGURATION
 * (assisted_manipulation.hpp:133-206). */
void mppi_default_frankaridgeback(mppi_frankaridgeback_desc *out);
void mppi_default_assisted_manipulation(mppi_assisted_manipulation_desc *out);
/* TrackPoint::DEFAULT_CONFIGURATION (track_point.hpp:72-107). */
void mppi_default_track_point(mppi_track_point_desc *out);

/* Trajectory::create (mppi.hpp:321-326, mppi.cpp:11-77).  Validation failures return
 * MPPI_ERR_INVALID with the reference's message available from mppi_last_error(NULL).
 * `device` is the HIP device ordinal the handle binds to. */
mppi_status mppi_create(const mppi_config *config, const mppi_dynamics_desc *dynamics,
                        const mppi_cost_desc *cost, int device, mppi_handle **out);
void mppi_destroy(mppi_handle *h);
/* Last error message of a handle (or of the last failed mppi_create when h == NULL). */
const char *mppi_last_error(const mppi_handle *h);

/* Multi-GPU sample sharding.  Rollouts [begin, end) of this rank are the ones
 * mppi_shard_range assigns; rollouts 0 and 1 always live on rank 0.  world == 1 disables it. */
mppi_status mppi_shard_range(int64_t rollout_count, int world, int rank, int64_t *begin,
                             int64_t *end);
/* Unique id for RCCL bootstrap (128 bytes, ncclUniqueId), produced on rank 0 and broadcast by
 * the caller (e.g. torch.distributed) before mppi_comm_init on every rank. */
mppi_status mppi_comm_unique_id(char out[128]);
mppi_status mppi_comm_init(mppi_handle *h, int world, int rank, const char unique_id[128]);
/* The engine communicator as RCCL reports it (ncclCommCount / ncclCommUserRank; 0 and -1 without
 * one), the handle's HIP device and its PCI bus id (hipDeviceGetPCIBusId, len bytes; may be null):
 * bench.py checks that N ranks form one N-rank communicator on N distinct devices. */
mppi_status mppi_comm_info(mppi_handle *h, int *nranks, int *rank, int *device, char *pci_bus_id, int len);
/* Shard without an engine communicator: the caller runs the two all-reduces between the
 * update phases (mppi_update_phase1..3).  Must precede the first update. */
mppi_status mppi_set_shard(mppi_handle *h, int world, int rank);

/* Parity hooks. */
mppi_status mppi_set_noise_source(mppi_handle *h, int source, uint64_t seed);
/* Supply eps columns (C doubles each) for the next update(s); consumed in draw order. */
mppi_status mppi_inject_noise(mppi_handle *h, const double *eps, int64_t columns);
/* Number of eps columns the next update at `time` will draw (K*shift + (S-K)*H). */
mppi_status mppi_noise_draws(mppi_handle *h, double time, int64_t *columns);
mppi_status mppi_set_index_semantics(mppi_handle *h, int semantics);

/* Per-update forecast table: row k = predicted end-effector wrench (fx fy fz tx ty tz) at
 * t0 + k*dt, k < H (KalmanForecast::forecast, forecast.cpp:342-367, sampled on the step grid). */
mppi_status mppi_set_forecast(mppi_handle *h, const double *wrench_Hx6);

/* Device-resident wrench forecast.  Replaces the caller's table: every
 * update samples Forecast::forecast(t0 + k*dt) for k < H on the device (the rollout queries it
 * through DynamicsForecast::get_end_effector_wrench, dynamics.hpp:275-278, in
 * AssistedManipulation::trajectory_cost, assisted_manipulation.cpp:237-290).  The three kinds of
 * Forecast::Configuration (forecast.hpp:377-416):
 *   LOCFForecast     (forecast.hpp:64-140)   the last observation, zero past its horison;
 *   AverageForecast  (forecast.cpp:41-129)   mean of the observations inside the window;
 *   KalmanForecast   (forecast.cpp:131-367, kalman.cpp:103-152)  Euler state-transition Kalman
 *                    filter over the wrench and its derivatives; each observation runs the filter
 *                    update and the horison of predictions in one device kernel. */
typedef enum mppi_forecast_type {
    MPPI_FORECAST_LOCF = 0,
    MPPI_FORECAST_AVERAGE = 1,
    MPPI_FORECAST_KALMAN = 2
} mppi_forecast_type;

#define MPPI_FORECAST_MAX_ORDER 3   /* Kalman states 6 (order + 1) <= 24 */

typedef struct mppi_forecast_config {
    int32_t type;                         /* mppi_forecast_type */
    /* LOCFForecast::Configuration */
    double locf_observation[6];
    double locf_horison;
    /* AverageForecast::Configuration */
    int32_t average_states;               /* 6: the end-effector wrench */
    double average_window;
    /* KalmanForecast::Configuration */
    int32_t kalman_observed_states;       /* 6: KalmanForecast::update works on Vector6d */
    double kalman_time_step;
    double kalman_horison;
    int32_t kalman_order;                 /* <= MPPI_FORECAST_MAX_ORDER */
    double kalman_initial_state[6];
    /* `variance` is read by create_euler_state_transition_covariance_matrix, which ignores
     * it (forecast.cpp:287-296: 1e-8 I), so it is not carried. */
} mppi_forecast_config;

/* Forecast::create (forecast.cpp:6-39) bound to the handle; failures return MPPI_ERR_INVALID
 * with the reference's message.  NULL detaches (back to mppi_set_forecast tables). */
mppi_status mppi_forecast_attach(mppi_handle *h, const mppi_forecast_config *config);
/* DynamicsForecast::observe_wrench -> Forecast::update(measurement, time). */
mppi_status mppi_forecast_observe(mppi_handle *h, const double *wrench6, double time);
/* DynamicsForecast::observe_time -> Forecast::update(time). */
mppi_status mppi_forecast_observe_time(mppi_handle *h, double time);
/* Forecast::forecast(time) (host copy of the device evaluation). */
mppi_status mppi_forecast_get(mppi_handle *h, double time, double *wrench6);
/* Parity hook: the per-step trajectory-cost constants the last update's rollouts read, H rows of
 * (target x y z, target.target, position cost, velocity target, gamma^k, active). */
mppi_status mppi_step_constants(mppi_handle *h, double *out_Hx8);

/* Trajectory::update (mppi.hpp:339, mppi.cpp:154-187): sample, rollout, optimise, filter,
 * publish.  Blocks until the update is complete on the device. */
mppi_status mppi_update(mppi_handle *h, const double *state, double time);

/* hipGraph path of mppi_update (default off; MPPI_GRAPH=1 at create turns it on): the steady-state
 * update's four launches (rollout, weights + gradient, finish, rank + draws ahead) are captured
 * once and replayed as one graph launch with each update's arguments written into its kernel
 * nodes.  Updates outside that configuration run the eager launches.  mppi_graph_updates counts
 * the updates that ran as the graph. */
mppi_status mppi_set_graph(mppi_handle *h, int enable);
mppi_status mppi_graph_updates(mppi_handle *h, int64_t *count);

/* FrankaRidgeback::Link (frankaridgeback/dynamics.hpp:65-80), in the enum's order: the universe,
 * then the bodies of the model descriptor (link L >= 1 is body L - 1).  mppi_link_name: the
 * reference's LINK_NAMES (dynamics.cpp:42-56); host only, NULL out of range. */
#define MPPI_LINK_OMNI_BASE_ROOT_LINK 0
#define MPPI_LINK_X_SLIDER 1
#define MPPI_LINK_Y_SLIDER 2
#define MPPI_LINK_PIVOT 3
#define MPPI_LINK_PANDA_LINK1 4
#define MPPI_LINK_PANDA_LINK2 5
#define MPPI_LINK_PANDA_LINK3 6
#define MPPI_LINK_PANDA_LINK4 7
#define MPPI_LINK_PANDA_LINK5 8
#define MPPI_LINK_PANDA_LINK6 9
#define MPPI_LINK_PANDA_LINK7 10
#define MPPI_LINK_PANDA_LEFTFINGER 11
#define MPPI_LINK_PANDA_RIGHTFINGER 12
#define MPPI_LINK_N 13
const char *mppi_link_name(int link);

/* What Dynamics::get_link_position(Link) answers (the spheres of both objectives'
 * self_collision_cost).  ZERO (the default): the reference's PinocchioDynamics stub,
 * Vector3d::Zero() for every link (pinocchio_dynamics.hpp:181-192), so the term is a constant of
 * the configuration.  KINEMATIC: the world translation of the link's body frame at the last
 * calculate(), oMi[body].translation() - it lags the state by one step exactly as the end-effector
 * position does: the cost of step k sees the links at q_0 for k = 0 and at q_{k-1} after.
 * mppi_set_link_positions: FrankaRidgeback handles only (MPPI_ERR_UNSUPPORTED otherwise), before
 * the first update (MPPI_ERR_INVALID after it, and for an unknown mode).  The environment variable
 * MPPI_LINK_POSITIONS=1 (or 0; anything else fails the create with MPPI_ERR_INVALID) sets the mode
 * new handles and dynamics objects start in.  Sharded handles take the mode per handle: every rank
 * must set the same one.  These functions came after ABI version 5 without a version change (no
 * struct changed): detect them by symbol. */
#define MPPI_LINK_POSITIONS_ZERO 0
#define MPPI_LINK_POSITIONS_KINEMATIC 1
mppi_status mppi_set_link_positions(mppi_handle *h, int mode);
mppi_status mppi_get_link_positions(mppi_handle *h, int *mode);

/* The simulated end-effector wrench: the push the rollouts' robot feels (the reference leaves
 * PinocchioDynamics::add_end_effector_simulated_wrench an empty body, pinocchio_dynamics.hpp:247-276).
 * A wrench w = (f, m) is a force and a moment at the origin of the grasp frame (panda_grasp_joint)
 * in world axes.  Its joint torque is tau_w = J_G(q)^T w, J_G the geometric Jacobian of the grasp
 * frame at its own origin in world axes (Pinocchio's LOCAL_WORLD_ALIGNED): column j is
 * (a_j x (p_ee - p_j); a_j) for a revolute joint under the frame and (a_j; 0) for a prismatic one,
 * zero for the two fingers; q is the configuration the step's own calculate() runs at.  The step is
 * tau = (0, 0, 0, u_arm, 0, 0) + tau_w, then calculate() as before (tau += NLE, qdd = M^-1 (u_arm +
 * tau_w)): the base joints take their tau_w too, and the tank's power is (u + tau_w + NLE) . v_new.
 * The external power stays 0.  (Not the Jacobian of the reference's commented-out line,
 * pinocchio_dynamics.cpp:237-240, which is the WORLD one with its corner overwritten; the objective
 * keeps reading that one.)
 * OFF (the default): the reference's stub, no term.  STATE: the six wrench slots of the update's
 * state, x[24..30), at every step.  FORECAST: at step k, row k of the forecast the objective reads
 * for that update - the mppi_set_forecast table, or the attached forecast at t0 + k dt; zeros without
 * either.  mppi_set_simulated_wrench: FrankaRidgeback handles only (MPPI_ERR_UNSUPPORTED otherwise),
 * before the first update (MPPI_ERR_INVALID after it, and for an unknown mode).  The environment
 * variable MPPI_SIMULATED_WRENCH=0|1|2 (anything else fails the create with MPPI_ERR_INVALID) sets
 * the mode new handles start in, and new dynamics objects' forecast mode (0: OFF, 1 or 2: ON).
 * Sharded handles take the mode per handle: every rank must set the same one.  Added after ABI
 * version 5 without a version change (no struct changed): detect by symbol. */
#define MPPI_SIMULATED_WRENCH_OFF 0
#define MPPI_SIMULATED_WRENCH_STATE 1
#define MPPI_SIMULATED_WRENCH_FORECAST 2
#define MPPI_SIMULATED_WRENCH_ON 1   /* the dynamics object's forecast mode */
mppi_status mppi_set_simulated_wrench(mppi_handle *h, int mode);
mppi_status mppi_get_simulated_wrench(mppi_handle *h, int *mode);

/* Obstacle avoidance: sphere and half-space obstacles in the rollouts' objective.  Nothing in the
 * reference computes this; it is this build's own addition, opt-in and off by default.
 * An obstacle set is at most MPPI_MAX_OBSTACLES obstacles with a reference time t_ref.  At the cost
 * of step k of an update at time t0 the elapsed time is tau_k = (t0 + k dt) - t_ref (the time
 * get_cost is called with, mppi.cpp:322-337, less t_ref) and obstacle o sits at
 * c_o(k) = position + velocity tau_k.  SPHERE: centre c_o(k), radius >= 0.  HALF_SPACE: the solid
 * {x : n . (x - c_o(k)) <= 0}, n a unit normal pointing into free space (radius ignored).
 * The robot is MPPI_OBSTACLE_POINTS spheres: points 0..7 are get_link_position(MPPI_LINK_PIVOT + i)
 * of the kinematic link-position model, lagged exactly as the self-collision term sees them (q_0
 * for k = 0, q_{k-1} after); point 8 is the end-effector (grasp-frame) position the objective
 * reads, with the same lag.  Their radii are the configuration's radii[]; the defaults are the
 * objective's default self-collision radii (0.75, then 0.1 x 7) and 0.1 for the end effector.
 * Point i is tested against obstacle o only if bit i of the obstacle's mask is set (a floor plane
 * leaves out the base sphere, which sits at z = 0 with radius 0.75).  Clearance:
 *   sphere      v = |p_i - c_o(k)| - (radii[i] + radius_o)
 *   half-space  v = n_o . (p_i - c_o(k)) - radii[i]
 * and the step's term is sum_o sum_{i in mask_o} Left(limit)(v), the reference's
 * LeftInverseBarrierFunction (cost.hpp:74-99; default limit {0, 1, 1e10}), obstacles and points in
 * index order.  It is added to the objective's get_cost of the step, before the discount, for
 * AssistedManipulation and TrackPoint, with or without the energy tank, in the rollouts and in
 * filter()'s optimal rollout; a NaN term makes the rollout NaN like any step cost.
 * mppi_set_obstacle_avoidance (config NULL: the defaults) selects the obstacle kernels for the
 * handle's life: FrankaRidgeback handles only (MPPI_ERR_UNSUPPORTED otherwise), before the first
 * update and with the handle in MPPI_LINK_POSITIONS_KINEMATIC (MPPI_ERR_INVALID otherwise, the
 * message says which; the link-position model is fixed from then on); the configuration's values
 * must be finite and its radii >= 0.  mppi_get_obstacle_avoidance: enabled = 0 for a handle that
 * never enabled it (out is then untouched).
 * mppi_set_obstacles replaces the whole set between any two updates, like mppi_set_forecast
 * (count = 0 clears it); the set and its time reach every later update, captured graphs included.
 * MPPI_ERR_INVALID when avoidance is not enabled, count is outside [0, MPPI_MAX_OBSTACLES], a kind
 * is unknown, a mask has bits above bit 8, a value is not finite, a radius is negative, or a
 * half-space normal is off unit length (| |n| - 1 | > 1e-9).  Not to be called concurrently with an
 * update.  Sharded handles take the configuration and the set per handle: every rank must set the
 * same ones.  mppi_get_obstacles: out16 has room for MPPI_MAX_OBSTACLES.
 * mppi_optimal_obstacle_cost: the obstacle term of the last update's filter() row summed over its
 * steps, undiscounted, next to mppi_optimal_terms' seven totals (which, like mppi_cost_evaluate,
 * keep their terms and totals as they are); waits for (or runs) that filter() the same way; 0 with
 * an empty set or before the first published update, MPPI_ERR_UNSUPPORTED when avoidance is off.
 * Added after ABI version 5 without a version change (new structs only): detect by symbol.
 *
 * Capsules (mppi_set_obstacle_capsules): the links between the robot's points, and capsule obstacles.
 * Robot segment s (s = 0..MPPI_OBSTACLE_SEGMENTS - 1) joins robot point s and robot point s + 1, with
 * the points' lag (q_0 for k = 0, q_{k-1} after) and its own radius segment_radii[s]; the pairs are
 * fixed.  Segments 1 and 5 have zero length on this robot (joints 1 and 2, and 5 and 6, coincide):
 * they are legal and behave as points.  Bits 0..8 of a mask keep their meaning; bit 16 + s selects
 * segment s (MPPI_OBSTACLE_MASK_SEGMENT(s), all of them MPPI_OBSTACLE_MASK_SEGMENTS).
 * MPPI_OBSTACLE_MASK_ALL stays the nine points: a set written for a handle without capsules means
 * on a capsule handle exactly what it meant.  MPPI_OBSTACLE_CAPSULE is the segment from c_o(k) to
 * c_o(k) + normal with radius >= 0: the normal field is the axis vector, any finite vector (zero: a
 * sphere), and the whole capsule translates with velocity.
 * The distance d(a, b; c, e) between segment a -> b and segment c -> c + e is Ericson's closest-point
 * form with exact-zero guards only.  d1 = b - a, r = a - c, A = d1 . d1, E = e . e, F = e . r:
 *   A = 0 and E = 0: s = t = 0.    A = 0, E != 0: s = 0, t = clamp01(F / E).
 *   otherwise C = d1 . r;  E = 0: t = 0, s = clamp01(-C / A);  else B = d1 . e, den = A E - B B,
 *     s = clamp01((B F - C E) / den) if den > 0 else 0,  t = (B s + F) / E,
 *     t < 0: t = 0, s = clamp01(-C / A);   t > 1: t = 1, s = clamp01((B - C) / A)
 *   d = |(a + s d1) - (c + t e)|
 * every operation rounded by itself.  A robot point is the segment (p, p), a sphere the capsule e = 0.
 * Clearance:
 *   point i,   sphere / half-space   as above
 *   point i,   capsule               v = d(p_i, p_i; c, e) - (radii[i] + radius_o)
 *   segment s, sphere or capsule     v = d(p_s, p_{s+1}; c, e) - (segment_radii[s] + radius_o)
 *   segment s, half-space            v = min(n . (p_s - c), n . (p_{s+1} - c)) - segment_radii[s]
 * and the step's term is, per obstacle in index order, the masked points in index order, then the
 * masked segments in index order, each through Left(limit); it is added where the obstacle term is.
 * mppi_set_obstacle_capsules (config NULL: mppi_default_capsule_config, 0.1 for every segment) selects
 * the capsule kernels for the handle's life: after mppi_set_obstacle_avoidance and before the first
 * update (MPPI_ERR_INVALID otherwise, the message says which), radii finite and >= 0.
 * mppi_get_obstacle_capsules: enabled = 0 for a handle that never enabled them (out untouched).
 * mppi_set_obstacles on a handle without capsules refuses the capsule kind and any mask bit above 8;
 * on a capsule handle bits 0..8 and 16..23 are legal, every other bit is invalid, and a capsule's
 * axis must be finite (it need not be a unit vector; a half-space normal still must).
 * mppi_optimal_obstacle_cost returns the capsule term's total on a capsule handle.
 * Added like the obstacle symbols, without a version change: detect by symbol. */
#define MPPI_MAX_OBSTACLES 16
#define MPPI_OBSTACLE_POINTS 9
#define MPPI_OBSTACLE_SPHERE 0
#define MPPI_OBSTACLE_HALF_SPACE 1
#define MPPI_OBSTACLE_CAPSULE 2
#define MPPI_OBSTACLE_MASK_ALL 0x1FFu
#define MPPI_OBSTACLE_SEGMENTS 8
#define MPPI_OBSTACLE_MASK_SEGMENT(s) (1u << (16 + (s)))
#define MPPI_OBSTACLE_MASK_SEGMENTS 0xFF0000u
typedef struct mppi_obstacle {
    int32_t kind;     /* MPPI_OBSTACLE_* */
    uint32_t mask;    /* bit i: robot point i is tested */
    double position[3], velocity[3], normal[3], radius;
} mppi_obstacle;
typedef struct mppi_obstacle_config {
    mppi_barrier limit;                       /* left */
    double radii[MPPI_OBSTACLE_POINTS];
} mppi_obstacle_config;
void mppi_default_obstacle_config(mppi_obstacle_config *out);
mppi_status mppi_set_obstacle_avoidance(mppi_handle *h, const mppi_obstacle_config *config);
mppi_status mppi_get_obstacle_avoidance(mppi_handle *h, int *enabled, mppi_obstacle_config *out);
mppi_status mppi_set_obstacles(mppi_handle *h, const mppi_obstacle *obstacles, int32_t count, double time);
mppi_status mppi_get_obstacles(mppi_handle *h, mppi_obstacle *out16, int32_t *count, double *time);
mppi_status mppi_optimal_obstacle_cost(mppi_handle *h, double *cost);
typedef struct mppi_capsule_config {
    double segment_radii[MPPI_OBSTACLE_SEGMENTS];
} mppi_capsule_config;
void mppi_default_capsule_config(mppi_capsule_config *out);
mppi_status mppi_set_obstacle_capsules(mppi_handle *h, const mppi_capsule_config *config);
mppi_status mppi_get_obstacle_capsules(mppi_handle *h, int *enabled, mppi_capsule_config *out);

/* The sensed environment as a signed-distance grid (mppi_set_distance_field_avoidance): one more part
 * of the obstacle term, behind the capsule term of the primitives.  What a depth camera and a mapper
 * (an ESDF, a voxel map) hand over several times a second, boxes and meshes included.
 *
 * Field: a regular grid of dims = (nx, ny, nz) samples, each dimension in [2, 512] and
 * nx ny nz <= 2^24; origin is the world position of sample (0, 0, 0); voxel > 0 is the edge length on
 * every axis; values are nx ny nz fp32 signed distances in metres, negative inside matter, in the
 * layout of a C-contiguous (nx, ny, nz) array (z fastest), all finite.  The field does not move; it
 * is replaced between updates.  The engine computes inv_voxel = 1.0 / voxel once in fp64; the device
 * never divides.
 * Sample D(p) at a world point p, every operation rounded by itself (no fused multiply-add):
 *   g_a = (p_a - origin_a) * inv_voxel                      a = x, y, z
 *   p is inside iff 0 <= g_a <= n_a - 1 on all three axes
 *   i_a = min(floor(g_a), n_a - 2)   (the top face belongs to the last cell),   f_a = g_a - i_a
 *   c[dx][dy][dz] = (double) values[((i_x + dx) ny + (i_y + dy)) nz + (i_z + dz)]
 *   with L(a, b, f) = a + f (b - a):  along z, then y, then x
 *     cz[dx][dy] = L(c[dx][dy][0], c[dx][dy][1], f_z),  cy[dx] = L(cz[dx][0], cz[dx][1], f_y),
 *     D = L(cy[0], cy[1], f_x)
 * The interpolant is continuous across cell faces.  A point outside the grid contributes exactly 0
 * (unknown space is free: the caller pads the grid); a NaN coordinate makes the contribution NaN.
 * What is sampled: the robot's nine points and eight segments of the capsule handle, with their
 * lag.  mask has the obstacle masks' bit meanings (bits 0..8 points, bits 16..23 segments), and
 * segment_samples m in [0, 8].  Point i gives v = D(p_i) - radii[i]; segment s gives, for j = 1..m,
 * p = p_s + phi_j (p_{s+1} - p_s), phi_j = j / (m + 1) computed on the host in fp64, and
 * v = D(p) - segment_radii[s] (the end points belong to the point bits; the zero-length segments 1
 * and 5 sample one point m times; a point is sampled as it is, with no arithmetic on it).  The step's term is the sum of Left(limit)(v) over the masked
 * points in index order, then the masked segments in index order, each segment's samples in order j,
 * with the avoidance configuration's limit; it is added to the capsule term, before gamma^k.
 *
 * mppi_set_distance_field_avoidance selects the field kernels for the handle's life: after
 * mppi_set_obstacle_capsules and before the first update (MPPI_ERR_INVALID otherwise, the message
 * says which).  mppi_set_distance_field replaces the field between any two updates (field NULL:
 * no field, values ignored); the values are copied before it returns control of them (the caller's
 * array may be reused once the call returns).  MPPI_ERR_INVALID for a dimension or the product out of
 * range, a non-finite value, origin or voxel, voxel <= 0, a mask bit outside 0..8 and 16..23, or
 * segment_samples outside [0, 8]; a refused call leaves the field in place.  Not to be called
 * concurrently with an update; on sharded handles every rank sets the same field.  The filter() row
 * of an update reads that update's field, also when the field was replaced before the row ran.
 * mppi_get_distance_field: the descriptor only; present = 0 with no field (out untouched).
 * mppi_optimal_field_cost: the field term of the last filter() row summed over its steps,
 * undiscounted (0 with no field or before the first published update; MPPI_ERR_UNSUPPORTED on a
 * handle without field avoidance); mppi_optimal_obstacle_cost returns the capsule term plus the
 * field term on a field handle.  Added like the capsule symbols, without a version change: detect
 * by symbol. */
#define MPPI_DISTANCE_FIELD_MIN_DIM 2
#define MPPI_DISTANCE_FIELD_MAX_DIM 512
#define MPPI_DISTANCE_FIELD_MAX_VALUES (1 << 24)
#define MPPI_DISTANCE_FIELD_MAX_SAMPLES 8
typedef struct mppi_distance_field {
    int32_t dims[3];
    int32_t segment_samples;
    uint32_t mask;
    int32_t pad;
    double origin[3];
    double voxel;
} mppi_distance_field;
mppi_status mppi_set_distance_field_avoidance(mppi_handle *h);
mppi_status mppi_get_distance_field_avoidance(mppi_handle *h, int *enabled);
mppi_status mppi_set_distance_field(mppi_handle *h, const mppi_distance_field *field, const float *values);
mppi_status mppi_get_distance_field(mppi_handle *h, mppi_distance_field *out, int *present);
mppi_status mppi_optimal_field_cost(mppi_handle *h, double *cost);

/* A held object (mppi_set_held_object_avoidance): what the gripper carries - a beam, a tray, a tool -
 * as spheres fixed in the grasp frame, one more part of the obstacle term behind the field term.
 *
 * The object is count in [0, MPPI_HELD_POINTS] spheres with centres c_i in the grasp frame, in metres,
 * and radii r_i >= 0.  For count >= 2 there are segments s = 0 .. count - 2: segment s joins held point
 * s and held point s + 1 and has its own radius segment_radii[s] >= 0 (a beam: two points and one
 * segment; a tray: about four points and three segments; a tool tip: one point).  Coincident points (a
 * zero-length segment) are legal and behave as a point, as robot segments 1 and 5 do.
 * World position at the cost of step k:  h_i = p_ee + Ree c_i, with p_ee the grasp-frame position that
 * obstacle point 8 reads and Ree = R9 ee_R (body 9's world rotation times the grasp placement's) taken at
 * the same lagged configuration (q_0 for k = 0, q_{k-1} after).  Row r is
 *   h_i[r] = p_ee[r] + ((Ree[r][0] c_x + Ree[r][1] c_y) + Ree[r][2] c_z)
 * every operation rounded by itself (no fused multiply-add).  A non-finite pose makes the term NaN, and
 * so the rollout, like any step cost.
 * Clearances are the robot's own formulas (above) with the held radii in place of radii[i] and
 * segment_radii[s]: a held point against a sphere, a half-space and a capsule; a held segment against a
 * sphere or a capsule through the one segment-segment distance d(a, b; c, e); a held segment against a
 * half-space by the minimum of its two ends; against the distance field D(h_i) - r_i for a point and,
 * for a segment, its segment_samples interior samples p = h_s + phi_j (h_{s+1} - h_s), phi_j = j / (m + 1),
 * with D(p) - segment_radii[s].  Each clearance goes through the avoidance configuration's Left(limit).
 * Mask bits, in an obstacle's mask and in the field's: held point i is bit 9 + i
 * (MPPI_OBSTACLE_MASK_HELD_POINT(i), i < 4), held segment s is bit 24 + s
 * (MPPI_OBSTACLE_MASK_HELD_SEGMENT(s), s < 3), MPPI_OBSTACLE_MASK_HELD is all seven.  A bit that names a
 * point or segment the current object does not have selects nothing; it is not an error, so one mask
 * constant serves every object.  MPPI_OBSTACLE_MASK_ALL and MPPI_OBSTACLE_MASK_SEGMENTS keep their
 * values: a set written for a robot without a held object means exactly what it meant.
 * Order: the held term of a step runs over the obstacles in index order, per obstacle the masked held
 * points in index order, then the masked held segments in index order; then, with a field present, the
 * masked held points, then the masked held segments' samples in order j.  The step's obstacle term is
 * (capsule term + field term) + held term, in that association.  With no object, or with nothing
 * masked, the held term is +0.0 and every cost keeps its bits.  It acts wherever the obstacle term acts.
 *
 * mppi_set_held_object_avoidance selects the held-object kernels for the handle's life: after
 * mppi_set_distance_field_avoidance and before the first update (MPPI_ERR_INVALID otherwise, the
 * message says which).  mppi_set_held_object replaces the object between any two updates (NULL or
 * count = 0: the object was put down).  MPPI_ERR_INVALID when the mode is off, count is outside [0, 4],
 * a centre or a radius is not finite, or a radius is negative (of the points and segments the object
 * has); a refused call leaves the object in place.  Not to be called concurrently with an update; on
 * sharded handles every rank sets the same object.  On a held handle mppi_set_obstacles and
 * mppi_set_distance_field accept the held bits; on every other handle they refuse them.  The filter()
 * row of an update reads that update's object, also when the object was replaced before the row ran;
 * captured graphs see each update's object.
 * mppi_get_held_object: present = 0 with no object (out untouched).
 * mppi_optimal_held_cost: the held term of the last filter() row summed over its steps, undiscounted (0
 * with no object or before the first published update; MPPI_ERR_UNSUPPORTED on a handle without the
 * mode); mppi_optimal_obstacle_cost returns capsule + field + held on a held handle.
 * mppi_predicted_held_optimal / mppi_predicted_held_rollouts: the world paths of the held points at q_k
 * itself (not lagged), as mppi_predicted_optimal / mppi_predicted_rollouts give the robot's:
 * out[k][i][0..2] with MPPI_HELD_POINTS rows a step; the rows of points the current object does not
 * have are NaN, and so is everything from a rollout's first non-finite step on.  The same error rules.
 * Added like the field symbols, without a version change: detect by symbol. */
#define MPPI_HELD_POINTS 4
#define MPPI_HELD_SEGMENTS 3
#define MPPI_OBSTACLE_MASK_HELD_POINT(i) (1u << (9 + (i)))
#define MPPI_OBSTACLE_MASK_HELD_SEGMENT(s) (1u << (24 + (s)))
#define MPPI_OBSTACLE_MASK_HELD 0x07001E00u
typedef struct mppi_held_object {
    int32_t count;
    int32_t pad;
    double centres[MPPI_HELD_POINTS][3];
    double radii[MPPI_HELD_POINTS];
    double segment_radii[MPPI_HELD_SEGMENTS];
} mppi_held_object;
mppi_status mppi_set_held_object_avoidance(mppi_handle *h);
mppi_status mppi_get_held_object_avoidance(mppi_handle *h, int *enabled);
mppi_status mppi_set_held_object(mppi_handle *h, const mppi_held_object *object);
mppi_status mppi_get_held_object(mppi_handle *h, mppi_held_object *out, int *present);
mppi_status mppi_optimal_held_cost(mppi_handle *h, double *cost);
mppi_status mppi_predicted_held_optimal(mppi_handle *h, double *out_Hx4x3);
mppi_status mppi_predicted_held_rollouts(mppi_handle *h, const int64_t *rollouts, int64_t n, double *out_nxHx4x3);

/* The held object against the robot's own links (mppi_set_held_self_avoidance): the one pair the held
 * term leaves out.  A beam or a tray in the grasp sweeps the largest volume of anything on the robot, and
 * the tower and the forearm are the nearest solid things to it; the reference's self-collision pairs are
 * link spheres only and cannot see it.  One more part of the obstacle term, behind the held term.
 *
 * Held unit u = 0..6: units 0..3 are held points 0..3, units 4..6 held segments 0..2 (held segment s'
 * joins held points s' and s' + 1).  Robot segment s = 0..7 joins robot points s and s + 1 (the nine
 * points of the obstacle term: the eight sphere links, then the end effector), as on a capsule handle,
 * at the same lagged configuration as the held points (q_0 for k = 0, q_{k-1} after).
 * The configuration (mppi_held_self): units, bit i (i < 4) held point i, bit 4 + s' (s' < 3) held
 * segment s' (MPPI_HELD_SELF_UNITS: all seven); segments, bit s (s < 8) robot segment s; radii[s], that
 * segment's radius for this term only, finite and >= 0 - apart from mppi_capsule_config::segment_radii,
 * so that segment 0 (pivot -> link 1, the 1.08-m tower) can be made as fat as the chassis.
 * mppi_default_held_self: units 0x7F, segments 0x1F, every radius 0.1 - without the wrist and hand
 * segments 5..7, which anything in the gripper touches.
 * Clearance of held unit u and robot segment s:  v = d(a, b; c, e) - (radii[s] + r_u), d the one
 * segment-segment distance above in capsule_term's orientation, the robot's segment first
 * (a = p_s, b = p_{s+1}) and the other body second (c -> c + e): a held point has c = h_i, e = 0 and
 * r_u = its radii[i]; a held segment has c = h_s', e = h_{s'+1} - h_s', each component one rounded
 * subtraction, E = e . e rounded operation by operation, and r_u = its segment_radii[s'].  Zero-length
 * robot segments (1 and 5) and held points are legal: every degenerate class of d occurs.
 * The step's term is the sum of Left(limit)(v), with the avoidance configuration's barrier, over the
 * masked held units that the current object has in order u = 0..6, per unit the masked robot segments in
 * order s = 0..7.  The step's obstacle term becomes ((capsule term + field term) + held term) + self
 * term, in that association.  With no object, no configuration or nothing masked the term is +0.0 and
 * every cost keeps its bits.  A non-finite pose makes the term NaN, and so the rollout.
 *
 * mppi_set_held_self_avoidance selects the held-self kernels for the handle's life: after
 * mppi_set_held_object_avoidance and before the first update (MPPI_ERR_INVALID otherwise, the message
 * says which).  There is no environment switch.  mppi_set_held_self replaces the configuration between
 * any two updates (NULL: none); it touches host state only, like mppi_set_held_object.
 * MPPI_ERR_INVALID when the mode is off, units has a bit above 6, segments a bit above 7, or a radius is
 * not finite or negative; a refused call changes nothing.  On sharded handles every rank sets the same
 * one.  The filter() row of an update reads that update's configuration, also when it was replaced
 * before the row ran; captured graphs see each update's configuration.
 * mppi_get_held_self: present = 0 with no configuration (out untouched).
 * mppi_optimal_held_self_cost: the self term of the last filter() row summed over its steps,
 * undiscounted (0 before the first published update; MPPI_ERR_UNSUPPORTED on a handle without the mode);
 * mppi_optimal_obstacle_cost returns capsule + field + held + self on such a handle.
 * Added like the held symbols, without a version change: detect by symbol. */
#define MPPI_HELD_SELF_UNITS 0x7Fu
#define MPPI_HELD_SELF_UNIT_POINT(i) (1u << (i))
#define MPPI_HELD_SELF_UNIT_SEGMENT(s) (1u << (4 + (s)))
#define MPPI_HELD_SELF_SEGMENTS 8
typedef struct mppi_held_self {
    uint32_t units;
    uint32_t segments;
    double radii[MPPI_HELD_SELF_SEGMENTS];
} mppi_held_self;
void mppi_default_held_self(mppi_held_self *cfg);
mppi_status mppi_set_held_self_avoidance(mppi_handle *h);
mppi_status mppi_get_held_self_avoidance(mppi_handle *h, int *enabled);
mppi_status mppi_set_held_self(mppi_handle *h, const mppi_held_self *cfg);
mppi_status mppi_get_held_self(mppi_handle *h, mppi_held_self *out, int *present);
mppi_status mppi_optimal_held_self_cost(mppi_handle *h, double *cost);

/* Target tracking: TrackPoint follows a timed end-effector pose path over the horizon instead of
 * one fixed point.  The reference describes such targets (controller/trajectory.hpp) but feeds none
 * to an objective; here they are an opt-in mode of TrackPoint.  Nothing changes unless it is enabled.
 *
 * mppi_set_target_tracking (config NULL: mppi_default_target_tracking_config, {10.0, 0}) selects the
 * mode for the handle's life: FrankaRidgeback handles with MPPI_COST_TRACK_POINT only
 * (MPPI_ERR_UNSUPPORTED otherwise), before the first update (MPPI_ERR_INVALID after it), and not
 * together with an attached forecast (mppi_forecast_attach, whose step constants share the fields the
 * targets live in: MPPI_ERR_INVALID either way round).  orientation_weight must be finite and >= 0.
 * track_orientation = 1 needs MPPI_LINK_POSITIONS_KINEMATIC (MPPI_ERR_INVALID otherwise, the message
 * says which condition failed), and the link-position model is fixed from then on; position tracking
 * works in every link mode.  mppi_get_target_tracking: enabled = 0 for a handle that never enabled
 * it (out untouched).
 *
 * A path (mppi_set_target_path, between any two updates; NULL clears it) is 1 <= count <=
 * MPPI_TARGET_WAYPOINTS_MAX waypoints: finite, strictly increasing times, finite positions and, with
 * has_orientation, finite quaternions (x, y, z, w, MPPI_EE_QUATERNION's order) of norm in [0.5, 2].
 * On set each quaternion is normalised in fp64, then waypoint i + 1's is negated whenever its dot
 * product with waypoint i's (already fixed) is negative; mppi_get_target_path returns the path as
 * stored (present = 0: none).  Anything invalid is MPPI_ERR_INVALID with a message, and the path
 * that was set before stays.  The sample at time t: waypoint 0 for t <= time[0], waypoint count - 1
 * for t >= time[count - 1]; otherwise, with i the greatest index with time[i] <= t and
 * f = (t - time[i]) * (1 / (time[i + 1] - time[i])), p = p_i + f (p_{i+1} - p_i) and
 * q = q_i + f (q_{i+1} - q_i) divided by its norm (>= sqrt(1/2) after the sign fix).
 *
 * The cost of step k of an update at t0 on a tracking handle, t_k = t0 + k dt (the time get_cost is
 * called with): the position term 100 pow(|p_EE - p(t_k)|, 2) (without a path p is the descriptor's
 * point), p_EE the grasp-frame position track_point_cost reads; then, with track_orientation and a
 * path that has orientations, orientation_weight * (3 - sum_ij Rt_ij Ree_ij) = 4 w sin^2(theta / 2),
 * Rt the rotation matrix of q(t_k), Ree = R_9 ee_R with R_9 body 9's world rotation at the lagged
 * configuration the link positions use (q_0 for step 0, else q - qd dt); then the joint-limit,
 * self-collision and reach terms, and the sum is discounted; the obstacle term follows as before.
 * The update that ran keeps its own targets for its filter() row.
 * mppi_optimal_target_cost: out2 = the position and the orientation totals of the last update's
 * filter() row, undiscounted (zeros before the first published update; MPPI_ERR_UNSUPPORTED when
 * tracking is off).  Added like the obstacle symbols, without a version change: detect by symbol. */
#define MPPI_TARGET_WAYPOINTS_MAX 32
typedef struct mppi_target_tracking_config {
    double orientation_weight;
    int32_t track_orientation;
} mppi_target_tracking_config;
typedef struct mppi_target_waypoint {
    double time;
    double position[3];
    double quaternion[4];
} mppi_target_waypoint;
typedef struct mppi_target_path {
    int32_t count;
    int32_t has_orientation;
    mppi_target_waypoint waypoints[MPPI_TARGET_WAYPOINTS_MAX];
} mppi_target_path;
void mppi_default_target_tracking_config(mppi_target_tracking_config *out);
mppi_status mppi_set_target_tracking(mppi_handle *h, const mppi_target_tracking_config *config);
mppi_status mppi_get_target_tracking(mppi_handle *h, int *enabled, mppi_target_tracking_config *out);
mppi_status mppi_set_target_path(mppi_handle *h, const mppi_target_path *path);
mppi_status mppi_get_target_path(mppi_handle *h, mppi_target_path *out, int *present);
mppi_status mppi_optimal_target_cost(mppi_handle *h, double *out2);

/* The trajectory safety filter: FrankaRidgeback::TrajectorySafetyFilter::Configuration
 * (frankaridgeback/safety.hpp:15-40) field for field.  The reference declares the class and leaves
 * its methods empty; here the configuration is live, opt-in (no filter unless one is set).  The
 * filter is stateless and acts on joints 0..9 (the fingers are not actuated).  Column k of the new
 * plan U* is corrected, while the plan is rolled out from the update's state with the handle's own
 * time step, so that the state after the step meets the enabled limits; the switches are applied
 * in the order position, velocity, acceleration and a later one wins (a position limit holds only
 * where the velocity and acceleration limits do not bind: there is no braking-distance rule).  The
 * arm's torque is corrected through the mass matrix with the other joints' torque untouched, the
 * base's velocity command directly.  A column that no limit binds is returned bit for bit, and U*
 * is not clamped to control_min / control_max again.  A limit may be +-inf (no limit on that side);
 * NaN, or a minimum above its maximum, is MPPI_ERR_INVALID.  limit_reach is refused
 * (MPPI_ERR_UNSUPPORTED): it needs a task-space solve, and both objectives carry a reach barrier.
 * The definition: DESIGN.md section 1, "Safety filter".
 *
 * mppi_set_safety_filter: FrankaRidgeback handles only (MPPI_ERR_UNSUPPORTED otherwise, and for a
 * horison past 384 steps); NULL turns the filter off; it may be set or changed between any two
 * updates.  With a filter set the update publishes the filtered plan only (mppi_get,
 * mppi_optimal_control, the optimal rollout and the next update all see it), mppi_unfiltered_control
 * returns the plan as optimise() left it (equal to mppi_optimal_control without a filter), and
 * updates do not run as a hipGraph.  mppi_safety_filter_stats: the number of steps of the last
 * update's plan the filter changed, and the filter kernel's time in ms (0 unless mppi_set_timing
 * is 1 or 2); either pointer may be NULL.
 * Added after ABI version 5 without a version change (one new struct, new symbols): detect by symbol. */
typedef struct mppi_safety_filter_desc {
    double position_minimum[MPPI_FR_JOINTS], position_maximum[MPPI_FR_JOINTS];
    double velocity_minimum[MPPI_FR_JOINTS], velocity_maximum[MPPI_FR_JOINTS];
    double acceleration_minimum[MPPI_FR_JOINTS], acceleration_maximum[MPPI_FR_JOINTS];
    double reach_maximum, reach_minimum;
    int32_t limit_joints, limit_velocity, limit_acceleration, limit_reach;
} mppi_safety_filter_desc;
/* Every switch off; robot.urdf's joint position limits and velocity limits (base 1, arm 2.175 /
 * 2.61, fingers 0.3); robot.urdf has no acceleration limits: +-inf; reach 0.8 / 0.15. */
void mppi_default_safety_filter(mppi_safety_filter_desc *out);
mppi_status mppi_set_safety_filter(mppi_handle *h, const mppi_safety_filter_desc *filter);
mppi_status mppi_get_safety_filter(mppi_handle *h, int *enabled, mppi_safety_filter_desc *out);
mppi_status mppi_unfiltered_control(mppi_handle *h, double *control_CxH);
mppi_status mppi_safety_filter_stats(mppi_handle *h, int64_t *changed_steps, float *kernel_ms);

/* Phase-split update for callers that run the collectives themselves (multi-GPU with an
 * external communicator, or two shards on one device in tests).  Between phase 1 and 2 the
 * caller all-reduces (sum) the R + 1 doubles of mppi_device_costs(h) - the R costs and slot R,
 * the ranks' in-launch wait timeouts, so that every rank fails an update whose costs some rank
 * lost (MPPI_ERR_DEVICE); between phase 2 and 3 it all-reduces (sum) mppi_device_gradient(h).
 * Buffers are fp64 device pointers on mppi_stream(h). */
mppi_status mppi_update_phase1(mppi_handle *h, const double *state, double time);
mppi_status mppi_update_phase2(mppi_handle *h);
mppi_status mppi_update_phase3(mppi_handle *h);
void *mppi_device_costs(mppi_handle *h);     /* R + 1 doubles (the costs, then the wait-timeout count) */
/* The number of doubles of mppi_device_costs the caller all-reduces: R + 1 since ABI version 4 (R
 * before; a caller that reduces only R loses the cross-rank wait-timeout failure).  Integrators
 * check mppi_abi_version() >= 5 and size the all-reduce from this. */
int64_t mppi_device_costs_count(mppi_handle *h);
void *mppi_device_gradient(mppi_handle *h);  /* C*H doubles */
void *mppi_stream(mppi_handle *h);           /* hipStream_t */

/* filter() (the optimal rollout, mppi.cpp:450-479) runs on a side stream overlapped with the
 * next update's sampling and rollouts; mppi_optimal_cost and mppi_kernel_times wait for it,
 * and mppi_synchronize waits for all device work of the handle. */
mppi_status mppi_synchronize(mppi_handle *h);

/* Trajectory::get (mppi.cpp:481-512): thread-safe against a concurrent update(). */
mppi_status mppi_get(mppi_handle *h, double time, double *control);

/* Observables (logger::MPPI::log reads these, logging/mppi.cpp:84-136). Host copies in the
 * reference layouts. */
mppi_status mppi_costs(mppi_handle *h, double *costs_R);
mppi_status mppi_weights(mppi_handle *h, double *weights_R);
mppi_status mppi_gradient(mppi_handle *h, double *gradient_CxH);
mppi_status mppi_optimal_control(mppi_handle *h, double *control_CxH);
mppi_status mppi_optimal_cost(mppi_handle *h, double *cost);
mppi_status mppi_argmin(mppi_handle *h, int64_t *rollout);
/* The optimal rollout's per-term totals: FrankaRidgeback::AssistedManipulation's accumulators after
 * filter() (thread 0's cost, reset at the optimal rollout's start; assisted_manipulation.cpp:24-35,
 * 74-319), which BaseTest reads by downcasting get_optimal_cost() (test/case/base.cpp:140-146) and
 * logger::AssistedManipulation logs (logging/assisted_manipulation.cpp:61-90).  terms7[MPPI_TERM_*];
 * a disabled term is 0.  AssistedManipulation objective only (MPPI_ERR_UNSUPPORTED otherwise). */
#define MPPI_TERM_JOINT_LIMIT 0      /* get_joint_limit_cost()      (.hpp:232-234) */
#define MPPI_TERM_SELF_COLLISION 1   /* get_self_collision_cost()   (.hpp:236-238) */
#define MPPI_TERM_WORKSPACE 2        /* get_workspace_cost()        (.hpp:240-242) */
#define MPPI_TERM_ENERGY_TANK 3      /* get_energy_tank_cost()      (.hpp:244-246) */
#define MPPI_TERM_JOINT_VELOCITY 4   /* get_joint_velocity_cost()   (.hpp:248-250) */
#define MPPI_TERM_TRAJECTORY 5       /* get_trajectory_cost()       (.hpp:252-254) */
#define MPPI_TERM_MANIPULABILITY 6   /* get_manipulability_cost()   (.hpp:256-258) */
mppi_status mppi_optimal_terms(mppi_handle *h, double *terms7);

/* Predicted trajectories: where the robot goes under the published plan (the filter() row
 * mppi_optimal_terms answers for) and under the rollouts of the last update.  The reference offers
 * only get_optimal_dynamics(), the last state of thread 0's object (mppi.hpp:456-462); the device
 * keeps every rollout's step records until the next launch and answers from them.  One row of
 * MPPI_PRED_N doubles per horizon step:
 *   row k (k < H) is the state x_k at which step k's cost is evaluated, so row 0 is the update's
 *   state; x_H is never computed.  The six wrench slots of the state do not change during a rollout
 *   and are left out.
 *   The positions are forward kinematics at q_k itself - not the one-step-lagged kinematics the
 *   objective sees (the end effector at q_{k-1}, as MPPI_LINK_POSITIONS_KINEMATIC's links).
 *   MPPI_PRED_LINKS: row 0 the universe, row 1 + i body i's frame origin in the world.
 * NaN rule: from the first step whose q, qd (or E, where the tank is integrated) is not finite, every
 * column of that row and of all later rows of the rollout is NaN, whatever the launch stored behind
 * it.  A rollout whose cost is NaN while its states stay finite keeps its finite rows.
 * FrankaRidgeback handles only (MPPI_ERR_UNSUPPORTED otherwise).  Like mppi_costs, not to be called
 * concurrently with an update.  These functions came after ABI version 5 without a version change
 * (no struct changed): detect them by symbol. */
#define MPPI_PRED_Q 0           /* q_k, 12 */
#define MPPI_PRED_QD 12         /* qd_k, 12 */
#define MPPI_PRED_ENERGY 24     /* tank level E_k; NaN unless the handle's launches integrate the tank */
#define MPPI_PRED_EE 25         /* grasp-frame position at q_k, 3 */
#define MPPI_PRED_ARM_MOUNT 28  /* arm-mount frame position at q_k, 3 */
#define MPPI_PRED_LINKS 31      /* world origin of link L (MPPI_LINK_*) at q_k, 13 x 3 */
#define MPPI_PRED_N 70
/* The optimal rollout of the last published update (H x MPPI_PRED_N): MPPI_ERR_INVALID before the
 * first published update; otherwise waits for (or runs) that update's filter() as mppi_optimal_terms
 * does. */
mppi_status mppi_predicted_optimal(mppi_handle *h, double *out_HxN);
/* n rollouts of the last rollout launch by global rollout index (n x H x MPPI_PRED_N, in the order
 * asked for; n = 0 is a no-op).  MPPI_ERR_INVALID before the first update, for an index outside
 * [0, R) and, on a sharded handle, outside its own [begin, begin + count); MPPI_ERR_DEVICE after an
 * update that failed with in-launch wait timeouts (rows were lost). */
mppi_status mppi_predicted_rollouts(mppi_handle *h, const int64_t *rollouts, int64_t n, double *out_nxHxN);
mppi_status mppi_update_duration(mppi_handle *h, double *seconds);
/* Trajectory::get_update_last (mppi.hpp:381-384): the time of the last successful update, whichever
 * entry made it (mppi_update, the phase-split calls); the count is MPPI_INFO_UPDATE_COUNT. */
mppi_status mppi_update_last(mppi_handle *h, double *time);
mppi_status mppi_noise(mppi_handle *h, double *noise_R_C_H);
mppi_status mppi_dims(mppi_handle *h, int64_t *rollouts_R, int64_t *steps_H,
                      int64_t *control_C, int64_t *state_X);

/* What the last update's rollout launch did (diagnostics for bench / tests; the engine decides it
 * from the device's CU count and the workload): info[i] for i < n (n <= MPPI_UPDATE_INFO_N). */
#define MPPI_INFO_COOPERATIVE 0           /* 1: the 16-lane cooperative kernel (FrankaRidgeback), 0: the point mass */
#define MPPI_INFO_FOLDED_FILTER 1         /* the previous update's filter() rode in the launch */
#define MPPI_INFO_OBJECTIVE_IN_LAUNCH 2   /* the objective ran in the launch (no cost kernel) */
#define MPPI_INFO_TAIL_DRAWS 3            /* the launch drew the next update's eps (main rows) */
#define MPPI_INFO_SAMPLING 4              /* 0 sample kernel, 1 sampled in the launch (point mass), 2 drawn ahead */
#define MPPI_INFO_ROWS 5                  /* rows rolled out (local rollouts + a folded filter()) */
#define MPPI_INFO_HANDOVER 6              /* step at which relay stage 1 took the rows left over
                                             (relay_stage), -1 none; read from the device */
#define MPPI_INFO_WAIT_TIMEOUTS 7         /* in-launch waits that gave up in the last update's
                                             rollout launch (a bug if nonzero: that update then
                                             failed with MPPI_ERR_DEVICE and published nothing) */
#define MPPI_INFO_WAIT_TIMEOUTS_TOTAL 8   /* the same, summed over every update since create */
#define MPPI_INFO_FUSED_UPDATE 9          /* 1: the whole update ran as one launch (point mass,
                                             pm_update_kernel) */
#define MPPI_INFO_GRAPH_UPDATES 10        /* updates since create that ran as the captured hipGraph */
#define MPPI_INFO_GRAPH_FAILURES 11       /* graph captures that failed (that update then ran eagerly,
                                             its collectives matched; the handle stays eager) */
#define MPPI_INFO_UPDATE_COUNT 12         /* successful updates since create (Trajectory::update
                                             calls that published, whichever entry made them) */
#define MPPI_INFO_STAGE_WORK 13           /* objective chunks that a later relay member's stage waves evaluated ahead
                                           * of their stage, counted on the device since create (0 with
                                           * MPPI_STAGE_WORK=0, one relay member, the tank or TrackPoint) */
#define MPPI_INFO_FINISH_PATH 14          /* which kernel finished the last update (gradient step, Savitzky-Golay,
                                           * clamp, publish): 0 finish_flat_kernel (no filter), 1 sg_finish_kernel
                                           * (a wave per dimension, the window in LDS), 2 finish_kernel (a thread
                                           * per dimension over global memory: windows sg_finish_kernel cannot
                                           * stage); -1 when the fused point-mass launch finished it itself */
#define MPPI_FINISH_FLAT 0
#define MPPI_FINISH_SG 1
#define MPPI_FINISH_SG_GLOBAL 2
#define MPPI_UPDATE_INFO_N 15
mppi_status mppi_update_info(mppi_handle *h, int64_t *info, int n);

/* Fault injection for the failure-detection tests (no reference counterpart; never set in
 * production): the next `updates` rollout launches carry fault bits `fault`.
 * MPPI_DEBUG_RELAY_NO_SIGNAL: relay stage 1 of the workgroup with rows left over never signals
 * stage 2, so the bounded in-launch waits give up and the update must fail (MPPI_ERR_DEVICE). */
#define MPPI_DEBUG_RELAY_NO_SIGNAL 1
/* MPPI_DEBUG_GRAPH_INSTANTIATE_FAIL: the next `updates` hipGraph captures report an instantiation
 * failure after recording the update (host side; no launch carries it): the update must still run,
 * eagerly, with its collectives, and the handle stays on the eager path. */
#define MPPI_DEBUG_GRAPH_INSTANTIATE_FAIL 2
mppi_status mppi_debug_inject(mppi_handle *h, int fault, int updates);
/* The optimal-rollout cost the device holds now, as the last launch left it, without running or
 * waiting for a pending filter() (tests only): after an update whose launch folded the previous
 * update's filter() (MPPI_INFO_FOLDED_FILTER), that filter()'s cost - which mppi_optimal_cost no
 * longer returns, since it answers for the latest update. */
mppi_status mppi_debug_folded_cost(mppi_handle *h, double *cost);

/* Savitzky-Golay window state (SavitzkyGolayFilter::get_windows(), filter.hpp): per control
 * dimension the value and time buffers (C x (H + 2w + 1), row per dimension) and start index. */
mppi_status mppi_smoothing_windows(mppi_handle *h, double *uu, double *tt, int64_t *start_idx);

/* HIP-event timing of the update path: 0 (default) none, 1 the rollout kernel alone (slot [5] of
 * mppi_kernel_times_detail), 2 every slot.  Each event recorded between two kernels delays the
 * second by a few microseconds, so timing is off unless asked for. */
mppi_status mppi_set_timing(mppi_handle *h, int level);
/* Kernel timing of the last update (HIP events on the engine stream, timing level 2), milliseconds:
 * [0] sample/rank, [1] rollout, [2] weight-reduce, [3] optimal rollout, [4] whole update. */
mppi_status mppi_kernel_times(mppi_handle *h, float *ms5);
/* As mppi_kernel_times without waiting for the side stream: [3] is the latest optimal rollout
 * already finished (possibly an earlier update's).  For timing loops that keep filter() overlapped. */
mppi_status mppi_kernel_times_nowait(mppi_handle *h, float *ms5);
/* The first n (<= 8) per-update times of mppi_kernel_times_nowait, where [5] is the rollout
 * (dynamics) kernel alone: [1] spans it and the FrankaRidgeback cost kernel that sums the step
 * costs from its records; [6] (timing level 2) the weights + gradient launch alone, without the
 * finish kernel that [2] also spans (and, sharded over the engine's RCCL communicator, without the
 * cost all-reduce ahead of it); [7] that cost all-reduce (0 otherwise). */
mppi_status mppi_kernel_times_detail(mppi_handle *h, float *ms, int n);
/* The rollout launch's HIP-event times (ms) of every update run at timing level 1 since the last
 * call, oldest first (at most the last 64): *count <- min(recorded, capacity), and the record is
 * cleared.  Reading them after a timed loop keeps the event queries out of it (querying an event
 * pair right behind the publish held the host ~70 us). */
mppi_status mppi_rollout_kernel_times(mppi_handle *h, float *ms, int capacity, int *count);


/* ------------------------------------------------------------------------------------------
 * FrankaRidgeback::PinocchioDynamics as a device object (one trajectory).  The reference's
 * plugin is also an object with its own state (mppi.hpp:47-84, dynamics.hpp:416-537): the Actor's
 * DynamicsForecast steps one forward every controller period (dynamics.cpp:104-138), and a cost
 * reads the dynamics' cached end-effector state.  Its state lives in HBM and each call is one
 * single-thread kernel (pinocchio_dynamics.cpp:142-260 semantics, quirks included: set_state's
 * calculate() adds NLE onto the torque the previous call left).  FrankaRidgeback only.
 * ---------------------------------------------------------------------------------------- */
typedef struct mppi_dynamics mppi_dynamics;

/* EndEffectorState (dynamics.hpp:95-117) of the last calculate(), doubles: */
#define MPPI_EE_POSITION 0               /* 3: oMf[panda_grasp_joint].translation() */
#define MPPI_EE_QUATERNION 3             /* 4: orientation, Eigen coefficient order (x, y, z, w) */
#define MPPI_EE_ROTATION 7               /* 9: the same orientation as a row-major rotation matrix */
#define MPPI_EE_LINEAR_VELOCITY 16       /* 3: getFrameVelocity(WORLD).linear() */
#define MPPI_EE_ANGULAR_VELOCITY 19      /* 3 */
#define MPPI_EE_LINEAR_ACCELERATION 22   /* 3: getFrameAcceleration(WORLD).linear() (no gravity) */
#define MPPI_EE_ANGULAR_ACCELERATION 25  /* 3 */
#define MPPI_EE_JACOBIAN 28              /* 72: 6 x 12 row-major, WORLD, top-left 3x3 = R_z(yaw) */
#define MPPI_EE_N 100

/* One row of DynamicsForecast::forecast per step (dynamics.cpp:113-127), doubles: */
#define MPPI_DF_JOINT_POSITION 0                   /* 12: m_joint_position[step] */
#define MPPI_DF_END_EFFECTOR 12                    /* MPPI_EE_N: m_end_effector[step] */
#define MPPI_DF_JOINT_POWER (12 + MPPI_EE_N)       /* m_joint_power[step] (0 for Pinocchio) */
#define MPPI_DF_EXTERNAL_POWER (13 + MPPI_EE_N)    /* m_external_power[step] (0 for Pinocchio) */
#define MPPI_DF_ENERGY (14 + MPPI_EE_N)            /* m_energy[step]: the tank */
#define MPPI_DF_WRENCH (15 + MPPI_EE_N)            /* 6: m_end_effector_wrench[step] = forecast(t) */
#define MPPI_DF_N (21 + MPPI_EE_N)

/* PinocchioDynamics::create (pinocchio_dynamics.cpp:19-83; the constructor's set_state of the
 * configuration's initial state, :84-115).  `initial_state`: X = 31 doubles. */
mppi_status mppi_dynamics_create(const mppi_dynamics_desc *desc, const double *initial_state, int device,
                                 mppi_dynamics **out);
void mppi_dynamics_destroy(mppi_dynamics *d);
/* set_state (pinocchio_dynamics.cpp:142-151). */
mppi_status mppi_dynamics_set_state(mppi_dynamics *d, const double *state, double time);
/* step (pinocchio_dynamics.cpp:226-260): control C = 12; the new state (X) into state_out (may be NULL). */
mppi_status mppi_dynamics_step(mppi_dynamics *d, const double *control, double dt, double *state_out);
/* get_state (m_state, X doubles). */
mppi_status mppi_dynamics_get_state(mppi_dynamics *d, double *state);
/* get_end_effector_state (MPPI_EE_N doubles). */
mppi_status mppi_dynamics_end_effector(mppi_dynamics *d, double *ee);
/* The object's other members after its last call: joint position, velocity, acceleration,
 * torque (12 each), tank energy, power, time, arm-mount frame position (3) = 54 doubles. */
#define MPPI_DYNAMICS_QUERY_N 54
mppi_status mppi_dynamics_query(mppi_dynamics *d, double *out);
/* DynamicsForecast::forecast(state, time) (dynamics.cpp:104-138): set_state, then `steps` times
 * record the row and step with Control::Zero() over time_step.  `wrench`: steps x 6 rows of
 * forecast(time + k time_step) (e.g. mppi_forecast_table), copied into the rows; NULL: zeros.
 * out: steps x MPPI_DF_N. */
mppi_status mppi_dynamics_forecast(mppi_dynamics *d, const double *state, double time, double time_step,
                                   int64_t steps, const double *wrench, double *out);
/* Cost::get_cost(state, control, dynamics, time) (mppi.hpp:127-132) of AssistedManipulation
 * (assisted_manipulation.cpp:37-72) or TrackPoint (track_point.cpp:10-34) on the device against the
 * object's cached kinematics.  wrench6: forecast(time) of the dynamics' forecast handle, or NULL
 * when it has none (trajectory_cost is then 0, :239-240).  out: the cost, then the seven
 * AssistedManipulation terms (MPPI_TERM_*; zeros for TrackPoint) = 8 doubles. */
mppi_status mppi_cost_evaluate(const mppi_cost_desc *cost, mppi_dynamics *d, const double *state,
                               const double *control, const double *wrench6, double *out8);
/* The object's link-position model (MPPI_LINK_POSITIONS_*; mppi_cost_evaluate follows it), and
 * get_link_position of every Link after the object's last call: MPPI_LINK_N x 3 doubles, zeros in
 * the zero mode. */
mppi_status mppi_dynamics_set_link_positions(mppi_dynamics *d, int mode);
mppi_status mppi_dynamics_link_positions(mppi_dynamics *d, double *out);
/* The obstacle term of mppi_set_obstacle_avoidance (above) at the object's cached link positions
 * and end-effector position after its last call, at tau = elapsed; stateless in the obstacles
 * (config NULL: the defaults; the set is validated as mppi_set_obstacles validates it).
 * MPPI_ERR_INVALID unless the object is in MPPI_LINK_POSITIONS_KINEMATIC. */
mppi_status mppi_dynamics_obstacle_cost(mppi_dynamics *d, const mppi_obstacle_config *config,
                                        const mppi_obstacle *obstacles, int32_t count, double elapsed, double *cost);
/* The same with capsules (mppi_set_obstacle_capsules above): the robot's segments with `capsules`' radii
 * (NULL: the defaults), capsule obstacles and segment mask bits legal. */
mppi_status mppi_dynamics_capsule_cost(mppi_dynamics *d, const mppi_obstacle_config *config, const mppi_capsule_config *capsules,
                                       const mppi_obstacle *obstacles, int32_t count, double elapsed, double *cost);
/* The distance field's term (mppi_set_distance_field above) of `field` / `values` at the same positions,
 * with `config`'s limit and point radii and `capsules`' segment radii (NULL: the defaults).  Stateless:
 * the grid is uploaded on every call - a diagnostic path. */
mppi_status mppi_dynamics_distance_field_cost(mppi_dynamics *d, const mppi_obstacle_config *config,
                                              const mppi_capsule_config *capsules, const mppi_distance_field *field,
                                              const float *values, double *cost);
/* The held term (mppi_set_held_object_avoidance above) of `object` at the object's cached grasp-frame
 * pose after its last call - its position and its rotation R9 ee_R - against `obstacles` at tau = elapsed
 * (held mask bits legal, the robot's bits ignored) and, with `field` not NULL, against the field, with
 * `config`'s limit (NULL: the defaults).  object NULL or count = 0: 0.  Stateless, the grid uploaded on
 * every call - a diagnostic path.  Works in either link-position mode: the object caches the frame's
 * pose in both. */
mppi_status mppi_dynamics_held_object_cost(mppi_dynamics *d, const mppi_obstacle_config *config, const mppi_obstacle *obstacles,
                                           int32_t count, double elapsed, const mppi_distance_field *field, const float *values,
                                           const mppi_held_object *object, double *cost);
/* The held-self term (mppi_set_held_self_avoidance above) of `object` under `self` at the object's cached
 * link positions and grasp-frame pose after its last call, with `config`'s limit (NULL: the defaults).
 * object NULL or count = 0, or self NULL or with an empty mask: 0.  Needs kinematic link positions
 * (MPPI_ERR_INVALID otherwise, like mppi_dynamics_capsule_cost): the robot's segments come from them. */
mppi_status mppi_dynamics_held_self_cost(mppi_dynamics *d, const mppi_obstacle_config *config, const mppi_held_object *object,
                                         const mppi_held_self *self, double *cost);
/* The target-tracking terms (mppi_set_target_tracking above) at the object's cached grasp-frame pose
 * after its last call: out2[0] = 100 pow(|p_EE - point|, 2), out2[1] = orientation_weight *
 * (3 - sum_ij Rt_ij Ree_ij) for `quaternion` (x, y, z, w; finite, norm in [0.5, 2], normalised here)
 * or 0 with quaternion NULL.  config NULL: the defaults; its track_orientation is not read.  Works
 * in either link-position mode: the object caches the frame's rotation in both. */
mppi_status mppi_dynamics_target_cost(mppi_dynamics *d, const double *point3, const double *quaternion4,
                                      const mppi_target_tracking_config *config, double *out2);
/* add_end_effector_simulated_wrench (6 doubles: force, moment; semantics above): cumulative; the
 * next mppi_dynamics_step applies the sum and zeroes it.  get_end_effector_simulated_wrench: the
 * wrench the last step applied, zeros before any step. */
mppi_status mppi_dynamics_add_end_effector_simulated_wrench(mppi_dynamics *d, const double *wrench6);
mppi_status mppi_dynamics_get_end_effector_simulated_wrench(mppi_dynamics *d, double *out6);
/* Whether mppi_dynamics_forecast adds row k of its `wrench` before step k, as dynamics.cpp:127 does
 * (MPPI_SIMULATED_WRENCH_ON), or only copies the rows into its output (_OFF, the default and the
 * reference's stub).  An explicit add is live in either mode. */
mppi_status mppi_dynamics_set_simulated_wrench(mppi_dynamics *d, int mode);
mppi_status mppi_dynamics_get_simulated_wrench(mppi_dynamics *d, int *mode);
/* The safety filter (mppi_safety_filter_desc, above) on one control at the object's current joint
 * position and velocity with time step dt: out12 is the filtered control.  A wrench added since the
 * last step joins the torque as the step would apply it, and is not consumed. */
mppi_status mppi_dynamics_safety_filter(mppi_dynamics *d, const mppi_safety_filter_desc *filter, const double *control12,
                                        double dt, double *out12);
/* forecast(t0 + k dt) for k < steps of the handle's attached forecast (steps x 6). */
mppi_status mppi_forecast_table(mppi_handle *h, double t0, double dt, int64_t steps, double *out);

#ifdef __cplusplus
}
#endif

#endif /* MPPI_AMD_H */
