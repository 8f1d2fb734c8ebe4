// engine_types.hpp — POD blocks shared by the host runtime and the kernels.
//
// The FrankaRidgeback kernel is specialised for the reference robot's kinematic *topology*
// (parents, joint kinds — frankaridgeback/dof.hpp and robot.urdf); every
// numeric model parameter (placements, masses, inertias, frames) is runtime data uploaded from
// the mppi_frankaridgeback_desc.  mppi_create checks the descriptor against the topology.
#pragma once

#include <stdint.h>

namespace mppi_eng {

// ---- FrankaRidgeback topology --------------------------------------------------------------
constexpr int FR_NB = 12;
constexpr int FR_C = 12;
constexpr int FR_X = 31;
enum JointKind : int { KIND_PX = 0, KIND_PY = 1, KIND_RZ = 2, KIND_PNY = 3 };   // PNY: axis (0,-1,0)
constexpr int FR_PARENT[FR_NB] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9};
constexpr int FR_KIND[FR_NB] = {KIND_PX, KIND_PY, KIND_RZ, KIND_RZ, KIND_RZ, KIND_RZ, KIND_RZ,
                                KIND_RZ, KIND_RZ, KIND_RZ, KIND_PY, KIND_PNY};
constexpr int FR_EE_PARENT = 9;   // panda_grasp_joint is on panda_joint7's body
constexpr int FR_AM_PARENT = 2;   // arm_mount_joint is on pivot_joint's body
constexpr int FR_ARM0 = 3, FR_ARM1 = 10;   // arm joints [3, 10): Jacobian columns of the cost

struct DevBody {
    double R[9];     // placement rotation (row-major) in the parent joint frame
    double p[3];
    double mass;
    double c[3];     // com in the joint frame
    double Ic[6];    // xx, xy, yy, xz, yz, zz about the com
};

struct DevModel {
    DevBody b[FR_NB];
    double ee_R[9], ee_p[3];
    double am_R[9], am_p[3];
    // placement of body 11 relative to body 10's placement, (R10^T R11, R10^T (p11 - p10)): the
    // cooperative kernel's prefix scan reaches finger 11 through finger 10 (fr_coop.hip)
    double f11_R[9], f11_p[3];
    double gravity[3];   // Pinocchio's model.gravity: the NLE of the energy tank's power
};

struct DevBarrier {
    double bound, scale, max;
};

// AssistedManipulation parameters in device form.  Per-step forecast-derived constants live in
// StepConst; the self-collision term is a per-step constant for PinocchioDynamics (link
// positions are the zero stub, pinocchio_dynamics.hpp:189-192) and is folded on the host, unless
// the handle runs the kinematic link-position model (sc_limit, sc_radii below).
struct DevCost {
    int en_joint, en_self, en_work, en_energy, en_vel, en_traj, en_manip, pad0;
    DevBarrier lower[FR_NB], upper[FR_NB];
    double self_collision;   // sum over the 20 pairs, evaluated on the host in fp64
    DevBarrier ws_above, ws_infront, ws_reach;
    double yaw_c, yaw_l, yaw_q;
    double vel_q[FR_NB];
    double manip_c, manip_l, manip_q;
    double traj_vel_c, traj_vel_l, traj_vel_q;
    // TrackPoint (frankaridgeback/objective/track_point.cpp) when kind == MPPI_COST_TRACK_POINT
    int kind, tp_en_joint, tp_en_self, tp_en_reach;
    double tp_point[3];
    double tp_lo[FR_NB], tp_up[FR_NB];   // joint_limit_cost's hard-coded limits (joints 0..9 read)
    double tp_self;                      // self_collision_cost with get_link_position == 0
    DevBarrier tp_reach;                 // maximum_reach_limit (right)
    // energy_cost (assisted_manipulation.cpp:211-222): Left / Right barriers of the tank energy
    DevBarrier en_below, en_above;
    // self_collision_cost on real link positions (the kinematic link-position model,
    // mppi_set_link_positions): the active objective's self_collision_limit and the radii of the
    // sphere links PIVOT, PANDA_LINK1..7 (radii[link - 3]).  Unread in the zero mode.
    DevBarrier sc_limit;
    double sc_radii[8];
    // Target tracking (mppi_set_target_tracking, TrackPoint only; zeros otherwise): the step's target is
    // read from its step constants (StepTarget) instead of tp_point, and with tp_track_orient the
    // orientation term tp_orient_w (3 - sum_ij Rt_ij Ree_ij) follows the position term.  Behind
    // everything the other kernels read: their offsets stay what they were.
    int tp_track, tp_track_orient;
    double tp_orient_w;
};

// FrankaRidgeback::Link (frankaridgeback/dynamics.hpp:65-80): the universe, then bodies 0..11.  The
// links self_collision_cost places a sphere on are SC_LINK0 .. SC_LINK0 + SC_LINKS - 1, bodies 2..9.
constexpr int FR_LINKS = 13;
constexpr int SC_LINK0 = 3, SC_LINKS = 8, SC_PAIRS = 20;

// trajectory_cost() constants of step k (assisted_manipulation.cpp:237-290): everything that
// depends only on the forecast wrench at t0 + k dt.
struct StepConst {
    double target[3];
    double tt;          // target . target
    double pos_cost;    // trajectory_position_cost(distance)
    double vtarget;     // clamp(exp(dropoff * distance) - 1, vmin, vmax)
    double gamma_k;     // pow(cost_discount_factor, k)
    int active;         // has forecast && distance > threshold
    int pad;
};

// A tracking TrackPoint handle's view of a StepConst (mppi_set_target_tracking): the step's target
// position and orientation (a unit quaternion x, y, z, w; all four 0: no orientation target) in the
// trajectory-term fields, which TrackPoint kernels do not read; gamma_k stays where it is.  Written
// per update by launch_target_table into the update's own step buffer.
struct StepTarget {
    double p[3];
    double q[3];
    double gamma_k;
    double qw;
};
static_assert(sizeof(StepTarget) == sizeof(StepConst), "a StepConst seen as a target");
static_assert(__builtin_offsetof(StepTarget, gamma_k) == __builtin_offsetof(StepConst, gamma_k), "gamma_k stays in place");
constexpr int TARGET_WAYPOINTS_MAX = 32;

// The obstacle set of one update (mppi_set_obstacle_avoidance, mppi_set_obstacles): the avoidance
// configuration, the update's time t0 and the set's reference time, and up to OB_MAX obstacles.
// Each update writes its own behind its step constants and wrench rows (steps + 2 H:
// launch_obstacle_table), so the filter() row reads the set and the time of the update it belongs
// to and a replayed graph needs no node for it.  OB_POINTS: the eight sphere links, then the end effector.
constexpr int OB_MAX = 16, OB_POINTS = 9;
constexpr int OB_SPHERE = 0, OB_HALF_SPACE = 1, OB_CAPSULE = 2;
// Capsules (mppi_set_obstacle_capsules): robot segment s joins points s and s + 1, mask bit
// OB_SEGMENT_BIT0 + s; its radius is in the table's tail, behind everything the point kernels read.
constexpr int OB_SEGMENTS = 8, OB_SEGMENT_BIT0 = 16;
// what the objective's obstacle term tests: nothing, the nine points, or points and segments
constexpr int OB_TERM_NONE = 0, OB_TERM_POINTS = 1, OB_TERM_CAPSULES = 2;
// ... or points and segments and, behind them, a signed-distance grid (mppi_set_distance_field_avoidance)
constexpr int OB_TERM_FIELD = 3;
// The distance field of one update: the grid (fp32, (nx, ny, nz) C order, z fastest; null: no field),
// its frame and what is sampled - the points of mask bits 0..8, and on the segments of bits 16..23
// `samples` interior points at the fractions phi[j] = (j + 1) / (samples + 1), made on the host.
constexpr int OB_FIELD_SAMPLES = 8;
struct DevField {
    const float *grid;
    int dims[3];
    unsigned mask;
    double origin[3];
    double inv_voxel;
    int samples, pad;
    double phi[OB_FIELD_SAMPLES];
};
// ... and, behind those, a held object (mppi_set_held_object_avoidance)
constexpr int OB_TERM_HELD = 4;
// The held object of one update: `count` spheres fixed in the grasp frame (centres in metres, radii)
// and the segments between consecutive ones; count 0: nothing is held.  Held point i is mask bit
// OB_HELD_POINT_BIT0 + i, held segment s bit OB_HELD_SEGMENT_BIT0 + s, in the obstacles' masks and the field's.
constexpr int OB_HELD_POINTS = 4, OB_HELD_SEGMENTS = 3, OB_HELD_POINT_BIT0 = 9, OB_HELD_SEGMENT_BIT0 = 24;
struct DevHeld {
    int count, pad;
    double centres[OB_HELD_POINTS][3];
    double radii[OB_HELD_POINTS];
    double seg_radii[OB_HELD_SEGMENTS];
};
// ... and, behind that, the held object against the robot's own segments (mppi_set_held_self_avoidance)
constexpr int OB_TERM_HELD_SELF = 5;
// The held-self configuration of one update: `units` bit i (i < 4) held point i, bit 4 + s held segment s;
// `segments` bit s robot segment s (points s and s + 1) with radii[s], this term's own; both 0: nothing is tested.
constexpr unsigned OB_HELD_SELF_UNITS = 0x7Fu, OB_HELD_SELF_SEGMENTS = 0xFFu;
struct DevHeldSelf {
    unsigned units, segments;
    double radii[OB_SEGMENTS];
};
struct DevObstacle {
    double position[3], velocity[3], normal[3], radius;
    int kind;
    unsigned mask;
};
struct ObstacleTable {
    DevBarrier limit;
    double radii[OB_POINTS];
    double t0, t_ref;
    int count, pad;
    DevObstacle ob[OB_MAX];
    double seg_radii[OB_SEGMENTS];   // capsule handles only (zeros otherwise)
    DevField field;                  // field handles only (zeros otherwise): behind everything the other kernels read
    DevHeld held;                    // held handles only (zeros otherwise): behind the field, so every older offset stays
    DevHeldSelf self;                // held-self handles only (zeros otherwise): behind the held object, likewise
};
// the table's room behind the 2 H step-constant slots, in StepConst units
constexpr int OB_TABLE_STEPS = (int)((sizeof(ObstacleTable) + sizeof(StepConst) - 1) / sizeof(StepConst));

// Quadratic point-mass plugin.
struct DevPointMass {
    double inv_mass;
    double target[3], q[3], r[3];
};

// Per-update sampling parameters (Trajectory::sample, mppi.cpp:189-270).
struct SampleParams {
    int64_t shift_by;     // steps shifted this update (<= 0: no shift)
    int64_t shifted;      // columns kept from the previous noise: H - min(shift_by, H)
    int64_t keep;         // number of kept rollouts K
    int64_t keep_draws;   // draws consumed by kept rollouts' tails: K * min(shift_by, H) or 0
    uint64_t update_index;
    uint64_t seed;
    int injected;         // 1: eps from the injected stream, 0: Philox
    int tdiag;            // 1: noise transform is diagonal
};

}  // namespace mppi_eng
