// kernels.hpp — launch interface of kernels.hip for the host runtime (engine.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coop_plan.hpp"
#include "engine_types.hpp"
#include "../../include/mppi_amd.h"

namespace mppi_eng {

// Device-side outcome of optimise() (mppi.cpp:344-375) and of the smoothing filter.
struct Status {
    int all_nan;     // <= 1 valid rollout: "all nan rollouts" (mppi.cpp:369-370)
    int early;       // max - min < 1e-6 (or all_nan): weights / gradient / U* untouched
    int sg_error;    // SavitzkyGolay window threw (filter.cpp:37-44, 73-82)
    int handover;    // fr_coop_x_kernel: the step relay stage 1 starts at (relay_stage), or -1 without the relay
    // fr_coop_x_kernel: bounded in-launch waits that gave up in this update's rollout launch (some
    // rows' costs were then never written): the finish kernels fail the update on it and reset it
    int wait_timeouts;
    // fr_coop_x_kernel: objective chunks that a later relay member's stage waves took ahead of their
    // stage (cost_work's `until`), counted since create (mppi_update_info, MPPI_INFO_STAGE_WORK)
    int ahead_chunks;
    int pad[2];
    double minimum, maximum, total;   // total: the softmin normaliser, summed by the finish kernels
    double tsplit[8];           // its GRAD_SPLIT partial sums (weights_gradient_kernel)
};

// min / max / count of the update's non-NaN costs, accumulated with order-independent atomics on
// order-preserving keys (exact, so deterministic) by whoever evaluates the objective (the rollout
// launch or fr_step_cost_kernel), and read by weights_gradient_kernel instead of a pass over all R
// costs in each of its blocks.  CS_SLOTS slots, one 128-byte line each, spread the atomics: on one
// address 4099 x 3 of them cost ~40 us.  Reset by the finish kernels (a launch boundary before the
// next update's folds).
constexpr int CS_SLOTS = 64;
struct CostStats {
    unsigned long long kmin[CS_SLOTS * 16];
    unsigned long long kmax[CS_SLOTS * 16];
    unsigned int count[CS_SLOTS * 32];
};

constexpr int MAX_X = 32;   // state dimension bound of the by-value state (FrankaRidgeback 31)
static_assert(FR_X <= MAX_X, "state dimension");

// sample(): the eps tensor of this update (mppi.cpp:242-269), one thread per (step, local rollout).
struct SampleArgs {
    const int *rank;          // [R] stable-order rank of rollouts 2..R-1
    const double *Uprev;      // [H][C]  U* of the previous update (rollout 1 = -U*)
    const double *inj;        // injected eps stream [draws][C]
    const double *T;          // [C][C] noise transform (row-major)
    const double *prev;       // [H][Rpad][C] eps of the previous update (kept rollouts shift it)
    double *noise;            // [H][Rpad][C] eps of this update
    double *Us;               // [H][C] U*_shifted, written when shift_by > 0
    SampleParams sp;
    int64_t begin, count, Rpad;
    int H, C;
    // the update's state, passed by value (no host-to-device copy on the update path): block
    // (0, 0) writes it to x0_out for the rollout kernels
    double x0v[MAX_X];
    double *x0_out;
    int X;
    double tdv[FR_C];   // diagonal noise transform by value (tdiag launches: no loads of T)
};

// optimise() and the partial gradient in one launch (kernels.hip weights_gradient_kernel)
struct WGradArgs {
    const double *cost;    // [R], global rollout index
    int64_t R;
    double cost_scale;
    Status *status;
    const double *noise;   // [H][Rpad][C]
    int64_t begin, count, Rpad;
    int H, C;
    double *gsplit;        // [GRAD_SPLIT][H][C]
    double *wexp;          // [R] unnormalised weights e_r (weights = e_r / Status::total)
    double *wpart;         // [4 * 64] scratch: per-chunk min / max / count / sum (R > SM_LARGE_R)
    const CostStats *stats;   // min / max / count from the cost kernel (unsharded), or null: a pass
};

struct FinishArgs {
    const Status *status;
    Status *status_w;
    const double *gsplit;       // [ns][H][C] gradient stage-1 partials (ns > 0: summed here)
    int ns;
    const double *gpart;        // [H][C] summed (all-reduced when sharded) gradient, ns == 0
    double *gradient;
    double *Ushift;
    const double *cmin, *cmax;
    double gradient_step;
    int control_bound;
    int H, C;
    double t0, dt;
    // Savitzky-Golay state (window 0 = disabled)
    int sg_window;
    const double *sg_weights;   // [2w+1]
    double *sg_uu, *sg_tt;      // [C][H + 2w + 1]
    int64_t *sg_start;          // [C]
    double *sg_last_trim;       // [C]
    // publish: U* <- U*_shifted and the host-visible block [U (H*C), optimal cost, status]
    double *U;
    const double *opt_cost;
    double *out;                // host block [HC + 8]: U*, then status words, then the sequence flag
    double seq;                 // written to out[HC + 6] last, system-scope release (host polls it)
    // filter()'s state: the update's x0 copied for the optimal rollout that runs after it
    const double *x0;
    double *x0_opt;
    int X;
    // the next rank launch accumulates into rank[]: zeroed here when it is the tiled kernel
    int *rank_zero;
    int64_t rank_n;
    // the cost statistics, consumed by weights_gradient_kernel ahead of this launch: reset here for
    // the next update's folds (stream-ordered before its rollout launch; may be null)
    CostStats *stats_reset;
    // the update's in-launch wait timeouts: every rank's (the all-reduced cost slot R) when sharded
    // over RCCL, else null (Status::wait_timeouts); wait_local: this rank's slot, reset here
    const double *wait_all;
    double *wait_local;
};

// The simulated end-effector wrench's rows of an update: [H][FR_WRENCH_ROW] doubles (six used: force,
// moment), written by launch_wrench_table behind the H StepConst of the same buffer (a row is as
// large as a StepConst), so that whatever reads an update's step constants finds its wrench rows.
constexpr int FR_WRENCH_ROW = 8;
static_assert(FR_WRENCH_ROW * sizeof(double) == sizeof(StepConst), "wrench rows behind the step constants");
// FrRolloutArgs / FrCostArgs::link_positions
constexpr int FR_LINKS_ZERO = 0, FR_LINKS_KINEMATIC = 1, FR_LINKS_OBSTACLES = 2, FR_LINKS_CAPSULES = 3, FR_LINKS_FIELD = 4, FR_LINKS_HELD = 5,
              FR_LINKS_HELD_SELF = 6;
static_assert(OB_TERM_NONE == 0 && FR_LINKS_OBSTACLES - 1 == OB_TERM_POINTS && FR_LINKS_CAPSULES - 1 == OB_TERM_CAPSULES &&
                  FR_LINKS_FIELD - 1 == OB_TERM_FIELD && FR_LINKS_HELD - 1 == OB_TERM_HELD &&
                  FR_LINKS_HELD_SELF - 1 == OB_TERM_HELD_SELF, "a link mode past the kinematic one is its obstacle term + 1");
constexpr int FR_TRACE_EXTRA = 128;   // trace slots past the main waves': the relay and the traced relay hosts' tasks
struct FrRolloutArgs {
    const DevModel *model;
    const DevCost *cost;
    const double *table;      // cooperative kernels: the per-body table (launch_fr_body_table)
    const StepConst *steps;   // [H]
    const double *x0;         // [X]
    const double *Ushift;     // [H][C]  U* shifted to this update
    const double *noise;      // [H][Rpad][C] eps of the local rollouts (sample_kernel)
    double *cost_out;         // [R] (global index) or the optimal-cost scalar
    const Status *status;     // optimal mode: skipped when the update failed (no filter())
    int64_t begin, count, Rpad;
    double dt;
    int H;
    int optimal;
    int cost_kind;            // mppi_cost_kind: AssistedManipulation or TrackPoint
    int energy;               // AssistedManipulation enable_energy_limit: the tank's NLE power
    uint32_t *trace;          // diagnostics (COOP_TRACE builds, MPPI_WAVE_TRACE): per block start, end, hw id, xcc
                              // (four words a slot: one per main wave, then FR_TRACE_EXTRA, fr_coop.hip TR_*)
    // filter() of the previous update folded into this launch as one extra row (fr_coop.hip):
    // its state, published U*, step constants and cost output
    const double *fx0, *fU;
    const StepConst *fsteps;
    double *fcost;
    int64_t xbase, xrows;     // fr_coop_x_kernel: the fifth waves' rows [xbase, xbase + xrows)
    // cooperative kernel: per-step records for the cost kernel, [count][H][FR_REC] (rollout-major:
    // one rollout's records are contiguous), and the folded / standalone filter() row's [H][FR_REC]
    double *rec, *frec;
    // U*_shifted row k is Ushift row min(k + ush, H - 1): ush = 0 with U*_shifted itself, the
    // update's shift with U* (draws made ahead)
    int ush;
    // drawn_ahead: the eps tensor holds this update's draws, made behind the previous update
    // (rank_draw_kernel, the previous launch's tail draws); the launch only copies the kept
    // rollouts' columns into it (samp), and x0 comes from samp.x0v.  Block 0 writes U*_shifted and
    // x0 back for the kernels after it.
    int drawn_ahead;
    SampleArgs samp;
    // costs_in_launch (set by fr_coop_launch_args from the plan): the waves evaluate the objective of
    // the rows after their horizon loops (fr_coop.hip launch_costs) instead of fr_step_cost_kernel;
    // stats as in FrCostArgs
    int costs_in_launch;
    // the kinematic link-position model (mppi_set_link_positions): the launches' objective evaluates
    // the self-collision term on each record's link positions (fr_coop.hip's *_lp_kernel; read by
    // the host's launch selection only).  In the padding behind costs_in_launch: the argument
    // block's size and every other offset stay what the default mode's kernels were built for.
    // FR_LINKS_OBSTACLES: the model with the obstacle term as well (mppi_set_obstacle_avoidance; the
    // *_ob_kernel units), its table behind the step constants and wrench rows (steps + 2 H, fsteps + 2 H).
    // FR_LINKS_CAPSULES: the obstacle term with segments and capsule obstacles (mppi_set_obstacle_capsules;
    // the *_cap_kernel units), the same table with its tail of segment radii.
    // FR_LINKS_FIELD: the capsule term and the distance field's (mppi_set_distance_field_avoidance; the
    // *_df_kernel units), the grid through the same table's second tail.
    // FR_LINKS_HELD: those two and the held object's (mppi_set_held_object_avoidance; the *_ho_kernel
    // units), the object in the same table's third tail.
    // FR_LINKS_HELD_SELF: those three and the held object against the robot's own segments
    // (mppi_set_held_self_avoidance; the *_hs_kernel units), the configuration in the table's fourth tail.
    int link_positions;
    CostStats *stats;
    // the next update's draws for the main waves' own rows, made in the launch's idle tail into
    // this buffer (fr_coop.hip tail_draws; null: none): rank_draw_kernel then draws only the rest
    double *ahead_noise;
    // fr_coop_x_kernel: the rows left over travel through four relay stages (fr_coop.hip
    // relay_stage; MPPI_HANDOVER=0 keeps them on one wave beside main wave 0)
    int handover;
    // the simulated end-effector wrench (mppi_set_simulated_wrench; read by the host's launch
    // selection only): the launches' step adds J_G^T w_k (fr_coop.hip's *_wr_kernel), w_k row k of
    // the wrench table behind the step constants (steps + H, fsteps + H: FR_WRENCH_ROW doubles a
    // row).  In the padding behind handover, like link_positions.
    int simulated_wrench;
    // sharded over RCCL: the rank's slot R of the cost vector the engine all-reduces, to which every
    // in-launch wait that gives up adds 1 (so every rank's finish kernel sees any rank's), or null
    double *wait_sum;
    // MPPI_DEBUG_* fault injection (mppi_debug_inject; 0 in production): bit 0, relay stage 1 of
    // the workgroup with rows left over never signals stage 2 (tests the wait-timeout failure)
    int debug;
    // MPPI_STAGE_WORK (0: off): the waves of a later relay member's stages 1 .. 3 evaluate objective
    // chunks until the stage before their own runs (fr_coop_x_kernel_body.inc).  In the padding
    // behind debug.
    int stage_work;
    // The relay over relay_k workgroups (fr_coop.hip relay_stage): member m of relay group q is
    // workgroup q + RELAY_STRIDE m and runs stages 4 m .. 4 m + 3 over its share of the horizon's
    // chunks; the lanes' state and the rows' partial cost sums cross between members through rx,
    // tagged with this launch's rtoken (nonzero, one per launch).  relay_k = 1: one workgroup.
    struct RelayXfer *rx;
    uint32_t rtoken;
    int relay_k;
};
// One relay group's hand-offs between consecutive members (m -> m + 1, m < RELAY_K_MAX - 1): the
// 64 lanes' (q, qd, E) and the four rows' partial cost sums, each behind a token on a line of its own
struct RelayXfer {
    double state[RELAY_K_MAX - 1][64 * 3];
    double sums[RELAY_K_MAX - 1][16];
    uint32_t state_tok[RELAY_K_MAX - 1][32];
    uint32_t sums_tok[RELAY_K_MAX - 1][32];
};

// What the objective reads at (step k, rollout): the state x_k the cost is evaluated at and the
// kinematics of the calculate() before it - the "derived record", FR_NREC doubles.
constexpr int FR_NREC = 42;   // 41 used, padded to 16 bytes
constexpr int REC_QQD = 0;    // [2j], [2j + 1]: q_j, qd_j (j < 12)
constexpr int REC_EE = 24;    // EE position (world)
constexpr int REC_AM = 27;    // arm-mount position (world)
constexpr int REC_E = 30;     // energy tank level (enable_energy_limit)
constexpr int REC_VL = 32;    // EE linear frame velocity J v (bodies 0..9)
constexpr int REC_JJ = 35;    // J_a J_a^T (arm joints 3..9), packed 00 01 02 11 12 22
// What the cooperative rollout kernel stores per (rollout, step) - the "stored record", FR_REC
// doubles: the derived record's first 32 doubles as they are, then two planes of one 16-byte slot
// per lane of the row instead of J v and J_a J_a^T: (S_j linear x, y) and (S_j linear z, qd_j) of
// the calculate() the kinematics come from (lanes 12..15 and the fingers' slots unused).  The
// objective forms J v = sum_j S_j qd_j and J_a J_a^T from them (fr_cost_terms.hpp kin_sums) with
// the FMA chains the rollout kernel's lanes used to run on every step (r05: 50 instructions off the
// dynamics chain, the objective's waves doing them in the slots it leaves idle).
constexpr int REC_S01 = 32;   // [32 + 2j], [33 + 2j]: S_j linear x, y (j < 10 read)
constexpr int REC_S2Q = 64;   // [64 + 2j], [65 + 2j]: S_j linear z, the calculate()'s qd_j (j < 10 read)
constexpr int FR_REC = 96;    // 768 B: sixteen records are 96 whole 128-byte lines
// The compact stored record (fr_coop_kernel: the one-wave and four-wave launches whose waves evaluate
// their own rows' objective after their loops, and the standalone filter()): the derived record
// itself - the rows form J v and J_a J_a^T on their own chain (lane m < 9 writes sum m at REC_VL + m)
// - plus a sink for the frame positions of the lanes that own neither the EE nor the arm mount.
// 384 B: half the 768-B record's bytes, written and read back (sixteen records are 48 lines).
// fr_coop_x_kernel keeps the 768-B record: its objective waves run the sums beside the loops.
constexpr int REC_SINK_C = 42;   // slots 42..44: the other lanes' frame positions, read by nobody
constexpr int FR_REC_C = 48;

// The rollout costs from the records (fr_cost.hip): one wave per rollout, one lane per step, the
// step costs summed in step order (the reference's J += cost, mppi.cpp:322-337).
struct FrCostArgs {
    int compact;              // the records are FR_REC_C compact ones (fr_coop_kernel), else FR_REC
    const DevCost *cost;
    const StepConst *steps;   // [H]
    const double *rec;        // [count][H][FR_REC]
    int64_t begin, count;
    double *cost_out;         // [R] (global index begin + row) or the optimal-cost scalar
    const Status *status;
    int H;
    int optimal;
    int cost_kind;
    int energy;
    // filter() row of the previous update (row == count): its records, constants and output
    const double *frec;
    const StepConst *fsteps;
    double *fcost;
    CostStats *stats;         // the update's rollout costs (not filter()'s) folded in, or null
    // the kinematic link-position model (mppi_set_link_positions): the self-collision term from the
    // records' link positions, which the objective rebuilds with the model and the rollout's dt
    // (FR_LINKS_OBSTACLES: with the obstacle term from the table at steps + 2 H, fsteps + 2 H)
    int link_positions;
    const DevModel *model;
    double dt;
};

struct PmRolloutArgs {
    const DevPointMass *pm;
    const StepConst *steps;
    const double *x0;
    const double *Ushift;
    const double *noise;      // [H][Rpad][3]
    double *cost_out;
    const Status *status;
    int64_t begin, count, Rpad;
    double dt;
    int H;
    int optimal;
};

// ---- wrench forecast on the device (forecast.hip) --------------------------------------------
constexpr int FC_NONE = -1, FC_LOCF = 0, FC_AVERAGE = 1, FC_KALMAN = 2;   // mppi_forecast_type
constexpr int KMAX = 24;   // Kalman states 6 (order + 1), order <= 3

// Forecast::forecast(t) inputs: LOCF observation / Average mean (value), LOCF validity, Kalman
// interpolation grid and its prediction table [steps + 1][6] in device memory.
struct ForecastArgs {
    int type;
    int steps;
    double value[6];
    double valid_until;
    double last_update, horison, time_step;
    const double *pred;
};

// trajectory_cost's configuration (assisted_manipulation.hpp) for the per-step constants
struct StepParams {
    int assisted_manipulation;
    int has_forecast;
    double target_scale, target_maximum, position_threshold;
    double pos_c, pos_l, pos_q;
    double vel_dropoff, vel_minimum, vel_maximum;
};

// KalmanFilter state (kalman.hpp) of the forecast's filter, row-major KMAX x KMAX
struct DevKalman {
    double F[KMAX * KMAX], P[KMAX * KMAX];
    double x[KMAX], xn[KMAX], meas[KMAX];
};

struct KalmanObserve {
    int n, order, steps;
    int64_t pending;   // update(time) calls since the last observation
    double dt;         // time - m_last_update
    double m[6];
};

hipError_t launch_forecast_steps(const ForecastArgs &f, const StepParams &p, const double *gamma, int H, double t0, double dt,
                                 StepConst *out, hipStream_t s);
hipError_t launch_kalman_observe(DevKalman *kf, double *pred, const KalmanObserve &a, hipStream_t s);
hipError_t launch_forecast_eval(const ForecastArgs &f, double time, double *out, hipStream_t s);

// stable rank of rollouts 2..S+1 by cost: one all-pairs tiled launch up to RANK_TILED_MAX (rank[]
// must be zero: finish_kernel clears it), chunk sort + merge beyond
constexpr int64_t RANK_TILED_MAX = 8192;
hipError_t launch_rank(const double *cost, int64_t S, int *rank, uint64_t *sorted, hipStream_t s);
inline int64_t rank_scratch(int64_t S) { return ((S + 255) / 256) * 256; }
hipError_t launch_sample(const SampleArgs &a, bool tdiag, hipStream_t s);
// The next update's draws before its state, time and stable order exist (FrankaRidgeback, diagonal
// transform, device Philox): rollout 0 zero, rollout 1 = -U*, the rest Philox by (rollout, step);
// with the stable rank of this update's costs (one launch when S <= RANK_TILED_MAX; rank[] cleared)
// sub_nxb > 0: the rollout launch's tail drew the rest, so only the rows it left are drawn - the
// first wave's rows of its first sub_nxb workgroups (sub_row0 + 16 b + i, i < 4: sub_row0 is the
// first row of the launch that carries the rows left over) and [sub_xbase, count).
// The rank_draw_kernel launch's arguments (the hipGraph path updates its node with them).
struct RankDrawLaunch {
    const double *cost;
    int64_t S;
    int *rank;
    unsigned nr, nx;
    SampleArgs a;
    int sub_nxb;
    int64_t sub_xbase, sub_row0;
    unsigned grid;
};
// dry: fill *out and launch nothing (past RANK_TILED_MAX the rank launches ahead of it are left out too)
hipError_t launch_draw_ahead(const SampleArgs &a, const double *cost, int64_t S, int *rank, uint64_t *sorted,
                             hipStream_t s, int sub_nxb = 0, int64_t sub_xbase = 0, int64_t sub_row0 = 0,
                             RankDrawLaunch *out = nullptr, bool dry = false);
hipError_t launch_pm_rollout(const PmRolloutArgs &a, hipStream_t s);
constexpr int GRAD_SPLIT = 8;   // rollout ranges per step in the gradient's first stage
static_assert(GRAD_SPLIT == sizeof(Status::tsplit) / sizeof(double), "normaliser partials");

// sum_splits (sharded): the GRAD_SPLIT partials are summed into gpart for the all-reduce
hipError_t launch_weights_gradient(const WGradArgs &a, double *gpart, bool sum_splits, hipStream_t s);
hipError_t launch_fr_coop(const FrRolloutArgs &a, hipStream_t s);
// whether launch_fr_coop writes compact records (FR_REC_C): every launch but the standalone filter()
// row's (a.optimal), which keeps the 768-B record and the shorter step of a latency-bound row
bool fr_coop_compact(const FrRolloutArgs &a);
// The update's rollouts (fr_coop.hip) as coop_plan (coop_plan.hpp) shaped them: one launch, or the
// split's two.  e0 / e1 = optional timing events around the launches.
hipError_t launch_fr_coop_update(const FrRolloutArgs &a, const CoopPlan &p, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// The arguments launch i of the plan takes (the hipGraph path updates its rollout nodes with them)
FrRolloutArgs fr_coop_launch_args(const FrRolloutArgs &a, const CoopPlan &p, int i);
bool fr_coop_costs_in_launch(const EnvSwitches &env);   // the objective runs in the update launch (MPPI_COSTS_IN_LAUNCH != 0)
EnvSwitches env_switches_read();
constexpr int FR_BODY_TABLE = 13 * 46;   // doubles of the cooperative kernels' body table (>= LDS_MODEL)
hipError_t launch_fr_body_table(const DevModel *model, const DevCost *cost, double *table, hipStream_t s);
hipError_t launch_finish(const FinishArgs &a, hipStream_t s);
// The kernel launch_finish takes for these arguments (MPPI_FINISH_*: MPPI_INFO_FINISH_PATH reports it)
int finish_path(const FinishArgs &a);
// The kernel nodes of a captured update graph (engine.cpp update_graph) by their kernel function:
// the ones whose arguments change per update (the rollout launches, the weight reduce, the finish,
// the rank + next draws) and the rest (RCCL's, the gradient sum, the O(S log S) rank), which replay
// with their captured arguments
enum GraphKernel : int { GK_OTHER = 0, GK_ROLLOUT = 1, GK_WGRAD = 2, GK_FINISH = 3, GK_RANKDRAW = 4 };
int graph_kernel_kind(const void *func);          // kernels.hip's kernels
bool fr_coop_is_update_kernel(const void *func);  // fr_coop.hip: an fr_coop_x_kernel instantiation

// FrankaRidgeback::PinocchioDynamics as one device-resident object (fr_object.hip): the members of
// pinocchio_dynamics.hpp:380-425 the methods read and write.
struct DevPinocchio {
    double q[FR_NB], v[FR_NB], tau[FR_NB], a[FR_NB];   // m_joint_position / velocity / torque / acceleration
    double energy, power, time, pad0;                  // EnergyTank, m_power, m_time
    double state[MAX_X];                               // m_state (X = 31 used)
    double ee[MPPI_EE_N];                              // m_end_effector_state (mppi_amd.h MPPI_EE_*)
    double am[3], pad1;                                // the arm-mount frame position (the cost's workspace term)
    double link[FR_LINKS][3];                          // oMi translations of the last calculate(), by Link (row 0: the universe)
};
enum ObjOp : int { OBJ_SET_STATE = 0, OBJ_STEP = 1, OBJ_FORECAST = 2, OBJ_COST = 3 };
struct ObjArgs {
    int op;
    DevPinocchio *obj;
    const DevModel *model;
    double x[MAX_X];      // set_state / forecast / cost: the state
    double u[FR_C];       // step: the control
    double time, dt;
    int64_t steps;        // forecast
    const double *wrench; // forecast: [steps][6] forecast(t_k), or null (zeros)
    double *out;          // forecast: [steps][MPPI_DF_N]; cost: [8] total + terms
    DevCost cost;         // cost: the objective
    StepConst sc;         // cost: trajectory_cost's constants of the wrench at `time`
    int link_positions;   // cost: the self-collision term on the object's cached link positions (kinematic model)
    // step / forecast: the simulated end-effector wrench (force, moment at the grasp frame's origin,
    // world axes) summed by add_end_effector_simulated_wrench since the last step; has_wrench = 0
    // runs the step without the term.  forecast with wrench_rows: row k of `wrench` is added before step k
    double w[6];
    int has_wrench, wrench_rows;
};
hipError_t launch_fr_object(const ObjArgs &a, hipStream_t s);

// The trajectory safety filter (fr_safety.hip; mppi_set_safety_filter, mppi_dynamics_safety_filter):
// per-joint limits and the three switches of mppi_safety_filter_desc (limit_reach is refused by the host).
struct SafetyLimits {
    double position_minimum[FR_NB], position_maximum[FR_NB];
    double velocity_minimum[FR_NB], velocity_maximum[FR_NB];
    double acceleration_minimum[FR_NB], acceleration_maximum[FR_NB];
    int limit_joints, limit_velocity, limit_acceleration, pad;
};
constexpr int SAFETY_MAX_H = 384;   // the plan, its wrench rows and the step's scratch share 64 KiB of LDS
struct SafetyArgs {
    SafetyLimits lim;
    const DevModel *model;
    const double *x0;       // the update's state
    const double *stage;    // [H C + 8] the finish kernel's block: the unfiltered plan, its status words
    const double *wrench;   // [H][FR_WRENCH_ROW] the update's simulated-wrench rows, or null
    double *U;              // [H][C] the plan on the device, rewritten
    double *out;            // the mapped host block [H C + 16]: the filtered plan, the forwarded status
                            // words, [H C + 8] the steps the filter changed, [H C + 6] the flag, last
    double seq, dt;
    int H;
};
struct SafetyColumn {
    double u[FR_C], w[6], dt;
    int has_wrench, pad;
};
size_t fr_safety_lds_bytes(int H);
hipError_t launch_fr_safety_filter(const SafetyArgs &a, hipStream_t s);
hipError_t launch_fr_safety_column(const DevPinocchio *obj, const DevModel *model, const SafetyLimits &lim, const SafetyColumn &c,
                                   double *out12, hipStream_t s);
// The update's simulated-wrench rows, out[H][FR_WRENCH_ROW]: source WT_CONST the wrench w in every row,
// WT_TABLE row k of table[H][6], WT_FORECAST forecast(t0 + k dt) as the step constants sample it
enum WrenchSource : int { WT_CONST = 0, WT_TABLE = 1, WT_FORECAST = 2 };
struct WrenchTableArgs {
    ForecastArgs f;
    int source, H;
    double w[6];
    const double *table;
    double t0, dt;
    double *out;
};
hipError_t launch_wrench_table(const WrenchTableArgs &a, hipStream_t s);
// forecast(t0 + k dt) for k < steps into out[steps][6] (mppi_forecast_table)
hipError_t launch_forecast_table(const ForecastArgs &f, double t0, double dt, int64_t steps, double *out, hipStream_t s);
hipError_t launch_fr_step_cost(const FrCostArgs &a, hipStream_t s);

// One launch per point-mass update (pm_fused.hip): sample, rollouts, optimise, finish, publish,
// filter() and the next update's rank and draws, with one grid barrier.  Device Philox noise with a
// diagonal transform, unsharded, no smoothing.
constexpr int PM_FUSED_THREADS = 256;
constexpr int64_t PM_FUSED_MAX_R = 4096;
constexpr int PM_FUSED_MAX_BLOCKS = 256;          // one per CU: the grid barrier needs them co-resident
// rollouts per block: the fewest of 16, 32, 64 whose grid (at most 256 blocks) and LDS (the
// finisher stages every block's partials) fit, so that the rank and the draws spread over the most
// CUs; 0 when none does
// (every block must be resident at once for the in-launch grid barrier: the handle's device's CUs
// and LDS per block (EnvSwitches::cus, lds_max), and a shape that does not fit takes the five launches)
int pm_fused_rows(int64_t R, int H, unsigned cus, int lds_max);
struct PmFusedArgs {
    DevPointMass pm;
    const StepConst *steps;     // [H] gamma_k
    SampleParams sp;
    double tdv[3];              // diagonal noise transform
    double x0v[8];              // the update's state by value (X = 6)
    double *x0_out;             // [X] the rollout state (block 0)
    int X;
    int H;
    int64_t R, Rpad;
    double dt;
    int *rank;                  // [R] stable order of the previous costs; rewritten for the next update
    const double *prev;         // [H][Rpad][3] the previous update's eps
    double *noise;              // [H][Rpad][3] this update's eps (draws made ahead when `ahead`)
    double *ahead_noise;        // [H][Rpad][3] the next update's draws, or null
    int ahead;
    double *cost;               // [R]
    double *wexp;               // [R] unnormalised weights e_r
    CostStats *stats;
    Status *status;
    double *gpart;              // [nblocks][H C] partial gradients
    double *tpart;              // [nblocks] partial normalisers
    unsigned *bar, *ticket;     // monotonic arrival counters (targets epoch * nblocks)
    unsigned epoch, nblocks;
    double cost_scale, gradient_step;
    int control_bound;
    const double *cmin, *cmax;
    double *U, *Us, *gradient;  // [H][3]
    double *out;                // the mapped host block [H C + 8]
    double seq;                 // its sequence flag value
    double *opt_cost;           // filter()'s cost of the published U*
    double *x0_opt;             // the update's state, for its filter()
    int fold_filter;            // the previous update's filter() is pending: run it in this launch
    const double *fx0;          // its state (x0_opt as the previous launch left it)
    uint64_t *stamps;           // diagnostics (MPPI_PM_STAMPS=1): [nblocks][PM_STAMPS] s_memrealtime, or null
};
// entry, sampled, rolled out (costs folded into the statistics), barrier passed, partials stored,
// ticket taken, staged, (finisher:) stored, published, ranked, end, costs computed
constexpr int PM_STAMPS = 12;
hipError_t launch_pm_update(const PmFusedArgs &a, hipStream_t s);
// AssistedManipulation's seven per-term totals of one rollout from its [H][FR_REC] records
// link_model: the kinematic link-position model's (else null: the zero stub's constant), dt the rollouts'
hipError_t launch_fr_terms(const DevCost *cost, const StepConst *steps, const double *rec, int H, bool compact, double *out7,
                           hipStream_t s, const DevModel *link_model = nullptr, double dt = 0.0);
// An update's obstacle table, by value into out (behind the update's step constants, engine_types.hpp)
hipError_t launch_obstacle_table(const ObstacleTable &t, ObstacleTable *out, hipStream_t s);
// One obstacle term alone (term: OB_TERM_POINTS .. OB_TERM_HELD_SELF, engine_types.hpp; any other:
// hipErrorInvalidValue), two ways.  launch_fr_term_total (fr_term_total_kernel): the term of one rollout's H
// records summed over its steps in step order, undiscounted (next to launch_fr_terms' seven totals), from the
// table behind `steps`.  launch_fr_object_term (fr_object_term_kernel, the mppi_dynamics_*_cost functions): the
// term at the object's cached link positions and grasp-frame pose, tau = t.t0 - t.t_ref.
hipError_t launch_fr_term_total(int term, const StepConst *steps, const double *rec, int H, bool compact, const DevModel *model,
                                double dt, double *out1, hipStream_t s);
hipError_t launch_fr_object_term(int term, const DevPinocchio *obj, const ObstacleTable &t, double *out1, hipStream_t s);

// Target tracking (mppi_set_target_tracking, mppi_set_target_path): the timed pose path as the host
// stored it - quaternions normalised and sign-fixed, inv[i] = 1 / (time[i + 1] - time[i]) - and the
// update's t0 and dt, all by value.  launch_target_table samples it at t0 + k dt for k < H into the
// target fields of out[k] (engine_types.hpp StepTarget; gamma_k is left alone): the ends are held,
// position and quaternion are interpolated linearly, the quaternion renormalised.  n = 0: `point`
// in every step and no orientation; has_q = 0: positions only (the zero quaternion).
struct TargetPathArgs {
    int n, has_q, H, pad;
    double t0, dt;
    double point[3];
    double time[TARGET_WAYPOINTS_MAX], inv[TARGET_WAYPOINTS_MAX];
    double p[TARGET_WAYPOINTS_MAX][3], q[TARGET_WAYPOINTS_MAX][4];
    StepConst *out;
};
hipError_t launch_target_table(const TargetPathArgs &a, hipStream_t s);
// The position and orientation terms of one rollout's H records, each summed over its steps in step
// order, undiscounted (mppi_optimal_target_cost), with the targets in `steps`; model: the kinematic
// link-position model's (null: no orientation term, out2[1] = 0)
hipError_t launch_fr_target_total(const DevCost *cost, const StepConst *steps, const double *rec, int H, bool compact,
                                  const DevModel *model, double dt, double *out2, hipStream_t s);
// mppi_dynamics_target_cost: 100 |p_EE - point|^2 and, with has_q, w (3 - sum_ij Rt_ij Ree_ij) at the
// object's cached grasp-frame pose; q is a unit quaternion (x, y, z, w)
struct ObjTarget {
    double point[3], q[4], w;
    int has_q, pad;
};
hipError_t launch_fr_object_target(const DevPinocchio *obj, const ObjTarget &t, double *out2, hipStream_t s);


}  // namespace mppi_eng
