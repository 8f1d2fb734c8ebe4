// fr_cost.hip — the rollout costs of the cooperative FrankaRidgeback kernel, from its step records.
//
// fr_coop_kernel writes, for every (rollout, step k), the state x_k and the kinematics of the
// calculate() before it (kernels.hpp FR_REC layout, rollout-major).  This kernel evaluates the
// objective on all of them at once: one wave per rollout, one lane per step, so every lane does distinct work
// (inside the rollout kernel the workspace, trajectory and manipulability terms are row-uniform
// and all 16 lanes of a row would repeat them).  The step costs are then summed in step order,
// J = ((c_0 + c_1) + c_2) + ..., as the reference accumulates them (mppi.cpp:322-337).
//
// NaN: the reference stops a rollout at its first NaN step cost and sets J = NaN; a NaN step cost
// makes this sum NaN as well, and the steps after it do not matter.  The sum is canonicalised to
// the quiet NaN the reference stores.
//
// AssistedManipulation::get_cost (assisted_manipulation.cpp:58-128) and TrackPoint::get_cost
// (frankaridgeback/objective/track_point.cpp:10-34), term order kept.  The joint-limit and
// velocity sums keep the association of the lane sums they replace: (joints 0..5) + (6..11).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_common.hpp"
#include "engine_types.hpp"
#include "kernels.hpp"
#include "fr_cost_terms.hpp"

using namespace mppi_eng;
using mppi_dev::smin;

namespace {

using namespace mppi_cost;

// Lane k loads its step's record straight into registers (21 16-byte loads, 336 B apart across the
// lanes: every byte of the rollout's records is used once, through L2).  Staging through LDS took
// 21.5 KB per wave and held a CU to seven waves, too few to hide the loads; without it the kernel
// is bounded by registers (four waves per SIMD).
// LP: the kinematic link-position model (FrCostArgs::link_positions): the self-collision term from
// each record's link positions (fr_cost_terms.hpp record_self_collision)
// (a kernel of its own, fr_step_cost_lp_kernel, from the same text: the default mode's keep their names and instructions)
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void fr_step_cost_kernel(FrCostArgs a)
{
    constexpr bool LP = false, OB = false;
#include "fr_step_cost_kernel_body.inc"
}
// Two waves per SIMD here: the link positions and the pose are live beside the barrier chains, and
// at four waves (128 VGPRs) this kernel spilled 84-164 of them; 0.223 against 0.300 ms/update at
// 4096 x 64 with MPPI_COSTS_IN_LAUNCH=0 (profiles/link_positions/bench_costkernel_*).
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_lp_kernel(FrCostArgs a)
{
    constexpr bool LP = true, OB = false;
#include "fr_step_cost_kernel_body.inc"
}
// The same with the obstacle term (FrCostArgs::link_positions == FR_LINKS_OBSTACLES)
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_ob_kernel(FrCostArgs a)
{
    constexpr bool LP = true, OB = true;
#include "fr_step_cost_kernel_body.inc"
}

// The same with segments and capsule obstacles (FR_LINKS_CAPSULES: fr_cost_terms.hpp capsule_term)
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_cap_kernel(FrCostArgs a)
{
    constexpr bool LP = true;
    constexpr int OB = OB_TERM_CAPSULES;
#include "fr_step_cost_kernel_body.inc"
}

// The same with the distance field behind the capsule term (FR_LINKS_FIELD: fr_cost_terms.hpp field_term)
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_df_kernel(FrCostArgs a)
{
    constexpr bool LP = true;
    constexpr int OB = OB_TERM_FIELD;
#include "fr_step_cost_kernel_body.inc"
}

// The same with a held object behind the field term (FR_LINKS_HELD: fr_cost_terms.hpp held_term)
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_ho_kernel(FrCostArgs a)
{
    constexpr bool LP = true;
    constexpr int OB = OB_TERM_HELD;
#include "fr_step_cost_kernel_body.inc"
}

// The same with the held object against the robot's own segments behind the held term (FR_LINKS_HELD_SELF:
// fr_cost_terms.hpp held_self_term)
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_hs_kernel(FrCostArgs a)
{
    constexpr bool LP = true;
    constexpr int OB = OB_TERM_HELD_SELF;
#include "fr_step_cost_kernel_body.inc"
}

// An update's obstacle table from the launch's arguments into its place behind the step constants
__global__ __launch_bounds__(64) void obstacle_table_kernel(ObstacleTable t, ObstacleTable *out)
{
    static_assert(sizeof(ObstacleTable) % sizeof(double) == 0, "copied as doubles");
    const double *src = reinterpret_cast<const double *>(&t);
    double *dst = reinterpret_cast<double *>(out);
    for (int i = threadIdx.x; i < (int)(sizeof(ObstacleTable) / sizeof(double)); i += 64) dst[i] = src[i];
}

// The obstacle term of the filter() row summed over its steps in step order, undiscounted, as
// fr_terms_kernel sums the reference's seven (one wave, lane = step)
// CAP: the capsule term (fr_capsule_total_kernel)
template <bool CAP>
__device__ __forceinline__ void obstacle_total(const StepConst *steps, const double *rec, int H, int compact,
                                               const DevModel *model, double dt, double *out1)
{
    const int lane = threadIdx.x;
    const ObstacleTableK T = obstacle_table_of(steps, H);
    double tot = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        const double *r = rec + (int64_t)k * (compact ? FR_REC_C : FR_REC);   // (q, qd) pairs and the EE position: both layouts
        double qj[10], lp[SC_LINKS][3];
        for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
        link_fk(*model, qj, lp);
        double t;
        if constexpr (CAP) t = capsule_term(T, lp, r + REC_EE, dt, k);
        else t = obstacle_term(T, lp, r + REC_EE, dt, k);
        for (int i = 0; i < n; i++) tot += readlane_f64(t, i);
    }
    if (lane == 0) *out1 = tot;
}
__global__ __launch_bounds__(64) void fr_obstacle_total_kernel(const StepConst *steps, const double *rec, int H, int compact,
                                                               const DevModel *model, double dt, double *out1)
{
    obstacle_total<false>(steps, rec, H, compact, model, dt, out1);
}
__global__ __launch_bounds__(64) void fr_capsule_total_kernel(const StepConst *steps, const double *rec, int H, int compact,
                                                              const DevModel *model, double dt, double *out1)
{
    obstacle_total<true>(steps, rec, H, compact, model, dt, out1);
}

// The field term of the filter() row the same way (mppi_optimal_field_cost), from the table - and so
// the grid - of the row's own update
__global__ __launch_bounds__(64) void fr_field_total_kernel(const StepConst *steps, const double *rec, int H, int compact,
                                                            const DevModel *model, double dt, double *out1)
{
    const int lane = threadIdx.x;
    const ObstacleTableK T = obstacle_table_of(steps, H);
    double tot = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        const double *r = rec + (int64_t)k * (compact ? FR_REC_C : FR_REC);
        double qj[10], lp[SC_LINKS][3];
        for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
        link_fk(*model, qj, lp);
        const double t = field_term(T, lp, r + REC_EE);
        for (int i = 0; i < n; i++) tot += readlane_f64(t, i);
    }
    if (lane == 0) *out1 = tot;
}

// The held term of the filter() row the same way (mppi_optimal_held_cost), from the table - and so the
// object and the grid - of the row's own update
__global__ __launch_bounds__(64) void fr_held_total_kernel(const StepConst *steps, const double *rec, int H, int compact,
                                                           const DevModel *model, double dt, double *out1)
{
    const int lane = threadIdx.x;
    const ObstacleTableK T = obstacle_table_of(steps, H);
    double tot = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        const double *r = rec + (int64_t)k * (compact ? FR_REC_C : FR_REC);
        double qj[10], lp[SC_LINKS][3], R9[9];
        for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
        link_fk(*model, qj, lp, R9);
        const double t = held_term(T, r + REC_EE, R9, model->ee_R, dt, k);
        for (int i = 0; i < n; i++) tot += readlane_f64(t, i);
    }
    if (lane == 0) *out1 = tot;
}

// The held-self term of the filter() row the same way (mppi_optimal_held_self_cost), from the table - and
// so the object and the configuration - of the row's own update.  (One wave a launch: the link and held
// coordinates stay in registers through the pair loop, 256 VGPRs; bounded to its twin's three waves a SIMD it
// spills 592 bytes a lane.)
__global__ __launch_bounds__(64) void fr_held_self_total_kernel(const StepConst *steps, const double *rec, int H, int compact,
                                                                const DevModel *model, double dt, double *out1)
{
    const int lane = threadIdx.x;
    const ObstacleTableK T = obstacle_table_of(steps, H);
    double tot = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        const double *r = rec + (int64_t)k * (compact ? FR_REC_C : FR_REC);
        double qj[10], lp[SC_LINKS][3], R9[9], Ree[9];
        for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
        link_fk(*model, qj, lp, R9);
        grasp_rotation(R9, model->ee_R, Ree);
        const double t = held_self_term_at(T, lp, r + REC_EE, Ree);
        for (int i = 0; i < n; i++) tot += readlane_f64(t, i);
    }
    if (lane == 0) *out1 = tot;
}

// The target terms of the filter() row the same way (mppi_optimal_target_cost): the position term
// 100 |p_EE - p(t_k)|^2 and the orientation term, each summed over the steps in step order,
// undiscounted, with the targets of the row's own update (its step constants).  model: the kinematic
// link-position model's, with the orientation switch on; else null and the orientation total is 0.
__global__ __launch_bounds__(64) void fr_target_total_kernel(const DevCost *cost, const StepConst *steps, const double *rec, int H,
                                                             int compact, const DevModel *model, double dt, double *out2)
{
    const int lane = threadIdx.x;
    const DevCost &Cs = *cost;
    double tp = 0.0, to = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        const double *r = rec + (int64_t)k * (compact ? FR_REC_C : FR_REC);   // (q, qd) pairs and the EE position: both layouts
        const StepTarget *tg = reinterpret_cast<const StepTarget *>(steps + k);
        const double *ee = r + REC_EE;
        const bool track = Cs.tp_track != 0;
        const double g0 = track ? tg->p[0] : Cs.tp_point[0], g1 = track ? tg->p[1] : Cs.tp_point[1], g2 = track ? tg->p[2] : Cs.tp_point[2];
        const double d0 = ee[0] - g0, d1 = ee[1] - g1, d2 = ee[2] - g2;
        const double distance = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        const double pt = 100.0 * (distance * distance);
        double ot = 0.0;
        if (model && track && Cs.tp_track_orient) {
            double qj[10], lp[SC_LINKS][3], R9[9], Ree[9];
            for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
            link_fk(*model, qj, lp, R9);
            grasp_rotation(R9, model->ee_R, Ree);
            ot = target_orientation_term(Cs.tp_orient_w, tg->q[0], tg->q[1], tg->q[2], tg->qw, Ree);
        }
        for (int i = 0; i < n; i++) {
            tp += readlane_f64(pt, i);
            to += readlane_f64(ot, i);
        }
    }
    if (lane == 0) {
        out2[0] = tp;
        out2[1] = to;
    }
}

// The optimal rollout's per-term totals (AssistedManipulation's accumulators after filter(),
// mppi.cpp:450-479 with thread 0's cost, reset at its start): one wave over the filter() row's
// records, lane = step, each term summed over the steps in step order (m_*_cost += per step).
// model != null: the kinematic link-position model, the self-collision total from the records' link
// positions.
__global__ __launch_bounds__(64) void fr_terms_kernel(const DevCost *cost, const StepConst *steps, const double *rec, int H,
                                                      int compact, double *out7, const DevModel *model, double dt)
{
    const int lane = threadIdx.x;
    double tot[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        double t[7], r[FR_NREC];
        derive_record(rec + (int64_t)k * (compact ? FR_REC_C : FR_REC), r, compact != 0);
        if (model) {
            double qj[10], lp[SC_LINKS][3];
            for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
            link_fk(*model, qj, lp);
            assisted_manipulation_terms(*cost, steps[k], r, r[REC_QQD + 4], t, lp);
        } else {
            assisted_manipulation_terms(*cost, steps[k], r, r[REC_QQD + 4], t);
        }
#pragma unroll
        for (int m = 0; m < 7; m++)
            for (int i = 0; i < n; i++) tot[m] += readlane_f64(t[m], i);
    }
    if (lane < 7) {
        double v = tot[0];
#pragma unroll
        for (int m = 1; m < 7; m++) v = lane == m ? tot[m] : v;
        out7[lane] = v;
    }
}

}  // namespace

namespace mppi_eng {

hipError_t launch_fr_terms(const DevCost *cost, const StepConst *steps, const double *rec, int H, bool compact, double *out7,
                           hipStream_t s, const DevModel *link_model, double dt)
{
    hipLaunchKernelGGL(fr_terms_kernel, dim3(1), dim3(64), 0, s, cost, steps, rec, H, compact ? 1 : 0, out7, link_model, dt);
    return hipGetLastError();
}

hipError_t launch_obstacle_table(const ObstacleTable &t, ObstacleTable *out, hipStream_t s)
{
    hipLaunchKernelGGL(obstacle_table_kernel, dim3(1), dim3(64), 0, s, t, out);
    return hipGetLastError();
}

hipError_t launch_fr_obstacle_total(const StepConst *steps, const double *rec, int H, bool compact, const DevModel *model,
                                    double dt, double *out1, hipStream_t s, bool capsules)
{
    if (capsules) hipLaunchKernelGGL(fr_capsule_total_kernel, dim3(1), dim3(64), 0, s, steps, rec, H, compact ? 1 : 0, model, dt, out1);
    else hipLaunchKernelGGL(fr_obstacle_total_kernel, dim3(1), dim3(64), 0, s, steps, rec, H, compact ? 1 : 0, model, dt, out1);
    return hipGetLastError();
}

hipError_t launch_fr_target_total(const DevCost *cost, const StepConst *steps, const double *rec, int H, bool compact,
                                  const DevModel *model, double dt, double *out2, hipStream_t s)
{
    hipLaunchKernelGGL(fr_target_total_kernel, dim3(1), dim3(64), 0, s, cost, steps, rec, H, compact ? 1 : 0, model, dt, out2);
    return hipGetLastError();
}

hipError_t launch_fr_field_total(const StepConst *steps, const double *rec, int H, bool compact, const DevModel *model,
                                 double dt, double *out1, hipStream_t s)
{
    hipLaunchKernelGGL(fr_field_total_kernel, dim3(1), dim3(64), 0, s, steps, rec, H, compact ? 1 : 0, model, dt, out1);
    return hipGetLastError();
}

hipError_t launch_fr_held_total(const StepConst *steps, const double *rec, int H, bool compact, const DevModel *model,
                                double dt, double *out1, hipStream_t s)
{
    hipLaunchKernelGGL(fr_held_total_kernel, dim3(1), dim3(64), 0, s, steps, rec, H, compact ? 1 : 0, model, dt, out1);
    return hipGetLastError();
}

hipError_t launch_fr_held_self_total(const StepConst *steps, const double *rec, int H, bool compact, const DevModel *model,
                                     double dt, double *out1, hipStream_t s)
{
    hipLaunchKernelGGL(fr_held_self_total_kernel, dim3(1), dim3(64), 0, s, steps, rec, H, compact ? 1 : 0, model, dt, out1);
    return hipGetLastError();
}

hipError_t launch_fr_step_cost(const FrCostArgs &a, hipStream_t s)
{
    const int64_t rows = a.count + (a.fcost ? 1 : 0);
    if (rows == 0) return hipSuccess;
    const dim3 grid((unsigned)rows), block(64);
    // the records' layout is the launch's that wrote them (FrCostArgs::compact)
    if (a.link_positions == FR_LINKS_HELD_SELF) {
        if (!a.model) return hipErrorInvalidValue;
        if (a.compact) {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_hs_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_hs_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_hs_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
        } else {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_hs_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_hs_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_hs_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
        }
    } else if (a.link_positions == FR_LINKS_HELD) {
        if (!a.model) return hipErrorInvalidValue;
        if (a.compact) {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_ho_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_ho_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_ho_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
        } else {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_ho_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_ho_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_ho_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
        }
    } else if (a.link_positions == FR_LINKS_FIELD) {
        if (!a.model) return hipErrorInvalidValue;
        if (a.compact) {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_df_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_df_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_df_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
        } else {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_df_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_df_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_df_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
        }
    } else if (a.link_positions == FR_LINKS_CAPSULES) {
        if (!a.model) return hipErrorInvalidValue;
        if (a.compact) {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_cap_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_cap_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_cap_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
        } else {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_cap_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_cap_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_cap_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
        }
    } else if (a.link_positions == FR_LINKS_OBSTACLES) {
        if (!a.model) return hipErrorInvalidValue;
        if (a.compact) {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_ob_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_ob_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_ob_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
        } else {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_ob_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_ob_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_ob_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
        }
    } else if (a.link_positions) {
        if (!a.model) return hipErrorInvalidValue;
        if (a.compact) {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_lp_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_lp_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_lp_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
        } else {
            if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_lp_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
            else if (a.energy) hipLaunchKernelGGL((fr_step_cost_lp_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fr_step_cost_lp_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
        }
    } else if (a.compact) {
        if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_kernel<CK_TRACK_POINT, false, true>), grid, block, 0, s, a);
        else if (a.energy) hipLaunchKernelGGL((fr_step_cost_kernel<CK_ASSISTED_MANIPULATION, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((fr_step_cost_kernel<CK_ASSISTED_MANIPULATION, false, true>), grid, block, 0, s, a);
    } else {
        if (a.cost_kind == CK_TRACK_POINT) hipLaunchKernelGGL((fr_step_cost_kernel<CK_TRACK_POINT, false, false>), grid, block, 0, s, a);
        else if (a.energy) hipLaunchKernelGGL((fr_step_cost_kernel<CK_ASSISTED_MANIPULATION, true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((fr_step_cost_kernel<CK_ASSISTED_MANIPULATION, false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace mppi_eng
