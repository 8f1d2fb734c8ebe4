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
// The kinematic link-position model and the obstacle terms behind it are kernels of their own,
// fr_step_cost_links_kernel below, from the same text: the default mode's keep their names and instructions.
template <int CK, bool EN, bool KC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void fr_step_cost_kernel(FrCostArgs a)
{
    constexpr bool LP = false, OB = false;
#include "fr_step_cost_kernel_body.inc"
}
// LP: the kinematic link-position model (FrCostArgs::link_positions != FR_LINKS_ZERO): the self-collision term
// from each record's link positions (fr_cost_terms.hpp record_self_collision), and behind it the obstacle
// term OB = link mode - 1 (fr_cost_terms.hpp obstacle_cost): OB_TERM_NONE (FR_LINKS_KINEMATIC), OB_TERM_POINTS
// (FR_LINKS_OBSTACLES: obstacle_term), OB_TERM_CAPSULES (FR_LINKS_CAPSULES: capsule_term), OB_TERM_FIELD
// (FR_LINKS_FIELD: field_term behind it), OB_TERM_HELD (FR_LINKS_HELD: held_term behind those) or
// OB_TERM_HELD_SELF (FR_LINKS_HELD_SELF: held_self_term behind those).
// Two waves per SIMD here: the link positions and the pose are live beside the barrier chains, and
// at four waves (128 VGPRs) this kernel spilled 84-164 of them; 0.223 against 0.300 ms/update at
// 4096 x 64 with MPPI_COSTS_IN_LAUNCH=0 (profiles/link_positions/bench_costkernel_*).
template <int CK, bool EN, bool KC, int OB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void fr_step_cost_links_kernel(FrCostArgs a)
{
    static_assert(OB >= OB_TERM_NONE && OB <= OB_TERM_HELD_SELF, "no such obstacle term");
    constexpr bool LP = true;
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

// One obstacle term of the filter() row alone, summed over its steps in step order, undiscounted, as
// fr_terms_kernel sums the reference's seven (one wave, lane = step), from the table of the row's own
// update - and so that update's set, grid, held object and held-self configuration.  TERM: OB_TERM_POINTS
// obstacle_term, OB_TERM_CAPSULES capsule_term, OB_TERM_FIELD field_term, OB_TERM_HELD held_term,
// OB_TERM_HELD_SELF held_self_term_at - each term by itself, not the sum up to it.
// (One wave a launch: the held-self term's link and held coordinates stay in registers through the pair
// loop, 256 VGPRs; bounded to its twin's three waves a SIMD it spills 592 bytes a lane.)
template <int TERM>
__global__ __launch_bounds__(64) void fr_term_total_kernel(const StepConst *steps, const double *rec, int H, int compact,
                                                           const DevModel *model, double dt, double *out1)
{
    static_assert(TERM >= OB_TERM_POINTS && TERM <= OB_TERM_HELD_SELF, "no such obstacle term");
    const int lane = threadIdx.x;
    const ObstacleTableK T = obstacle_table_of(steps, H);
    double tot = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        const double *r = rec + (int64_t)k * (compact ? FR_REC_C : FR_REC);   // (q, qd) pairs and the EE position: both layouts
        double qj[10], lp[SC_LINKS][3];
        double R9[TERM >= OB_TERM_HELD ? 9 : 1];   // body 9's rotation with the positions: the held object turns with the grasp
        for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], dt, k == 0);
        if constexpr (TERM >= OB_TERM_HELD) link_fk(*model, qj, lp, R9);
        else link_fk(*model, qj, lp);
        double t;
        if constexpr (TERM == OB_TERM_HELD_SELF) {
            double Ree[9];
            grasp_rotation(R9, model->ee_R, Ree);
            t = held_self_term_at(T, lp, r + REC_EE, Ree);
        } else if constexpr (TERM == OB_TERM_HELD) t = held_term(T, r + REC_EE, R9, model->ee_R, dt, k);
        else if constexpr (TERM == OB_TERM_FIELD) t = field_term(T, lp, r + REC_EE);
        else if constexpr (TERM == OB_TERM_CAPSULES) t = capsule_term(T, lp, r + REC_EE, dt, k);
        else t = obstacle_term(T, lp, r + REC_EE, dt, k);
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

// One link mode's kernel of the launch's objective and record layout (FrCostArgs::cost_kind, energy, compact:
// the layout is the launch's that wrote the records).  LINKS: FR_LINKS_ZERO the default mode's kernel, else the
// links kernel with the obstacle term LINKS - 1 (kernels.hpp).
using StepCostKernel = void (*)(FrCostArgs);
template <int LINKS, int CK, bool EN, bool KC>
constexpr StepCostKernel step_cost_kernel_of()
{
    if constexpr (LINKS == FR_LINKS_ZERO) return fr_step_cost_kernel<CK, EN, KC>;
    else return fr_step_cost_links_kernel<CK, EN, KC, LINKS - 1>;
}
template <int LINKS>
StepCostKernel step_cost_cell(const FrCostArgs &a)
{
    if (a.cost_kind == CK_TRACK_POINT)
        return a.compact ? step_cost_kernel_of<LINKS, CK_TRACK_POINT, false, true>() : step_cost_kernel_of<LINKS, CK_TRACK_POINT, false, false>();
    if (a.energy)
        return a.compact ? step_cost_kernel_of<LINKS, CK_ASSISTED_MANIPULATION, true, true>()
                         : step_cost_kernel_of<LINKS, CK_ASSISTED_MANIPULATION, true, false>();
    return a.compact ? step_cost_kernel_of<LINKS, CK_ASSISTED_MANIPULATION, false, true>()
                     : step_cost_kernel_of<LINKS, CK_ASSISTED_MANIPULATION, false, false>();
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

hipError_t launch_fr_term_total(int term, const StepConst *steps, const double *rec, int H, bool compact, const DevModel *model,
                                double dt, double *out1, hipStream_t s)
{
    using Kernel = void (*)(const StepConst *, const double *, int, int, const DevModel *, double, double *);
    static constexpr Kernel TOTALS[] = {fr_term_total_kernel<OB_TERM_POINTS>, fr_term_total_kernel<OB_TERM_CAPSULES>,
                                        fr_term_total_kernel<OB_TERM_FIELD>, fr_term_total_kernel<OB_TERM_HELD>,
                                        fr_term_total_kernel<OB_TERM_HELD_SELF>};
    static_assert(sizeof(TOTALS) / sizeof(TOTALS[0]) == OB_TERM_HELD_SELF - OB_TERM_POINTS + 1, "one row a term");
    if (term < OB_TERM_POINTS || term > OB_TERM_HELD_SELF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(TOTALS[term - OB_TERM_POINTS], dim3(1), dim3(64), 0, s, steps, rec, H, compact ? 1 : 0, model, dt, out1);
    return hipGetLastError();
}

hipError_t launch_fr_target_total(const DevCost *cost, const StepConst *steps, const double *rec, int H, bool compact,
                                  const DevModel *model, double dt, double *out2, hipStream_t s)
{
    hipLaunchKernelGGL(fr_target_total_kernel, dim3(1), dim3(64), 0, s, cost, steps, rec, H, compact ? 1 : 0, model, dt, out2);
    return hipGetLastError();
}

hipError_t launch_fr_step_cost(const FrCostArgs &a, hipStream_t s)
{
    const int64_t rows = a.count + (a.fcost ? 1 : 0);
    if (rows == 0) return hipSuccess;
    if (a.link_positions && !a.model) return hipErrorInvalidValue;
    StepCostKernel kernel;
    switch (a.link_positions) {
    case FR_LINKS_ZERO: kernel = step_cost_cell<FR_LINKS_ZERO>(a); break;
    case FR_LINKS_OBSTACLES: kernel = step_cost_cell<FR_LINKS_OBSTACLES>(a); break;
    case FR_LINKS_CAPSULES: kernel = step_cost_cell<FR_LINKS_CAPSULES>(a); break;
    case FR_LINKS_FIELD: kernel = step_cost_cell<FR_LINKS_FIELD>(a); break;
    case FR_LINKS_HELD: kernel = step_cost_cell<FR_LINKS_HELD>(a); break;
    case FR_LINKS_HELD_SELF: kernel = step_cost_cell<FR_LINKS_HELD_SELF>(a); break;
    default: kernel = step_cost_cell<FR_LINKS_KINEMATIC>(a); break;   // and any other nonzero mode
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mppi_eng
