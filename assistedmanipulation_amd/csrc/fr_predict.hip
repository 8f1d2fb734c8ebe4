// fr_predict.hip — predicted trajectories (mppi_predicted_optimal / mppi_predicted_rollouts) from the
// step records the rollout launches leave in HBM (kernels.hpp FR_REC / FR_REC_C): for every
// requested rollout and step k the state x_k the record holds (q, qd, the tank level) and forward
// kinematics at q_k itself - the records' own kinematics are the calculate() before x_k, one step
// behind - as one row of MPPI_PRED_N doubles.
//
// One wave per requested rollout, the lanes over the steps in chunks of 64.  A lane loads its
// record's (q_j, qd_j) pairs and E as 16-byte loads (both record strides are multiples of 16 B),
// runs the chain of fr_predict.hpp on the model in HBM and stores its row.
//
// NaN rule: from the first step whose q, qd (or E, with the tank integrated) is not finite, that row
// and every later row of the rollout is NaN in every column: a 64-bit ballot per chunk, the first
// bad step carried from chunk to chunk.  What a launch stored behind a rollout that went NaN (the
// Euler step of a NaN, or an inf that came back finite) so never shows.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "engine_types.hpp"
#include "kernels.hpp"
#include "predict_plan.hpp"
#include "fr_predict.hpp"
#include "fr_cost_terms.hpp"

using namespace mppi_eng;

static_assert(PRED_REC == FR_REC && PRED_REC_C == FR_REC_C, "predict_plan.hpp's record sizes");
static_assert(REC_QQD == 0 && REC_E % 2 == 0 && FR_REC % 2 == 0 && FR_REC_C % 2 == 0, "16-byte loads of the (q, qd) pairs and E");
static_assert(REC_E + 2 <= FR_REC_C, "q, qd and E sit at the same slots of both records");
static_assert(MPPI_PRED_QD == MPPI_PRED_Q + FR_NB && MPPI_PRED_ENERGY == MPPI_PRED_QD + FR_NB && MPPI_PRED_EE == MPPI_PRED_ENERGY + 1 &&
                  MPPI_PRED_ARM_MOUNT == MPPI_PRED_EE + 3 && MPPI_PRED_LINKS == MPPI_PRED_ARM_MOUNT + 3 &&
                  MPPI_PRED_N == MPPI_PRED_LINKS + 3 * FR_LINKS && MPPI_LINK_N == FR_LINKS,
              "row layout");

namespace {

__device__ __forceinline__ bool finite64(double x) { return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000; }

__global__ __launch_bounds__(64) void fr_predict_kernel(const DevModel *model, const double *rec, const PredictRow *rows, int H,
                                                        int energy, double *out)
{
    const int lane = threadIdx.x;
    const PredictRow row = rows[blockIdx.x];
    const int RS = row.compact ? FR_REC_C : FR_REC;
    const double *rp = rec + row.offset;
    double *op = out + (int64_t)blockIdx.x * H * MPPI_PRED_N;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int first_bad = 0x7fffffff;   // the rollout's first step with a non-finite state (wave-uniform)
    for (int base = 0; base < H; base += 64) {
        const int k = base + lane;
        const bool act = k < H;
        // the lanes past the horizon read its last record (in bounds) and store nothing
        const double2 *r2 = reinterpret_cast<const double2 *>(rp + (int64_t)(act ? k : H - 1) * RS);
        double q[FR_NB], qd[FR_NB];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < FR_NB; j++) {
            const double2 v = r2[REC_QQD / 2 + j];
            q[j] = v.x;
            qd[j] = v.y;
            ok = ok && finite64(v.x) && finite64(v.y);
        }
        double E = nan;
        if (energy) {
            E = r2[REC_E / 2].x;
            ok = ok && finite64(E);
        }
        const unsigned long long bad = __ballot(act && !ok);
        if (first_bad == 0x7fffffff && bad) first_bad = base + __ffsll(bad) - 1;
        if (!act) continue;   // (after the chunk's last wave-wide operation)
        const bool dead = k >= first_bad;
        double *o = op + (int64_t)k * MPPI_PRED_N;
#pragma unroll
        for (int j = 0; j < FR_NB; j++) {
            o[MPPI_PRED_Q + j] = dead ? nan : q[j];
            o[MPPI_PRED_QD + j] = dead ? nan : qd[j];
        }
        o[MPPI_PRED_ENERGY] = dead ? nan : E;
        full_fk(*model, q, [&](int slot, double v) { o[MPPI_PRED_EE + slot] = dead ? nan : v; });
    }
}

// The held points' world paths (mppi_predicted_held_optimal / mppi_predicted_held_rollouts): one thread
// per (requested rollout, step), the same wave layout and NaN rule.  link_fk (fr_cost_terms.hpp) at the
// record's q_k itself gives body 9's pose; the grasp frame sits at p9 + R9 ee_p with Ree = R9 ee_R, and
// held point i at p_ee + Ree c_i as the cost terms form it.  Rows of points the object does not have are NaN.
__global__ __launch_bounds__(64) void fr_predict_held_kernel(const DevModel *model, const double *rec, const PredictRow *rows, int H,
                                                             DevHeld held, double *out)
{
    const int lane = threadIdx.x;
    const PredictRow row = rows[blockIdx.x];
    const int RS = row.compact ? FR_REC_C : FR_REC;
    const double *rp = rec + row.offset;
    double *op = out + (int64_t)blockIdx.x * H * (OB_HELD_POINTS * 3);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int hc = held.count < 0 ? 0 : (held.count > OB_HELD_POINTS ? OB_HELD_POINTS : held.count);
    int first_bad = 0x7fffffff;
    for (int base = 0; base < H; base += 64) {
        const int k = base + lane;
        const bool act = k < H;
        const double2 *r2 = reinterpret_cast<const double2 *>(rp + (int64_t)(act ? k : H - 1) * RS);
        double q[FR_NB];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < FR_NB; j++) {
            const double2 v = r2[REC_QQD / 2 + j];
            q[j] = v.x;
            ok = ok && finite64(v.x) && finite64(v.y);
        }
        const unsigned long long bad = __ballot(act && !ok);
        if (first_bad == 0x7fffffff && bad) first_bad = base + __ffsll(bad) - 1;
        if (!act) continue;   // (after the chunk's last wave-wide operation)
        const bool dead = k >= first_bad;
        double lp[SC_LINKS][3], R9[9], Ree[9], pe[3], hp[OB_HELD_POINTS][3];
        mppi_cost::link_fk(*model, q, lp, R9);
#pragma unroll
        for (int r = 0; r < 3; r++)
            pe[r] = lp[SC_LINKS - 1][r] + ((R9[3 * r] * model->ee_p[0] + R9[3 * r + 1] * model->ee_p[1]) + R9[3 * r + 2] * model->ee_p[2]);
        mppi_cost::grasp_rotation(R9, model->ee_R, Ree);
        mppi_cost::held_points(&held, pe, Ree, hp);
        double *o = op + (int64_t)k * (OB_HELD_POINTS * 3);
#pragma unroll
        for (int i = 0; i < OB_HELD_POINTS; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) o[3 * i + c] = (dead || i >= hc) ? nan : hp[i][c];
    }
}

}  // namespace

namespace mppi_eng {

hipError_t launch_fr_predict_held(const DevModel *model, const double *rec, const PredictRow *rows, int64_t n, int H,
                                  const DevHeld &held, double *out, hipStream_t s)
{
    if (n <= 0 || H <= 0) return hipSuccess;
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fr_predict_held_kernel, dim3((unsigned)n), dim3(64), 0, s, model, rec, rows, H, held, out);
    return hipGetLastError();
}

hipError_t launch_fr_predict(const DevModel *model, const double *rec, const PredictRow *rows, int64_t n, int H, int energy,
                             double *out, hipStream_t s)
{
    if (n <= 0 || H <= 0) return hipSuccess;
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fr_predict_kernel, dim3((unsigned)n), dim3(64), 0, s, model, rec, rows, H, energy, out);
    return hipGetLastError();
}

}  // namespace mppi_eng
