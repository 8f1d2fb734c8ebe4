// fr_predict.hpp — predicted trajectories from the rollout launches' step records (fr_predict.hip):
// the launch interface, and the forward-kinematics chain over all twelve bodies and both frames.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine_types.hpp"
#include "fsincos.hpp"

namespace mppi_eng {

// One requested rollout: where its H step records start (doubles into the record buffer) and
// whether they are compact ones (FR_REC_C) or 768-B ones (FR_REC).  The kernel needs no knowledge
// of the launch plan (predict_plan.hpp).
struct PredictRow {
    int64_t offset;
    int32_t compact;
    int32_t pad;
};

// out[n][H][MPPI_PRED_N] from rec and rows[n] (device pointers); energy: the records' tank level is
// live (the launch integrated it), else the energy column is NaN
hipError_t launch_fr_predict(const DevModel *model, const double *rec, const PredictRow *rows, int64_t n, int H, int energy,
                             double *out, hipStream_t s);

// out[n][H][OB_HELD_POINTS][3]: the held points' world positions at q_k (mppi_predicted_held_*), NaN rows
// for the points `held` does not have
hipError_t launch_fr_predict_held(const DevModel *model, const double *rec, const PredictRow *rows, int64_t n, int H,
                                  const DevHeld &held, double *out, hipStream_t s);

// World translations of every body frame (lp[1 + i]: body i; lp[0]: the universe) and of the grasp
// and arm-mount frames at joint positions q[0..11]: link_fk's chain (fr_cost_terms.hpp), pose_i =
// pose_parent o placement_i o joint_i term for term with the rollout kernel's fsincos, carried past
// body 9 to the fingers (both on body 9, FR_PARENT) and to the frames on bodies FR_EE_PARENT and
// FR_AM_PARENT.  store(slot, value) takes the 3 x 15 results as they come: slots 0..2 the grasp
// frame, 3..5 the arm mount, 6 + 3 L + c link L.
template <class Store>
__device__ __forceinline__ void full_fk(const DevModel &M, const double *q, Store store)
{
    const SinCosK K = sincos_constants();
    double R[9], p[3];   // the chain's pose: body i - 1 for i <= 10, then body 9 for both fingers
#pragma unroll
    for (int c = 0; c < 3; c++) store(6 + c, 0.0);
#pragma unroll
    for (int i = 0; i < FR_NB; i++) {
        const DevBody &b = M.b[i];
        double Rl[9], pl[3];
        if (FR_KIND[i] == KIND_RZ) {
            double s, c;
            fsincos(q[i], &s, &c, K);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                Rl[3 * r + 0] = b.R[3 * r + 0] * c + b.R[3 * r + 1] * s;
                Rl[3 * r + 1] = b.R[3 * r + 0] * (-s) + b.R[3 * r + 1] * c;
                Rl[3 * r + 2] = b.R[3 * r + 2];
                pl[r] = b.p[r];
            }
        } else {
            const int col = FR_KIND[i] == KIND_PX ? 0 : 1;
            const double d = FR_KIND[i] == KIND_PNY ? -q[i] : q[i];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) Rl[3 * r + k] = b.R[3 * r + k];
                pl[r] = b.p[r] + b.R[3 * r + col] * d;
            }
        }
        double Rn[9], pn[3];
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) Rn[k] = Rl[k];
#pragma unroll
            for (int k = 0; k < 3; k++) pn[k] = pl[k];
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int cc = 0; cc < 3; cc++) Rn[3 * r + cc] = (R[3 * r] * Rl[cc] + R[3 * r + 1] * Rl[3 + cc]) + R[3 * r + 2] * Rl[6 + cc];
                pn[r] = p[r] + ((R[3 * r] * pl[0] + R[3 * r + 1] * pl[1]) + R[3 * r + 2] * pl[2]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) store(6 + 3 * (i + 1) + c, pn[c]);
        if (i == FR_AM_PARENT || i == FR_EE_PARENT) {
            const double *fp = i == FR_EE_PARENT ? M.ee_p : M.am_p;
#pragma unroll
            for (int r = 0; r < 3; r++)
                store((i == FR_EE_PARENT ? 0 : 3) + r, pn[r] + ((Rn[3 * r] * fp[0] + Rn[3 * r + 1] * fp[1]) + Rn[3 * r + 2] * fp[2]));
        }
        if (i < FR_NB - 2) {   // bodies 10 and 11 hang on body 9: the chain's pose stays there
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = pn[k];
        }
    }
}

}  // namespace mppi_eng
