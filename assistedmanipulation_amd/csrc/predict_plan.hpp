// predict_plan.hpp — where the last rollout launch left a row's step records (d_rec), from the
// update's launch plan alone.  Plain C++17 with no HIP include, like coop_plan.hpp: the engine
// (mppi_predicted_rollouts) and a host-only test read the same function.
#pragma once

#include <stdint.h>

#include "coop_plan.hpp"

namespace mppi_eng {

// doubles per stored step record (kernels.hpp FR_REC, FR_REC_C; fr_predict.hip asserts they agree)
constexpr int PRED_REC = 96, PRED_REC_C = 48;

// The records of shard row lr (0 <= lr < count: global rollout begin + lr) of an update of H steps:
// *offset doubles into d_rec, H records of PRED_REC_C (*compact = 1) or PRED_REC doubles each.
//  - Launch i of the plan covers shard rows [row0, row0 + rows); row_slice (fr_coop.hip) starts its
//    records at row0 H PRED_REC doubles, whatever the launch's own record size.  A single-launch
//    plan is not sliced: its records start at 0.
//  - Within a launch, row lr' = lr - row0 is at lr' H RS: RS = PRED_REC for fr_coop_x_kernel (COOP_X:
//    the main waves' rows and the rows left over alike), PRED_REC_C for the one-wave and four-wave
//    launches of fr_coop_kernel.
//  - The folded filter() row is counted in the last launch's xrows but is no row of the shard: its
//    records are in d_rec_opt, and no lr reaches it.
// false: lr is no row of the plan.
inline bool predict_row(const CoopPlan &p, int H, int64_t lr, int64_t *offset, int *compact)
{
    for (int i = 0; i < p.nlaunch; i++) {
        const CoopLaunch &l = p.l[i];
        if (lr < l.row0 || lr >= l.row0 + l.rows) continue;
        const int64_t row0 = p.nlaunch > 1 ? l.row0 : 0;
        const bool c = l.kind != COOP_X;
        *offset = row0 * H * PRED_REC + (lr - l.row0) * H * (c ? PRED_REC_C : PRED_REC);
        *compact = c ? 1 : 0;
        return true;
    }
    return false;
}

}  // namespace mppi_eng
