// coop_plan.hpp — the launch shape of an update's FrankaRidgeback rollouts (fr_coop.hip), decided in
// one place: which kernel, over which rows, with how many workgroups, where the rows left over and
// the folded filter() row go, and what the launch does besides the rollouts.  Plain C++17 with no
// HIP include: the engine, the launcher and a host-only test all read the same function.
#pragma once

#include <stdint.h>

namespace mppi_eng {

// A/B switches from the environment, read once per mppi_create into the handle (tests set them
// before creating a handle): a handle's launch paths never change under it, and no getenv runs on
// the update path (~80 ns each)
struct EnvSwitches {
    bool draw_ahead_off, tail_draws_off, pm_fused_off, costs_in_launch_off, handover_off, split_off, stream_prio_off;
    int relay_k;   // MPPI_RELAY_K: workgroups the rows left over travel through (1..RELAY_K_MAX; 0: the default)
    // MPPI_STAGE_WORK=0: a later relay member's stage waves do no objective work before their stage
    bool stage_work_off;
    // the handle's device: its CU count (the rollout launches' rounds of workgroups) and LDS per
    // block (the fused point mass's residency check), set at create for that device - per handle, so
    // that handles created on different devices from several threads never read each other's
    unsigned cus;
    int lds_max;
};

constexpr int ROWS_PER_WAVE = 4;                 // one rollout per 16-lane row
constexpr int WG_ROWS = 4 * ROWS_PER_WAVE;       // rows of a four-wave workgroup's main waves
constexpr int CH = 16;                           // steps per chunk of the objective in the launch
constexpr int HC_MAX = 128;                      // the horizon bound of the objective in fr_coop_x_kernel (its Lcs)
constexpr int RELAY_K_MAX = 4, RELAY_STRIDE = 8, RELAY_GROUPS_MAX = 4;
// Relay members by default: at 4096 x 64 (profiles/r06/relay_k) K = 2 ran 0.1838-0.1848 ms/update
// against 0.1881-0.1892 for K = 1, 0.1858-0.1880 for K = 3 and 0.1871-0.1879 for K = 4 (each member's
// first stage pays ~10 us of hand-over and its own setup, so more members stop paying off past two);
// with gj_rows K = 2 0.1757-0.1772, K = 1 0.1789-0.1823, K = 3 0.1776-0.1791 (ab_gjrows.txt).
constexpr int RELAY_K_DEFAULT = 2;

// Where rank_draw_kernel finds the rows a launch with tail draws left to it
struct CoopTail {
    int64_t row0 = 0;    // first row of the launch with the rows left over
    int64_t xbase = 0;   // the rows left over start here (launch rows)
    int nxb = 0;         // workgroups of that launch whose first wave's rows rank_draw_kernel draws
    int launches = 1;
};

enum CoopKind : int {
    COOP_ONE_WAVE = 0,    // fr_coop_kernel<1>: one-wave workgroups, any number of rounds
    COOP_FOUR_WAVE = 1,   // fr_coop_kernel<4>: one round of four-wave workgroups, no rows left over
    COOP_X = 2            // fr_coop_x_kernel: one round, the rows left over on the relay
};

struct CoopLaunch {
    int kind;            // CoopKind
    int64_t row0, rows;  // the launch's rows of the shard (row_slice)
    unsigned grid;       // workgroups
    int64_t xbase, xrows;   // COOP_X: the rows left over [xbase, xbase + xrows), launch rows; xrows counts the folded row
    int relay_k;         // workgroups the rows left over travel through
};

struct CoopPlan {
    bool error;          // drawn_ahead on a shape that takes one-wave workgroups, which sample nothing
    int nlaunch;         // 1, or 2 for the split
    CoopLaunch l[2];
    bool x_kernel;       // fr_coop_x_kernel runs (768-B records), else fr_coop_kernel (compact ones)
    bool folded;         // the pending filter() rides as one more row of the last launch
    bool costs_in_launch;   // the launch evaluates the objective: no fr_step_cost_kernel after it
    bool tail_draws;     // the launch makes the next update's draws for its main waves' rows
    bool handover;       // the rows left over travel through relay stages (MPPI_HANDOVER=0, H < 5: one wave beside main wave 0)
    CoopTail tail;
};

// The rows left over travel through relay stages: four stages of a member share its loop steps,
// stage r from step (r (H - 1)) / 4, and a stage that starts at step 0 does not wait for the stage
// before it.  With fewer than four loop steps two stages would start at 0 and store the hand-over
// state and the stage word unordered, so such a horizon keeps the rows on one wave (the members'
// four-step rule below, for the one-member relay).
inline bool coop_handover(int H, const EnvSwitches &env) { return !env.handover_off && H - 1 >= 4; }

// Relay members for a launch of `groups` workgroups with xrows rows left over: needs the engine's
// exchange buffer, the hand-over, a member workgroup q + RELAY_STRIDE m in the grid for every relay
// group q, and at least one chunk and four steps per member; else one workgroup.
inline int coop_relay_members(int H, int64_t groups, int64_t xrows, bool relay_buffer, const EnvSwitches &env)
{
    if (!coop_handover(H, env) || !relay_buffer || xrows <= 0) return 1;
    const int64_t nxb = (xrows + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE;
    const int nch = (H + CH - 1) / CH;
    int K = env.relay_k ? env.relay_k : RELAY_K_DEFAULT;
    if (K > RELAY_K_MAX) K = RELAY_K_MAX;
    if (K > nch) K = nch;
    if (nxb > RELAY_GROUPS_MAX) return 1;
    for (; K > 1; K--) {
        if (nxb + (int64_t)RELAY_STRIDE * (K - 1) > groups) continue;
        bool ok = true;
        for (int m = 0; m < K && ok; m++) {
            const int k0 = m == 0 ? 0 : (m * nch / K) * CH - 1, k1 = m + 1 == K ? H - 1 : ((m + 1) * nch / K) * CH - 1;
            ok = k1 - k0 >= 4;
        }
        if (ok) break;
    }
    return K;
}

// The plan for `count` rows of H steps.  filter_pending: the previous update's filter() waits to be
// folded in; drawn_ahead: the eps tensor holds this update's draws already; tail_buffer: there is a
// buffer for the next update's draws; relay_buffer: the engine's relay exchange buffer exists.
//
// One round is one four-wave workgroup per CU (EnvSwitches::cus), WG_ROWS rows each.
//  - `count` fills at most one round and the rows left over (count mod WG_ROWS, plus the folded
//    filter() row, which rides along only when there are rows left over anyway: alone it would add
//    a wave, so then it stays pending) fit the relay of its workgroups: fr_coop_x_kernel, or
//    fr_coop_kernel<4> when nothing is left over.
//  - The split: one-wave workgroups hold two waves per SIMD, 32 rows per CU and round (8192 on 256
//    CUs), and a count just past that - R = S + 2 at S = 8192 - leaves one wave for a second round
//    that runs alone for the whole horizon (1.49 + 1 lone-wave horizons, plus the separate cost
//    kernel).  Two launches of one wave per SIMD (each 1.06-1.1 lone-wave horizons with the
//    objective beside the loops) take less: fr_coop_x_kernel over one round of full groups, then
//    over the rest, whose rows left over and the folded filter() row travel through its relay.
//    Taken when the rest fits one round with room for a folded row, pending or not (MPPI_SPLIT=0:
//    never).
//  - Anything else: one-wave workgroups throughout, each wave its own rows' objective.
inline CoopPlan coop_plan(int64_t count, int H, bool filter_pending, bool drawn_ahead, bool tail_buffer, bool relay_buffer,
                          const EnvSwitches &env)
{
    CoopPlan p{};
    p.nlaunch = 1;
    const int64_t cus = env.cus ? (int64_t)env.cus : 256, round = cus * WG_ROWS;
    const bool x_costs = !env.costs_in_launch_off && H <= HC_MAX;   // fr_coop_x_kernel's Lcs holds HC_MAX steps
    // the x-kernel launch over n rows from row0; tail draws ride in its objective waves only, and
    // need the draws made ahead (the sampling arguments)
    auto x_launch = [&](int64_t row0, int64_t n, bool frow) {
        const int64_t groups = n / WG_ROWS, xrows = n - groups * WG_ROWS + (frow ? 1 : 0);
        p.x_kernel = p.nlaunch == 2 || xrows != 0;
        p.l[p.nlaunch - 1] = {p.x_kernel ? COOP_X : COOP_FOUR_WAVE, row0, n, (unsigned)groups, groups * WG_ROWS, xrows,
                              coop_relay_members(H, groups, xrows, relay_buffer, env)};
        p.folded = frow;
        p.costs_in_launch = x_costs;
        p.handover = coop_handover(H, env);
        p.tail_draws = p.x_kernel && x_costs && drawn_ahead && tail_buffer;
        p.tail = {row0, row0 + groups * WG_ROWS, (int)((xrows + 3) / 4), p.nlaunch};
    };
    const int64_t groups = count / WG_ROWS, extra = count - groups * WG_ROWS;
    const int64_t rest = count - round, gb = rest / WG_ROWS, xb = rest - gb * WG_ROWS;
    if (count > 2 * round && !env.split_off && gb > 0 && gb <= cus && xb + 1 <= gb * ROWS_PER_WAVE) {
        p.nlaunch = 2;
        p.l[0] = {COOP_X, 0, round, (unsigned)cus, round, 0, 1};
        x_launch(round, rest, filter_pending);
        return p;
    }
    const bool frow = filter_pending && extra > 0;
    if (groups > 0 && groups <= cus && extra + (frow ? 1 : 0) <= groups * ROWS_PER_WAVE) {
        x_launch(0, count, frow);
        return p;
    }
    p.error = drawn_ahead;
    p.l[0] = {COOP_ONE_WAVE, 0, count, (unsigned)((count + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE), 0, 0, 1};
    p.costs_in_launch = groups > 0 && !env.costs_in_launch_off;
    return p;
}

// The launch shape as far as it depends on the row count and the switches alone (a filter() taken
// as pending, which never changes the kernel kind).
// Rounds of four-wave workgroups - the launches that can take draws made ahead - run for `count` rows
inline bool coop_fusable(int64_t count, const EnvSwitches &env)
{
    return coop_plan(count, 1, true, false, false, false, env).l[0].kind != COOP_ONE_WAVE;
}
// A pending filter() folds into the update launch with the objective in it (the hipGraph path's shape)
inline bool coop_folds(int64_t count, int H, const EnvSwitches &env)
{
    const CoopPlan p = coop_plan(count, H, true, false, false, false, env);
    return p.folded && p.costs_in_launch;
}

}  // namespace mppi_eng
