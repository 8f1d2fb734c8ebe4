// fr_coop_wr_lp_ob.hip - the rollout launches of obstacle avoidance (mppi_set_obstacle_avoidance): the simulated end-effector wrench and the kinematic
// link-position objective with the obstacle term
// (fr_coop_wr_lp_ob_kernel, fr_coop_x_wr_lp_ob_kernel; fr_cost_terms.hpp obstacle_term): fr_coop.hip's text
// as a translation unit of its own, like fr_coop_lp.hip, so that the other units' code objects are
// what they were without it.
#define FR_COOP_WR_UNIT 1
#define FR_COOP_LP_UNIT 1
#define FR_COOP_OB_UNIT 1
#include "fr_coop.hip"
