// fr_coop_lp_cap.hip - the rollout launches of obstacle avoidance with capsules (mppi_set_obstacle_capsules): the
// kinematic link-position objective with the obstacle term on the robot's points and segments, capsule obstacles included
// (fr_coop_lp_cap_kernel, fr_coop_x_lp_cap_kernel; fr_cost_terms.hpp capsule_term): fr_coop.hip's text
// as a translation unit of its own, like fr_coop_lp_ob.hip, so that the other units' code objects are
// what they were without it.
#define FR_COOP_LP_UNIT 1
#define FR_COOP_OB_UNIT 1
#define FR_COOP_CAP_UNIT 1
#include "fr_coop.hip"
