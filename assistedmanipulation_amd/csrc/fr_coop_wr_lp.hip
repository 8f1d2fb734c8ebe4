// fr_coop_wr_lp.hip - the rollout launches with the simulated end-effector wrench and the kinematic
// link-position objective together (fr_coop_wr_lp_kernel, fr_coop_x_wr_lp_kernel): fr_coop.hip's
// text with both switches, a translation unit of its own like fr_coop_lp.hip and fr_coop_wr.hip.
#define FR_COOP_WR_UNIT 1
#define FR_COOP_LP_UNIT 1
#include "fr_coop.hip"
