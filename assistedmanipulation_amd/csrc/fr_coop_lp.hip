// fr_coop_lp.hip - the rollout launches of the kinematic link-position model (mppi_set_link_positions):
// fr_coop.hip's kernels with the objective that evaluates the self-collision term on each record's
// link positions (fr_coop_lp_kernel, fr_coop_x_lp_kernel), compiled from the same text as a
// translation unit of their own, so that the default mode's code object is what it was without them.
#define FR_COOP_LP_UNIT 1
#include "fr_coop.hip"
