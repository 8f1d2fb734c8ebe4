// fr_coop_wr.hip - the rollout launches with the simulated end-effector wrench (mppi_set_simulated_wrench):
// fr_coop.hip's kernels with tau_w = J_G(q_k)^T w_k added to the step's torque (coop_rows' WR;
// fr_coop_wr_kernel, fr_coop_x_wr_kernel), compiled from the same text as a translation unit of
// their own, so that the default mode's code object is what it was without them.
#define FR_COOP_WR_UNIT 1
#include "fr_coop.hip"
