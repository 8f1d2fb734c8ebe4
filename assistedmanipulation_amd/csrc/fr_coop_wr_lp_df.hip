// fr_coop_wr_lp_df.hip - the rollout launches of obstacle avoidance with a distance field on the pushed
// robot: the simulated end-effector wrench in the step, the capsule term and the field term in the
// objective (fr_coop_wr_lp_df_kernel, fr_coop_x_wr_lp_df_kernel): fr_coop.hip's text as a translation unit
// of its own, like fr_coop_wr_lp_cap.hip.
#define FR_COOP_LP_UNIT 1
#define FR_COOP_WR_UNIT 1
#define FR_COOP_OB_UNIT 1
#define FR_COOP_CAP_UNIT 1
#define FR_COOP_DF_UNIT 1
#include "fr_coop.hip"
