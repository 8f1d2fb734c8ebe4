// fr_coop_lp_df.hip - the rollout launches of obstacle avoidance with a distance field
// (mppi_set_distance_field_avoidance): the capsule units' objective with the field term behind the capsule
// term (fr_coop_lp_df_kernel, fr_coop_x_lp_df_kernel; fr_cost_terms.hpp field_term): fr_coop.hip's text as a
// translation unit of its own, like fr_coop_lp_cap.hip, so that the other units' code objects are what
// they were without it.
#define FR_COOP_LP_UNIT 1
#define FR_COOP_OB_UNIT 1
#define FR_COOP_CAP_UNIT 1
#define FR_COOP_DF_UNIT 1
#include "fr_coop.hip"
