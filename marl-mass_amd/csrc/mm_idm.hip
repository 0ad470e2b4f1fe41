// mm_idm.hip -- merge-multi-agent-hdv-v1 (MergeEnvLCHDV): the general unshielded kernels with every vehicle an IDM / MOBIL
// observer; the step reads no actions.  Power-of-two groups for the reset (like every kind), the step's layouts as step_group()
// picks them (object mm_idm.o)
#include "mm_step_host.h"

void mm_launch_reset_idm(MMHandle h, int mode, const uint8_t *mask, const uint64_t *seeds, void *obs, uint8_t *avail, hipStream_t s) {
#define MM_IDM_CASE(GG) launch_reset_t<GG, MM_ENV_HDV_V1>(h, mode, mask, seeds, obs, avail, s)
  MM_FOR_GROUP(group_size(h->N), MM_IDM_CASE, MM_NO_GROUP);
#undef MM_IDM_CASE
}
void mm_launch_step_idm(MMHandle h, int g, const MMStepOut *out, hipStream_t s) {
#define MM_IDM_CASE(GG) launch_step_t<GG, MM_ENV_HDV_V1, MM_SHIELD_NONE, true>(h, nullptr, out, s)
  MM_FOR_GROUP(g, MM_IDM_CASE, MM_IDM_CASE);
#undef MM_IDM_CASE
}
