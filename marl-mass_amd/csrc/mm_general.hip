// mm_general.hip -- the step kernels that carry HDVs (IDM / MOBIL) and steer_vel, power-of-two groups (object mm_general.o)
#include "mm_step_host.h"

void mm_launch_step_general(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
#define MM_GENERAL_CASE(GG) launch_step_m<GG, true>(h, actions, out, s)
  MM_FOR_GROUP(step_group(h), MM_GENERAL_CASE, MM_NO_GROUP);
#undef MM_GENERAL_CASE
}
