// mm_lanes_ipm.hip -- the interior-point step kernels in the 6- / 12-lane rotation layouts (object mm_lanes_ipm.o)
#include "mm_step_host.h"

void mm_launch_step_lanes_ipm(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
#define MM_LANES_CASE(GG) launch_step_ipm_g<GG>(h, actions, out, s)
  MM_FOR_GROUP(g, MM_NO_GROUP, MM_LANES_CASE);
#undef MM_LANES_CASE
}
