// mm_lanes.hip -- the exact-mode step kernels in the 6- / 12-lane rotation layouts, N = 5..6 and 9..12 (object mm_lanes.o)
#include "mm_step_host.h"

void mm_launch_step_lanes(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  if (fused_ipm(h)) {  // interior-point mode (mm_lanes_ipm.hip)
    mm_launch_step_lanes_ipm(h, g, actions, out, s);
  } else if (needs_general(h)) {  // HDVs / steer_vel: the kernels that carry IDM / MOBIL
#define MM_LANES_CASE(GG) launch_step_m<GG, true>(h, actions, out, s)
    MM_FOR_GROUP(g, MM_NO_GROUP, MM_LANES_CASE);
#undef MM_LANES_CASE
  } else {
#define MM_LANES_CASE(GG) launch_step_m<GG, false>(h, actions, out, s)
    MM_FOR_GROUP(g, MM_NO_GROUP, MM_LANES_CASE);
#undef MM_LANES_CASE
  }
}
