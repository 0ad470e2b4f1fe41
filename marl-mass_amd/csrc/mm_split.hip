// mm_split.hip -- the split interior-point step of a CAV-only batch: the phase form of the step kernel and the lane-per-env
// sweep kernel (object mm_split.o)
#include "mm_step_host.h"

void mm_launch_step_split(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  if (needs_general(h)) mm_launch_step_split_general(h, g, actions, out, s);  // HDVs / steer_vel (mm_split_general.hip)
  else launch_split_all<false>(h, g, actions, out, s);
}
