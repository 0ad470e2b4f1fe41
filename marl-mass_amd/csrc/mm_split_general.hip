// mm_split_general.hip -- the split interior-point step with the kernels that carry IDM / MOBIL and steer_vel (object
// mm_split_general.o)
#include "mm_step_host.h"

void mm_launch_step_split_general(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) { launch_split_all<true>(h, g, actions, out, s); }
