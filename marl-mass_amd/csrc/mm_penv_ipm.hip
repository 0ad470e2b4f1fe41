// mm_penv_ipm.hip -- the interior-point step kernels with per-env cbf_eta / cbf_tau / HEADWAY_TIME (object mm_penv_ipm.o)
#include "mm_step_host.h"

void mm_launch_step_penv_ipm(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) { launch_step_penv_all<true>(h, g, actions, out, s); }
