// mm_penv.hip -- the exact-mode step kernels with per-env cbf_eta / cbf_tau / HEADWAY_TIME, include/mm_env_params.h (object
// mm_penv.o)
#include "mm_step_host.h"

void mm_launch_step_penv(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  if (h->cfg.qp_solver == MM_QP_IPM) mm_launch_step_penv_ipm(h, g, actions, out, s);  // (mm_penv_ipm.hip)
  else launch_step_penv_all<false>(h, g, actions, out, s);
}
