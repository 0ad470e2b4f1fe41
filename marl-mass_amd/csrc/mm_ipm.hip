// mm_ipm.hip -- the MM_QP_IPM fidelity-mode step kernels: the fused kernels with the QP solved by cvxopt's interior-point
// algorithm (include/mm_qp.h), CAV-only and general, power-of-two groups (object mm_ipm.o)
#include "mm_step_host.h"

void mm_launch_step_ipm(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
#define MM_IPM_CASE(GG) launch_step_ipm_g<GG>(h, actions, out, s)
  MM_FOR_GROUP(step_group(h), MM_IPM_CASE, MM_NO_GROUP);
#undef MM_IPM_CASE
}
