// mm_step_all.hip -- the step library as ONE object: the form of `make tuning` and of the stamps builds (-DMM_STAMPS), whose
// __device__ stamp arrays (mm_kernels.hip) the debug readers of mm_main.hip read and which therefore cannot be spread over
// objects.  The tuning short-cuts that keep such a build small are described in mm_step_host.h.
#include "mm_main.hip"
#include "mm_general.hip"
#include "mm_ipm.hip"
#include "mm_lanes.hip"
#include "mm_lanes_ipm.hip"
#include "mm_split.hip"
#include "mm_split_general.hip"
#include "mm_idm.hip"
#include "mm_penv.hip"
#include "mm_penv_ipm.hip"
