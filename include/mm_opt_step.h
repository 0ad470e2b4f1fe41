/*
 * mm_opt_step.h -- the tail of one agent step of the learners in ONE launch: clip_grad_norm_, the optimiser step
 * (torch.optim.RMSprop or Adam with torch's defaults) and the soft update of the target network.
 *
 * One MMOptGroup is one network = one clipping group = one optimiser: MAPPO_GI's shared actor-critic is one group of twelve
 * tensors, MAPPO's actor and critic are two groups of six.  The arithmetic is torch's float32 arithmetic, so that optimiser
 * state and parameters move between this path and torch.optim (a checkpoint written by one loads into the other):
 *
 *   clip      total = sqrt(sum over the group's tensors of sum g^2)  (accumulated in double, narrowed to float)
 *             coef  = min(1, max_grad_norm / (total + 1e-6)); every gradient is USED as float(g * coef).
 *             The gradient buffers are READ ONLY: unlike torch.nn.utils.clip_grad_norm_, which scales .grad in place, they
 *             still hold what the gradient kernels wrote.  max_grad_norm < 0: no clipping (coef = 1).
 *   RMSprop   (no momentum, not centred)   v = alpha v + (1 - alpha) g g;   p = p - lr * g / (sqrt(v) + eps)
 *   Adam      (no weight decay, no amsgrad) step += 1;  m = m + (1 - b1)(g - m);  v = b2 v + (1 - b2) g g
 *             p = p - (lr / (1 - b1^step)) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 *             The two bias corrections are computed in double from the DEVICE counter `step` and then narrowed to float, as
 *             torch computes them on the host: the call has no host state, so a captured graph replays correctly.
 *   blend     t = float(1 - tau) * t + float(tau) * p_new: two products and a sum, each rounded (1 - tau taken in double),
 *             the learners' `t.copy_((1.0 - tau) * t + tau * s)`.  Runs after the update when soft_update != 0.
 *   Hyperparameters are doubles here and narrowed to float where torch narrows them (1 - alpha, 1 - b1, 1 - b2, lr / bias
 *   correction are taken in double first).  Non-finite gradients propagate as in torch: no special case.
 *
 * One launch per call, one workgroup per group (blockIdx.x = group).  Phase 1: every thread squares a fixed strided share of
 * the group's gradients into a double, the wave is reduced by __shfl_xor and the waves through LDS in a fixed order; phase 2,
 * after a workgroup barrier: the element update of parameter, state and target, 16 bytes per access where all of a tensor's
 * pointers are 16-byte aligned, scalar accesses for the other tensors and for tails.  No atomics and no second launch: two
 * calls on equal inputs give bit-identical outputs.  Only enqueues work on `stream` (no allocation, no synchronisation):
 * graph-capturable.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_opt_step.hip), like mm_policy_train: no oracle twin, not part of
 * include/mm_abi.h's symbol list or version.  torch.optim on the same tensors is the CPU form.
 */
#ifndef MM_OPT_STEP_H
#define MM_OPT_STEP_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_OPT_RMSPROP 0
#define MM_OPT_ADAM    1
#define MM_OPT_BLEND   2           /* no optimiser: only target = (1 - tau) target + tau param */
#define MM_OPT_MAX_TENSORS 16
#define MM_OPT_MAX_GROUPS 4

typedef struct MMOptGroup {        /* one network = one clipping group = one optimiser */
  int32_t algo, n_tensors;
  int64_t count[MM_OPT_MAX_TENSORS];      /* elements per tensor, >= 0 */
  float *param[MM_OPT_MAX_TENSORS];       /* DEV, contiguous, 4-byte aligned is enough */
  const float *grad[MM_OPT_MAX_TENSORS];  /* DEV, read only: NOT scaled in place */
  float *state1[MM_OPT_MAX_TENSORS];      /* RMSprop square_avg | Adam exp_avg */
  float *state2[MM_OPT_MAX_TENSORS];      /* Adam exp_avg_sq (NULL for RMSprop) */
  float *target[MM_OPT_MAX_TENSORS];      /* optional: blended after the update when soft_update != 0 */
  int32_t *step;                          /* DEV int32[1], incremented by the kernel: Adam needs it, RMSprop may have one */
  double lr, alpha_or_beta1, beta2, eps, max_grad_norm /* < 0: no clipping */, tau;
  int32_t soft_update;
  float *grad_norm;                       /* optional DEV float[1]: total norm before clipping */
} MMOptGroup;

/*
 * groups: HOST array of n_groups (1..MM_OPT_MAX_GROUPS) groups; every pointer inside is a DEVICE pointer.  The tensors of all
 * groups must not overlap one another (a gradient may of course be read by nobody else).
 * A tensor with count == 0 contributes nothing (its pointers are not looked at); a group with n_tensors == 0 does nothing
 * (not even the step increment or grad_norm), and so does one whose tensors are all empty.
 * MM_OPT_RMSPROP reads param, grad, state1 (and target when soft_update != 0); lr, alpha_or_beta1 = alpha, eps.  Its arithmetic
 *                does not depend on a step count; a `step`, when given, is incremented all the same (torch keeps one too).
 * MM_OPT_ADAM    reads param, grad, state1, state2, step (and target when soft_update != 0); lr, alpha_or_beta1 = b1, beta2, eps.
 * MM_OPT_BLEND   reads param (the source) and target only, always blends (soft_update is not looked at), takes no norm.
 * grad_norm, when given, receives the float total norm of an RMSprop / Adam group whether it clips or not.
 * MM_ERR_INVALID_ARG, with the reason in mm_last_error(NULL): groups NULL, n_groups outside 1..4, an unknown algo, n_tensors
 *   outside 0..16, a negative count, more than 2^33 elements in one group, a NULL param / grad / state1 of a tensor with
 *   count > 0, state2 or step missing for Adam, soft_update (or MM_OPT_BLEND) with a NULL target, a pointer that is not
 *   4-byte aligned, lr negative or not finite, eps <= 0, alpha / b1 / b2 outside [0, 1), tau outside [0, 1], max_grad_norm
 *   NaN.  Nothing is enqueued when any group is refused.
 */
int32_t mm_opt_step(const MMOptGroup *groups /* HOST */, int32_t n_groups /* 1..4 */, MMStream stream);

/*
 * The same tail for K stacked members per group, in ONE launch of n_groups * K workgroups (marl-mass_amd/csrc/
 * mm_opt_step_bank.hip): the policy bank's optimiser step (include/mm_policy_bank_train.h).  Every group is a PROTOTYPE: tensor i
 * of member k (param, grad, state1, state2, target alike) sits at the prototype's pointer + k * count[i] elements -- the stacked
 * [K][...] storage of the bank -- `step` is DEV int32[K] and `grad_norm` an optional DEV float[K], member k's at index k.  The
 * hyperparameters are shared by the members.  soft_mask: bit k says whether member k blends its target this call; the
 * prototype's soft_update field is not looked at (an MM_OPT_BLEND prototype blends the members whose bit is set and leaves the
 * others alone).  1 <= K <= 64 (MM_BANK_MAX_GROUPS); bits of soft_mask at and above K are ignored.
 * The defining property: member k's parameters, state, targets, step and norm after the call are bit for bit what mm_opt_step
 * gives on member k's tensors alone with soft_update = bit k.  Deterministic, only enqueues on `stream`: graph-capturable.
 * MM_ERR_INVALID_ARG, with the reason in mm_last_error(NULL): K outside 1..64 and everything mm_opt_step refuses, a prototype
 *   being checked as a group with soft_update = (some member blends).  Nothing is enqueued when any group is refused.
 */
int32_t mm_opt_step_bank(const MMOptGroup *groups /* HOST */, int32_t n_groups /* 1..4 */, int32_t K, uint64_t soft_mask,
                         MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_OPT_STEP_H */
