/*
 * mm_supervisor.h -- the reference's action-replacement safety supervisor on the device.
 *
 * safety_guarantee = "priority" (abstract.py:460-462 -> central_layer.py:16-178 safety_supervisor, the reference's
 * default) rewrites the joint action before the env steps: controlled vehicles are taken in priority order, each one
 * rolled (simulation_frequency // policy_frequency) * n_step sub-steps ahead together with its four lane neighbours on a
 * copy of the env, and an action whose lookahead crashes is replaced by the available action with the largest safety
 * room (abstract.py:219-280).  Exported by libmm_hip.so (marl-mass_amd/csrc/mm_supervisor.hip, DEV = device pointers) and, as
 * test infrastructure, by the CPU oracle (oracle/mm_oracle.c: a twin written from the reference on a plain per-env copy,
 * DEV = host pointers, same error codes and contracts; in the oracle's math mode 1 it matches the kernel bit for bit).
 *
 * Scope: merge-multi-agent-v0, CAV-only and mixed traffic.  HDVs (MM_B_KIND 2, IDMVehicle) in the lookahead follow
 * idm_controller.py (generate_actions once at its first sub-step, two draws; a crashed HDV's points alias its live
 * position).  safety_guarantee = "dmc" (abstract.py:463-464 -> decentralised_dmc.py:70-193 safety_layer_dmc) is the
 * second entry, mm_supervise_dmc, for the same envs (marl-mass_amd/csrc/mm_supervisor_dmc.hip; the device only: the oracle
 * has no twin of it, its one-lane-per-env MM_DMC_LITERAL form is what is read against the reference).  v1 is not covered
 * by either (the reference's own v1 supervisor fails on IDMVehicleHist HDVs).
 */
#ifndef MM_SUPERVISOR_H
#define MM_SUPERVISOR_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_SUP_PRIORITY 1 /* central_layer.py safety_supervisor(env, actions, is_priority=True) */

/* Bytes of the caller-owned lookahead scratch for E envs x N slots and a horizon of n_step policy steps of sub_steps
 * simulation steps each (simulation_frequency // policy_frequency: 3 at the default 15 / 5 Hz). */
int32_t mm_supervise_scratch_bytes(int32_t E, int32_t N, int32_t n_step, int32_t sub_steps, uint64_t *bytes);

/*
 * new_actions = safety_supervisor(env, actions) for every env of the handle, on its CURRENT state (nothing in the state
 * buffer changes).  actions / new_actions: DEV int32[E][N] (may not alias); slots that are absent or not controlled
 * are copied through.  Codes outside 0..4 pass through unless the lookahead replaces them.
 * uniforms: DEV double[E][uniform_stride] (stride >= 9 * N): the np.random.rand() values the reference would draw, in
 *           its order -- one priority tie-breaker per controlled vehicle, in controlled order, then two per HDV
 *           whose actions a lookahead generates, as they happen (at most N_cav + 8 N_cav <= 9 N).  NULL: the device draws
 *           them (Philox4x32-10 keyed on the env's seed plane, MM_E_EPISODE, MM_E_STEPS and the draw index), so a
 *           checkpoint, a sharded batch (first_env) or a graph replay draws what an unbroken run would.  Draw d of env e is
 *           u53(w[0], w[1]) = ((w[0] >> 5) * 2^26 + (w[1] >> 6)) / 2^53 of the four output words w of Philox4x32-10 with the
 *           counter (d, MM_E_EPISODE[e], MM_E_STEPS[e], 0x53555056 -- the supervisor's domain word) and the key (low, high
 *           half of seed[e]).
 * n_draws:  DEV int32[E] or NULL -- uniforms each env consumed.
 * scratch:  DEV, >= mm_supervise_scratch_bytes(E, N, n_step, sub_steps), 8-byte aligned, contents irrelevant.
 * Only enqueues work on `stream` (no allocation, no synchronisation): graph-capturable.
 * MM_ERR_INVALID_ARG: v1 handle, unknown kind, n_step < 1, stride < 9 * N, scratch too small, NULL actions / outputs.
 */
int32_t mm_supervise(MMHandle h, int32_t kind, int32_t n_step, const int32_t *actions, const double *uniforms,
                     int32_t uniform_stride, void *scratch, uint64_t scratch_bytes, int32_t *new_actions,
                     int32_t *n_draws, MMStream stream);

/*
 * safety_guarantee = "dmc": new_actions = safety_layer_dmc(env, actions).  Decentralised: every controlled vehicle is
 * propagated n_points = sub_steps * n_step sub-steps ONCE with its original action, every HDV behind them, and a vehicle
 * whose stored points collide with those of its four lane neighbours (or the obstacle) takes the available action with
 * the largest summed safety room.  Contracts as mm_supervise (current state, nothing in it changes, absent / uncontrolled
 * slots copied through, only enqueues work on `stream`) except:
 * uniforms: DEV double[E][uniform_stride], stride >= 2 * N.  An env always draws n_cav + 2 n_hdv values: draw i is the
 *           tie-breaker of controlled vehicle i, draws n_cav + 2 j and n_cav + 2 j + 1 scale the steering and the
 *           acceleration of the j-th HDV.  NULL: Philox as mm_supervise, same counter, key and domain word, with that index.
 * flags:    0: the lane-parallel form (four launches).  MM_DMC_LITERAL: one lane per env in the reference's order.  Both
 *           write the same bits to new_actions, n_draws and trace.
 * scratch:  DEV, >= mm_supervise_dmc_scratch_bytes(E, N, n_step, sub_steps), 8-byte aligned, contents irrelevant.
 *           n_points is at most 128 (n_step <= 42 at the default 15 / 5 Hz).
 * trace:    DEV double[E][N][MM_DMC_TRACE_DOUBLES] or NULL, per slot:
 *             0      position in key order (smallest key first); -1 for a slot that is not controlled
 *             1      key (NaN: not controlled)
 *             2      crash_t: first sub-step whose point collides, -1 if the lookahead did not crash
 *             3..6   neighbour slots v_fl, v_rr, v_fr, v_rl (-1 none; -2 is reserved for an obstacle, which
 *                    surrounding_vehicles never returns)
 *             7      bit mask of the available actions (bit a = action a); 0: not controlled
 *             8..12  room[a] of action a = 0..4 (NaN where unavailable or not scored)
 *             13..16 x, y, heading, speed at the end of the propagation (NaN: absent slot)
 *             17..18 an HDV's generated steering and acceleration (NaN otherwise)
 *             19     the x at which the vehicle stands in the copy after its evaluation (its crash-time point, else 13)
 * MM_ERR_INVALID_ARG: v1 / hdv-v1 handle, n_step < 1, n_points > 128, stride < 2 * N, scratch too small or misaligned,
 * NULL actions / new_actions / scratch, flag bits other than MM_DMC_LITERAL.  Nothing is written then.
 */
#define MM_SUP_DMC 2 /* decentralised_dmc.py safety_layer_dmc(env, actions); mm_supervise does not take it */
#define MM_DMC_LITERAL 1u
#define MM_DMC_TRACE_DOUBLES 20
int32_t mm_supervise_dmc_scratch_bytes(int32_t E, int32_t N, int32_t n_step, int32_t sub_steps, uint64_t *bytes);
int32_t mm_supervise_dmc(MMHandle h, int32_t n_step, uint32_t flags, const int32_t *actions, const double *uniforms,
                         int32_t uniform_stride, void *scratch, uint64_t scratch_bytes, int32_t *new_actions,
                         int32_t *n_draws, double *trace, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_SUPERVISOR_H */
