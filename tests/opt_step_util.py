"""Shared by tests/test_opt_step_host.py and tests/test_opt_step_gpu.py: the formulas of include/mm_opt_step.h restated in
numpy, and the recorded optimiser steps of the reference (tests/golden/mappo_train_*.npz, gi_train_*.npz) as a flat list."""
import numpy as np

import gi_train_util as gi
import policy_train_util as pt

MAPPO_NETS = {"actor": ["actor." + k for k in pt.NAMES], "critic": ["critic." + k for k in pt.NAMES]}


def restated_step(algo, dtype, params, grads, state1, state2, step, lr, a, b2, eps, max_grad_norm):
    """One optimiser step of one network by the formulas of include/mm_opt_step.h with every stored value and every
    intermediate in `dtype`: returns (new params, new state1, new state2, total norm).  Lists of arrays in, lists out."""
    f = dtype
    total = np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads))
    coef = f(1.0)
    if max_grad_norm is not None:
        coef = min(f(1.0), f(max_grad_norm) / (f(total) + f(1e-6)))
    out_p, out_1, out_2 = [], [], []
    for i, (p, g) in enumerate(zip(params, grads)):
        p, g = np.asarray(p, f), np.asarray(g, f) * f(coef)
        if algo == "rmsprop":
            v = np.asarray(state1[i], f) * f(a) + (f(1.0 - a) * g) * g
            p = p - f(lr) * g / (np.sqrt(v) + f(eps))
            out_1.append(v)
        else:
            m = np.asarray(state1[i], f)
            m = m + f(1.0 - a) * (g - m)
            v = np.asarray(state2[i], f) * f(b2) + (f(1.0 - b2) * g) * g
            p = p - f(lr / (1.0 - a ** step)) * m / (np.sqrt(v) / f(np.sqrt(1.0 - b2 ** step)) + f(eps))
            out_1.append(m)
            out_2.append(v)
        out_p.append(p.astype(f))
    return out_p, out_1, out_2, total


def recorded_runs():
    """Every recorded run as (name, meta of its train 0, networks, steps): networks {net: [tensor keys]}, steps the list over
    both trains and all agent steps of (z, meta, a): pre-step parameters z[pre_step_prefix(a) + key], gradients
    z["a%d_g_" % a + key], post-step parameters z["a%d_q_" % a + key].  One RMSprop per network runs through all of them."""
    out = []
    for run in pt.RUNS:
        steps = []
        for t in (0, 1):
            z, meta = pt.load_fixture(run, t)
            steps += [(z, meta, a) for a in range(meta["agent_steps"])]
        out.append(("mappo_" + run, steps[0][1], MAPPO_NETS, steps))
    for loss in ("mse", "huber"):
        steps = []
        for t in (0, 1):
            z, meta = gi.load_fixture(loss, t)
            steps += [(z, meta, a) for a in range(meta["agent_steps"])]
        out.append(("gi_" + loss, steps[0][1], {"policy": list(gi.GRAD_NAMES)}, steps))
    return out


def run_lr(meta, net):
    return meta["lr"] if net == "policy" else meta[net + "_lr"]


pre_step_prefix_of = pt.pre_step_prefix  # "p_" before agent step 0, the previous step's "a%d_q_" after (both fixture families)
