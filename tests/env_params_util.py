"""Shared pieces of the per-env shield parameter tests (include/mm_env_params.h): test_env_params_gpu.py drives the HIP
library, test_env_params_host.py the host-side validation and the oracle library's refusal.

Every env here is merge-multi-agent-v1, shielded, auto-reset on, float64 observations, env seed 7, stepped T = 40 times from
reset() with uniform-random actions (generator seed 3, created once per N).  E = 40 envs, env e carrying parameter set e % 5:
neighbouring lane groups of a wave always differ, and 40 envs are no whole number of waves in any group layout."""
import functools

import torch

from marl_mass_amd import _cabi as abi

E, T, SEED = 40, 40, 7
KEYS = ("cbf_eta", "cbf_tau", "HEADWAY_TIME")
# (cbf_eta, cbf_tau, HEADWAY_TIME); set 4 differs from set 0 in the reward's headway term only
SETS = ((0.03125, 0.5, 0.5), (0.5, 0.5, 0.5), (0.03125, 1.2, 0.5), (0.125, 0.8, 1.2), (0.03125, 0.5, 2.5))
# (N, safety_guarantee, qp_solver, n_hdv): 4- / 8- / 2-lane groups, the 6- and 12-lane rotation layouts (N = 6; 12, 11), both
# shields, both QP modes, the general kernels (HDVs)
CASES = ((4, "cbf-cav", "exact", 0), (6, "cbf-avs_cint", "ipm", 0), (8, "cbf-cav", "ipm", 3), (12, "cbf-cav", "exact", 0),
         (2, "cbf-avs_cint", "exact", 0), (11, "cbf-cav", "ipm", 5))
WRONG = (0.9, 3.0, 3.0)  # uniform values no set uses: what an env built with them computes if the planes are not read


def case_id(c):
    return "N%d-%s-%s-hdv%d" % c


def group_of(n_env=E, first_env=0):
    """Parameter set of every env: keyed by the GLOBAL env index, as the RNG streams are."""
    return torch.arange(first_env, first_env + n_env) % len(SETS)


def planes(n_env=E, first_env=0):
    """env_params= for the mixed batch: {key: float64 [n_env]}."""
    g = group_of(n_env, first_env)
    tab = torch.tensor(SETS, dtype=torch.float64)
    return {k: tab[g, p].clone() for p, k in enumerate(KEYS)}


def env_kw(case, uniform=SETS[0], **over):
    """Constructor arguments of an env of `case` whose CONFIG carries the parameter set `uniform`."""
    _, safety, qp, n_hdv = case
    eta, tau, ht = uniform
    kw = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": safety, "HEADWAY_TIME": ht}, cbf_eta=eta, cbf_tau=tau,
              qp_solver=qp, obs_f64=True, seed=SEED, auto_reset=True, n_hdv=n_hdv)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def tape(N, n_env=E, steps=T):
    """[steps] int32 [n_env, N] host tensors, read-only (cached)."""
    g = torch.Generator().manual_seed(3)
    return tuple(torch.randint(0, 5, (n_env, N), dtype=torch.int32, generator=g) for _ in range(steps))


OUT_KEYS = ("agents_rewards", "regional_rewards")


def record(env, step_result):
    """Everything a step leaves behind, as host tensors (first axis of every entry: the env, so that a group or a shard is
    one index): every state plane, the env counters, obs, reward, agents_rewards, regional_rewards, done."""
    obs, reward, done, info = step_result
    r = {"f64": env.f64.cpu().nan_to_num().permute(1, 0, 2).clone(), "u8": env.u8.cpu().permute(1, 0, 2).clone(),
         "env_i32": env.env_i32.cpu().t().clone(), "obs": obs.cpu().clone(), "reward": reward.cpu().clone(),
         "done": done.cpu().clone()}
    for k in OUT_KEYS:
        r[k] = info[k].cpu().clone()
    return r


def run(env, actions, fresh=True):
    if fresh:
        env.reset()
    return [record(env, env.step(a.to(env.device))) for a in actions]


def assert_same(got, want, where, got_idx=None, want_idx=None):
    """Bit equality of two records, optionally on env subsets of either side."""
    for k, x in got.items():
        y = want[k]
        if got_idx is not None:
            x = x[got_idx]
        if want_idx is not None:
            y = y[want_idx]
        assert torch.equal(x, y), (where, k)


def assert_groups(mixed, uniform_runs, where, first_env=0):
    """mixed[t] on the envs of group j == uniform_runs[j][t] on the same (global) envs, for every set j and step t.
    uniform_runs[j]: records of the whole E-env batch under uniform set j."""
    n_env = mixed[0]["reward"].shape[0]
    g = group_of(n_env, first_env)
    for j in range(len(SETS)):
        idx = torch.nonzero(g == j).flatten()
        for t, rec in enumerate(mixed):
            assert_same(rec, uniform_runs[j][t], (where, "set", j, "step", t), idx, idx + first_env)


def envs_that_differ(run_a, run_b, idx):
    """How many of the envs idx differ between two runs in trajectory (any state plane) or agent rewards at some step."""
    diff = torch.zeros(len(idx), dtype=torch.bool)
    for a, b in zip(run_a, run_b):
        diff |= (a["f64"][idx] != b["f64"][idx]).flatten(1).any(1) | (a["u8"][idx] != b["u8"][idx]).flatten(1).any(1)
        diff |= (a["agents_rewards"][idx] != b["agents_rewards"][idx]).flatten(1).any(1)
    return int(diff.sum())


_ORACLE = {}


def oracle_runs(case):
    """Five OracleEnv runs of `case`, one per uniform parameter set, E envs and T steps each, computed once per process in
    the oracle's math mode 1 (include/mm_math.h: the kernels' arithmetic) and never modified.  Checks the precondition that
    keeps the comparison honest: the sets really lead to different results on the envs they are compared on."""
    if case in _ORACLE:
        return _ORACLE[case]
    import oracle_env
    N = case[0]
    oracle_env.set_math_mode(1)
    try:
        runs = []
        for s in SETS:
            env = oracle_env.OracleEnv(E, N, **env_kw(case, s))
            runs.append(run(env, tape(N)))
            env.poll_errors()
            env.close()
    finally:
        oracle_env.set_math_mode(0)
    g = group_of()
    per_group = int((g == 0).sum())
    assert per_group == 8
    if N >= 4:
        for j in range(len(SETS)):
            idx = torch.nonzero(g == j).flatten()
            for k in range(len(SETS)):
                if k != j:
                    n = envs_that_differ(runs[j], runs[k], idx)
                    assert n >= 4, ("sets %d and %d give the same results on %d of group %d's envs" % (j, k, per_group - n, j), case)
    else:  # two vehicles: the eta / tau pairs barely separate; the reward-only set does, everywhere
        idx = torch.nonzero(g == 4).flatten()
        for k in range(4):
            assert envs_that_differ(runs[4], runs[k], idx) == per_group, (k, case)
    _ORACLE[case] = runs
    return runs


def dones(run_, idx=None):
    return int(sum((r["done"] if idx is None else r["done"][idx]).sum() for r in run_))


def group_ext_info_numpy(ext_info, groups):
    """numpy restatement of rollout.group_ext_info: per-group means and counts of evaluate()'s per-env results."""
    import numpy as np
    groups = np.asarray(groups)
    n_g = int(groups.max()) + 1
    out = {"count": np.array([(groups == j).sum() for j in range(n_g)], dtype=np.int64)}
    for k, v in ext_info.items():
        v = np.asarray(v, dtype=np.float64)
        out[k] = np.array([v[groups == j].mean() if (groups == j).any() else np.nan for j in range(n_g)])
    return out
