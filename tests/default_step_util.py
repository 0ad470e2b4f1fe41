"""Shared pieces of the default-mode (qp_solver = "ipm") tests: test_default_step_gpu.py drives the HIP library, in both
forms of its interior-point step, test_default_step_host.py drives the oracle alone.

Every env here is merge-multi-agent-v1, shielded, eta = 0.03125, tau = 0.5, auto-reset on, and is stepped from reset() with
the suite's lane-change-heavy tape (generator seed 3, env seed 515: candidate-B commits and capped QPs from step ~11 on).
No episode ends by itself within 60 steps of a reset (T = 100, the shield prevents the crashes), so `start()` puts every env
at a phase of its episode of its own -- the STEPS counter, keyed by the GLOBAL env index as the RNG streams are -- and envs
reach T, finish and re-spawn all through the window (test_full_size_bit_exact_vs_oracle starts mid-episode the same way)."""
import functools

import torch

from marl_mass_amd import _cabi as abi

P_LC = (0.3, 0.2, 0.3, 0.1, 0.1)
TRACE_PLANES = ("QP_ROWS", "QP_D", "STATUS", "SAFE_ACC")  # the IPM's iterate, its status and what was integrated
# (safety, N, n_hdv): MASS in 8-lane groups; HSS in 4-lane groups; the general kernels (HDVs); the 6-lane rotation layout
# (10 envs per wave: the running layout's wave count is not the power-of-two layout's)
CASES = [("cbf-cav", 8, 0), ("cbf-avs_cint", 4, 0), ("cbf-cav", 7, 3), ("cbf-cav", 6, 0)]
FORMS = {"fused": 4, "split": 8}  # debug_flags: bit2 keeps the fused kernel, bit3 forces the phase + sweep launches


def case_id(c):
    return "%s-N%d-hdv%d" % c


def env_kw(safety, n_hdv=0, seed=515, **over):
    """Constructor arguments of a default-mode env; qp_solver is left out on purpose: the default is what runs."""
    kw = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": safety, "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, cbf_tau=0.5,
              obs_f64=True, seed=seed, auto_reset=True, n_hdv=n_hdv)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def tape(E, N, steps, seed=3):
    """[steps] int32 [E, N] host tensors; read-only (cached)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.tensor(P_LC)
    return tuple(torch.multinomial(p, E * N, True, generator=g).view(E, N).int() for _ in range(steps))


def phases(count, first_env=0):
    return ((torch.arange(first_env, first_env + count, dtype=torch.int64) * 37) % 90).to(torch.int32)


def start(env, first_env=0):
    """reset() + a phase of the episode per env (see the module docstring)."""
    env.reset()
    env.env_i32[abi.EP["STEPS"]] = phases(env.E, first_env).to(env.device)
    return env


def record(env, step_result=None, trace=False):
    """Everything a step leaves behind, as host tensors: state planes, counters, and (given step()'s return) obs / reward /
    done; the trace planes the interior-point QP shows in."""
    r = {"u8": env.u8.cpu().clone(), "env_i32": env.env_i32.cpu().clone(), "f64": env.f64.cpu().nan_to_num()}
    if step_result is not None:
        obs, reward, done = step_result[:3]
        r.update(obs=obs.cpu().clone(), reward=reward.cpu().clone(), done=done.cpu().clone())
    if trace:
        for name in TRACE_PLANES:
            r["trace." + name] = env.trace[:, abi.T[name]].cpu().nan_to_num(nan=-7.0)
        r["_commits_b"] = candidate_b_commits(env)  # (keys with "_": the record's own bookkeeping, not compared)
    return r


def assert_same(a, b, where, sl=None):
    """Bit equality of two records on the keys both carry; sl: b is a whole batch and a the shard of envs sl."""
    for k in a:
        if k not in b or k.startswith("_"):
            continue
        y = b[k]
        if sl is not None:
            y = y[sl] if k in ("obs", "reward", "done") else y[:, sl]  # (planes and trace planes: [plane or sub-step, E, ...])
        assert torch.equal(a[k], y), (where, k)


def capped_qps(rec):
    """QPs of a record's trace that ran to the iteration cap: status 'ran' without 'is_optimal'."""
    st = rec["trace.STATUS"].clamp(min=0).to(torch.int64)
    return int(((st & (abi.ST_RAN | abi.ST_IS_OPTIMAL)) == abi.ST_RAN).sum())


def candidate_b_commits(env):
    """Vetoes that re-steer in the last step: the integrated steering differs from the nominal command (needs trace=True)."""
    tr = env.trace
    return int((tr[:, abi.T["SAFE_STEER"]].nan_to_num() != tr[:, abi.T["ACT_STEER"]].nan_to_num()).sum())


def respawns(before, after):
    """Envs whose EPISODE counter moved between two records."""
    return int((after["env_i32"][abi.EP["EPISODE"]] > before["env_i32"][abi.EP["EPISODE"]]).sum())


def run(env, actions, trace=False, first_env=0, fresh=True):
    """Step `env` through `actions` (host tensors) and return one record per step."""
    if fresh:
        start(env, first_env)
    out = []
    for a in actions:
        out.append(record(env, env.step(a.to(env.device)), trace))
    return out


SWITCH_PLANS = {"exact-ipm": (("exact", 10), ("ipm", 20)), "ipm-exact-ipm": (("ipm", 10), ("exact", 5), ("ipm", 20))}


def switch_run(env, plan, actions, trace=False):
    """`env` was built with plan[0]'s solver; before every later leg configure(qp_solver=...) switches the live handle.
    Returns (one record per step, the state_dict() taken right before each switch)."""
    start(env)
    recs, snaps, t = [], [], 0
    for leg, (solver, n) in enumerate(plan):
        if leg:
            snaps.append(env.state_dict())
            env.configure(qp_solver=solver)
        recs += run(env, actions[t:t + n], trace, fresh=False)
        t += n
    return recs, snaps


def host_metric_sums(steps):
    """The 8 rollout metrics (the kernel's metrics block) from per-step outputs, on the host in float64 with
    math.fsum: steps is a list of info-like dicts of host tensors (reward, done, crashed [E, N], average_speed,
    traffic_speed, merge_percent, min_headway).  [0] reward, [1] episodes that ended with a crashed vehicle, [2] average speed,
    [3] traffic speed, [4] env-steps, [5] merge percent of the finished episodes, [6] finished episodes, [7] min headway."""
    import math
    cols = [[] for _ in range(8)]
    for s in steps:
        done = s["done"].bool()
        cols[0] += s["reward"].tolist()
        cols[1].append(float((done & s["crashed"].bool().any(-1)).sum()))
        cols[2] += s["average_speed"].tolist()
        cols[3] += s["traffic_speed"].tolist()
        cols[4].append(float(done.numel()))
        cols[5] += s["merge_percent"][done].tolist()
        cols[6].append(float(done.sum()))
        cols[7].append(float(s["min_headway"].min()))
    return torch.tensor([math.fsum(c) for c in cols[:7]] + [min(cols[7])], dtype=torch.float64)


def assert_metrics(got, want, where):
    """Counts (crashed episodes, env-steps, finished episodes) and the min exactly; the four re-associated sums to the
    project's rtol = 1e-12."""
    got, want = got.cpu(), want.cpu()
    assert torch.equal(got[[1, 4, 6, 7]], want[[1, 4, 6, 7]]), (where, got.tolist(), want.tolist())
    assert torch.allclose(got[:7], want[:7], rtol=1e-12, atol=0), (where, got.tolist(), want.tolist())


_ORACLE_RUNS = {}


def oracle_run(case, E, steps, math_mode):
    """The oracle's records of the shared tape for `case` at E envs (with trace), computed once per process and never
    modified: the ground truth every HIP run of that shape is compared with.  math_mode: what oracle_env.set_math_mode was
    given by the caller (1: include/mm_math.h, the kernels' arithmetic) -- part of the key, the records depend on it."""
    import oracle_env
    safety, N, n_hdv = case
    key = (case, E, math_mode)
    have = _ORACLE_RUNS.get(key)
    if have is None or len(have) < steps:
        env = oracle_env.OracleEnv(E, N, trace=True, **env_kw(safety, n_hdv))
        start(env)
        have = [record(env, env.step(a), True) for a in tape(E, N, max(steps, 60))]
        env.poll_errors()  # check_bounds never fired
        # what the shared tape is reused for: candidate-B commits (they invalidate the phase kernel's slot selection), QPs at
        # the iteration cap (the sweep's speculation) and re-spawns, all inside the first 30 steps (the shortest reuse)
        assert sum(r["_commits_b"] for r in have[:30]) > 0 and sum(capped_qps(r) for r in have[:30]) > 0 and respawns(have[0], have[29]) > 0
        _ORACLE_RUNS[key] = have
    return have[:steps]
