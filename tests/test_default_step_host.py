"""The default mode (qp_solver = "ipm") around the step, on the oracle alone: checkpoint / resume, shards against the whole
batch and configure(qp_solver=...) on a live env.  tests/test_default_step_gpu.py asserts the same properties of the HIP
library with this oracle as its twin; here the twin itself is shown to have them (no GPU involved)."""
import pytest
import torch

import oracle_env
from marl_mass_amd import shard_range
import default_step_util as U

E, N, CASE = 48, 4, ("cbf-cav", 4, 0)  # the size of test_sharding_gloo.py


def _env(count=E, **over):
    return oracle_env.OracleEnv(count, N, **U.env_kw(CASE[0], CASE[2], **over))


def test_default_is_the_interior_point_mode():
    """Leaving qp_solver out runs "ipm" (make_config / BatchedMergeEnv's default): the mode these tests are about."""
    from marl_mass_amd import _cabi as abi
    env = _env()
    assert env.qp_solver == "ipm" and env._cfg.qp_solver == abi.QP_IPM


def test_checkpoint_resume_ipm_oracle():
    """state_dict() after k steps, loaded into a fresh env: the continuation k..T is the uninterrupted one, bit for bit
    (state, obs, reward, done, the QP planes of the trace), with re-spawns and capped QPs after the snapshot."""
    k, T = 25, 50
    acts = U.tape(E, N, T)
    a = _env(trace=True)
    head = U.run(a, acts[:k], trace=True)
    ck = a.state_dict()
    ref = U.run(a, acts[k:], trace=True, fresh=False)
    assert U.respawns(head[-1], ref[-1]) > 0, "no episode ended after the snapshot"
    assert sum(U.capped_qps(r) for r in ref) > 0, "no QP ran to the iteration cap after the snapshot"
    b = _env(trace=True)
    b.load_state_dict(ck)
    for t, (got, want) in enumerate(zip(U.run(b, acts[k:], trace=True, fresh=False), ref)):
        U.assert_same(got, want, ("resumed", k + t))
    a.poll_errors(); b.poll_errors()


def test_two_shards_equal_whole_ipm_oracle():
    """Two shards (first_env keys the RNG streams) against the whole batch, every step; metrics: sums up to
    re-association, counts and the min exactly."""
    T = 60
    acts = U.tape(E, N, T)
    whole = _env()
    mw = whole.enable_metrics()
    ref = U.run(whole, acts)
    assert U.respawns(ref[0], ref[-1]) > 0
    total = torch.zeros(8, dtype=torch.float64)
    total[7] = float("inf")
    for r in range(2):
        first, count = shard_range(E, r, 2)
        sl = slice(first, first + count)
        shard = _env(count, first_env=first)
        m = shard.enable_metrics()
        for t, got in enumerate(U.run(shard, [a[sl].contiguous() for a in acts], first_env=first)):
            U.assert_same(got, ref[t], ("shard", r, t), sl)
        total[:7] += m[:7]
        total[7] = min(float(total[7]), float(m[7]))
        shard.poll_errors()
    U.assert_metrics(total, mw, "shards vs whole")
    assert float(mw[4]) == E * T and float(mw[6]) > 0
    whole.poll_errors()


@pytest.mark.parametrize("plan", sorted(U.SWITCH_PLANS))
def test_configure_switches_the_qp_solver_oracle(plan):
    """configure(qp_solver=...) on a live env: from the switch on, the env continues as one BUILT in the new mode and
    loaded with the state at the switch does -- every leg of exact -> ipm and ipm -> exact -> ipm -- and the two modes do
    give different bits on this tape (the switch is visible)."""
    legs = U.SWITCH_PLANS[plan]
    T = sum(n for _, n in legs)
    acts = U.tape(E, N, T)
    live = _env(qp_solver=legs[0][0])
    recs, snaps = U.switch_run(live, legs, acts)
    t = legs[0][1]
    for (solver, n), ck in zip(legs[1:], snaps):
        built = _env(qp_solver=solver)
        built.load_state_dict(ck)
        for i, got in enumerate(U.run(built, acts[t:t + n], fresh=False)):
            U.assert_same(got, recs[t + i], (plan, solver, t + i))
        t += n
    other = _env(qp_solver="exact" if legs[-1][0] == "ipm" else "ipm")  # the last leg in the other mode: different bits
    other.load_state_dict(snaps[-1])
    last = U.run(other, acts[T - legs[-1][1]:], fresh=False)[-1]
    assert not torch.equal(last["f64"], recs[-1]["f64"]), "exact and ipm agree bit for bit: the switch cannot be seen"
    live.poll_errors()
