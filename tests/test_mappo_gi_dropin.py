"""Drop-in proof for MAPPO_GI (shared_network = True), replayed: what the reference's own shared actor-critic learner
(marl/mappo_gi.py) produced on the reference env is reproduced by `compat.make(env_id)` driven the way MAPPO_GI drives it.

The fixtures (tests/golden/mappo_gi_*.npz) were recorded by tools/gen_mappo_gi_dropin.py, which runs MAPPO_GI.interact()
x 6 and MAPPO_GI.evaluation() with the env configured from the case's .ini.  For the two v1 cases the same MAPPO_GI code
was also run on the drop-in (oracle backend) at generation time and drew the identical action sequence; v0prio was recorded
from the reference alone (the oracle had no "priority" supervisor then: its meta says dropin_checked = False) and is replayed
here on both backends -- on the oracle through the supervisor's CPU twin (oracle/mm_oracle.c mm_supervise), on the HIP
backend through the device kernel -- with the supervisor's draws taken from the global numpy stream under the reference's
own learner.  The loop below restates `interact`
and `evaluation` (marl/mappo_gi.py:168-229, 397-520): per-agent forward of the shared policy, np.random.choice on the
global stream, and the bootstrap `action(final_state)` then `policy(final_state, out_type="v")` (:355-395).
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle_env
from golden_util import GOLDEN
from marl_mass_amd import compat
from marl_mass_amd.rollout import ActorCriticNetwork

CPU_CASES = ["v1mass", "v1none", "v0prio"]
CASES = ["v1mass", "v1none", "v0prio"]


def _load(tag):
    z = np.load(os.path.join(GOLDEN, "mappo_gi_%s.npz" % tag))
    return z, json.loads(str(z["meta"])), json.loads(str(z["ext"]))


def _policy(z, meta):
    net = ActorCriticNetwork(meta["n_s"], meta["n_a"], 128, 1, state_split=True)
    net.load_state_dict({k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w_")})
    return net


def _make_env(meta, factory):
    compat.CBFType.GAMMA_B, compat.CBFType.TAU, compat.CBFType.QP_SOLVER = meta["eta"], meta["headway_time"], meta["qp_solver"]
    env = compat.make(meta["env_id"], **({"backend_factory": factory} if factory else {}))
    for k, v in meta["env_config"].items():  # run_mappo.py:145-171: written after construction
        env.config[k] = v
    env.config["seed"] = meta["env_seed"]
    env.seed = meta["env_seed"]
    return env


def _softmax_actions(policy, state):
    """_softmax_action + exploration_action / action (marl/mappo_gi.py:340-377): np.random.choice on the GLOBAL stream."""
    with torch.no_grad():
        p = torch.exp(policy(torch.tensor(np.asarray(state), dtype=torch.float32))).numpy()
    return [int(np.random.choice(np.arange(len(pi)), p=pi)) for pi in p]


def _replay(tag, factory):
    z, meta, ext_ref = _load(tag)
    policy = _policy(z, meta)
    env = _make_env(meta, factory)
    env_state, _ = env.reset()  # MAPPO_GI.__init__ (marl/mappo_gi.py:65)
    gamma, scale, T = meta["reward_gamma"], meta["reward_scale"], meta["roll_out_n_steps"]
    drawn_equal = drawn_total = 0
    for k in range(meta["K"]):
        st_ref, ac_ref, ret_ref = z["ro%d_states" % k], z["ro%d_actions" % k], z["ro%d_returns" % k]
        n_agents = len(env.controlled_vehicles)
        states, rewards, done = [], [], True
        for i in range(T):  # interact(), marl/mappo_gi.py:178-205
            states.append(env_state)
            drawn = _softmax_actions(policy, env_state)
            drawn_equal += int(np.sum(np.array(drawn) == ac_ref[i])); drawn_total += n_agents
            next_state, global_reward, done, info = env.step(tuple(int(a) for a in ac_ref[i]))
            rewards.append(info["regional_rewards"])
            env_state = final_state = next_state
            if done:
                env_state, _ = env.reset()
                break
        assert len(states) == st_ref.shape[0] and done == bool(z["ro%d_done" % k]), (k, len(states), done)
        np.testing.assert_allclose(np.array(states), st_ref, rtol=0, atol=1e-9)
        if done:
            final_value = np.zeros(n_agents)
        else:  # bootstrap: action(final_state) draws, value() reads the shared critic (marl/mappo_gi.py:215-218, :379-395)
            _softmax_actions(policy, final_state)
            with torch.no_grad():
                final_value = policy(torch.tensor(np.asarray(final_state), dtype=torch.float32), out_type="v").numpy()[:, 0]
        r = np.array(rewards) / scale
        ret = np.zeros_like(r)
        for a in range(n_agents):  # _discount_reward
            run = final_value[a]
            for t in reversed(range(len(r))):
                run = run * gamma + r[t, a]
                ret[t, a] = run
        np.testing.assert_allclose(ret, ret_ref, rtol=0, atol=2e-6)  # float32 critic value in the bootstrap
        with torch.no_grad():
            s = torch.tensor(st_ref, dtype=torch.float32).reshape(-1, meta["n_s"])
            lp, v = policy(s).numpy(), policy(s, out_type="v").numpy()
        np.testing.assert_allclose(lp, z["ro%d_logp" % k].reshape(lp.shape), rtol=0, atol=2e-5)
        np.testing.assert_allclose(v[:, 0], z["ro%d_value" % k].reshape(-1), rtol=0, atol=2e-5)
    assert drawn_equal >= 0.98 * drawn_total, (drawn_equal, drawn_total)  # same global stream, same probabilities -> same draws
    # evaluation(), marl/mappo_gi.py:397-520 on a second env object (run_mappo.py uses env_eval)
    ev = _make_env(meta, factory)
    steps, avg_speeds, crash, merge, tspeeds, min_headway = [], [], [], [], [], float("inf")
    for i, seed in enumerate(meta["test_seeds"]):
        state, _ = ev.reset(is_training=False, testing_seeds=seed)
        rew_ref = z["ev%d_rewards" % i]
        step, avg, tsp, done = 0, 0.0, 0.0, False
        while not done:
            acts = _softmax_actions(policy, state)
            state, reward, done, info = ev.step(acts)
            assert abs(reward - rew_ref[step]) <= 1e-9, (i, step, reward, rew_ref[step])
            step += 1
            avg += info["average_speed"]; tsp += info["traffic_speed"]
            min_headway = min(min_headway, info["min_headway"])
        steps.append(step); avg_speeds.append(avg / step); tspeeds.append(tsp / step); crash.append(float(ev.is_crashed()))
        merge.append(info["merge_percent"])
    assert steps == [int(s) for s in ext_ref["steps"]] and crash == [float(c) for c in ext_ref["crash_count"]]
    np.testing.assert_allclose(avg_speeds, ext_ref["avg_speeds"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(tspeeds, ext_ref["traffic_speeds"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(merge, ext_ref["merge_percents"], rtol=0, atol=1e-9)
    assert abs(min_headway - ext_ref["min_headway"]) <= 1e-9
    return meta


@pytest.mark.parametrize("tag", CPU_CASES)
def test_mappo_gi_loop_on_dropin_oracle_backend(tag):
    meta = _replay(tag, lambda **kw: oracle_env.OracleEnv(**kw))
    if meta["dropin_checked"]:  # (v0prio: no cross-check existed at generation time; the replay above is the check)
        assert meta["dropin_vs_reference_max_abs"] <= 1e-9
    else:
        assert tag == "v0prio" and meta["dropin_vs_reference_max_abs"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASES)
def test_mappo_gi_loop_on_dropin_hip_backend(tag):
    """The same replay with the product backend (`marl_mass_amd.compat.make(env_id)`); v0prio steps through the device
    "priority" supervisor, whose draws must leave the global numpy stream where the reference's left it."""
    _replay(tag, None)
