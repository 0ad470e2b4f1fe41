#!/usr/bin/env python3
"""Fixtures of the reference learner's separate actor / critic update (build container only; the reference cannot travel).

Imports the reference's marl/mappo.py under the stand-ins of tools/refshim (as tools/gen_mappo_dropin.py does), fills MAPPO's
memory from three `interact()` calls on merge-multi-agent-v1 with no shield and CAVs only (the "v1none" case of
tools/gen_mappo_gi_dropin.py) and runs `MAPPO.train()` twice:

  train 0  on fresh targets: ratio = 1 on agent step 0 only (the actor moves after every agent step, its target does not);
  train 1  after three more `interact()` calls.

Three runs: critic_loss "mse" and "huber" with the reference's defaults (target_update_steps 5: no soft update inside either
train), and "soft": mse with target_update_steps = 2, target_tau = 0.5, where train 1 (n_episodes == 2) ends with the soft
update of both targets and the blended targets are recorded too.

`memory.sample` is made deterministic by seeding Python's `random` right before each train().  Nothing of the reference is
edited: `torch.min`, `F.smooth_l1_loss`, `nn.MSELoss.forward`, `Tensor.backward`, `nn.utils.clip_grad_norm_` and both
optimisers' `step` are wrapped from outside while train() runs.  Recorded per agent step k of train t, three files per train
to stay under the committed-file size limit (tests/golden/mappo_train_<run>_t<t>_{batch,actor,critic}.npz):

  batch:   states [B, n_agents, n_s], actions [B, n_agents], returns [B, n_agents]   the batch as train() views it
           a{k}_losses      [actor_loss, critic_loss] (float32, as the reference computed them)
           a{k}_min_shape   the shape of th.min's operands (the [B, B] broadcast of ratio [B] * advantages [B, 1])
  <net>:   p_<net>.<name>        the network before agent step 0 of train 0 (t0 files only).  It is also the target of train 0,
                                 and of train 1 (no soft update after train 0); train 1 starts from train 0's last q; step k
                                 starts from step k - 1's q; the targets are constant inside a train(): all asserted here.
           a{k}_g_<net>.<name>   the gradients after backward(), before clip_grad_norm_
           a{k}_q_<net>.<name>   the parameters after that network's optimiser step
           after_tp_<net>.<name> ("soft" run, t1 files) the target after train 1's soft update
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_mappo_gi_dropin as gi  # noqa: E402  (puts the reference, the shims and this repo on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import gym  # noqa: E402
import cvxopt  # noqa: E402
from marl.mappo import MAPPO  # noqa: E402  (the reference's caller)

OUT = gi.OUT
CASE = gi.CASES["v1none"]
T_ROLL, K_INTERACT = 30, 3
RUNS = {"mse": dict(critic_loss="mse"), "huber": dict(critic_loss="huber"),
        "soft": dict(critic_loss="mse", target_update_steps=2, target_tau=0.5)}


def snapshot(module):
    return {k: v.detach().numpy().copy() for k, v in module.named_parameters()}


def grads(module):
    return {k: v.grad.detach().numpy().copy() for k, v in module.named_parameters()}


def run_train(mappo, seed):
    """One MAPPO.train() with everything of interest recorded from outside."""
    F = torch.nn.functional
    rec = {"steps": []}
    cur = {}
    saved = dict(min=torch.min, mse=torch.nn.MSELoss.forward, sl1=F.smooth_l1_loss, backward=torch.Tensor.backward,
                 clip=torch.nn.utils.clip_grad_norm_, astep=mappo.actor_optimizer.step, cstep=mappo.critic_optimizer.step,
                 sample=mappo.memory.sample)

    def w_sample(n):
        batch = saved["sample"](n)
        rec["batch"] = batch
        return batch

    def w_min(a, b):
        out = saved["min"](a, b)
        cur["min_shape"] = list(out.shape)
        cur["actor_loss"] = float(-torch.mean(out))
        return out

    def w_mse(self, *a, **k):
        out = saved["mse"](self, *a, **k)
        cur["critic_loss"] = float(out)
        return out

    def w_sl1(*a, **k):
        out = saved["sl1"](*a, **k)
        cur["critic_loss"] = float(out)
        return out

    def w_backward(self, *a, **k):
        if "p" not in cur:  # the actor's backward: the state before this agent step
            cur["p"] = {"actor": snapshot(mappo.actor), "critic": snapshot(mappo.critic)}
            cur["tp"] = {"actor": snapshot(mappo.actor_target), "critic": snapshot(mappo.critic_target)}
        return saved["backward"](self, *a, **k)

    def w_clip(params, *a, **k):
        net = "critic" if "actor" in cur.get("g", {}) else "actor"  # train() clips the actor first
        cur.setdefault("g", {})[net] = grads(getattr(mappo, net))
        return saved["clip"](params, *a, **k)

    def w_astep(*a, **k):
        out = saved["astep"](*a, **k)
        cur.setdefault("q", {})["actor"] = snapshot(mappo.actor)
        return out

    def w_cstep(*a, **k):
        out = saved["cstep"](*a, **k)
        cur["q"]["critic"] = snapshot(mappo.critic)
        rec["steps"].append(dict(cur))
        cur.clear()
        return out

    random.seed(seed)
    torch.min, torch.nn.MSELoss.forward, F.smooth_l1_loss = w_min, w_mse, w_sl1
    torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = w_backward, w_clip
    mappo.actor_optimizer.step, mappo.critic_optimizer.step, mappo.memory.sample = w_astep, w_cstep, w_sample
    try:
        mappo.train()
    finally:
        torch.min, torch.nn.MSELoss.forward, F.smooth_l1_loss = saved["min"], saved["mse"], saved["sl1"]
        torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = saved["backward"], saved["clip"]
        mappo.actor_optimizer.step, mappo.critic_optimizer.step, mappo.memory.sample = saved["astep"], saved["cstep"], saved["sample"]
    b, N = rec["batch"], mappo.n_agents
    rec["states"] = np.array(b.states, dtype=np.float64).reshape(-1, N, mappo.state_dim).astype(np.float32)
    rec["actions"] = np.array(b.actions, dtype=np.float64).reshape(-1, N, mappo.action_dim).argmax(-1).astype(np.int32)
    rec["returns"] = np.array(b.rewards, dtype=np.float64).reshape(-1, N).astype(np.float32)
    rec["after_tp"] = {"actor": snapshot(mappo.actor_target), "critic": snapshot(mappo.critic_target)}
    return rec


def same(a, b):
    return all(np.array_equal(a[net][k], b[net][k]) for net in a for k in a[net])


def save(name, meta, arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    size = os.path.getsize(path)
    assert size <= 1000 * 1024, (path, size)
    return size


def main():
    os.makedirs(OUT, exist_ok=True)
    cfg = CASE["cfg"]
    for run, kw in RUNS.items():
        cvxopt.solvers.mode = "exact"
        env = gi.configure(gym.make(CASE["env_id"]), cfg, seed=0)
        torch.manual_seed(1234)
        mappo = MAPPO(env=env, state_dim=env.n_s, action_dim=env.n_a, memory_capacity=10000, roll_out_n_steps=T_ROLL,
                      reward_gamma=0.99, reward_scale=20.0, use_cuda=False, traffic_density=cfg["traffic_density"],
                      reward_type="regionalR", test_seeds="0", max_steps=None, **kw)
        for t in range(2):
            for _ in range(K_INTERACT):
                mappo.interact()
            n_eps = int(mappo.n_episodes)
            soft = n_eps % mappo.target_update_steps == 0 and n_eps > 0
            assert soft == (run == "soft" and t == 1), (run, t, n_eps)
            rec = run_train(mappo, seed=100 + t)
            steps = rec["steps"]
            assert len(steps) == mappo.n_agents
            if t == 0:
                first = steps[0]["p"]
                assert same(steps[0]["tp"], first)  # fresh targets
            else:
                assert same(steps[0]["p"], last_q) and same(steps[0]["tp"], first)  # no soft update after train 0
            last_q = steps[-1]["q"]
            for k, st in enumerate(steps):
                if k:  # the targets are constant inside a train(), and step k starts where k - 1 ended
                    assert same(st["tp"], steps[0]["tp"]) and same(st["p"], steps[k - 1]["q"])
                assert list(st["min_shape"]) == [rec["states"].shape[0]] * 2
            # the soft update runs once, after the loop: before it the targets are still the initial networks
            assert same(rec["after_tp"], first) != soft
            meta = dict(env_id=CASE["env_id"], ini="configs_marl-cav-unsafe.ini", shield=cfg["safety_guarantee"],
                        env_config=dict(gi.BASE, **cfg), torch_seed=1234, env_seed=0, roll_out_n_steps=T_ROLL,
                        interacts_per_train=K_INTERACT, train_index=t, run=run, critic_loss=mappo.critic_loss,
                        clip_param=float(mappo.clip_param), actor_lr=float(mappo.actor_lr), critic_lr=float(mappo.critic_lr),
                        optimizer_type=mappo.optimizer_type, max_grad_norm=float(mappo.max_grad_norm),
                        target_tau=float(mappo.target_tau), target_update_steps=int(mappo.target_update_steps),
                        batch_size=int(mappo.batch_size), n_s=int(env.n_s), n_a=int(env.n_a), hidden=128, shared_network=False,
                        n_agents=int(mappo.n_agents), batch=int(rec["states"].shape[0]), n_episodes=n_eps, agent_steps=len(steps),
                        sample_seed=100 + t, soft_update_after_train=bool(soft),
                        param_names=[k for k, _ in mappo.actor.named_parameters()],
                        note="recorded from the reference's MAPPO.train() (CPU, float32) on the reference env; train_index 0 runs "
                             "on fresh targets, 1 on targets the networks have moved away from")
            arrays = dict(states=rec["states"], actions=rec["actions"], returns=rec["returns"])
            for k, st in enumerate(steps):
                arrays["a%d_losses" % k] = np.array([st["actor_loss"], st["critic_loss"]], dtype=np.float32)
                arrays["a%d_min_shape" % k] = np.array(st["min_shape"], dtype=np.int64)
            sizes = [save("mappo_train_%s_t%d_batch.npz" % (run, t), meta, arrays)]
            for net in ("actor", "critic"):
                arrays = {}
                if t == 0:
                    arrays.update({"p_%s.%s" % (net, name): v for name, v in first[net].items()})
                if soft:
                    arrays.update({"after_tp_%s.%s" % (net, name): v for name, v in rec["after_tp"][net].items()})
                for k, st in enumerate(steps):
                    for grp in ("q", "g"):
                        for name, v in st[grp][net].items():
                            arrays["a%d_%s_%s.%s" % (k, grp, net, name)] = v
                sizes.append(save("mappo_train_%s_t%d_%s.npz" % (run, t, net), meta, arrays))
            print("mappo_train_%s_t%d: batch %d x %d agents, n_episodes %d, soft update %s, %s bytes"
                  % (run, t, meta["batch"], meta["n_agents"], n_eps, soft, sizes))


if __name__ == "__main__":
    main()
