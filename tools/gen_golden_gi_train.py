#!/usr/bin/env python3
"""Fixtures of the reference learner's shared-network update (build container only; the reference cannot travel).

Imports the reference's marl/mappo_gi.py under the stand-ins of tools/refshim (as tools/gen_mappo_gi_dropin.py does), fills
MAPPO_GI(shared_network=True)'s memory from three `interact()` calls on merge-multi-agent-v1 with no shield and CAVs only
(the "v1none" case, configs_marl-cav-heading-t_headway-shared-unsafe.ini) and runs `MAPPO_GI.train()` twice:

  train 0  on a fresh target network: ratio = 1 for every sample;
  train 1  after three more `interact()` calls and before any soft update of the target: ratio != 1.

`memory.sample` is made deterministic by seeding Python's `random` right before each train().  Nothing of the reference is
edited: `torch.min`, `F.mse_loss` / `F.smooth_l1_loss`, `Tensor.backward`, `nn.utils.clip_grad_norm_` and the optimiser's
`step` are wrapped from outside while train() runs.  Recorded per agent step k of train t

(tests/golden/gi_train_<critic_loss>_t<t>.npz, one file per train() to stay under the committed-file size limit):

  states [B, n_agents, n_s], actions [B, n_agents], returns [B, n_agents]   the batch as train() views it
  p_<name>          the policy's parameters before agent step 0 of train 0 (step k starts from step k - 1's q: asserted here).
                    Stored once, in the t0 file: it is also the target network of BOTH trains (the same for every agent step,
                    no soft update: asserted here), and train 1 starts from train 0's last q (asserted here) -- tests/
                    gi_train_util.py:load_fixture fills p_ / tp_ in from there.
  a{k}_g_<name>     the gradients after loss.backward(), before clip_grad_norm_
  a{k}_q_<name>     the policy's parameters after the optimiser step
  a{k}_losses       [actor_loss, critic_loss, loss] (float32, as the reference computed them)
  a{k}_min_shape    the shape of th.min's operands (the [B, B] broadcast of ratio [B] * advantages [B, 1])
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
from marl.mappo_gi import MAPPO_GI  # noqa: E402  (the reference's caller)

OUT = gi.OUT
CASE = gi.CASES["v1none"]
T_ROLL, K_INTERACT = 30, 3


def snapshot(module):
    return {k: v.detach().numpy().copy() for k, v in module.named_parameters()}


def run_train(mappo, seed):
    """One MAPPO_GI.train() with everything of interest recorded from outside."""
    F = torch.nn.functional
    rec = {"steps": []}
    cur = {}
    saved = dict(min=torch.min, mse=F.mse_loss, sl1=F.smooth_l1_loss, backward=torch.Tensor.backward,
                 clip=torch.nn.utils.clip_grad_norm_, step=mappo.policy_optimizer.step, sample=mappo.memory.sample)

    def w_sample(n):
        batch = saved["sample"](n)
        rec["batch"] = batch
        return batch

    def w_min(a, b):
        out = saved["min"](a, b)
        cur["min_shape"] = list(out.shape)
        cur["actor"] = float(-torch.mean(out))
        return out

    def w_mse(*a, **k):
        out = saved["mse"](*a, **k)
        cur["critic"] = float(out)
        return out

    def w_sl1(*a, **k):
        out = saved["sl1"](*a, **k)
        cur["critic"] = float(out)
        return out

    def w_backward(self, *a, **k):
        cur["loss"] = float(self)
        cur["p"] = snapshot(mappo.policy)
        cur["tp"] = snapshot(mappo.policy_target)
        return saved["backward"](self, *a, **k)

    def w_clip(params, *a, **k):
        cur["g"] = {k_: v.grad.detach().numpy().copy() for k_, v in mappo.policy.named_parameters()}
        return saved["clip"](params, *a, **k)

    def w_step(*a, **k):
        out = saved["step"](*a, **k)
        cur["q"] = snapshot(mappo.policy)
        rec["steps"].append(dict(cur))
        cur.clear()
        return out

    random.seed(seed)
    torch.min, F.mse_loss, F.smooth_l1_loss = w_min, w_mse, w_sl1
    torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = w_backward, w_clip
    mappo.policy_optimizer.step, mappo.memory.sample = w_step, w_sample
    try:
        mappo.train()
    finally:
        torch.min, F.mse_loss, F.smooth_l1_loss = saved["min"], saved["mse"], saved["sl1"]
        torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = saved["backward"], saved["clip"]
        mappo.policy_optimizer.step, mappo.memory.sample = saved["step"], saved["sample"]
    b, N = rec["batch"], mappo.n_agents
    rec["states"] = np.array(b.states, dtype=np.float64).reshape(-1, N, mappo.state_dim).astype(np.float32)
    rec["actions"] = np.array(b.actions, dtype=np.float64).reshape(-1, N, mappo.action_dim).argmax(-1).astype(np.int32)
    rec["returns"] = np.array(b.rewards, dtype=np.float64).reshape(-1, N).astype(np.float32)
    return rec


def main():
    os.makedirs(OUT, exist_ok=True)
    cfg = CASE["cfg"]
    for critic_loss in ("mse", "huber"):
        cvxopt.solvers.mode = "exact"
        env = gi.configure(gym.make(CASE["env_id"]), cfg, seed=0)
        torch.manual_seed(1234)
        mappo = MAPPO_GI(env=env, state_dim=env.n_s, action_dim=env.n_a, memory_capacity=10000, roll_out_n_steps=T_ROLL,
                         reward_gamma=0.99, reward_scale=20.0, use_cuda=False, traffic_density=cfg["traffic_density"],
                         reward_type="regionalR", shared_network=True, test_seeds="0", max_steps=None, critic_loss=critic_loss)
        for t in range(2):
            for _ in range(K_INTERACT):
                mappo.interact()
            n_eps = int(mappo.n_episodes)
            soft = n_eps % mappo.target_update_steps == 0 and n_eps > 0
            assert not soft, "a soft update would run inside this train(): pick other rollout lengths"
            rec = run_train(mappo, seed=100 + t)
            arrays = dict(states=rec["states"], actions=rec["actions"], returns=rec["returns"])
            if t == 0:
                first = rec["steps"][0]["p"]
                arrays.update({"p_" + name: v for name, v in first.items()})
            else:
                assert all(np.array_equal(v, last_q[name]) for name, v in rec["steps"][0]["p"].items())
            assert all(np.array_equal(v, first[name]) for name, v in rec["steps"][0]["tp"].items())
            last_q = rec["steps"][-1]["q"]
            for k, st in enumerate(rec["steps"]):
                if k:  # train() never touches the target between agent steps here, and step k starts where k - 1 ended
                    assert all(np.array_equal(st["tp"][n], rec["steps"][0]["tp"][n]) for n in st["tp"])
                    assert all(np.array_equal(st["p"][n], rec["steps"][k - 1]["q"][n]) for n in st["p"])
                for grp in ("q", "g"):
                    for name, v in st[grp].items():
                        arrays["a%d_%s_%s" % (k, grp, name)] = v
                arrays["a%d_losses" % k] = np.array([st["actor"], st["critic"], st["loss"]], dtype=np.float32)
                arrays["a%d_min_shape" % k] = np.array(st["min_shape"], dtype=np.int64)
            meta = dict(env_id=CASE["env_id"], ini=CASE["ini"], shield=cfg["safety_guarantee"], env_config=dict(gi.BASE, **cfg),
                        torch_seed=1234, env_seed=0, roll_out_n_steps=T_ROLL, interacts_per_train=K_INTERACT, train_index=t,
                        critic_loss=critic_loss, clip_param=float(mappo.clip_param), lr=float(mappo.actor_lr),
                        optimizer_type=mappo.optimizer_type, max_grad_norm=float(mappo.max_grad_norm),
                        target_tau=float(mappo.target_tau), target_update_steps=int(mappo.target_update_steps),
                        batch_size=int(mappo.batch_size), n_s=int(env.n_s), n_a=int(env.n_a), hidden=128, state_split=True,
                        shared_network=True, n_agents=int(mappo.n_agents), batch=int(rec["states"].shape[0]), n_episodes=n_eps,
                        agent_steps=len(rec["steps"]), sample_seed=100 + t,
                        param_names=[k for k, _ in mappo.policy.named_parameters()],
                        note="recorded from the reference's MAPPO_GI.train() (shared_network=True, CPU, float32) on the "
                             "reference env; train_index 0 runs on a fresh target (ratio = 1), 1 before any soft update")
            path = os.path.join(OUT, "gi_train_%s_t%d.npz" % (critic_loss, t))
            np.savez_compressed(path, meta=json.dumps(meta), **arrays)
            size = os.path.getsize(path)
            assert size <= 1000 * 1024, (path, size)
            print("%s: batch %d x %d agents, %d agent steps, n_episodes %d, %d bytes"
                  % (os.path.basename(path), meta["batch"], meta["n_agents"], meta["agent_steps"], n_eps, size))


if __name__ == "__main__":
    main()
