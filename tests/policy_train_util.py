"""Shared by tests/test_policy_train_host.py and tests/test_policy_train_gpu.py: one agent step of MAPPO.train()
(marl/mappo.py:170-201) restated in torch, and the loader of the fixtures recorded from the reference
(tools/gen_golden_mappo_train.py)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import GOLDEN
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork

RUNS = ("mse", "huber", "soft")  # "soft": mse with target_update_steps = 2, target_tau = 0.5 (a soft update after train 1)
FIXTURES = [(run, t) for run in RUNS for t in (0, 1)]
NAMES = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
GRAD_NAMES = ["actor." + k for k in NAMES] + ["critic." + k for k in NAMES]


def _load(run, t, part):
    return dict(np.load(os.path.join(GOLDEN, "mappo_train_%s_t%d_%s.npz" % (run, t, part))))


def load_fixture(run, t):
    """(arrays, meta) of train t of a run: the batch file and the two per-network files merged, keys
    states / actions / returns, a{k}_losses, a{k}_min_shape, a{k}_g_<net>.<name>, a{k}_q_<net>.<name>, and
    p_<net>.<name> / tp_<net>.<name>: the networks / targets before agent step 0 of this train.  The initial networks are
    stored once (train 0's file); the targets of train 0 are those initial networks and train 1 starts from train 0's last q
    with the targets unchanged (no soft update ran after train 0: asserted by the generator).  The "soft" run also has
    after_tp_<net>.<name>, both targets after train 1."""
    z = _load(run, t, "batch")
    meta = json.loads(str(z["meta"]))
    for net in ("actor", "critic"):
        z.update({k: v for k, v in _load(run, t, net).items() if k != "meta"})
    z0 = z if t == 0 else load_fixture(run, 0)[0]
    last = json.loads(str(_load(run, 0, "batch")["meta"]))["agent_steps"] - 1
    for k in GRAD_NAMES:
        z["tp_" + k] = z0["p_" + k] if t == 0 else z0["tp_" + k]
        if t:
            z["p_" + k] = z0["a%d_q_%s" % (last, k)]
    return z, meta


def fixture_nets(z, meta, prefix, dtype=torch.float32, device="cpu"):
    """(actor, critic) from the arrays with the given key prefix ("p_", "tp_", "a0_q_", ...)."""
    actor = ActorNetwork(meta["n_s"], meta["hidden"], meta["n_a"])
    critic = CriticNetwork(meta["n_s"], meta["n_a"], meta["hidden"], 1)
    actor.load_state_dict({k: torch.tensor(z[prefix + "actor." + k]) for k in NAMES})
    critic.load_state_dict({k: torch.tensor(z[prefix + "critic." + k]) for k in NAMES})
    return actor.to(device=device, dtype=dtype), critic.to(device=device, dtype=dtype)


def pre_step_prefix(a):
    return "p_" if a == 0 else "a%d_q_" % (a - 1)


def one_hot(actions, n_a, dtype):
    return F.one_hot(actions.long(), n_a).to(dtype)


def objective(actor, critic, obs, actions, returns, old_logp, clip, critic_loss, form, advantages=None, adv_sums=None, valid=None):
    """(actor_loss, critic_loss) of one agent step, each differentiable w.r.t. its own network.

    advantages [B]: returns - critic_target(s, a), a constant here (it comes from another network).
    form "literal":   the reference line by line -- ratio [B] * advantages [B, 1] broadcast to [B, B], th.min, th.mean.
    form "reference": the same objective in O(B) from adv_sums = (S+, S-), the sums of the non-negative / negative advantages.
    form "flat":      per-sample PPO-clip, -mean_j min(r_j A_j, c_j A_j).
    valid: samples with valid == 0 are dropped before anything is computed (B = the number of valid ones)."""
    if valid is not None:
        keep = valid.bool().nonzero().squeeze(1)
        obs, actions, returns, old_logp = obs[keep], actions[keep], returns[keep], old_logp[keep]
        if advantages is not None:
            advantages = advantages[keep]
    B = obs.shape[0]
    n_a = actor.fc3.weight.shape[0]
    oh = one_hot(actions, n_a, obs.dtype)
    logp = torch.sum(actor(obs) * oh, 1)
    ratio = torch.exp(logp - old_logp)
    clipped = torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    if form == "literal":
        adv = advantages.detach().unsqueeze(1)  # [B, 1]
        surr1, surr2 = ratio * adv, clipped * adv  # [B, B]
        assert surr1.shape == (B, B)
        actor_loss = -torch.mean(torch.min(surr1, surr2))
    elif form == "reference":
        sp, sn = adv_sums[0].to(ratio.dtype), adv_sums[1].to(ratio.dtype)
        actor_loss = -(sp * torch.min(ratio, clipped) + sn * torch.max(ratio, clipped)).sum() / float(B) ** 2
    else:
        adv = advantages.detach()
        actor_loss = -torch.mean(torch.min(ratio * adv, clipped * adv))
    values = critic(obs, oh)  # [B, 1]
    target = returns.unsqueeze(1)
    critic_loss_v = F.smooth_l1_loss(values, target) if critic_loss == "huber" else F.mse_loss(values, target)
    return actor_loss, critic_loss_v


def loss_and_grads(actor, critic, *args, **kw):
    """[actor, critic] losses and the twelve gradients (GRAD_NAMES order) by torch.autograd."""
    nets = (actor, critic)
    for net in nets:
        for p in net.parameters():
            p.grad = None
    la, lc = objective(actor, critic, *args, **kw)
    if args[0].shape[0] and (kw.get("valid") is None or bool(kw["valid"].any())):
        la.backward()
        lc.backward()
    else:
        la, lc = torch.zeros_like(la), torch.zeros_like(lc)
    grads = []
    for net in nets:
        named = dict(net.named_parameters())
        grads += [named[k].grad.detach().clone() if named[k].grad is not None else torch.zeros_like(named[k]) for k in NAMES]
    return torch.stack([la.detach(), lc.detach()]), grads


def sums_of(adv):
    return torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])
