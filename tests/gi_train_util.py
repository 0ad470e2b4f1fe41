"""Shared by tests/test_policy_gi_train_host.py and tests/test_policy_gi_train_gpu.py: the objective of MAPPO_GI.train()'s
shared branch (marl/mappo_gi.py:305-339) restated in torch, and the fixtures' loader."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import GOLDEN
from marl_mass_amd.rollout import ActorCriticNetwork

FIXTURES = [(loss, t) for loss in ("mse", "huber") for t in (0, 1)]
GRAD_NAMES = ["fc11.weight", "fc11.bias", "fc12.weight", "fc12.bias", "fc13.weight", "fc13.bias", "fc2.weight", "fc2.bias",
              "actor_linear.weight", "actor_linear.bias", "critic_linear.weight", "critic_linear.bias"]


def load_fixture(loss, t):
    """(arrays, meta) of train t.  p_ (the parameters before agent step 0) and tp_ (the target network) are stored once, as
    train 0's p_: the target of both trains is that initial network, and train 1 starts from train 0's last q."""
    z = dict(np.load(os.path.join(GOLDEN, "gi_train_%s_t%d.npz" % (loss, t))))
    meta = json.loads(str(z["meta"]))
    z0 = z if t == 0 else dict(np.load(os.path.join(GOLDEN, "gi_train_%s_t0.npz" % loss)))
    last = json.loads(str(z0["meta"]))["agent_steps"] - 1
    for k in GRAD_NAMES:
        z["tp_" + k] = z0["p_" + k]
        if t:
            z["p_" + k] = z0["a%d_q_%s" % (last, k)]
    return z, meta


def fixture_net(z, meta, prefix, dtype=torch.float32, device="cpu"):
    net = ActorCriticNetwork(meta["n_s"], meta["n_a"], meta["hidden"], 1, state_split=True)
    net.load_state_dict({k: torch.tensor(z[prefix + k]) for k in GRAD_NAMES})
    return net.to(device=device, dtype=dtype)


def objective(net, obs, actions, returns, old_logp, clip, critic_loss, form, adv_sums=None, valid=None):
    """(actor_loss, critic_loss) of one batch, differentiable w.r.t. net's parameters.

    form "literal":   the reference line by line -- ratio [B] * advantages [B, 1] broadcast to [B, B], th.min, th.mean.
    form "reference": the same objective in O(B) from adv_sums = (S+, S-), the sums of the non-negative / negative advantages.
    form "flat":      per-sample PPO-clip, -mean_j min(r_j A_j, c_j A_j).
    valid: samples with valid == 0 are dropped before anything is computed (B = the number of valid ones)."""
    if valid is not None:
        keep = valid.bool().nonzero().squeeze(1)
        obs, actions, returns, old_logp = obs[keep], actions[keep], returns[keep], old_logp[keep]
    B = obs.shape[0]
    logp = net(obs).gather(1, actions.long().unsqueeze(1)).squeeze(1)  # th.sum(action_log_probs * one_hot, 1)
    values = net(obs, out_type="v")  # [B, 1]
    target = returns.unsqueeze(1)
    ratio = torch.exp(logp - old_logp)
    clipped = torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    if form == "literal":
        advantages = target - values.detach()  # [B, 1]
        surr1, surr2 = ratio * advantages, clipped * advantages  # [B, B]
        assert surr1.shape == (B, B)
        actor = -torch.mean(torch.min(surr1, surr2))
    elif form == "reference":
        sp, sn = adv_sums[0].to(ratio.dtype), adv_sums[1].to(ratio.dtype)
        actor = -(sp * torch.min(ratio, clipped) + sn * torch.max(ratio, clipped)).sum() / float(B) ** 2
    else:
        adv = (target - values.detach()).squeeze(1)
        actor = -torch.mean(torch.min(ratio * adv, clipped * adv))
    critic = F.smooth_l1_loss(values, target) if critic_loss == "huber" else F.mse_loss(values, target)
    return actor, critic


def loss_and_grads(net, *args, **kw):
    """[actor, critic, sum] and the twelve gradients (GRAD_NAMES order) by torch.autograd."""
    for p in net.parameters():
        p.grad = None
    actor, critic = objective(net, *args, **kw)
    loss = actor + critic
    if loss.requires_grad and args[0].shape[0]:
        loss.backward()
    named = dict(net.named_parameters())
    grads = [named[k].grad if named[k].grad is not None else torch.zeros_like(named[k]) for k in GRAD_NAMES]
    return torch.stack([actor.detach(), critic.detach(), loss.detach()]), [g.detach().clone() for g in grads]
