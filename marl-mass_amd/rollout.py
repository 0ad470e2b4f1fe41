"""On-device rollout: the batched counterpart of MAPPO.interact / evaluation.

The reference collects experience one env-step at a time on the host (marl/mappo.py:102-158): per
agent a shared actor MLP forward, `np.random.choice` over the softmax, `env.step`, regional rewards
scaled by `reward_scale`, and a discounted return bootstrapped from the critic when the rollout
ends mid-episode (`_discount_reward`, :364-370).  Here the same quantities are produced for E
envs at once with every tensor staying in HBM: observations come straight out of `mm_step`, the
actor forward + categorical sample is ONE launch (`mm_policy_act`: f32-input MFMA, inverse-CDF sampling exactly
as `np.random.choice` does it, Philox uniforms; other actor modules run their own forward followed by
`mm_sample_actions`), and the discounting is a reversed scan over the rollout with episode boundaries taken from
`done`.

The loop is launch-bound once `mm_step` takes < 0.5 ms (about a dozen small launches per policy
step), so `use_graph=True` captures the WHOLE rollout -- T x (policy forward, sample, mm_step,
bookkeeping) + bootstrap + discounting -- into one hipGraph on first use and replays it afterwards
(static output buffers; the env state, the carried observation and the RNG offset advance inside
the graph exactly as they do eagerly).

Networks mirror marl/single_agent/Model_common.py:5-41 (state -> hidden -> hidden -> n_a, log-softmax, hidden 128 or, in the
steer_vel configurations, 512: both have a fused act launch on the device;
critic takes the one-hot action after the first layer) and, for MAPPO_GI with shared_network = True,
marl/single_agent/Model_gi.py:137-216 (ActorCriticNetwork: split first layer, shared trunk, actor and
critic heads; fused on the device as `mm_policy_gi_act`, include/mm_policy_gi.h).

Bank mode: the reference trains one model per configuration and seed; a list of K actors with `group_envs` drives the K
contiguous env groups of one batch, hidden-128 ActorNetworks in ONE launch (`mm_policy_bank_act`, include/mm_policy_bank.h,
on the stacked copies a `PolicyBank` keeps), hidden-128 state-split ActorCriticNetworks likewise (`mm_policy_gi_bank_act`,
include/mm_policy_gi_bank.h, on a `SharedPolicyBank`; the bootstrap value comes from the same launch).
"""
import torch
from torch import nn

from . import _cabi as abi


class ActorNetwork(nn.Module):
    """Model_common.py:5-22."""

    def __init__(self, state_dim, hidden_size, output_size):
        super().__init__()
        self.fc1 = nn.Linear(state_dim, hidden_size)
        self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.fc3 = nn.Linear(hidden_size, output_size)

    def forward(self, state):
        out = torch.relu(self.fc1(state))
        out = torch.relu(self.fc2(out))
        return torch.log_softmax(self.fc3(out), dim=-1)


class CriticNetwork(nn.Module):
    """Model_common.py:25-41."""

    def __init__(self, state_dim, action_dim, hidden_size, output_size=1):
        super().__init__()
        self.fc1 = nn.Linear(state_dim, hidden_size)
        self.fc2 = nn.Linear(hidden_size + action_dim, hidden_size)
        self.fc3 = nn.Linear(hidden_size, output_size)

    def forward(self, state, action_one_hot):
        out = torch.relu(self.fc1(state))
        out = torch.relu(self.fc2(torch.cat([out, action_one_hot], dim=-1)))
        return self.fc3(out)


# Model_gi.py:170-199: the state split reads columns 0..24 as five 5-column blocks, whatever the row width (on
# merge-multi-agent-v1, 6 columns per row, it straddles rows and never reads columns 25..29 -- the reference's behaviour)
SPLIT_COLS = ([5 * b for b in range(5)],
              [5 * b + c for b in range(5) for c in (1, 2)],
              [5 * b + c for b in range(5) for c in (3, 4)])


class ActorCriticNetwork(nn.Module):
    """Model_gi.py:137-216, MAPPO_GI's network with shared_network = True (marl/mappo_gi.py:138-146 builds it with
    state_split=True).  Parameter names are the reference's, so `load_state_dict(checkpoint["model_state_dict"])` of a
    MAPPO_GI checkpoint loads."""

    def __init__(self, state_dim, action_dim, hidden_size, critic_output_size=1, state_split=False):
        super().__init__()
        self.state_split = state_split
        if state_split:
            self.fc11 = nn.Linear(5, hidden_size // 4)
            self.fc12 = nn.Linear(10, hidden_size // 2)
            self.fc13 = nn.Linear(10, hidden_size // 2)
            self.fc2 = nn.Linear(hidden_size // 4 + hidden_size // 2 + hidden_size // 2, hidden_size)
        else:
            self.fc1 = nn.Linear(state_dim, hidden_size)
            self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.actor_linear = nn.Linear(hidden_size, action_dim)
        self.critic_linear = nn.Linear(hidden_size, critic_output_size)
        for k, cols in enumerate(SPLIT_COLS):
            self.register_buffer("_split%d" % (k + 1), torch.tensor(cols, dtype=torch.long), persistent=False)

    def split(self, state):
        """(state1, state2, state3) of Model_gi.py:170-199."""
        return tuple(state.index_select(1, idx) for idx in (self._split1, self._split2, self._split3))

    def trunk(self, state):
        if self.state_split:
            s1, s2, s3 = self.split(state)
            out = torch.cat([torch.relu(self.fc11(s1)), torch.relu(self.fc12(s2)), torch.relu(self.fc13(s3))], 1)
        else:
            out = torch.relu(self.fc1(state))
        return torch.relu(self.fc2(out))

    def forward(self, state, action_mask=None, out_type="p"):
        """out_type "p": log-softmax of the actor head (invalid actions at -1e8, then log_softmax(logits + 1e-8), when a
        mask is given); anything else: the critic head (Model_gi.py:205-216)."""
        out = self.trunk(state)
        if out_type != "p":
            return self.critic_linear(out)
        logits = self.actor_linear(out)
        if action_mask is None:
            return torch.log_softmax(logits, dim=1)
        logits = logits.masked_fill(action_mask == 0, -1e8)
        return torch.log_softmax(logits + 1e-8, dim=1)


def discount_rewards(rewards, dones, final_value, gamma):
    """`_discount_reward` (marl/mappo.py:364-370) over a batch.

    rewards [T, E, N], dones [T, E] (episode ended AT step t), final_value [E, N] (bootstrap for the
    envs whose last step did not end an episode; the reference uses 0 after `done`).
    running = final; for t reversed: running = running * gamma + r[t]; a `done` at step t cuts the
    chain coming from later steps (they belong to the next episode of that env slot)."""
    T = rewards.shape[0]
    out = torch.empty_like(rewards)
    running = final_value.clone()
    for t in range(T - 1, -1, -1):
        running = torch.where(dones[t].bool().unsqueeze(-1), torch.zeros_like(running), running)
        running = running * gamma + rewards[t]
        out[t] = running
    return out


class PolicyBank(object):
    """K ActorNetworks of one shape as six stacked float32 tensors, the operand of mm_policy_bank_act
    (include/mm_policy_bank.h): W1 [K, H, n_s], b1 [K, H], W2 [K, H, H], b2 [K, H], W3 [K, n_a, H], b3 [K, n_a], on the
    members' device.  The stack is a COPY of the members' parameters: refresh() brings it up to date in place (the addresses
    never change, so a captured graph that reads the stack sees what the last refresh() wrote)."""

    NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")

    def __init__(self, actors):
        self.actors = list(actors)
        if not self.actors:
            raise ValueError("a policy bank needs at least one member")
        if len(self.actors) > abi.BANK_MAX_GROUPS:
            raise ValueError("a policy bank has at most %d members, got %d" % (abi.BANK_MAX_GROUPS, len(self.actors)))
        shapes = [tuple(tuple(p.shape) for p in self._params(a)) for a in self.actors]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("the members of a policy bank must have one shape, got %s" % sorted(set(shapes)))
        first = self._params(self.actors[0])
        self.K, self.hidden = len(self.actors), first[2].shape[0]
        self.n_s, self.n_a = first[0].shape[1], first[4].shape[0]
        dev = first[0].device
        self.tensors = [torch.empty((self.K,) + tuple(p.shape), dtype=torch.float32, device=dev) for p in first]
        for name, t in zip(self.NAMES, self.tensors):
            setattr(self, name, t)
        self.params = abi.MMMlpParams(*[t.data_ptr() for t in self.tensors])
        self.refresh()

    @staticmethod
    def _params(a):
        return (a.fc1.weight, a.fc1.bias, a.fc2.weight, a.fc2.bias, a.fc3.weight, a.fc3.bias)

    @torch.no_grad()
    def refresh(self):
        """Copies every member's current parameters into the stack, in place: one launch per stacked tensor."""
        for j, t in enumerate(self.tensors):
            torch.stack([self._params(a)[j].detach().to(t.dtype) for a in self.actors], out=t)


class SharedPolicyBank(object):
    """K state-split hidden-128 ActorCriticNetworks of one shape as twelve stacked float32 tensors in MMGiParams order, the
    operand of mm_policy_gi_bank_act (include/mm_policy_gi_bank.h): W11 [K, 32, 5], b11 [K, 32], W12 [K, 64, 10], b12 [K, 64],
    W13, b13 likewise, W2 [K, 128, 160], b2 [K, 128], Wa [K, n_a, 128], ba [K, n_a], Wc [K, 1, 128], bc [K, 1], on the members'
    device.  A COPY of the members' parameters, as PolicyBank: refresh() brings it up to date in place."""

    NAMES = abi.GI_PARAMS

    def __init__(self, members):
        self.members = list(members)
        if not self.members:
            raise ValueError("a shared policy bank needs at least one member")
        if len(self.members) > abi.BANK_MAX_GROUPS:
            raise ValueError("a shared policy bank has at most %d members, got %d" % (abi.BANK_MAX_GROUPS, len(self.members)))
        if not all(type(m) is ActorCriticNetwork and m.state_split and m.fc2.weight.shape[0] == 128 for m in self.members):
            raise ValueError("the members of a shared policy bank must be state_split ActorCriticNetworks of hidden 128")
        shapes = [tuple(tuple(p.shape) for p in self._params(m)) for m in self.members]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("the members of a shared policy bank must have one shape, got %s" % sorted(set(shapes)))
        first = self._params(self.members[0])
        self.K, self.hidden, self.n_a = len(self.members), first[6].shape[0], first[8].shape[0]
        dev = first[0].device
        self.tensors = [torch.empty((self.K,) + tuple(p.shape), dtype=torch.float32, device=dev) for p in first]
        for name, t in zip(self.NAMES, self.tensors):
            setattr(self, name, t)
        self.params = abi.MMGiParams(*[t.data_ptr() for t in self.tensors])
        self.refresh()

    @staticmethod
    def _params(m):
        return tuple(p for l in (m.fc11, m.fc12, m.fc13, m.fc2, m.actor_linear, m.critic_linear) for p in (l.weight, l.bias))

    @torch.no_grad()
    def refresh(self):
        """Copies every member's current parameters into the stack, in place: one launch per stacked tensor."""
        for j, t in enumerate(self.tensors):
            torch.stack([self._params(m)[j].detach().to(t.dtype) for m in self.members], out=t)


class DeviceRollout(object):
    """MAPPO.interact for a whole env batch; see the module docstring.

    Bank mode: `actor` a list of K modules (and `critic` None or a list of K critics), `group_envs` the K env counts of the
    contiguous blocks of envs, in env order, that each member drives (they sum to env.E; zeros are allowed) -- the layout of a
    group-major env_params grid, or of K independent training runs stepped as one batch.  act() is then ONE
    mm_policy_bank_act launch when every member is an ActorNetwork of hidden 128 in float32 on the device, `generator` is
    None, `fused_policy` is on and the library has the entry; with ActorCriticNetwork members (state_split, hidden 128) under
    the same conditions it is ONE mm_policy_gi_bank_act launch on `shared_bank`, and the bootstrap's draw + value one more;
    otherwise each member's forward writes its slice of one log-probability buffer and ONE mm_sample_actions draws for the whole
    batch (given the same rows, the same draws).
    `group_index` ([E], for group_ext_info) and group_slice(k) (of the E axis: batch["states"][:, roll.group_slice(k)]) say
    which env belongs to whom."""

    def __init__(self, env, actor, critic=None, roll_out_n_steps=100, reward_gamma=0.99, reward_scale=20.0,
                 reward_type="regionalR", generator=None, use_graph=False, sample_seed=0, fused_policy=True, group_envs=None):
        assert reward_type in ("regionalR", "global_R")  # marl/mappo.py:39
        self.bank_mode, self.bank, self.shared_bank = isinstance(actor, (list, tuple)), None, None
        if self.bank_mode:
            actor, critic = self._init_bank(env, list(actor), critic, group_envs)
        elif group_envs is not None:
            raise ValueError("group_envs belongs to bank mode: pass the members as a list")
        # shared mode (MAPPO_GI, shared_network = True): one ActorCriticNetwork is the actor (out_type "p") and the
        # critic (out_type "v"); pass it as `actor`, with critic None or the same module
        self.shared = isinstance(actor[0] if self.bank_mode else actor, ActorCriticNetwork)
        if self.shared and not self.bank_mode:
            if critic is not None and critic is not actor:
                raise ValueError("an ActorCriticNetwork is its own critic: pass critic=None or the same module")
            critic = None
        self.env, self.actor, self.critic = env, actor, critic
        self.T, self.gamma, self.reward_scale, self.reward_type = roll_out_n_steps, reward_gamma, reward_scale, reward_type
        self.generator = generator
        self.n_a = env.n_a
        self.sample_seed = int(sample_seed) & 0xFFFFFFFFFFFFFFFF
        self.obs, _ = env.reset()
        self.obs = self.obs.clone()
        # fused actor + sampling launch for the reference's ActorNetwork (hidden 128 or 512), and for its state-split
        # ActorCriticNetwork (hidden 128) on the device; anything else goes through the module's own forward
        f32 = all(next(a.parameters()).dtype == torch.float32 for a in (actor if self.bank_mode else [actor]))
        if self.bank_mode and self.shared:
            # mm_policy_gi_bank_act is a HIP-library entry for state-split hidden-128 members; anything else and the CPU oracle
            # take the members' own forwards (self.bank stays None: it is the ActorNetwork stack)
            self.fused_policy = bool(fused_policy) and generator is None and f32 and self.obs.device.type == "cuda" \
                and env.clib.has_policy_gi_bank and len(actor) <= abi.BANK_MAX_GROUPS \
                and all(type(a) is ActorCriticNetwork and a.state_split and a.fc2.weight.shape[0] == 128
                        and a.actor_linear.weight.shape[0] == self.n_a and a.fc2.weight.device == self.obs.device for a in actor)
            if self.fused_policy:
                self.shared_bank = SharedPolicyBank(actor)
        elif self.bank_mode:
            # mm_policy_bank_act is a HIP-library entry at hidden 128; hidden 512 and the CPU oracle take the members' own forwards
            b = self.bank
            self.fused_policy = bool(fused_policy) and b is not None and f32 and b.hidden == 128 and b.W1.device == self.obs.device \
                and self.obs.device.type == "cuda" and env.clib.has_policy_bank
        elif self.shared:
            # mm_policy_gi_act is a HIP-library entry (the CPU oracle has no twin: there the module is the CPU form)
            self.fused_policy = bool(fused_policy) and type(actor) is ActorCriticNetwork and actor.state_split and f32 \
                and actor.fc2.weight.shape[0] == 128 and self.obs.device.type == "cuda"
            if self.fused_policy:
                env.clib.require_policy_gi()
        else:
            # hidden 128: mm_policy_act in both libraries.  hidden 512 (the steer_vel configurations): mm_policy_act forwards
            # to mm_policy_wide_act, a HIP-library entry; on the CPU oracle such an actor goes through the module
            hidden = actor.fc2.weight.shape[0] if type(actor) is ActorNetwork else 0
            wide = hidden == 512 and self.obs.device.type == "cuda" and env.clib.has_policy_wide
            self.fused_policy = bool(fused_policy) and type(actor) is ActorNetwork and f32 and (hidden == 128 or wide)
        self._sample_counter = torch.zeros(1, dtype=torch.int64, device=self.obs.device)  # advanced by mm_sample_actions
        self.use_graph = bool(use_graph)
        if self.use_graph:
            if self.obs.device.type != "cuda":
                raise RuntimeError("use_graph needs the device backend (hipGraph capture)")
            if generator is not None:
                raise ValueError("use_graph samples from the default CUDA generator (captured Philox offset)")
        self._graph, self._static = None, None

    def _init_bank(self, env, actors, critics, group_envs):
        """Bank mode's argument checks and group tables; returns the member lists."""
        K = len(actors)
        if K < 1:
            raise ValueError("bank mode needs at least one member")
        kinds = {isinstance(a, ActorCriticNetwork) for a in actors}
        if len(kinds) != 1:
            raise ValueError("the members are either all ActorCriticNetworks (each its own critic) or none of them is")
        if critics is not None:
            if kinds == {True}:
                raise ValueError("ActorCriticNetwork members are their own critics: pass critic=None")
            if not isinstance(critics, (list, tuple)) or len(critics) != K:
                raise ValueError("bank mode takes critic=None or one critic per member (%d)" % K)
            critics = list(critics)
        if group_envs is None or len(group_envs) != K:
            raise ValueError("group_envs must hold one env count per member (%d)" % K)
        group_envs = [int(e) for e in group_envs]
        if min(group_envs) < 0 or sum(group_envs) != env.E:
            raise ValueError("group_envs must be non-negative and sum to the batch's %d envs, got %s" % (env.E, group_envs))
        # the fused launch's operand: ActorNetwork members only (a ValueError for more than 64 members or differing shapes)
        self.bank = PolicyBank(actors) if all(type(a) is ActorNetwork for a in actors) else None
        self.group_envs = group_envs
        self._env_start = [sum(group_envs[:k]) for k in range(K + 1)]
        self._group_start = (abi.C.c_int64 * (K + 1))(*[e * env.N for e in self._env_start])  # in agents, for the launch
        self.group_index = torch.repeat_interleave(torch.arange(K), torch.tensor(group_envs)).to(env.device)
        return actors, critics

    def group_slice(self, k):
        """The envs of member k, as a slice of the E axis."""
        return slice(self._env_start[k], self._env_start[k + 1])

    def _agent_slices(self, N):
        """(k, slice of the flat [E * N] agent axis) of every non-empty group."""
        return [(k, slice(self._env_start[k] * N, self._env_start[k + 1] * N)) for k in range(len(self.actor))
                if self._env_start[k + 1] > self._env_start[k]]

    def state_dict(self):
        """Resume point of a rollout stream: env batch + carried observation + sampler counter."""
        return {"env": self.env.state_dict(), "obs": self.obs.clone(), "sample_counter": self._sample_counter.clone(),
                "sample_seed": self.sample_seed}

    def load_state_dict(self, d):
        self.env.load_state_dict(d["env"])
        self.obs.copy_(d["obs"].to(self.obs.device))  # in place: with a captured graph self.obs IS its static carry buffer
        self._sample_counter.copy_(d["sample_counter"].to(self._sample_counter.device))
        if int(d["sample_seed"]) != self.sample_seed:
            self.sample_seed = int(d["sample_seed"])
            self._graph, self._static = None, None  # the seed is a kernel argument baked into the capture: re-capture

    @torch.no_grad()
    def act(self, obs, out=None):
        """exploration_action / action (marl/mappo.py:220-236): sample from softmax(actor(obs)).
        out: optional int32 [E, N] buffer (contiguous, on the device) the actions are written to -- a rollout's actions[t]."""
        if out is not None:
            assert out.shape == obs.shape[:2] and out.dtype == torch.int32 and out.device == obs.device and out.is_contiguous()
            return self._act(obs, out.view(-1))
        return self._act(obs, None)

    def _policy_gi(self, obs, actions, value):
        """One mm_policy_gi_act launch on the env's stream (include/mm_policy_gi.h).  actions: int32 [E*N] or None
        (value-only: the sampler's counter is untouched); value: float32 [E*N] or None."""
        a, clib = self.actor, self.env.clib
        E, N, S = obs.shape
        ptr = lambda t: t.detach().contiguous().data_ptr()  # noqa: E731  (nn.Linear parameters are contiguous)
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        clib.check(clib.lib.mm_policy_gi_act(obs.contiguous().data_ptr(), E * N, S, ptr(a.fc11.weight), ptr(a.fc11.bias),
                                             ptr(a.fc12.weight), ptr(a.fc12.bias), ptr(a.fc13.weight), ptr(a.fc13.bias),
                                             ptr(a.fc2.weight), ptr(a.fc2.bias), ptr(a.actor_linear.weight),
                                             ptr(a.actor_linear.bias), ptr(a.critic_linear.weight), ptr(a.critic_linear.bias),
                                             a.fc2.weight.shape[0], self.n_a, self.sample_seed,
                                             self._sample_counter.data_ptr() if actions is not None else None, opt(actions),
                                             None, opt(value), self.env._stream()))

    def _policy_gi_bank(self, obs, actions, value):
        """One mm_policy_gi_bank_act launch on the env's stream (include/mm_policy_gi_bank.h), on the stack
        shared_bank.refresh() keeps.  actions: int32 [E*N]; value: float32 [E*N] or None."""
        b, clib = self.shared_bank, self.env.clib
        E, N, S = obs.shape
        clib.check(clib.lib.mm_policy_gi_bank_act(obs.contiguous().data_ptr(), E * N, S, abi.C.byref(b.params), b.K,
                                                  self._group_start, b.hidden, self.n_a, self.sample_seed,
                                                  self._sample_counter.data_ptr(), actions.data_ptr(),
                                                  None, None if value is None else value.data_ptr(), self.env._stream()))

    def _bank_logp(self, obs):
        """Bank mode without the fused launch: each member's forward on its slice, into one [E*N, n_a] buffer."""
        E, N, S = obs.shape
        flat = obs.reshape(E * N, S).float()
        logp = torch.empty(E * N, self.n_a, dtype=torch.float32, device=obs.device)
        for k, s in self._agent_slices(N):
            logp[s] = self.actor[k](flat[s])
        return logp

    def _act(self, obs, dst):
        E, N, S = obs.shape
        if self.shared_bank is not None and self.generator is None and self.fused_policy and obs.dtype == torch.float32:
            # every group's shared actor-critic forward + sampling in ONE launch (mm_policy_gi_bank_act)
            actions = dst if dst is not None else torch.empty(E * N, dtype=torch.int32, device=obs.device)
            self._policy_gi_bank(obs, actions, None)
            return actions.view(E, N)
        if self.bank is not None and self.generator is None and self.fused_policy and obs.dtype == torch.float32:
            # every group's actor forward + sampling in ONE launch (mm_policy_bank_act on the stack bank.refresh() keeps)
            b, clib = self.bank, self.env.clib
            actions = dst if dst is not None else torch.empty(E * N, dtype=torch.int32, device=obs.device)
            clib.check(clib.lib.mm_policy_bank_act(obs.contiguous().data_ptr(), E * N, S, abi.C.byref(b.params), b.K,
                                                   self._group_start, b.hidden, self.n_a, self.sample_seed,
                                                   self._sample_counter.data_ptr(), actions.data_ptr(), None, self.env._stream()))
            return actions.view(E, N)
        if self.generator is None and self.fused_policy and self.shared and obs.dtype == torch.float32:
            # shared actor-critic forward + sampling in ONE launch (mm_policy_gi_act)
            actions = dst if dst is not None else torch.empty(E * N, dtype=torch.int32, device=obs.device)
            self._policy_gi(obs, actions, None)
            return actions.view(E, N)
        if self.generator is None and self.fused_policy and type(self.actor) is ActorNetwork and obs.dtype == torch.float32:
            # actor forward + sampling in ONE launch (mm_policy_act: f32 MFMA, activations in registers)
            a, clib = self.actor, self.env.clib
            actions = dst if dst is not None else torch.empty(E * N, dtype=torch.int32, device=obs.device)
            ptr = lambda t: t.detach().contiguous().data_ptr()  # noqa: E731  (nn.Linear parameters are contiguous)
            clib.check(clib.lib.mm_policy_act(obs.contiguous().data_ptr(), E * N, S, ptr(a.fc1.weight), ptr(a.fc1.bias),
                                              ptr(a.fc2.weight), ptr(a.fc2.bias), ptr(a.fc3.weight), ptr(a.fc3.bias),
                                              a.fc2.weight.shape[0], self.n_a, self.sample_seed,
                                              self._sample_counter.data_ptr(), actions.data_ptr(), None, self.env._stream()))
            return actions.view(E, N)
        logp = self._bank_logp(obs) if self.bank_mode else self.actor(obs.reshape(E * N, S).float())
        # np.random.choice(n_a, p=softmax) (marl/mappo.py:229) is inverse-CDF sampling: cdf.searchsorted(u, "right").
        if self.generator is None:
            # fused in the library (mm_sample_actions): softmax -> cdf -> search, Philox uniform per agent, one
            # pass over 24 B/agent instead of five elementwise / scan kernels over fp64 temporaries
            logp = logp.contiguous()
            actions = dst if dst is not None else torch.empty(E * N, dtype=torch.int32, device=obs.device)
            clib = self.env.clib
            stream = self.env._stream()
            clib.check(clib.lib.mm_sample_actions(logp.data_ptr(), E * N, self.n_a, self.sample_seed,
                                                  self._sample_counter.data_ptr(), actions.data_ptr(), stream))
            return actions.view(E, N)
        # caller-supplied torch generator: same arithmetic with torch ops
        cdf = logp.exp().double().cumsum(-1)
        cdf = cdf / cdf[:, -1:]
        u = torch.rand(E * N, 1, dtype=torch.float64, device=obs.device, generator=self.generator)
        a = (cdf <= u).sum(-1).clamp_(max=self.n_a - 1).to(torch.int32)
        if dst is not None:
            dst.copy_(a)
            a = dst
        return a.view(E, N)

    @torch.no_grad()
    def interact(self):
        """One rollout of `roll_out_n_steps` policy steps on every env (auto-reset on).
        Returns states [T,E,N,S], actions [T,E,N], discounted returns [T,E,N], dones [T,E] and the
        per-step info means the reference logs (average speed, min headway).  With `use_graph` the
        returned tensors are the graph's static buffers: consume them before the next call."""
        for b in (self.bank, self.shared_bank):
            if b is not None:
                b.refresh()  # outside the capture: a replayed graph reads the stack this call has just updated
        if not self.use_graph:
            return self._interact()
        if self._graph is None:
            dev = self.obs.device
            if not getattr(self, "_warmed", False):
                # first capture only: one eager rollout outside capture (lazy library init, allocator warm-up).  It is a
                # real rollout of the stream (state, RNG counter advance); its tensors are simply not returned.
                self._carry = self.obs  # static input/output of the graph: the observation carried between rollouts
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    self._interact()
                    self._carry.copy_(self.obs)
                    self.obs = self._carry
                torch.cuda.current_stream(dev).wait_stream(side)
                self._warmed = True
            torch.cuda.synchronize(dev)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._static = self._interact()
                self._carry.copy_(self.obs)
            self.obs = self._carry
        self._graph.replay()
        return self._static

    @torch.no_grad()
    def _interact(self):
        env, T = self.env, self.T
        E, N, S = self.obs.shape
        dev = self.obs.device
        states = torch.empty(T + 1, E, N, S, dtype=self.obs.dtype, device=dev)  # slot t + 1 is written by step t itself
        actions = torch.empty(T, E, N, dtype=torch.int32, device=dev)
        rewards = torch.empty(T, E, N, dtype=torch.float64, device=dev)
        dones = torch.empty(T, E, dtype=torch.uint8, device=dev)
        speeds = torch.empty(T, E, dtype=torch.float64, device=dev)
        headways = torch.empty(T, E, dtype=torch.float64, device=dev)
        states[0] = self.obs
        obs = states[0]
        regional = self.reward_type == "regionalR"
        for t in range(T):
            # every per-step quantity lands in its [t] slot straight from the two launches (policy + step): no copy kernels
            a = self.act(obs, out=actions[t])
            slots = {"done": dones[t], "average_speed": speeds[t], "min_headway": headways[t]}
            if regional:
                slots["regional_rewards"] = rewards[t]
            obs, global_reward, _, _ = env.step(a, obs_out=states[t + 1], out=slots)
            if not regional:
                rewards[t] = global_reward.unsqueeze(-1).expand(E, N)
        speed_sum = speeds.sum(0)
        min_headway = headways.min(0).values
        self.obs = obs.clone()
        # bootstrap value for envs still mid-episode (marl/mappo.py:147-150); 0 where the last step ended one
        final_value = torch.zeros(E, N, dtype=torch.float64, device=dev)
        if self.shared_bank is not None and self.generator is None and self.fused_policy and obs.dtype == torch.float32:
            # every group's draw + value in one launch, as the single shared network's branch below
            fa = torch.empty(E * N, dtype=torch.int32, device=dev)
            val = torch.empty(E * N, dtype=torch.float32, device=dev)
            self._policy_gi_bank(obs, fa, val)
            final_value = torch.where(dones[-1].bool().unsqueeze(-1), final_value, val.view(E, N).double())
        elif self.bank_mode:
            # each group's own critic on its slice (torch: ActorNetwork members' critics, and shared members without the fused
            # launch); the final actions are drawn as in act()
            if self.shared or self.critic is not None:
                fa = self.act(obs)
                flat = obs.reshape(E * N, S).float()
                one_hot = (fa.unsqueeze(-1) == torch.arange(self.n_a, device=dev, dtype=fa.dtype)).float().view(E * N, self.n_a)
                val = torch.zeros(E * N, dtype=torch.float64, device=dev)
                for k, s in self._agent_slices(N):
                    v = self.actor[k](flat[s], out_type="v") if self.shared else self.critic[k](flat[s], one_hot[s])
                    val[s] = v.view(-1).double()
                final_value = torch.where(dones[-1].bool().unsqueeze(-1), final_value, val.view(E, N))
        elif self.shared:
            # MAPPO_GI.action(final_state) then .value (marl/mappo_gi.py:371-395): the final actions are drawn (the stream
            # advances as in act()) but the shared critic does not read them
            if self.generator is None and self.fused_policy and obs.dtype == torch.float32:
                fa = torch.empty(E * N, dtype=torch.int32, device=dev)
                val = torch.empty(E * N, dtype=torch.float32, device=dev)
                self._policy_gi(obs, fa, val)  # draw + value in one launch
            else:
                self.act(obs)
                val = self.actor(obs.reshape(E * N, S).float(), out_type="v")
            final_value = torch.where(dones[-1].bool().unsqueeze(-1), final_value, val.view(E, N).double())
        elif self.critic is not None:
            fa = self.act(obs)
            # (not F.one_hot: its device-side range asserts do not survive hipGraph capture)
            one_hot = (fa.unsqueeze(-1) == torch.arange(self.n_a, device=dev, dtype=fa.dtype)).float()
            val = self.critic(obs.reshape(E * N, S).float(), one_hot.view(E * N, self.n_a)).view(E, N).double()
            final_value = torch.where(dones[-1].bool().unsqueeze(-1), final_value, val)
        # reward scaling (:152-153) + _discount_reward (:364-370) in one launch (mm_discount_returns; `discount_rewards`
        # above is the same arithmetic in torch ops, 3 launches per step of the rollout)
        returns = torch.empty_like(rewards)
        clib = env.clib  # (errors the reference raises inside step() are latched on the device: the training loop polls them,
        #                   env.poll_errors(), where it synchronises anyway -- a poll per rollout here would break hipGraph capture)
        clib.check(clib.lib.mm_discount_returns(rewards.data_ptr(), dones.data_ptr(), final_value.contiguous().data_ptr(), T, E, N,
                                                float(self.gamma), float(self.reward_scale), returns.data_ptr(), env._stream()))
        return {"states": states[:T], "actions": actions, "returns": returns, "dones": dones,
                "average_speed": speed_sum / T, "min_headway": min_headway}

    @torch.no_grad()
    def evaluate(self, seeds=None):
        """MAPPO.evaluation (marl/mappo.py:255-361) for a whole batch: every env slot runs ONE evaluation
        episode (its own seed, `env.reset(is_training=False, testing_seeds=seed)` in the reference) to its
        terminal step while the others keep stepping; per-episode results are taken at each env's own end.

        Returns (rewards [T_max, E] with NaN after an episode's end, (vehicle_speed, vehicle_position)
        [T_max, E, N] likewise, ext_info) where ext_info has the reference's keys: steps, avg_speeds,
        crash_count, min_headway (one number, min over all steps of all episodes), traffic_speeds,
        merge_percents -- per env as tensors."""
        env = self.env
        E, N, dev = env.E, env.N, self.obs.device
        missing = [k for k in ("agents_info", "crashed") if k not in env.out]
        if missing:  # MAPPO.evaluation reads info["vehicle_speed"/"vehicle_position"] and env.is_crashed() (:300-330)
            raise ValueError("evaluate() needs the step outputs %s: this env was built with skip_outputs" % ", ".join(missing))
        was_auto = env.auto_reset
        for b in (self.bank, self.shared_bank):
            if b is not None:
                b.refresh()
        # The reference evaluates on a SEPARATE env (env_eval, run_mappo.py:146-171,300-306) and its training env keeps
        # its own seed sequence and in-progress episode.  Here the batch is borrowed: snapshot everything an evaluation
        # touches (state planes, episode counters, per-env RNG seeds, carried observation) and put it back afterwards,
        # so the training stream continues exactly where it was instead of restarting from the test seeds.
        saved_env, saved_obs, saved_counter = env.state_dict(), self.obs.clone(), self._sample_counter.clone()
        env.configure(auto_reset=False)
        try:
            # an evaluation episode is a function of its seed alone (the reference re-seeds the global RNG):
            # restart the per-slot episode counter that the device RNG mixes in
            env.env_i32[abi.EP["EPISODE"]].zero_()
            obs, _ = env.reset(seeds=None if seeds is None else torch.as_tensor(seeds, dtype=torch.int64))
            T = env.T
            nan = float("nan")
            rewards = torch.full((T, E), nan, dtype=torch.float64, device=dev)
            vspeed = torch.full((T, E, N), nan, dtype=torch.float64, device=dev)
            vpos = torch.full((T, E, N), nan, dtype=torch.float64, device=dev)
            alive = torch.ones(E, dtype=torch.bool, device=dev)
            steps = torch.zeros(E, dtype=torch.int32, device=dev)
            speed_sum = torch.zeros(E, dtype=torch.float64, device=dev)
            tspeed_sum = torch.zeros(E, dtype=torch.float64, device=dev)
            crash = torch.zeros(E, dtype=torch.bool, device=dev)
            merge = torch.full((E,), nan, dtype=torch.float64, device=dev)
            min_headway = torch.full((), float("inf"), dtype=torch.float64, device=dev)
            for t in range(T):
                a = self.act(obs)
                obs, reward, done, info = env.step(a)
                rewards[t] = torch.where(alive, reward, rewards[t])
                vspeed[t] = torch.where(alive[:, None], info["agents_info"][..., 2], vspeed[t])
                vpos[t] = torch.where(alive[:, None], info["agents_info"][..., 0], vpos[t])
                steps += alive.int()
                speed_sum += torch.where(alive, info["average_speed"], torch.zeros_like(speed_sum))
                tspeed_sum += torch.where(alive, info["traffic_speed"], torch.zeros_like(tspeed_sum))
                mh = torch.where(alive, info["min_headway"], torch.full_like(info["min_headway"], float("inf")))
                min_headway = torch.minimum(min_headway, mh.min())
                ending = alive & done.bool()
                crash |= ending & info["crashed"].bool().any(-1)  # env.is_crashed() at the episode's end
                merge = torch.where(ending, info["merge_percent"], merge)
                alive = alive & ~done.bool()
                if not bool(alive.any()):  # one host sync per policy step; evaluation is not the hot loop
                    break
            n = steps.clamp(min=1).double()
            ext_info = {"steps": steps, "avg_speeds": speed_sum / n, "crash_count": crash, "min_headway": float(min_headway),
                        "traffic_speeds": tspeed_sum / n, "merge_percents": merge}
            tmax = int(steps.max())
            return rewards[:tmax], (vspeed[:tmax], vpos[:tmax]), ext_info
        finally:
            env.configure(auto_reset=was_auto)
            env.load_state_dict(saved_env)
            # in place: after a graph capture self.obs is the graph's static carry buffer and must stay that tensor
            self.obs.copy_(saved_obs)
            # the sampler's counter as well (the evaluation's own act() calls advanced it): with a stochastic actor the
            # training rollouts after an evaluation are then the ones a twin that never evaluated draws
            self._sample_counter.copy_(saved_counter)


def group_ext_info(ext_info, groups, n_groups=None):
    """Per-group means of evaluate()'s per-env results, for a batch whose envs fall into groups -- the points of a per-env
    cbf_eta / cbf_tau / HEADWAY_TIME grid (VecMergeEnv(env_params=...)), each with several seeds.

    ext_info: evaluate()'s dict; groups: int [E], the group index of every env (0 .. n_groups - 1; n_groups defaults to
    max + 1).  Returns {"count": int64 [G], "steps", "avg_speeds", "crash_rate", "traffic_speeds", "merge_percents": float64 [G]}
    on the device of the inputs: the mean over the group's envs (crash_rate: the fraction of its episodes that ended with a
    crashed vehicle), NaN for a group without envs."""
    groups = torch.as_tensor(groups, device=ext_info["steps"].device).long().flatten()
    G = int(groups.max()) + 1 if n_groups is None else int(n_groups)
    if groups.numel() != ext_info["steps"].numel() or int(groups.min()) < 0 or int(groups.max()) >= G:
        raise ValueError("groups must hold one index in 0..%d per env" % (G - 1))
    count = torch.zeros(G, dtype=torch.int64, device=groups.device).index_add_(0, groups, torch.ones_like(groups))
    out = {"count": count}
    for key, src in (("steps", "steps"), ("avg_speeds", "avg_speeds"), ("crash_rate", "crash_count"),
                     ("traffic_speeds", "traffic_speeds"), ("merge_percents", "merge_percents")):
        v = ext_info[src].to(torch.float64).flatten()
        out[key] = torch.zeros(G, dtype=torch.float64, device=groups.device).index_add_(0, groups, v) / count  # (0 / 0: NaN)
    return out


def idm_evaluation(env, seeds):
    """eval_idm.py:70-160 (idm_evaluation of merge-multi-agent-hdv-v1) for a batch of episodes at once.

    env: a VecMergeEnv of merge-multi-agent-hdv-v1 with one env per seed (E == len(seeds)); every env is spawned from the
    reference's own draws of reset(is_training=False, testing_seeds=seed) (compat.hdv_spawn, the global numpy stream) and
    then stepped with step(None) until every episode has ended.  Returns eval_idm.py's ext_info, one entry per seed:
    steps, avg_speeds, crash_count (any road vehicle crashed, MergeEnvLCHDV.is_crashed), min_headways (max(0, min) over the
    episode), traffic_speeds, merge_percents -- and step_time, which here is the DEVICE time of one batched step of all E
    episodes (seconds, the same value for every entry), not the host time of one env.step."""
    import numpy as np
    from .compat import hdv_spawn, MAX_VEHICLES

    if env.kind != abi.ENV_HDV_V1:
        raise ValueError("idm_evaluation runs merge-multi-agent-hdv-v1, got %r" % (env.env_id,))
    E, N = env.E, env.N
    if len(seeds) != E:
        raise ValueError("one env per seed: E = %d, %d seeds" % (E, len(seeds)))
    x = np.full((E, N), np.nan)
    y, v = np.zeros((E, N)), np.zeros((E, N))
    for e, s in enumerate(seeds):
        xe, ye, ve = hdv_spawn(env.config, int(s))
        if len(xe) > min(N, MAX_VEHICLES):
            raise ValueError("seed %s spawns %d vehicles, the batch has %d slots per env" % (s, len(xe), N))
        x[e, :len(xe)], y[e, :len(xe)], v[e, :len(xe)] = xe, ye, ve
    dev = env.device
    env.configure(auto_reset=False)
    env.set_kinematics(x, y, np.zeros((E, N)), v, n_merge=np.zeros(E, dtype=np.int32), kind=np.where(np.isnan(x), 0, 2))
    f64 = torch.float64
    alive = torch.ones(E, dtype=torch.bool, device=dev)
    steps = torch.zeros(E, dtype=torch.int64, device=dev)
    avg, traffic = torch.zeros(E, dtype=f64, device=dev), torch.zeros(E, dtype=f64, device=dev)
    min_hw = torch.full((E,), float("inf"), dtype=f64, device=dev)
    crashed = torch.zeros(E, dtype=torch.bool, device=dev)
    merge = torch.full((E,), float("nan"), dtype=f64, device=dev)
    timed = dev.type == "cuda"
    if timed:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
    n_steps = 0
    for n_steps in range(1, env.T + 1):  # every episode ends by steps >= T at the latest
        _, _, done, info = env.step(None)
        steps += alive.long()
        avg += torch.where(alive, info["average_speed"], 0.0)
        traffic += torch.where(alive, info["traffic_speed"], 0.0)
        min_hw = torch.where(alive, torch.clamp(torch.minimum(min_hw, info["min_headway"]), min=0.0), min_hw)
        end = alive & done.bool()
        crashed |= end & info["crashed"].bool().any(dim=1)
        merge = torch.where(end, info["merge_percent"], merge)
        alive &= ~done.bool()
        if n_steps % 20 == 0 and not bool(alive.any()):
            break
    if timed:
        t1.record()
        t1.synchronize()
        step_time = t0.elapsed_time(t1) / 1000.0 / n_steps
    else:
        step_time = float("nan")
    env.poll_errors()
    st = steps.cpu().numpy()
    return {"steps": [int(s) for s in st], "avg_speeds": list((avg.cpu().numpy() / st).astype(float)),
            "crash_count": [bool(c) for c in crashed.cpu().numpy()], "step_time": [step_time] * E,
            "min_headways": list(min_hw.cpu().numpy().astype(float)),
            "traffic_speeds": list((traffic.cpu().numpy() / st).astype(float)),
            "merge_percents": list(merge.cpu().numpy().astype(float))}
