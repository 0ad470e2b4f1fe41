"""The learners on the device.  `PPOLearner` (below `SharedPPOLearner`) is plain MAPPO's (marl/mappo.py:161-206): separate actor
and critic, their targets and two optimisers, with both losses and both parameter gradients taken by one library call
(`mm_policy_train`, include/mm_policy_train.h) and the targets evaluated by `mm_policy_eval`; with hidden-512 networks (the
steer_vel configurations) the same two calls are `mm_policy_wide_train` / `mm_policy_wide_eval` (include/mm_policy_wide_train.h).

`SharedPPOLearner` is the learner of MAPPO_GI with shared_network = True on the device: `MAPPO_GI.train()` (marl/mappo_gi.py:232-352, the shared
branch :305-352) with the loss and the full parameter gradient taken by one library call (`mm_policy_gi_train`,
include/mm_policy_gi_train.h) instead of torch autograd.

What the library does: the network forward on every sample, the PPO-clip and critic losses, and the backward into all twelve
parameter tensors, deterministically (no floating-point atomics).  The end of the agent step -- `clip_grad_norm_`, the
optimiser arithmetic (RMSprop / Adam on 22 982 parameters) and the soft target update -- is torch by default, a few dozen
launches on 90 KB; with `fused_step=True` it is ONE library call (`mm_opt_step`, include/mm_opt_step.h) with torch's
arithmetic, the optimiser state in tensors the learner owns and Adam's step count on the device, which makes train()
capturable in a graph.  The fused step reads the gradients without scaling them: `.grad` keeps what the gradient kernels
wrote, where torch's `clip_grad_norm_` leaves the clipped gradient there.

The reference's actor loss is kept literally.  There `ratio` has shape [B] and `advantages = returns - values.detach()` has
shape [B, 1], so `ratio * advantages` broadcasts to [B, B]: every sample's ratio is weighted by EVERY sample's advantage,
-mean_{i,j} min(r_j A_i, clip(r_j) A_i) = -(1 / B^2) sum_j [S+ min(r_j, c_j) + S- max(r_j, c_j)] with S+ / S- the sums of the
non-negative / negative advantages.  `form="reference"` computes exactly that (it is what the reference's checkpoints were
trained with, and tests/golden/gi_train_*.npz pin it to the reference's own run); `form="flat"` is textbook per-sample
PPO-clip on all B * N samples in one optimiser step.

The gradient kernels keep 2 496 B (shared network) / 2 240 B (separate networks; 8 384 B at hidden 512) of scratch per sample.
With `scratch_budget_bytes` a learner never holds more than that: a call whose unchunked scratch does not fit takes the same
gradient of ONE loss over all its samples with `mm_policy_gi_train_chunked` / `mm_policy_train_chunked` /
`mm_policy_wide_train_chunked` (hidden 512), in passes through the rows of the largest chunk that fits -- still one optimiser
step, the same losses bit for bit.

With `shard_group` (a torch.distributed process group, or "world") a learner trains on a batch that is SHARDED over ranks, as the
rollout's envs are: every agent step of train() takes the gradient of ONE loss over all ranks' samples.  Each rank runs
`shard_block` on its own samples (`mm_policy_gi_train_partial` / `mm_policy_train_partial`, hidden 512:
`mm_policy_wide_train_partial`: the chunked entry's passes into a caller-visible fp64 block, scaled by the whole batch's count), the R blocks are gathered in rank order and `finish_shards`
(`mm_policy_*_train_finish`) folds them in that order on every rank: the same bits from the same blocks, so replicas that start
equal stay bit-equal without a broadcast (`replicas_in_sync()` checks it).  Both phases are public and need no process group.
At hidden 512 a block is 4.9 MB per rank and agent step, and one pass of a whole shard is 8 384 bytes per sample: a sharded
learner there wants `scratch_budget_bytes`.  Limit: a sharded train() is not graph-capturable (it runs collectives).

`BankPPOLearner` (at the end) is K `PPOLearner(fused_step=True)`s of one shape as one learner, for the K env groups of a bank-mode
`DeviceRollout`: stacked storage that the member modules alias, and per agent step one `mm_policy_bank_eval`, one
`mm_policy_bank_train` (include/mm_policy_bank_train.h) and one `mm_opt_step_bank` whatever K is.  `SharedBankPPOLearner` is
the same for K `SharedPPOLearner(fused_step=True)`s -- the `*-shared` configurations -- on `mm_policy_gi_bank_eval` /
`mm_policy_gi_bank_train` (include/mm_policy_gi_bank_train.h).
"""
import copy
import ctypes as C

import torch

from . import _cabi as abi
from .rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork

PARAM_ORDER = ("fc11", "fc12", "fc13", "fc2", "actor_linear", "critic_linear")  # MMGiParams' order: weight, bias of each


def _params(net):
    out = []
    for name in PARAM_ORDER:
        m = getattr(net, name)
        out += [m.weight, m.bias]
    return out


def _optimizer_class(optimizer_type):
    if optimizer_type not in ("adam", "rmsprop"):
        raise ValueError("optimizer_type must be 'rmsprop' or 'adam', got %r" % (optimizer_type,))
    return torch.optim.Adam if optimizer_type == "adam" else torch.optim.RMSprop


OPT_ALGO = {"rmsprop": abi.OPT_RMSPROP, "adam": abi.OPT_ADAM}
_STATE_KEYS = {"rmsprop": ("square_avg",), "adam": ("exp_avg", "exp_avg_sq")}


def optimizer_state_to_torch(optimizer_type, param_groups, step, state1, state2=None):
    """The fused step's optimiser state -> torch.optim's own state_dict(): {"state": {i: {"step", "square_avg"} or {"step",
    "exp_avg", "exp_avg_sq"}}, "param_groups": param_groups}.  `step` (an int: every parameter of a network has taken the same
    number of steps) is stored as torch stores it, a float32 0-dim CPU tensor per parameter; the state tensors are cloned.  A
    network that has taken no step has an empty "state", as a fresh torch optimiser has."""
    keys = _STATE_KEYS[optimizer_type]
    state = {}
    if step > 0:
        for i, tensors in enumerate(zip(*([state1, state2][:len(keys)]))):
            state[i] = {"step": torch.tensor(float(step), dtype=torch.float32)}
            state[i].update({k: t.detach().clone() for k, t in zip(keys, tensors)})
    return {"state": state, "param_groups": copy.deepcopy(param_groups)}


def optimizer_state_from_torch(state_dict, optimizer_type, n_params):
    """torch.optim's state_dict() of an RMSprop / Adam with torch's defaults -> (step, state1, state2): the common step count
    as an int and the lists of n_params state tensors (None where torch has no state yet: zeros; state2 is None for RMSprop).
    ValueError for what the fused step does not implement (momentum, centred, amsgrad) or parameters at different steps."""
    keys = _STATE_KEYS[optimizer_type]
    state = state_dict["state"]
    if sum(len(g["params"]) for g in state_dict["param_groups"]) != n_params or any(i not in range(n_params) for i in state):
        raise ValueError("the state dict is not that of an optimiser over %d parameters" % n_params)
    steps, out = set(), [[None] * n_params for _ in keys]
    for i in range(n_params):
        st = state.get(i, {})
        extra = set(st) - set(keys) - {"step"}
        if extra:
            raise ValueError("optimiser state %s is not supported by the fused step" % sorted(extra))
        if st and set(keys) - set(st):
            raise ValueError("the state dict is not a torch.optim %s state: parameter %d lacks %s"
                             % (optimizer_type, i, sorted(set(keys) - set(st))))
        steps.add(int(st["step"]) if st else 0)
        for j, k in enumerate(keys):
            out[j][i] = st.get(k)
    if len(steps) > 1:
        raise ValueError("the fused step keeps one step count per network, the state dict has %s" % sorted(steps))
    return (steps.pop() if steps else 0), out[0], (out[1] if len(keys) > 1 else None)


class _FusedOptimizer(object):
    """One network's optimiser for mm_opt_step: the state in tensors allocated here, once (nothing is allocated under graph
    capture), and the MMOptGroup that points at parameters, state and targets.  Hyperparameters are read from the torch
    optimiser's param_groups at every step (that object is kept for them and for the state-dict format; it never steps)."""

    def __init__(self, optimizer_type, optimizer, params, targets, grad_norm):
        if len(params) > abi.OPT_MAX_TENSORS:
            raise ValueError("mm_opt_step takes at most %d tensors per network" % abi.OPT_MAX_TENSORS)
        self.optimizer_type, self.optimizer, self.params, self.targets = optimizer_type, optimizer, params, targets
        new = lambda p: torch.zeros_like(p, memory_format=torch.contiguous_format)  # noqa: E731
        self.state1 = [new(p) for p in params]
        self.state2 = [new(p) for p in params] if optimizer_type == "adam" else None
        self.step = torch.zeros(1, dtype=torch.int32, device=params[0].device)
        g = self.group = abi.MMOptGroup()
        g.algo, g.n_tensors = OPT_ALGO[optimizer_type], len(params)
        for i, (p, t) in enumerate(zip(params, targets)):
            if not p.is_contiguous() or not t.is_contiguous():
                raise ValueError("the fused step needs contiguous parameters")
            g.count[i], g.param[i], g.target[i], g.state1[i] = p.numel(), p.data_ptr(), t.data_ptr(), self.state1[i].data_ptr()
            if self.state2 is not None:
                g.state2[i] = self.state2[i].data_ptr()
        g.step, g.grad_norm = self.step.data_ptr(), grad_norm.data_ptr()

    def fill(self, max_grad_norm, tau, soft_update):
        """The group for one step: current hyperparameters and gradient buffers."""
        g, h = self.group, self.optimizer.param_groups[0]
        for i, p in enumerate(self.params):
            _ensure_grad(p)
            g.grad[i] = p.grad.data_ptr()
        g.lr, g.eps = h["lr"], h["eps"]
        if self.optimizer_type == "adam":
            g.alpha_or_beta1, g.beta2 = h["betas"]
        else:
            g.alpha_or_beta1 = h["alpha"]
        g.max_grad_norm = -1.0 if max_grad_norm is None else max_grad_norm
        g.tau, g.soft_update = tau, int(bool(soft_update))
        return g

    def blend_group(self, tau):
        g = abi.MMOptGroup()
        g.algo, g.n_tensors, g.tau = abi.OPT_BLEND, self.group.n_tensors, tau
        for i in range(g.n_tensors):
            g.count[i], g.param[i], g.target[i] = self.group.count[i], self.group.param[i], self.group.target[i]
        return g

    def state_dict(self):
        return optimizer_state_to_torch(self.optimizer_type, self.optimizer.state_dict()["param_groups"], int(self.step.item()),
                                        self.state1, self.state2)

    def load_state_dict(self, state_dict):
        step, s1, s2 = optimizer_state_from_torch(state_dict, self.optimizer_type, len(self.params))
        self.optimizer.load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})  # (the hyperparameters)
        for mine, theirs in ((self.state1, s1), (self.state2, s2)):
            if mine is not None:
                for m, t in zip(mine, theirs):
                    m.zero_() if t is None else m.copy_(t)  # (in place: the group's pointers stay valid)
        self.step.fill_(step)


def _ensure_grad(p):
    """The library writes the gradients straight into .grad: a contiguous one must exist."""
    if p.grad is None or not p.grad.is_contiguous():
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)


def _batch(states, actions, returns, valid):
    """The preamble of both train(): `DeviceRollout.interact()`'s dict or the three tensors -> states float32 [B, N, S],
    actions int32 [B, N], returns float32 [B, N], valid uint8 [B, N] or None, and N, S."""
    if isinstance(states, dict):
        states, actions, returns = states["states"], states["actions"], states["returns"]
    N, S = states.shape[-2], states.shape[-1]
    states = states.reshape(-1, N, S)
    if states.dtype != torch.float32:
        states = states.float()
    actions = actions.reshape(-1, N)
    if actions.dtype != torch.int32:
        actions = actions.to(torch.int32)
    returns = returns.reshape(-1, N)
    if returns.dtype != torch.float32:
        returns = returns.float()  # (DeviceRollout's returns are float64: converted once)
    if valid is not None:
        valid = valid.reshape(-1, N).to(torch.uint8)
    return states, actions, returns, valid, N, S


def gather_in_rank_order(tensor, group=None):
    """`tensor` of every rank of `group` (None: the default group), stacked in rank order: [R, *tensor.shape] on tensor's device,
    identical on every rank.  On the device where the backend can (nccl, which is RCCL here); under gloo a device tensor goes
    through a host copy, as reduce_rollout_metrics does."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    src = tensor.detach().contiguous()
    if src.is_cuda and "nccl" in str(dist.get_backend(group)):
        out = torch.empty((world,) + tuple(src.shape), dtype=src.dtype, device=src.device)
        dist.all_gather_into_tensor(out, src, group=group)
        return out
    host = src.cpu()
    parts = [torch.empty_like(host) for _ in range(world)]
    dist.all_gather(parts, host, group=group)
    return torch.stack(parts).to(tensor.device)


def fold_rank_sums(packed, with_sums):
    """[R, 3] float64 (each rank's float32 S+, S- and its count of valid samples) -> (the whole batch's float32 [2] adv_sums, or
    None without with_sums; its int32 [1] count), added in rank order: every rank gets the same bits."""
    count = packed[:, 2].sum().to(torch.int32).reshape(1)
    if not with_sums:
        return None, count
    parts = packed[:, :2].to(torch.float32)
    sums = parts[0]
    for r in range(1, parts.shape[0]):
        sums = sums + parts[r]
    return sums, count


class _DeviceLearner(object):
    """What both learners need around a library call: the current stream and a scratch buffer that only grows.
    `scratch_bytes` is the library's size query of the subclass's call, n -> bytes."""

    def __init__(self, clib, device, scratch_bytes):
        self.clib, self.device = clib, device
        self._scratch, self._scratch_bytes = None, scratch_bytes

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _init_fused(self, fused_step, optimizer_type, networks):
        """networks: (torch optimiser, parameters, target's parameters) per network, in the order of the launch's groups.
        Also the clipping norm's home: `last_grad_norm`, float32 [number of networks] on the device."""
        self.fused_step = bool(fused_step)
        self._torch_optimizers = [n[0] for n in networks]
        self._norms = None
        if self.fused_step:
            self.clib.require_opt_step()
            self._grad_norm = torch.zeros(len(networks), dtype=torch.float32, device=self.device)
            self._fused = [_FusedOptimizer(optimizer_type, opt, list(params), list(targets), self._grad_norm[i:i + 1])
                           for i, (opt, params, targets) in enumerate(networks)]

    def _fused_launch(self, soft_update):
        """clip + optimiser step (+ soft update) of every network: one mm_opt_step launch."""
        self.clib.opt_step([f.fill(self.max_grad_norm, self.target_tau, soft_update) for f in self._fused], self._stream())

    @property
    def last_grad_norm(self):
        """The total gradient norm(s) before clipping of the last optimiser step, float32 on the device, one per network
        (fused: written by the launch; torch path: clip_grad_norm_'s return values).  None before the first step and, on
        the torch path, without clipping."""
        if self.fused_step:
            return self._grad_norm
        return None if not self._norms else torch.stack([n.to(torch.float32) for n in self._norms])

    def _state_dicts(self):
        if self.fused_step:
            return [f.state_dict() for f in self._fused]
        return [o.state_dict() for o in self._torch_optimizers]

    def _load_state_dicts(self, state_dicts):
        for target, sd in zip(self._fused if self.fused_step else self._torch_optimizers, state_dicts):
            target.load_state_dict(sd)

    def _ensure_scratch(self, n):
        return self._grow(self._scratch_bytes(n))

    # -- a batch sharded over ranks ------------------------------------------------------------
    def _init_shards(self, shard_group, require_sharded, block_doubles):
        """shard_group None: train() is the single-device one.  A process group or "world" (the default group): every agent
        step of train() is partial + gather + finish over the group's ranks."""
        self.sharded, self._shard_n_s = shard_group is not None, 25
        self._shard_group = None if (shard_group is None or shard_group == "world") else shard_group
        self._require_sharded, self._block_doubles = require_sharded, block_doubles
        if self.sharded:
            require_sharded()

    def shard_doubles(self):
        """K, the length of a shard block in doubles."""
        self._require_sharded()
        return self._block_doubles()

    def _shard_plan(self, n):
        """(chunk, scratch) of shard_block on n samples: _plan's chunk, or one pass (the multiple of 64 at or above n) where
        _plan would take the unchunked entry."""
        chunk, scratch = self._plan(n)
        if chunk is None:
            chunk = max(64, (n + 63) // 64 * 64)
            scratch = self._grow(self._chunked_bytes(n, chunk))
        return chunk, scratch

    def _shard_out(self, out):
        K = self.shard_doubles()
        if out is None:
            return torch.empty(K, dtype=torch.float64, device=self.device)
        if out.dtype != torch.float64 or tuple(out.shape) != (K,) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float64 [%d] tensor on the learner's device" % K)
        return out

    def _shard_blocks(self, blocks):
        K = self.shard_doubles()
        if (blocks.dtype != torch.float64 or blocks.dim() != 2 or blocks.shape[1] != K or not 1 <= blocks.shape[0] <= 64
                or blocks.stride(1) != 1 or (blocks.shape[0] > 1 and blocks.stride(0) < K) or blocks.device != self.device):
            raise ValueError("blocks must be float64 [R, %d] on the learner's device, 1 <= R <= 64, rows contiguous" % K)
        return blocks, max(blocks.stride(0), K)

    def _sharded_grad(self, obs, actions, returns, old_logp, valid=None, adv_sums=None, **kw):
        """One agent step's gradient over all ranks' samples: the local (S+, S-) and count, gathered and added in rank order;
        shard_block on the local samples; the R blocks gathered in rank order; finish_shards."""
        packed = torch.zeros(3, dtype=torch.float64, device=self.device)
        if adv_sums is not None:
            packed[:2] = adv_sums.to(torch.float32).double()
        packed[2] = obs.shape[0] if valid is None else (valid != 0).sum()
        sums, count = fold_rank_sums(gather_in_rank_order(packed, self._shard_group), adv_sums is not None)
        block = self.shard_block(obs, actions, returns, old_logp, count, valid=valid, adv_sums=sums, **kw)
        return self.finish_shards(gather_in_rank_order(block, self._shard_group))

    def _replica_tensors(self):
        raise NotImplementedError

    def replicas_in_sync(self):
        """Whether every rank of the shard group holds the same parameter bytes (the networks and their targets): one gather
        of a 64-bit checksum per rank.  Synchronises with the host.  Without a shard group there is one replica: True."""
        if not self.sharded:
            return True
        words = torch.cat([t.detach().reshape(-1) for t in self._replica_tensors()]).view(torch.int32).to(torch.int64)
        weights = torch.arange(1, words.numel() + 1, dtype=torch.int64, device=words.device) * 0x9E3779B1 + 1
        checksum = ((words + 0x7F4A7C15) * weights).sum().reshape(1)  # (int64 arithmetic wraps: a position-dependent sum)
        every = gather_in_rank_order(checksum, self._shard_group)
        return bool((every == every[0]).all())

    def _grow(self, need):
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)  # (allocate before a graph capture)
        return self._scratch

    def _init_budget(self, scratch_budget_bytes, require_chunked, chunked_bytes):
        """scratch_budget_bytes None: the unchunked entry, whatever it needs.  A budget: the scratch never exceeds it -- the
        unchunked entry where its scratch fits, else the chunked one (`chunked_bytes`: its size query, (n, chunk) -> bytes)
        with the largest chunk that fits.  ValueError for a budget below the smallest pass, 64 samples."""
        self.scratch_budget_bytes = None if scratch_budget_bytes is None else int(scratch_budget_bytes)
        self._chunked_bytes, self._chunks = chunked_bytes, {}
        if self.scratch_budget_bytes is not None:
            require_chunked()
            least = chunked_bytes(64, 64)
            if self.scratch_budget_bytes < least:
                raise ValueError("scratch_budget_bytes=%d is below the %d bytes of the smallest pass (64 samples)"
                                 % (self.scratch_budget_bytes, least))

    def _plan(self, n):
        """(chunk, scratch) of a gradient call on n samples: chunk None for the unchunked entry."""
        budget = self.scratch_budget_bytes
        if budget is None:
            return None, self._ensure_scratch(n)
        if n not in self._chunks:
            need = self._scratch_bytes(n)
            if need <= budget:
                self._chunks[n] = (None, need)
            else:
                if self._chunked_bytes(n, 64) > budget:
                    raise ValueError("scratch_budget_bytes=%d is below the %d bytes %d samples need in passes of 64"
                                     % (budget, self._chunked_bytes(n, 64), n))
                lo, hi = 1, (n + 63) // 64  # the size grows with the chunk: the largest multiple of 64 that fits
                while lo < hi:
                    mid = (lo + hi + 1) // 2
                    lo, hi = (mid, hi) if self._chunked_bytes(n, 64 * mid) <= budget else (lo, mid - 1)
                self._chunks[n] = (64 * lo, self._chunked_bytes(n, 64 * lo))
        chunk, need = self._chunks[n]
        return chunk, self._grow(need)


class SharedPPOLearner(_DeviceLearner):
    """`MAPPO_GI(shared_network=True)`'s policy / policy_target / policy_optimizer and its train(); defaults are
    MAPPO_GI.__init__'s (marl/mappo_gi.py:28-57).  `policy` is a rollout.ActorCriticNetwork(state_split=True), hidden 128,
    float32, on the device -- typically the module a DeviceRollout acts with, so the next rollout uses the updated weights."""

    def __init__(self, policy, clib, lr=1e-4, optimizer_type="rmsprop", clip_param=0.2, critic_loss="mse", max_grad_norm=0.5,
                 target_tau=1.0, target_update_steps=5, fused_step=False, scratch_budget_bytes=None, shard_group=None):
        # (first: a budget no call can meet is refused whatever else is passed)
        self._init_budget(scratch_budget_bytes, clib.require_policy_gi_train_chunked, clib.policy_gi_train_chunked_scratch_bytes)
        self._init_shards(shard_group, clib.require_policy_gi_train_sharded, clib.policy_gi_train_shard_doubles)
        if type(policy) is not ActorCriticNetwork or not policy.state_split or policy.fc2.weight.shape[0] != 128:
            raise ValueError("SharedPPOLearner needs rollout.ActorCriticNetwork(state_split=True) with hidden size 128")
        p0 = policy.fc2.weight
        if p0.dtype != torch.float32 or p0.device.type != "cuda":
            raise ValueError("SharedPPOLearner needs a float32 policy on the device")
        if critic_loss not in abi.GI_CRITIC_LOSS:
            raise ValueError("critic_loss must be 'mse' or 'huber', got %r" % (critic_loss,))
        clib.require_policy_gi()
        clib.require_policy_gi_train()
        _DeviceLearner.__init__(self, clib, p0.device, clib.policy_gi_train_scratch_bytes)
        self.policy = policy
        self.policy_target = copy.deepcopy(policy)
        self.optimizer = _optimizer_class(optimizer_type)(policy.parameters(), lr=lr)
        self.clip_param, self.critic_loss, self.max_grad_norm = float(clip_param), critic_loss, max_grad_norm
        self.target_tau, self.target_update_steps = float(target_tau), int(target_update_steps)
        self.n_a = policy.actor_linear.weight.shape[0]
        for p in policy.parameters():
            _ensure_grad(p)
        # fused_step: clip + optimiser + soft update as one mm_opt_step launch (see the module docstring); self.optimizer
        # then only holds the hyperparameters
        self._init_fused(fused_step, optimizer_type, [(self.optimizer, _params(policy), _params(self.policy_target))])

    def optimizer_state_dict(self):
        """The optimiser's state in torch.optim's state_dict() format, whichever path steps: it loads into either."""
        return self._state_dicts()[0]

    def load_optimizer_state_dict(self, state_dict):
        self._load_state_dicts([state_dict])

    # -- plumbing ----------------------------------------------------------------------------
    def _act(self, net, obs, logp=None, value=None):
        """Value-only mm_policy_gi_act of `net` on contiguous obs [n, S] (nothing sampled)."""
        n, S = obs.shape
        w = [p.detach().data_ptr() for p in _params(net)]
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self.clib.lib.mm_policy_gi_act(obs.data_ptr(), n, S, *w, 128, self.n_a, 0, None, None, opt(logp), opt(value),
                                                       self._stream()))

    def old_log_probs(self, obs, actions):
        """policy_target's log-probability of the taken actions (marl/mappo_gi.py:317-322).  obs [n, S], actions [n]."""
        obs = obs.contiguous()
        logp = torch.empty(obs.shape[0], self.n_a, dtype=torch.float32, device=self.device)
        if obs.shape[0]:
            self._act(self.policy_target, obs, logp=logp)
        return logp.gather(1, actions.long().clamp(0, self.n_a - 1).unsqueeze(1)).squeeze(1)

    def advantage_sums(self, obs, returns, valid=None):
        """[S+, S-] of advantages = returns - policy(obs, "v").detach() (:313-314), float32 [2] on the device."""
        obs = obs.contiguous()
        value = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        if obs.shape[0]:
            self._act(self.policy, obs, value=value)
        adv = returns - value
        if valid is not None:
            adv = torch.where(valid.bool(), adv, torch.zeros_like(adv))
        return torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])

    def _inputs(self, obs, actions, returns, old_logp, valid, adv_sums):
        n, S = obs.shape
        if obs.dtype != torch.float32 or (n and obs.stride(1) != 1):
            raise ValueError("obs must be float32 [n, S] with contiguous rows")
        if actions.dtype != torch.int32 or returns.dtype != torch.float32 or actions.dim() != 1 or returns.dim() != 1:
            raise ValueError("actions must be int32 [n] and returns float32 [n]")
        if actions.shape[0] != n or returns.shape[0] != n or old_logp.shape[0] != n:
            raise ValueError("obs, actions, returns and old_logp must have the same length")
        old_logp = old_logp.to(torch.float32).contiguous()
        if valid is not None:
            valid = valid.to(torch.uint8).contiguous()
        if adv_sums is not None:
            adv_sums = adv_sums.to(torch.float32).contiguous()
        return n, S, old_logp, valid, adv_sums

    def _structs(self, grads):
        """(the parameters' MMGiParams, the gradients' or None)."""
        W, G = abi.MMGiParams(), abi.MMGiParams() if grads else None
        for name, p in zip(abi.GI_PARAMS, _params(self.policy)):
            setattr(W, name, p.detach().data_ptr())
            if grads:
                _ensure_grad(p)
                setattr(G, name, p.grad.data_ptr())
        return W, G

    def loss_and_grad(self, obs, actions, returns, old_logp, valid=None, adv_sums=None, diagnostics=False):
        """The bare launch: writes d(actor_loss + critic_loss)/d(parameter) into every policy parameter's .grad and returns
        the float32 [3] tensor (actor loss, critic loss, their sum); with diagnostics also (logp_taken, value, ratio) [n].
        obs float32 [n, S] (unit column stride, any row stride), actions int32 [n] and returns float32 [n] (any stride),
        old_logp float32 [n], valid uint8 / bool [n] or None.  adv_sums: float32 [2] (S+, S-) for the reference's [B, B]
        objective, None for per-sample PPO-clip (see the module docstring).  Only enqueues work: no host synchronisation.
        With a scratch budget that the unchunked call's scratch exceeds, the same gradient comes from
        mm_policy_gi_train_chunked in passes of the largest chunk that fits."""
        n, S, old_logp, valid, adv_sums = self._inputs(obs, actions, returns, old_logp, valid, adv_sums)
        W, G = self._structs(True)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        diag = [torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(3)] if diagnostics else [None] * 3
        chunk, scratch = self._plan(n)
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        args = (
            obs.data_ptr(), obs.stride(0) if n else S, n, S, actions.data_ptr(), actions.stride(0) if n else 1, returns.data_ptr(),
            returns.stride(0) if n else 1, old_logp.data_ptr(), opt(valid), C.byref(W), self.policy.fc2.weight.shape[0], self.n_a,
            self.clip_param, abi.GI_CRITIC_LOSS[self.critic_loss], opt(adv_sums), C.byref(G), loss.data_ptr(), opt(diag[0]),
            opt(diag[1]), opt(diag[2]), scratch.data_ptr(), scratch.numel(), self._stream())
        if chunk is None:
            self.clib.check(self.clib.lib.mm_policy_gi_train(*args))
        else:
            self.clib.check(self.clib.lib.mm_policy_gi_train_chunked(*args, chunk))
        return (loss, tuple(diag)) if diagnostics else loss

    # -- the two phases of a gradient over rank-sharded batches --------------------------------
    def shard_block(self, obs, actions, returns, old_logp, count, valid=None, adv_sums=None, diagnostics=False, out=None):
        """Phase one, on this rank's samples (mm_policy_gi_train_partial): the float64 [K] shard block on the device (written
        into `out` when given); with diagnostics also (logp_taken, value, ratio) [n].  The inputs are loss_and_grad's, n == 0
        included (an empty shard); `count` is an int32 [1] device tensor holding B, the number of valid samples of the WHOLE
        batch over all ranks, and adv_sums is the whole batch's (S+, S-).  The passes are _plan(n)'s chunk; without a budget, or
        where the unchunked scratch fits it, one pass.  Touches no .grad.  Only enqueues work."""
        self.clib.require_policy_gi_train_sharded()
        n, S, old_logp, valid, adv_sums = self._inputs(obs, actions, returns, old_logp, valid, adv_sums)
        if count.dtype != torch.int32 or count.numel() != 1 or count.device != self.device:
            raise ValueError("count must be an int32 tensor of one element on the learner's device")
        block = self._shard_out(out)
        self._shard_n_s = S
        W, _ = self._structs(False)
        diag = [torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(3)] if diagnostics else [None] * 3
        chunk, scratch = self._shard_plan(n)
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self.clib.lib.mm_policy_gi_train_partial(
            obs.data_ptr(), obs.stride(0) if n else S, n, S, actions.data_ptr(), actions.stride(0) if n else 1, returns.data_ptr(),
            returns.stride(0) if n else 1, old_logp.data_ptr(), opt(valid), C.byref(W), self.policy.fc2.weight.shape[0], self.n_a,
            self.clip_param, abi.GI_CRITIC_LOSS[self.critic_loss], opt(adv_sums), count.data_ptr(), block.data_ptr(), opt(diag[0]),
            opt(diag[1]), opt(diag[2]), scratch.data_ptr(), scratch.numel(), self._stream(), chunk))
        return (block, tuple(diag)) if diagnostics else block

    def finish_shards(self, blocks, n_s=None):
        """Phase two (mm_policy_gi_train_finish): blocks float64 [R, K], the R ranks' shard blocks in rank order.  Writes every
        policy parameter's .grad -- float32 of the blocks' fp64 sum in row order -- and returns the float32 [3] loss tensor of
        loss_and_grad.  Blocks that do not belong together (another B or configuration, local counts that do not add up to
        B) give NaN everywhere.  n_s: the state columns the blocks were built with; None: those of this learner's last
        shard_block."""
        self.clib.require_policy_gi_train_sharded()
        blocks, stride = self._shard_blocks(blocks)
        _, G = self._structs(True)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        n_s = self._shard_n_s if n_s is None else n_s  # (the network reads columns 0..24 whatever S is: only the blocks say)
        self.clib.check(self.clib.lib.mm_policy_gi_train_finish(blocks.data_ptr(), blocks.shape[0], stride, n_s, self.n_a, C.byref(G),
                                                                loss.data_ptr(), self._stream()))
        return loss

    def _replica_tensors(self):
        return _params(self.policy) + _params(self.policy_target)

    def _grad(self, *args, **kw):
        return self._sharded_grad(*args, **kw) if self.sharded else self.loss_and_grad(*args, **kw)

    # -- MAPPO_GI.train() ----------------------------------------------------------------------
    def _step(self, n_episodes):
        soft = n_episodes % self.target_update_steps == 0 and n_episodes > 0  # _soft_update_target (:348-352, :545-547)
        if self.fused_step:
            return self._fused_launch(soft)
        if self.max_grad_norm is not None:
            self._norms = [torch.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)]
        self.optimizer.step()
        if soft:
            with torch.no_grad():
                for t, s in zip(self.policy_target.parameters(), self.policy.parameters()):
                    t.copy_((1.0 - self.target_tau) * t + self.target_tau * s)

    @torch.no_grad()
    def train(self, states, actions=None, returns=None, n_episodes=0, form="reference", valid=None):
        """One call of MAPPO_GI.train() on a batch.

        states [B, N, S] (or [T, E, N, S]: B = T * E), actions [B, N], returns [B, N]; or `DeviceRollout.interact()`'s dict
        as the first argument.  form "reference": for agent_id in order, one optimiser step on the B samples of that agent
        with the reference's [B, B] objective -- N sequential steps, the target's log-probabilities and the advantages taken
        with the parameters as they are at that step, as the reference does.  form "flat": ONE optimiser step on all B * N
        samples with the per-sample PPO-clip objective; `valid` [B, N] masks the empty slots of ragged batches (kind == 0).
        The soft update of the target runs after each optimiser step when n_episodes % target_update_steps == 0 and
        n_episodes > 0.  Returns the list of float32 [3] loss tensors (one per optimiser step); nothing is synchronised."""
        states, actions, returns, valid, N, S = _batch(states, actions, returns, valid)
        losses = []
        if form == "reference":
            for agent_id in range(N):
                obs, act, ret = states[:, agent_id, :], actions[:, agent_id], returns[:, agent_id]
                v = None if valid is None else valid[:, agent_id]
                dense = obs.contiguous()
                old = self.old_log_probs(dense, act)
                sums = self.advantage_sums(dense, ret, v)
                losses.append(self._grad(obs, act, ret, old, valid=v, adv_sums=sums))
                self._step(n_episodes)
        elif form == "flat":
            obs, act, ret = states.reshape(-1, S), actions.reshape(-1), returns.reshape(-1)
            v = None if valid is None else valid.reshape(-1)
            old = self.old_log_probs(obs, act)
            losses.append(self._grad(obs, act, ret, old, valid=v))
            self._step(n_episodes)
        else:
            raise ValueError("form must be 'reference' or 'flat', got %r" % (form,))
        return losses


def _mlp_params(net):
    """MMMlpParams' order: weight, bias of fc1, fc2, fc3."""
    return [net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias, net.fc3.weight, net.fc3.bias]


def _hidden_of(net):
    """The hidden size of an fc1 / fc2 / fc3 network, None for anything else (the constructor's checks refuse that later)."""
    w = getattr(getattr(net, "fc2", None), "weight", None)
    return w.shape[0] if isinstance(w, torch.Tensor) and w.dim() == 2 else None


def _mlp_struct(net, grads=False):
    st = abi.MMMlpParams()
    for name, p in zip(abi.MLP_PARAMS, _mlp_params(net)):
        if grads:
            _ensure_grad(p)
        setattr(st, name, p.grad.data_ptr() if grads else p.detach().data_ptr())
    return st


# hidden size -> the name stem of the library's entries, size queries and require functions for it (mm_<stem>, mm_<stem>_chunked,
# <stem>_chunked_scratch_bytes, require_<stem>_sharded, ...); hidden 128 is "policy_train"
_PT_STEM = {128: "policy_train", 512: "policy_wide_train"}


class PPOLearner(_DeviceLearner):
    """`MAPPO`'s actor / critic / actor_target / critic_target / two optimisers and its train() (marl/mappo.py:70-95, :161-206);
    defaults are MAPPO.__init__'s.  `actor` is a rollout.ActorNetwork and `critic` a rollout.CriticNetwork, both of hidden size 128
    or both 512 (the steer_vel configurations; `mm_policy_wide_train` / `mm_policy_wide_eval`, include/mm_policy_wide_train.h), float32,
    on the device -- typically the modules a DeviceRollout acts with, so the next rollout uses the updated weights.  With
    `scratch_budget_bytes` the scratch never exceeds the budget at either size: a call whose unchunked scratch does not fit runs
    `mm_policy_train_chunked` (hidden 512: `mm_policy_wide_train_chunked`) in passes of the largest multiple of 64 samples that
    fits; a budget below that entry's smallest call (64 samples in one pass: 10.8 MB at hidden 512) is a ValueError.

    Per agent step the reference takes the actor's loss with advantages from the CRITIC TARGET and old log-probabilities from
    the ACTOR TARGET, then the critic's loss; the two read disjoint parameters, so one `mm_policy_train` call returns both
    gradients from the pre-step parameters.  The soft update of both targets runs ONCE per train(), after the agent loop
    (:203-206), not per agent step as in MAPPO_GI."""

    def __init__(self, actor, critic, clib, actor_lr=1e-4, critic_lr=1e-4, optimizer_type="rmsprop", clip_param=0.2,
                 critic_loss="mse", max_grad_norm=0.5, target_tau=1.0, target_update_steps=5, fused_step=False,
                 soft_update_every="train", scratch_budget_bytes=None, shard_group=None):
        # (first: a budget no call can meet is refused whatever else is passed; the smallest pass is that of the hidden size)
        stem = _PT_STEM.get(_hidden_of(actor), "policy_train")  # (a size that is neither is refused below)
        self._init_budget(scratch_budget_bytes, getattr(clib, "require_%s_chunked" % stem), getattr(clib, "%s_chunked_scratch_bytes" % stem))
        self._init_shards(shard_group, getattr(clib, "require_%s_sharded" % stem), getattr(clib, "%s_shard_doubles" % stem))
        if soft_update_every not in ("train", "agent_step"):
            raise ValueError("soft_update_every must be 'train' or 'agent_step', got %r" % (soft_update_every,))
        if type(actor) is not ActorNetwork or type(critic) is not CriticNetwork:
            raise ValueError("PPOLearner needs a rollout.ActorNetwork and a rollout.CriticNetwork")
        n_s, n_a, hid = actor.fc1.weight.shape[1], actor.fc3.weight.shape[0], actor.fc2.weight.shape[0]
        if (hid not in (128, 512) or tuple(actor.fc1.weight.shape) != (hid, n_s) or tuple(actor.fc2.weight.shape) != (hid, hid)
                or tuple(actor.fc3.weight.shape) != (n_a, hid) or tuple(critic.fc1.weight.shape) != (hid, n_s)
                or tuple(critic.fc2.weight.shape) != (hid, hid + n_a) or tuple(critic.fc3.weight.shape) != (1, hid)):
            raise ValueError("PPOLearner needs hidden size 128 or 512, the same in both networks, the same state and action sizes, "
                             "one critic output")
        if not 1 <= n_a <= 8 or not 25 <= n_s <= 32:
            raise ValueError("PPOLearner supports 25..32 state columns and 1..8 actions, got %d and %d" % (n_s, n_a))
        for p in list(actor.parameters()) + list(critic.parameters()):
            if p.dtype != torch.float32 or p.device.type != "cuda":
                raise ValueError(("scratch_budget_bytes is a budget of device memory: " if scratch_budget_bytes is not None else "")
                                 + ("shard_group gathers device blocks: " if shard_group is not None else "")
                                 + "PPOLearner needs float32 networks on the device")
        if critic_loss not in abi.PT_CRITIC_LOSS:
            raise ValueError("critic_loss must be 'mse' or 'huber', got %r" % (critic_loss,))
        opt = _optimizer_class(optimizer_type)
        # the library's entries for this hidden size: (gradient, evaluation, scratch query, the gradient in passes, and the two
        # phases over rank-sharded batches where the library has them: without a shard group nothing requires them)
        chunked = scratch_budget_bytes is not None  # (_init_budget required the entry)
        getattr(clib, "require_" + stem)()
        sharded = getattr(clib, "has_%s_sharded" % stem)
        entry = lambda suffix: getattr(clib.lib, "mm_" + stem + suffix)  # noqa: E731
        self._entries = (entry(""), getattr(clib.lib, "mm_" + stem.replace("train", "eval")), getattr(clib, stem + "_scratch_bytes"),
                         entry("_chunked") if chunked else None, entry("_partial") if sharded else None,
                         entry("_finish") if sharded else None)
        _DeviceLearner.__init__(self, clib, actor.fc1.weight.device, self._entries[2])
        self.actor, self.critic = actor, critic
        self.actor_target, self.critic_target = copy.deepcopy(actor), copy.deepcopy(critic)
        self.actor_optimizer = opt(actor.parameters(), lr=actor_lr)
        self.critic_optimizer = opt(critic.parameters(), lr=critic_lr)
        self.clip_param, self.critic_loss, self.max_grad_norm = float(clip_param), critic_loss, max_grad_norm
        self.target_tau, self.target_update_steps = float(target_tau), int(target_update_steps)
        self.n_s, self.n_a, self.hidden = n_s, n_a, hid
        for p in list(actor.parameters()) + list(critic.parameters()):
            _ensure_grad(p)
        # soft_update_every "train": MAPPO's, once per train(); "agent_step": MAPPO_GI's non-shared branch (marl/mappo_gi.py:
        # 247-304: the same networks and optimisers), both targets blended after EVERY agent step of a train() that updates
        self.soft_update_every = soft_update_every
        # fused_step: both networks' clip + optimiser (+ soft update) as one mm_opt_step launch of two workgroups
        self._init_fused(fused_step, optimizer_type, [
            (self.actor_optimizer, _mlp_params(actor), _mlp_params(self.actor_target)),
            (self.critic_optimizer, _mlp_params(critic), _mlp_params(self.critic_target))])

    def optimizer_state_dict(self):
        """{"actor_optimizer", "critic_optimizer"}: each optimiser's state in torch.optim's state_dict() format, whichever
        path steps: it loads into either."""
        return dict(zip(("actor_optimizer", "critic_optimizer"), self._state_dicts()))

    def load_optimizer_state_dict(self, state_dict):
        self._load_state_dicts([state_dict["actor_optimizer"], state_dict["critic_optimizer"]])

    # -- plumbing ----------------------------------------------------------------------------
    def _check_batch(self, obs, actions):
        n, S = obs.shape
        if obs.dtype != torch.float32 or (n and obs.stride(1) != 1) or S != self.n_s:
            raise ValueError("obs must be float32 [n, %d] with contiguous rows" % self.n_s)
        if actions.dtype != torch.int32 or actions.dim() != 1 or actions.shape[0] != n:
            raise ValueError("actions must be int32 [n]")
        return n, S

    def evaluate(self, obs, actions, actor=None, critic=None, valid=None):
        """The bare mm_policy_eval (hidden 512: mm_policy_wide_eval): (logp_taken, value), float32 [n] each (None for a network that is not given), zeros in
        masked slots.  obs [n, S] with any row stride, actions int32 [n] with any stride."""
        n, S = self._check_batch(obs, actions)
        if valid is not None:
            valid = valid.to(torch.uint8).contiguous()
        logp = torch.empty(n, dtype=torch.float32, device=self.device) if actor is not None else None
        value = torch.empty(n, dtype=torch.float32, device=self.device) if critic is not None else None
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        ref = lambda net: None if net is None else C.byref(_mlp_struct(net))  # noqa: E731
        self.clib.check(self._entries[1](
            obs.data_ptr(), obs.stride(0) if n else S, n, S, actions.data_ptr(), actions.stride(0) if n else 1, opt(valid), ref(actor),
            ref(critic), self.hidden, self.n_a, opt(logp), opt(value), self._stream()))
        return logp, value

    def old_log_probs(self, obs, actions, valid=None):
        """actor_target's log-probability of the taken actions (marl/mappo.py:178-179)."""
        return self.evaluate(obs, actions, actor=self.actor_target, valid=valid)[0]

    def advantages(self, obs, actions, returns, valid=None):
        """returns - critic_target(obs, one_hot(actions)) (:173-174), float32 [n], zeros in masked slots."""
        value = self.evaluate(obs, actions, critic=self.critic_target, valid=valid)[1]
        return self._adv(returns, value, valid)

    @staticmethod
    def _adv(returns, value, valid):
        adv = returns - value
        return adv if valid is None else torch.where(valid.bool(), adv, torch.zeros_like(adv))

    def advantage_sums(self, obs, actions, returns, valid=None):
        """[S+, S-] of those advantages, float32 [2] on the device: what the reference's [B, B] objective depends on."""
        adv = self.advantages(obs, actions, returns, valid)
        return torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])

    def _inputs(self, obs, actions, returns, old_logp, valid, adv_sums, advantages, networks):
        n, S = self._check_batch(obs, actions)
        if networks not in ("both", "actor", "critic"):
            raise ValueError("networks must be 'both', 'actor' or 'critic', got %r" % (networks,))
        if returns.dtype != torch.float32 or returns.dim() != 1 or returns.shape[0] != n or old_logp.shape[0] != n:
            raise ValueError("returns must be float32 [n] and old_logp [n]")
        old_logp = old_logp.to(torch.float32).contiguous()
        if valid is not None:
            valid = valid.to(torch.uint8).contiguous()
        if adv_sums is not None:
            adv_sums = adv_sums.to(torch.float32).contiguous()
        if advantages is not None:
            if advantages.shape[0] != n:
                raise ValueError("advantages must be [n]")
            advantages = advantages.to(torch.float32).contiguous()
        return n, S, old_logp, valid, adv_sums, advantages, networks != "critic", networks != "actor"

    def loss_and_grad(self, obs, actions, returns, old_logp, valid=None, adv_sums=None, advantages=None, diagnostics=False,
                      networks="both"):
        """The bare launch: writes d(actor loss)/d(actor parameter) and d(critic loss)/d(critic parameter) into every
        parameter's .grad and returns the float32 [2] tensor (actor loss, critic loss); with diagnostics also
        (logp_taken, value, ratio) [n].  obs float32 [n, S] (unit column stride, any row stride), actions int32 [n] and returns
        float32 [n] (any stride), old_logp float32 [n], valid uint8 / bool [n] or None.  Exactly one of adv_sums -- float32
        [2] (S+, S-): the reference's [B, B] objective -- and advantages -- float32 [n]: per-sample PPO-clip.  networks
        "both" | "actor" | "critic": the other one's gradient and loss are left out (its .grad is not touched, its loss is 0).
        Only enqueues work: no host synchronisation.  With a scratch budget that the unchunked call's scratch exceeds, the
        same gradients come from mm_policy_train_chunked (hidden 512: mm_policy_wide_train_chunked) in passes of the largest chunk
        that fits."""
        n, S, old_logp, valid, adv_sums, advantages, with_a, with_c = self._inputs(obs, actions, returns, old_logp, valid, adv_sums,
                                                                                    advantages, networks)
        W = [_mlp_struct(self.actor) if with_a else None, _mlp_struct(self.critic) if with_c else None]
        G = [_mlp_struct(self.actor, True) if with_a else None, _mlp_struct(self.critic, True) if with_c else None]
        ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
        loss = torch.empty(2, dtype=torch.float32, device=self.device)
        new = lambda on: torch.empty(n, dtype=torch.float32, device=self.device) if (diagnostics and on) else None  # noqa: E731
        diag = [new(with_a), new(with_c), new(with_a)]
        chunk, scratch = self._plan(n)
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        args = (
            obs.data_ptr(), obs.stride(0) if n else S, n, S, actions.data_ptr(), actions.stride(0) if n else 1, returns.data_ptr(),
            returns.stride(0) if n else 1, old_logp.data_ptr(), opt(valid), ref(W[0]), ref(W[1]), self.hidden, self.n_a, self.clip_param,
            abi.PT_CRITIC_LOSS[self.critic_loss], opt(adv_sums) if with_a else None, opt(advantages) if with_a else None, ref(G[0]),
            ref(G[1]), loss.data_ptr(), opt(diag[0]), opt(diag[1]), opt(diag[2]), scratch.data_ptr(), scratch.numel(), self._stream())
        if chunk is None:
            self.clib.check(self._entries[0](*args))
        else:
            self.clib.check(self._entries[3](*args, chunk))
        return (loss, tuple(diag)) if diagnostics else loss

    # -- the two phases of a gradient over rank-sharded batches --------------------------------
    def shard_block(self, obs, actions, returns, old_logp, count, valid=None, adv_sums=None, advantages=None, diagnostics=False,
                    out=None, networks="both"):
        """Phase one, on this rank's samples (mm_policy_train_partial; hidden 512: mm_policy_wide_train_partial): the float64 [K]
        shard block on the device (written into `out` when given); with diagnostics also (logp_taken, value, ratio) [n].  The inputs are loss_and_grad's, n == 0 included
        (an empty shard); `count` is an int32 [1] device tensor holding B, the number of valid samples of the WHOLE batch over
        all ranks, and adv_sums is the whole batch's (S+, S-).  The passes are _plan(n)'s chunk; without a budget, or where the
        unchunked scratch fits it, one pass (at hidden 512 one pass of a whole shard is 8 384 bytes per sample: a sharded learner
        there wants a budget).  Touches no .grad.  Only enqueues work."""
        self._require_sharded()
        n, S, old_logp, valid, adv_sums, advantages, with_a, with_c = self._inputs(obs, actions, returns, old_logp, valid, adv_sums,
                                                                                    advantages, networks)
        if count.dtype != torch.int32 or count.numel() != 1 or count.device != self.device:
            raise ValueError("count must be an int32 tensor of one element on the learner's device")
        block = self._shard_out(out)
        W = [_mlp_struct(self.actor) if with_a else None, _mlp_struct(self.critic) if with_c else None]
        ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
        new = lambda on: torch.empty(n, dtype=torch.float32, device=self.device) if (diagnostics and on) else None  # noqa: E731
        diag = [new(with_a), new(with_c), new(with_a)]
        chunk, scratch = self._shard_plan(n)
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self._entries[4](
            obs.data_ptr(), obs.stride(0) if n else S, n, S, actions.data_ptr(), actions.stride(0) if n else 1, returns.data_ptr(),
            returns.stride(0) if n else 1, old_logp.data_ptr(), opt(valid), ref(W[0]), ref(W[1]), self.hidden, self.n_a, self.clip_param,
            abi.PT_CRITIC_LOSS[self.critic_loss], opt(adv_sums) if with_a else None, opt(advantages) if with_a else None,
            count.data_ptr(), block.data_ptr(), opt(diag[0]), opt(diag[1]), opt(diag[2]), scratch.data_ptr(), scratch.numel(),
            self._stream(), chunk))
        return (block, tuple(diag)) if diagnostics else block

    def finish_shards(self, blocks, networks="both"):
        """Phase two (mm_policy_train_finish; hidden 512: mm_policy_wide_train_finish): blocks float64 [R, K], the R ranks' shard
        blocks in rank order, K = shard_doubles() (53 798; hidden 512: 608 294, 4.9 MB).  Writes the .grad
        of every parameter of the requested networks -- float32 of the blocks' fp64 sum in row order -- and returns the float32
        [2] loss tensor of loss_and_grad (0 for a network that is not requested).  Blocks that do not belong together (another B
        or configuration, local counts that do not add up to B, a requested network missing from a block) give NaN everywhere."""
        if networks not in ("both", "actor", "critic"):
            raise ValueError("networks must be 'both', 'actor' or 'critic', got %r" % (networks,))
        self._require_sharded()
        blocks, stride = self._shard_blocks(blocks)
        G = [_mlp_struct(self.actor, True) if networks != "critic" else None, _mlp_struct(self.critic, True) if networks != "actor" else None]
        ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
        loss = torch.empty(2, dtype=torch.float32, device=self.device)
        self.clib.check(self._entries[5](blocks.data_ptr(), blocks.shape[0], stride, self.n_s, self.n_a, ref(G[0]), ref(G[1]),
                                         loss.data_ptr(), self._stream()))
        return loss

    def _replica_tensors(self):
        return [p for net in (self.actor, self.critic, self.actor_target, self.critic_target) for p in _mlp_params(net)]

    def _grad(self, *args, **kw):
        return self._sharded_grad(*args, **kw) if self.sharded else self.loss_and_grad(*args, **kw)

    # -- MAPPO.train() -------------------------------------------------------------------------
    def _step(self, soft=False):
        """clip_grad_norm_ + step, the actor's then the critic's (:186-188, :199-201): each its own norm and optimiser; then,
        with soft, the soft update of both targets.  Fused: all of it is one launch."""
        if self.fused_step:
            return self._fused_launch(soft)
        norms = []
        for net, optimizer in ((self.actor, self.actor_optimizer), (self.critic, self.critic_optimizer)):
            if self.max_grad_norm is not None:
                norms.append(torch.nn.utils.clip_grad_norm_(net.parameters(), self.max_grad_norm))
            optimizer.step()
        self._norms = norms
        if soft:
            self.soft_update()

    @torch.no_grad()
    def soft_update(self):
        """_soft_update_target of both targets: t = (1 - tau) t + tau s."""
        if self.fused_step:
            return self.clib.opt_step([f.blend_group(self.target_tau) for f in self._fused], self._stream())
        for target, source in ((self.actor_target, self.actor), (self.critic_target, self.critic)):
            for t, s in zip(target.parameters(), source.parameters()):
                t.copy_((1.0 - self.target_tau) * t + self.target_tau * s)

    @torch.no_grad()
    def train(self, states, actions=None, returns=None, n_episodes=0, form="reference", valid=None):
        """One call of MAPPO.train() on a batch.

        states [B, N, S] (or [T, E, N, S]: B = T * E), actions [B, N], returns [B, N]; or `DeviceRollout.interact()`'s dict
        as the first argument.  form "reference": for agent_id in order, one actor and one critic optimiser step on the B
        samples of that agent with the reference's [B, B] actor objective -- N sequential steps, each on the parameters as
        they then are.  form "flat": ONE step per network on all B * N samples with the per-sample PPO-clip objective;
        `valid` [B, N] masks the empty slots of ragged batches (kind == 0).  The soft update of both targets runs when
        n_episodes % target_update_steps == 0 and n_episodes > 0: once, after the loop (soft_update_every "train"; fused, it
        rides in the launch of the last agent step) or after every agent step ("agent_step").  Returns the list of float32
        [2] loss tensors (one per agent step); nothing is synchronised."""
        states, actions, returns, valid, N, S = _batch(states, actions, returns, valid)
        losses = []
        update = n_episodes % self.target_update_steps == 0 and n_episodes > 0
        every = self.soft_update_every == "agent_step"
        # the soft update a step carries: every step's, or (fused only) the one after the loop in the last step's launch
        carried = lambda last: update and (every or (last and self.fused_step))  # noqa: E731
        if form == "reference":
            for agent_id in range(N):
                obs, act, ret = states[:, agent_id, :], actions[:, agent_id], returns[:, agent_id]
                v = None if valid is None else valid[:, agent_id].contiguous()
                old, value = self.evaluate(obs, act, actor=self.actor_target, critic=self.critic_target, valid=v)
                adv = self._adv(ret, value, v)
                sums = torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])
                losses.append(self._grad(obs, act, ret, old, valid=v, adv_sums=sums))
                self._step(carried(agent_id == N - 1))
        elif form == "flat":
            obs, act, ret = states.reshape(-1, S), actions.reshape(-1), returns.reshape(-1)
            v = None if valid is None else valid.reshape(-1)
            old, value = self.evaluate(obs, act, actor=self.actor_target, critic=self.critic_target, valid=v)
            losses.append(self._grad(obs, act, ret, old, valid=v, advantages=self._adv(ret, value, v)))
            self._step(carried(True))
        else:
            raise ValueError("form must be 'reference' or 'flat', got %r" % (form,))
        if update and not every and not (self.fused_step and losses):
            self.soft_update()
        return losses


class BankPPOLearner(_DeviceLearner):
    """The training half of bank mode: K `PPOLearner(fused_step=True)`s as ONE learner whose launches do not multiply with K.
    `actors` / `critics` are K rollout.ActorNetwork / rollout.CriticNetwork of one shape, hidden 128, float32, on the device --
    typically the members a `DeviceRollout(env, actors, critics, group_envs=...)` acts with; `group_envs` are that rollout's env
    counts (member k trains on `batch[:, roll.group_slice(k)]`).  The hyperparameters are PPOLearner's and are shared by the
    members; the optimiser step is always the fused one.

    The learner owns STACKED storage, member k at index k of the leading axis: parameters, gradients, optimiser state, targets
    (deep copies at construction) and the per-member Adam steps.  At construction every member module's `param.data` and `.grad`
    are re-pointed at views of the stacks, so the modules -- and a DeviceRollout / PolicyBank built on them -- see every update
    with no copy back.

    Per agent step (or once, form "flat") train() issues one `mm_policy_bank_eval` on the stacked targets, one
    `mm_policy_bank_train` (include/mm_policy_bank_train.h) fed the critic targets' values, and one `mm_opt_step_bank`
    (include/mm_opt_step.h).  Member k's parameters, targets and optimiser state are bit for bit those of a K = 1 learner on its
    slice.  Against `PPOLearner` the one difference is the reference form's S+ / S-: torch's float32 sums there, one fp64
    accumulation rounded once here.  ActorCriticNetwork members (MAPPO_GI's shared network) are SharedBankPPOLearner's.  Out of
    scope: hidden 512, scratch budgets and shard groups, per-member hyperparameters."""

    def __init__(self, actors, critics, clib, group_envs, actor_lr=1e-4, critic_lr=1e-4, optimizer_type="rmsprop", clip_param=0.2,
                 critic_loss="mse", max_grad_norm=0.5, target_tau=1.0, target_update_steps=5, soft_update_every="train"):
        actors, critics = list(actors), list(critics)
        K = len(actors)
        if K < 1 or len(critics) != K:
            raise ValueError("BankPPOLearner needs at least one member and one critic per actor")
        if K > abi.BANK_MAX_GROUPS:
            raise ValueError("a policy bank has at most %d members, got %d" % (abi.BANK_MAX_GROUPS, K))
        if any(isinstance(m, ActorCriticNetwork) for m in actors + critics):
            raise ValueError("BankPPOLearner does not train ActorCriticNetwork members (MAPPO_GI's shared network): use "
                             "SharedBankPPOLearner")
        if any(type(a) is not ActorNetwork for a in actors) or any(type(c) is not CriticNetwork for c in critics):
            raise ValueError("BankPPOLearner needs rollout.ActorNetwork and rollout.CriticNetwork members")
        shapes = [tuple(tuple(p.shape) for p in _mlp_params(a) + _mlp_params(c)) for a, c in zip(actors, critics)]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("the members of a bank learner must have one shape, got %d different ones" % len(set(shapes)))
        n_s, n_a, hid = actors[0].fc1.weight.shape[1], actors[0].fc3.weight.shape[0], actors[0].fc2.weight.shape[0]
        if hid != 128:
            raise ValueError("BankPPOLearner trains hidden-128 members only (hidden %d: one PPOLearner per member)" % hid)
        if shapes[0] != ((hid, n_s), (hid,), (hid, hid), (hid,), (n_a, hid), (n_a,), (hid, n_s), (hid,), (hid, hid + n_a), (hid,),
                         (1, hid), (1,)):
            raise ValueError("BankPPOLearner needs the same state and action sizes in actor and critic and one critic output")
        if not 1 <= n_a <= 8 or not 25 <= n_s <= 32:
            raise ValueError("BankPPOLearner supports 25..32 state columns and 1..8 actions, got %d and %d" % (n_s, n_a))
        for m in actors + critics:
            for p in m.parameters():
                if p.dtype != torch.float32 or p.device.type != "cuda":
                    raise ValueError("BankPPOLearner needs float32 networks on the device")
        if critic_loss not in abi.PT_CRITIC_LOSS:
            raise ValueError("critic_loss must be 'mse' or 'huber', got %r" % (critic_loss,))
        if soft_update_every not in ("train", "agent_step"):
            raise ValueError("soft_update_every must be 'train' or 'agent_step', got %r" % (soft_update_every,))
        _optimizer_class(optimizer_type)
        group_envs = [int(e) for e in group_envs]
        if len(group_envs) != K or min(group_envs) < 0:
            raise ValueError("group_envs must hold one non-negative env count per member (%d)" % K)
        clib.require_policy_bank_train()
        _DeviceLearner.__init__(self, clib, actors[0].fc1.weight.device, None)
        self.actors, self.critics, self.K, self.group_envs = actors, critics, K, group_envs
        self.env_start = [sum(group_envs[:k]) for k in range(K + 1)]
        self.n_s, self.n_a, self.hidden = n_s, n_a, hid
        self.optimizer_type, self.lrs = optimizer_type, (float(actor_lr), float(critic_lr))
        self.clip_param, self.critic_loss, self.max_grad_norm = float(clip_param), critic_loss, max_grad_norm
        self.target_tau, self.target_update_steps = float(target_tau), int(target_update_steps)
        self.soft_update_every, self.fused_step = soft_update_every, True
        # the stacks, per network (0 actor, 1 critic) a list of six [K, ...] tensors
        dev = self.device
        stack = lambda nets: [torch.stack([_mlp_params(m)[i].detach() for m in nets]).contiguous() for i in range(6)]  # noqa: E731
        self.params = [stack(actors), stack(critics)]
        self.grads = [[torch.zeros_like(t) for t in net] for net in self.params]
        self.targets = [[t.clone() for t in net] for net in self.params]
        self.state1 = [[torch.zeros_like(t) for t in net] for net in self.params]
        self.state2 = [[torch.zeros_like(t) for t in net] for net in self.params] if optimizer_type == "adam" else [None, None]
        self.steps = torch.zeros(2, K, dtype=torch.int32, device=dev)
        self._grad_norm = torch.zeros(2, K, dtype=torch.float32, device=dev)
        for net, members in enumerate((actors, critics)):
            for k, m in enumerate(members):
                for i, p in enumerate(_mlp_params(m)):
                    p.data = self.params[net][i][k]
                    p.grad = self.grads[net][i][k]
        struct = lambda ts: abi.MMMlpParams(*[t.data_ptr() for t in ts])  # noqa: E731
        self._W = [struct(net) for net in self.params]
        self._G = [struct(net) for net in self.grads]
        self._T = [struct(net) for net in self.targets]
        self._groups = []
        for net in range(2):
            g = abi.MMOptGroup()
            g.algo, g.n_tensors = OPT_ALGO[optimizer_type], 6
            for i in range(6):
                g.count[i] = self.params[net][i][0].numel()
                g.param[i], g.grad[i] = self.params[net][i].data_ptr(), self.grads[net][i].data_ptr()
                g.target[i], g.state1[i] = self.targets[net][i].data_ptr(), self.state1[net][i].data_ptr()
                if self.state2[net] is not None:
                    g.state2[i] = self.state2[net][i].data_ptr()
            g.step, g.grad_norm = self.steps[net].data_ptr(), self._grad_norm[net].data_ptr()
            self._groups.append(g)

    # -- plumbing ----------------------------------------------------------------------------
    def _torch_optimizer(self, net, k):
        """A torch optimiser over member k's network: the home of the hyperparameters in torch's format (it never steps)."""
        members = self.critics if net else self.actors
        return _optimizer_class(self.optimizer_type)(members[k].parameters(), lr=self.lrs[net])

    def _cols(self, col_start, row_len):
        cols = [int(c) for c in (self.env_start if col_start is None else col_start)]
        if len(cols) != self.K + 1 or cols[0] != 0 or cols[-1] != row_len or any(b < a for a, b in zip(cols, cols[1:])):
            raise ValueError("group_envs %s do not match the batch: the column prefix %s must run from 0 to the row length %d"
                             % (self.group_envs, cols, row_len))
        return cols, (C.c_int64 * (self.K + 1))(*cols)

    def _samples(self, obs, actions, rows):
        n, S = obs.shape
        if obs.dtype != torch.float32 or (n and obs.stride(1) != 1) or S != self.n_s:
            raise ValueError("obs must be float32 [n, %d] with contiguous rows" % self.n_s)
        if actions.dtype != torch.int32 or actions.dim() != 1 or actions.shape[0] != n:
            raise ValueError("actions must be int32 [n]")
        rows = int(rows)
        row_len = n // rows if rows > 0 else self.env_start[-1]
        if rows < 0 or rows * row_len != n:
            raise ValueError("%d samples are not %d rows" % (n, rows))
        return n, S, rows, row_len

    def evaluate(self, obs, actions, rows, col_start=None, valid=None, targets=True, actor=True, critic=True):
        """The bare mm_policy_bank_eval: (logp_taken, value), float32 [n] each (None for a network that is not asked for), of
        every sample's own member -- the stacked targets, or with targets=False the stacked networks.  obs [n, S] with any row
        stride, actions int32 [n] with any stride, n = rows * row_len; col_start: the K + 1 column prefix (None: group_envs')."""
        n, S, rows, row_len = self._samples(obs, actions, rows)
        _, cs = self._cols(col_start, row_len)
        if valid is not None:
            valid = valid.reshape(-1).to(torch.uint8).contiguous()
        logp = torch.empty(n, dtype=torch.float32, device=self.device) if actor else None
        value = torch.empty(n, dtype=torch.float32, device=self.device) if critic else None
        W = self._T if targets else self._W
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self.clib.lib.mm_policy_bank_eval(
            obs.data_ptr(), obs.stride(0) if n else S, rows, row_len, S, actions.data_ptr(), actions.stride(0) if n else 1, opt(valid),
            C.byref(W[0]) if actor else None, C.byref(W[1]) if critic else None, self.K, cs, self.hidden, self.n_a, opt(logp),
            opt(value), self._stream()))
        return logp, value

    def loss_and_grad(self, obs, actions, returns, old_logp, rows, col_start=None, valid=None, form="reference", advantages=None,
                      target_value=None, diagnostics=False, networks="both"):
        """The bare mm_policy_bank_train: writes every member's gradients into the stacked gradients (the modules' .grad) and
        returns the float32 [K, 2] losses (actor, critic); with diagnostics also the [K, 2] (S+, S-) that were used and
        (logp_taken, value, ratio) [n].  Inputs as PPOLearner.loss_and_grad's, n = rows * row_len; exactly one of advantages and
        target_value (float32 [n]) with the actors; form "reference" | "flat".  Only enqueues work."""
        n, S, rows, row_len = self._samples(obs, actions, rows)
        cols, cs = self._cols(col_start, row_len)
        if networks not in ("both", "actor", "critic"):
            raise ValueError("networks must be 'both', 'actor' or 'critic', got %r" % (networks,))
        if form not in ("reference", "flat"):
            raise ValueError("form must be 'reference' or 'flat', got %r" % (form,))
        if returns.dtype != torch.float32 or returns.dim() != 1 or returns.shape[0] != n or old_logp.shape[0] != n:
            raise ValueError("returns must be float32 [n] and old_logp [n]")
        with_a, with_c = networks != "critic", networks != "actor"
        flat32 = lambda t: None if t is None else t.reshape(-1).to(torch.float32).contiguous()  # noqa: E731
        old_logp, advantages, target_value = flat32(old_logp), flat32(advantages), flat32(target_value)
        if valid is not None:
            valid = valid.reshape(-1).to(torch.uint8).contiguous()
        loss = torch.empty(self.K, 2, dtype=torch.float32, device=self.device)
        sums = torch.empty(self.K, 2, dtype=torch.float32, device=self.device) if diagnostics else None
        new = lambda on: torch.empty(n, dtype=torch.float32, device=self.device) if (diagnostics and on) else None  # noqa: E731
        diag = [new(with_a), new(with_c), new(with_a)]
        scratch = self._grow(self.clib.policy_bank_train_scratch_bytes(rows, row_len, cols))
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self.clib.lib.mm_policy_bank_train(
            obs.data_ptr(), obs.stride(0) if n else S, rows, row_len, S, actions.data_ptr(), actions.stride(0) if n else 1,
            returns.data_ptr(), returns.stride(0) if n else 1, old_logp.data_ptr(), opt(valid),
            C.byref(self._W[0]) if with_a else None, C.byref(self._W[1]) if with_c else None, self.K, cs, self.hidden, self.n_a,
            self.clip_param, abi.PT_CRITIC_LOSS[self.critic_loss], abi.PT_FORM["reference" if form == "reference" else "per_sample"],
            opt(advantages) if with_a else None, opt(target_value) if with_a else None, C.byref(self._G[0]) if with_a else None,
            C.byref(self._G[1]) if with_c else None, loss.data_ptr(), opt(sums), opt(diag[0]), opt(diag[1]), opt(diag[2]),
            scratch.data_ptr(), scratch.numel(), self._stream()))
        return (loss, sums, tuple(diag)) if diagnostics else loss

    def _fill(self):
        for net, g in enumerate(self._groups):
            g.lr, g.eps = self.lrs[net], 1e-8  # (torch's default eps of both optimisers)
            g.alpha_or_beta1, g.beta2 = (0.9, 0.999) if self.optimizer_type == "adam" else (0.99, 0.0)
            g.max_grad_norm = -1.0 if self.max_grad_norm is None else self.max_grad_norm
            g.tau = self.target_tau
        return self._groups

    def step(self, soft_mask=0):
        """clip + optimiser step of all 2 K networks, and the soft update of the members whose bit is set: one launch."""
        self.clib.opt_step_bank(self._fill(), self.K, int(soft_mask), self._stream())

    def last_grad_norm(self):
        """The total gradient norms before clipping of the last step, float32 [K, 2] (actor, critic) on the device."""
        return self._grad_norm.t()

    def optimizer_state_dict(self, k):
        """Member k's {"actor_optimizer", "critic_optimizer"} in torch.optim's state_dict() format: it loads into a PPOLearner
        (either path) and into torch.optim.  Reads the member's step counts: synchronises."""
        out = {}
        for net, name in enumerate(("actor_optimizer", "critic_optimizer")):
            s2 = None if self.state2[net] is None else [t[k] for t in self.state2[net]]
            out[name] = optimizer_state_to_torch(self.optimizer_type, self._torch_optimizer(net, k).state_dict()["param_groups"],
                                                 int(self.steps[net, k].item()), [t[k] for t in self.state1[net]], s2)
        return out

    def load_optimizer_state_dict(self, k, state_dict):
        """The reverse, in place.  The state dict's hyperparameters are not taken: the members share the learner's."""
        for net, name in enumerate(("actor_optimizer", "critic_optimizer")):
            step, s1, s2 = optimizer_state_from_torch(state_dict[name], self.optimizer_type, 6)
            for mine, theirs in ((self.state1[net], s1), (self.state2[net], s2)):
                if mine is not None:
                    for m, t in zip(mine, theirs):
                        m[k].zero_() if t is None else m[k].copy_(t)
            self.steps[net, k] = step

    def _soft_mask(self, n_episodes):
        eps = [int(n_episodes)] * self.K if isinstance(n_episodes, int) else [int(e) for e in n_episodes]
        if len(eps) != self.K:
            raise ValueError("n_episodes must be an int or one int per member (%d)" % self.K)
        return sum(1 << k for k, e in enumerate(eps) if e % self.target_update_steps == 0 and e > 0)

    @torch.no_grad()
    def train(self, states, actions=None, returns=None, n_episodes=0, form="reference", valid=None):
        """PPOLearner.train() for every member on its env group at once.  states [T, E, N, S] (or [T * E, N, S]),
        E = sum(group_envs), actions and returns [T, E, N], or `DeviceRollout.interact()`'s dict.  n_episodes: an
        int or K ints; member k's targets are blended, by PPOLearner's rule (soft_update_every included), when
        n_episodes[k] % target_update_steps == 0 and n_episodes[k] > 0.  Returns the list of float32 [K, 2] loss tensors, one
        per agent step (one in all, form "flat"); nothing is synchronised."""
        if isinstance(states, dict):
            states, actions, returns = states["states"], states["actions"], states["returns"]
        if form not in ("reference", "flat"):
            raise ValueError("form must be 'reference' or 'flat', got %r" % (form,))
        N, S, E = states.shape[-2], states.shape[-1], self.env_start[-1]
        if states.dim() == 4 and states.shape[1] == E:
            rows = states.shape[0]
        elif states.dim() == 3 and E > 0 and states.shape[0] % E == 0:
            rows = states.shape[0] // E
        else:
            raise ValueError("group_envs %s do not match the batch: states %s must be [T, %d, N, S] or [T * %d, N, S]"
                             % (self.group_envs, tuple(states.shape), E, E))
        if actions.numel() != rows * E * N or returns.numel() != rows * E * N:
            raise ValueError("actions and returns must hold one entry per state row")
        states = states.reshape(rows, E, N, S).to(torch.float32).contiguous()
        actions = actions.reshape(rows, E, N).to(torch.int32).contiguous()
        returns = returns.reshape(rows, E, N).to(torch.float32).contiguous()
        if valid is not None:
            valid = valid.reshape(rows, E, N).to(torch.uint8)
        mask = self._soft_mask(n_episodes)
        every = self.soft_update_every == "agent_step"
        losses = []
        if form == "reference":
            passes = [(states.view(rows * E, N, S)[:, a, :], actions.view(rows * E, N)[:, a], returns.view(rows * E, N)[:, a],
                       None if valid is None else valid[:, :, a].reshape(-1).contiguous(), None) for a in range(N)]
        else:
            passes = [(states.view(rows * E * N, S), actions.view(-1), returns.view(-1), None if valid is None else valid.reshape(-1),
                       [e * N for e in self.env_start])]
        for i, (obs, act, ret, v, cols) in enumerate(passes):
            old, value = self.evaluate(obs, act, rows, col_start=cols, valid=v)
            losses.append(self.loss_and_grad(obs, act, ret, old, rows, col_start=cols, valid=v, form=form, target_value=value))
            self.step(mask if (every or i == len(passes) - 1) else 0)
        return losses


class SharedBankPPOLearner(_DeviceLearner):
    """Bank mode's training half for MAPPO_GI's shared network: K `SharedPPOLearner(fused_step=True)`s as ONE learner whose
    launches do not multiply with K.  `members` are K rollout.ActorCriticNetwork(state_split=True) of one shape, hidden 128,
    float32, on the device -- typically the members a `DeviceRollout(env, members, group_envs=...)` acts with; `group_envs` are
    that rollout's env counts (member k trains on `batch[:, roll.group_slice(k)]`).  The hyperparameters are SharedPPOLearner's
    and are shared by the members; the optimiser step is always the fused one.

    The learner owns STACKED storage, member k at index k of the leading axis: the twelve parameter tensors, their gradients,
    optimiser state and targets (deep copies at construction) and the per-member Adam steps.  At construction every member
    module's `param.data` and `.grad` are re-pointed at views of the stacks, so the modules -- and a DeviceRollout /
    SharedPolicyBank built on them, at its next refresh -- see every update.

    Per agent step train() in form "reference" issues one `mm_policy_gi_bank_eval` on the stacked targets (the old
    log-probabilities), one on the live stacks (the values behind S+ / S-), one `mm_policy_gi_bank_train`
    (include/mm_policy_gi_bank_train.h) and one `mm_opt_step_bank` (include/mm_opt_step.h); form "flat" does the same once on all
    agents' samples, without the value pass.  Member k's parameters, targets and optimiser state are bit for bit those of a
    K = 1 learner on its slice, and in form "flat" those of a `SharedPPOLearner(fused_step=True)` on it.  Against
    `SharedPPOLearner` the one difference is the reference form's S+ / S-: torch's float32 sums there, one fp64 accumulation
    rounded once here.  Out of scope: hidden 512, scratch budgets and shard groups, per-member hyperparameters."""

    def __init__(self, members, clib, group_envs, lr=1e-4, optimizer_type="rmsprop", clip_param=0.2, critic_loss="mse",
                 max_grad_norm=0.5, target_tau=1.0, target_update_steps=5):
        members = list(members)
        K = len(members)
        if K < 1:
            raise ValueError("SharedBankPPOLearner needs at least one member")
        if K > abi.BANK_MAX_GROUPS:
            raise ValueError("a policy bank has at most %d members, got %d" % (abi.BANK_MAX_GROUPS, K))
        if any(type(m) is not ActorCriticNetwork or not m.state_split or m.fc2.weight.shape[0] != 128 for m in members):
            raise ValueError("SharedBankPPOLearner needs rollout.ActorCriticNetwork(state_split=True) members with hidden size 128")
        shapes = [tuple(tuple(p.shape) for p in _params(m)) for m in members]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("the members of a bank learner must have one shape, got %d different ones" % len(set(shapes)))
        n_a = members[0].actor_linear.weight.shape[0]
        if shapes[0] != ((32, 5), (32,), (64, 10), (64,), (64, 10), (64,), (128, 160), (128,), (n_a, 128), (n_a,), (1, 128), (1,)):
            raise ValueError("SharedBankPPOLearner needs the state-split network of 25 split columns and one critic output")
        if not 1 <= n_a <= 8:
            raise ValueError("SharedBankPPOLearner supports 1..8 actions, got %d" % n_a)
        for m in members:
            for p in m.parameters():
                if p.dtype != torch.float32 or p.device.type != "cuda":
                    raise ValueError("SharedBankPPOLearner needs float32 networks on the device")
        if critic_loss not in abi.GI_CRITIC_LOSS:
            raise ValueError("critic_loss must be 'mse' or 'huber', got %r" % (critic_loss,))
        _optimizer_class(optimizer_type)
        group_envs = [int(e) for e in group_envs]
        if len(group_envs) != K or min(group_envs) < 0:
            raise ValueError("group_envs must hold one non-negative env count per member (%d)" % K)
        clib.require_policy_gi_bank_train()
        _DeviceLearner.__init__(self, clib, members[0].fc2.weight.device, None)
        self.members, self.K, self.group_envs = members, K, group_envs
        self.env_start = [sum(group_envs[:k]) for k in range(K + 1)]
        self.n_a, self.hidden = n_a, 128
        self.optimizer_type, self.lr = optimizer_type, float(lr)
        self.clip_param, self.critic_loss, self.max_grad_norm = float(clip_param), critic_loss, max_grad_norm
        self.target_tau, self.target_update_steps, self.fused_step = float(target_tau), int(target_update_steps), True
        # the stacks: twelve [K, ...] tensors each, in MMGiParams' order
        self.params = [torch.stack([_params(m)[i].detach() for m in members]).contiguous() for i in range(12)]
        self.grads = [torch.zeros_like(t) for t in self.params]
        self.targets = [t.clone() for t in self.params]
        self.state1 = [torch.zeros_like(t) for t in self.params]
        self.state2 = [torch.zeros_like(t) for t in self.params] if optimizer_type == "adam" else None
        self.steps = torch.zeros(K, dtype=torch.int32, device=self.device)
        self._grad_norm = torch.zeros(K, dtype=torch.float32, device=self.device)
        for k, m in enumerate(members):
            for i, p in enumerate(_params(m)):
                p.data = self.params[i][k]
                p.grad = self.grads[i][k]
        struct = lambda ts: abi.MMGiParams(*[t.data_ptr() for t in ts])  # noqa: E731
        self._W, self._G, self._T = struct(self.params), struct(self.grads), struct(self.targets)
        g = self._group = abi.MMOptGroup()
        g.algo, g.n_tensors = OPT_ALGO[optimizer_type], 12
        for i in range(12):
            g.count[i] = self.params[i][0].numel()
            g.param[i], g.grad[i] = self.params[i].data_ptr(), self.grads[i].data_ptr()
            g.target[i], g.state1[i] = self.targets[i].data_ptr(), self.state1[i].data_ptr()
            if self.state2 is not None:
                g.state2[i] = self.state2[i].data_ptr()
        g.step, g.grad_norm = self.steps.data_ptr(), self._grad_norm.data_ptr()

    # -- plumbing ----------------------------------------------------------------------------
    def _torch_optimizer(self, k):
        """A torch optimiser over member k: the home of the hyperparameters in torch's format (it never steps)."""
        return _optimizer_class(self.optimizer_type)(self.members[k].parameters(), lr=self.lr)

    def _cols(self, col_start, row_len):
        cols = [int(c) for c in (self.env_start if col_start is None else col_start)]
        if len(cols) != self.K + 1 or cols[0] != 0 or cols[-1] != row_len or any(b < a for a, b in zip(cols, cols[1:])):
            raise ValueError("group_envs %s do not match the batch: the column prefix %s must run from 0 to the row length %d"
                             % (self.group_envs, cols, row_len))
        return cols, (C.c_int64 * (self.K + 1))(*cols)

    def _samples(self, obs, actions, rows):
        n, S = obs.shape
        if obs.dtype != torch.float32 or (n and obs.stride(1) != 1) or not 25 <= S <= 32:
            raise ValueError("obs must be float32 [n, 25..32] with contiguous rows")
        if actions.dtype != torch.int32 or actions.dim() != 1 or actions.shape[0] != n:
            raise ValueError("actions must be int32 [n]")
        rows = int(rows)
        row_len = n // rows if rows > 0 else self.env_start[-1]
        if rows < 0 or rows * row_len != n:
            raise ValueError("%d samples are not %d rows" % (n, rows))
        return n, S, rows, row_len

    def evaluate(self, obs, actions, rows, col_start=None, valid=None, targets=True, logp=True, value=True):
        """The bare mm_policy_gi_bank_eval: (logp_taken, value), float32 [n] each (None for an output that is not asked for), of
        every sample's own member -- the stacked targets, or with targets=False the live stacks.  obs [n, S] with any row
        stride, actions int32 [n] with any stride, n = rows * row_len; col_start: the K + 1 column prefix (None: group_envs')."""
        n, S, rows, row_len = self._samples(obs, actions, rows)
        _, cs = self._cols(col_start, row_len)
        if not logp and not value:
            raise ValueError("evaluate needs at least one of logp and value")
        if valid is not None:
            valid = valid.reshape(-1).to(torch.uint8).contiguous()
        out_l = torch.empty(n, dtype=torch.float32, device=self.device) if logp else None
        out_v = torch.empty(n, dtype=torch.float32, device=self.device) if value else None
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self.clib.lib.mm_policy_gi_bank_eval(
            obs.data_ptr(), obs.stride(0) if n else S, rows, row_len, S, actions.data_ptr(), actions.stride(0) if n else 1, opt(valid),
            C.byref(self._T if targets else self._W), self.K, cs, self.hidden, self.n_a, opt(out_l), opt(out_v), self._stream()))
        return out_l, out_v

    def loss_and_grad(self, obs, actions, returns, old_logp, rows, col_start=None, valid=None, form="reference", value_now=None,
                      diagnostics=False):
        """The bare mm_policy_gi_bank_train: writes every member's gradients into the stacked gradients (the modules' .grad) and
        returns the float32 [K, 3] losses (actor, critic, sum); with diagnostics also the [K, 2] (S+, S-) that were used and
        (logp_taken, value, ratio) [n].  Inputs as SharedPPOLearner.loss_and_grad's, n = rows * row_len; form "reference" needs
        value_now (float32 [n], the live members' values), form "flat" takes none.  Only enqueues work."""
        n, S, rows, row_len = self._samples(obs, actions, rows)
        cols, cs = self._cols(col_start, row_len)
        if form not in ("reference", "flat"):
            raise ValueError("form must be 'reference' or 'flat', got %r" % (form,))
        if (form == "reference") != (value_now is not None):
            raise ValueError("form 'reference' needs value_now, form 'flat' takes none")
        if returns.dtype != torch.float32 or returns.dim() != 1 or returns.shape[0] != n or old_logp.shape[0] != n:
            raise ValueError("returns must be float32 [n] and old_logp [n]")
        flat32 = lambda t: None if t is None else t.reshape(-1).to(torch.float32).contiguous()  # noqa: E731
        old_logp, value_now = flat32(old_logp), flat32(value_now)
        if value_now is not None and value_now.shape[0] != n:
            raise ValueError("value_now must be float32 [n]")
        if valid is not None:
            valid = valid.reshape(-1).to(torch.uint8).contiguous()
        loss = torch.empty(self.K, 3, dtype=torch.float32, device=self.device)
        sums = torch.empty(self.K, 2, dtype=torch.float32, device=self.device) if diagnostics else None
        diag = [torch.empty(n, dtype=torch.float32, device=self.device) if diagnostics else None for _ in range(3)]
        scratch = self._grow(self.clib.policy_gi_bank_train_scratch_bytes(rows, row_len, cols))
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.clib.check(self.clib.lib.mm_policy_gi_bank_train(
            obs.data_ptr(), obs.stride(0) if n else S, rows, row_len, S, actions.data_ptr(), actions.stride(0) if n else 1,
            returns.data_ptr(), returns.stride(0) if n else 1, old_logp.data_ptr(), opt(valid), C.byref(self._W), self.K, cs,
            self.hidden, self.n_a, self.clip_param, abi.GI_CRITIC_LOSS[self.critic_loss],
            abi.PT_FORM["reference" if form == "reference" else "per_sample"], opt(value_now), C.byref(self._G), loss.data_ptr(),
            opt(sums), opt(diag[0]), opt(diag[1]), opt(diag[2]), scratch.data_ptr(), scratch.numel(), self._stream()))
        return (loss, sums, tuple(diag)) if diagnostics else loss

    def _fill(self):
        g = self._group
        g.lr, g.eps = self.lr, 1e-8  # (torch's default eps of both optimisers)
        g.alpha_or_beta1, g.beta2 = (0.9, 0.999) if self.optimizer_type == "adam" else (0.99, 0.0)
        g.max_grad_norm = -1.0 if self.max_grad_norm is None else self.max_grad_norm
        g.tau = self.target_tau
        return [g]

    def step(self, soft_mask=0):
        """clip + optimiser step of all K networks, and the soft update of the members whose bit is set: one launch."""
        self.clib.opt_step_bank(self._fill(), self.K, int(soft_mask), self._stream())

    def last_grad_norm(self):
        """The total gradient norms before clipping of the last step, float32 [K] on the device."""
        return self._grad_norm

    def optimizer_state_dict(self, k):
        """Member k's optimiser state in torch.optim's state_dict() format: it loads into a SharedPPOLearner (either path) and
        into torch.optim.  Reads the member's step count: synchronises."""
        s2 = None if self.state2 is None else [t[k] for t in self.state2]
        return optimizer_state_to_torch(self.optimizer_type, self._torch_optimizer(k).state_dict()["param_groups"],
                                        int(self.steps[k].item()), [t[k] for t in self.state1], s2)

    def load_optimizer_state_dict(self, k, state_dict):
        """The reverse, in place.  The state dict's hyperparameters are not taken: the members share the learner's."""
        step, s1, s2 = optimizer_state_from_torch(state_dict, self.optimizer_type, 12)
        for mine, theirs in ((self.state1, s1), (self.state2, s2)):
            if mine is not None:
                for m, t in zip(mine, theirs):
                    m[k].zero_() if t is None else m[k].copy_(t)
        self.steps[k] = step

    def _soft_mask(self, n_episodes):
        eps = [int(n_episodes)] * self.K if isinstance(n_episodes, int) else [int(e) for e in n_episodes]
        if len(eps) != self.K:
            raise ValueError("n_episodes must be an int or one int per member (%d)" % self.K)
        return sum(1 << k for k, e in enumerate(eps) if e % self.target_update_steps == 0 and e > 0)

    @torch.no_grad()
    def train(self, states, actions=None, returns=None, n_episodes=0, form="reference", valid=None):
        """SharedPPOLearner.train() for every member on its env group at once.  states [T, E, N, S] (or [T * E, N, S]),
        E = sum(group_envs), actions and returns [T, E, N], or `DeviceRollout.interact()`'s dict.  n_episodes: an int or K
        ints; member k's targets are blended after every optimiser step of this call when
        n_episodes[k] % target_update_steps == 0 and n_episodes[k] > 0 (SharedPPOLearner's rule).  Returns the list of float32
        [K, 3] loss tensors, one per agent step (one in all, form "flat"); nothing is synchronised."""
        if isinstance(states, dict):
            states, actions, returns = states["states"], states["actions"], states["returns"]
        if form not in ("reference", "flat"):
            raise ValueError("form must be 'reference' or 'flat', got %r" % (form,))
        N, S, E = states.shape[-2], states.shape[-1], self.env_start[-1]
        if states.dim() == 4 and states.shape[1] == E:
            rows = states.shape[0]
        elif states.dim() == 3 and E > 0 and states.shape[0] % E == 0:
            rows = states.shape[0] // E
        else:
            raise ValueError("group_envs %s do not match the batch: states %s must be [T, %d, N, S] or [T * %d, N, S]"
                             % (self.group_envs, tuple(states.shape), E, E))
        if actions.numel() != rows * E * N or returns.numel() != rows * E * N:
            raise ValueError("actions and returns must hold one entry per state row")
        states = states.reshape(rows, E, N, S).to(torch.float32).contiguous()
        actions = actions.reshape(rows, E, N).to(torch.int32).contiguous()
        returns = returns.reshape(rows, E, N).to(torch.float32).contiguous()
        if valid is not None:
            valid = valid.reshape(rows, E, N).to(torch.uint8)
        mask = self._soft_mask(n_episodes)
        losses = []
        if form == "reference":
            for a in range(N):
                obs, act, ret = states.view(rows * E, N, S)[:, a, :], actions.view(rows * E, N)[:, a], returns.view(rows * E, N)[:, a]
                v = None if valid is None else valid[:, :, a].reshape(-1).contiguous()
                old, _ = self.evaluate(obs, act, rows, valid=v, value=False)
                _, now = self.evaluate(obs, act, rows, valid=v, targets=False, logp=False)
                losses.append(self.loss_and_grad(obs, act, ret, old, rows, valid=v, form=form, value_now=now))
                self.step(mask)
        else:
            obs, act, ret = states.view(rows * E * N, S), actions.view(-1), returns.view(-1)
            v = None if valid is None else valid.reshape(-1)
            cols = [e * N for e in self.env_start]
            old, _ = self.evaluate(obs, act, rows, col_start=cols, valid=v, value=False)
            losses.append(self.loss_and_grad(obs, act, ret, old, rows, col_start=cols, valid=v, form=form))
            self.step(mask)
        return losses
