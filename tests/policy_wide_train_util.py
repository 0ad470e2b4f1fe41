"""Shared by tests/test_policy_wide_train_host.py and tests/test_policy_wide_train_gpu.py: the hidden-512 networks, the
launch constants of include/mm_policy_wide_train.h, and the inputs of the synthetic batches with their knife-edge filter.
The torch objective is tests/policy_train_util.py's: it does not depend on the hidden size.

Everything here is drawn from host generators and decided with the float64 modules on the host, so which samples the filter
redraws is a property of (seed, n, n_s, n_a, strided) alone: the same with and without a GPU."""
import copy
import os
import re

import torch

from marl_mass_amd.rollout import ActorNetwork, CriticNetwork
from policy_train_util import one_hot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mm_policy_wide_train.h")
HIDDEN = 512


def header_macros():
    """The integer macros of the header whose value is a plain literal."""
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"^#define (MM_POLICY_WIDE_TRAIN_\w+) (\d+)\b", text, re.M)}


M = header_macros()
TILE, WAVES, MAX_GRID = M["MM_POLICY_WIDE_TRAIN_TILE"], M["MM_POLICY_WIDE_TRAIN_WAVES"], M["MM_POLICY_WIDE_TRAIN_MAX_GRID"]
MAX_SLICES, MIN_SLICE_TILES = M["MM_POLICY_WIDE_TRAIN_MAX_SLICES"], M["MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES"]
FIXED_BYTES = 256 + 4 * 512 * 512 * 4                      # MM_POLICY_WIDE_TRAIN_FIXED_BYTES, as the header spells it out
ROW_BYTES = (32 + 4 * 512 + 16) * 4                        # MM_POLICY_WIDE_TRAIN_ROW_BYTES
PARTIAL_BYTES = (512 * 544 + 16 * 512 + 512 * 32 + 512 + 16 + 512) * 4  # MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES


def slicing(n):
    """(tiles, tiles per slice, slices) of kernel B for n samples: the rule stated in the header."""
    tiles = (n + TILE - 1) // TILE
    per = max(MIN_SLICE_TILES, (tiles + MAX_SLICES - 1) // MAX_SLICES)
    return tiles, per, max(1, (tiles + per - 1) // per)


# the per-sample launch's persistent loop wraps (more tiles than MAX_GRID * WAVES) with a ragged last tile, and the
# weight-gradient pass has more than one slice with a shorter last one
N_WRAP = (MAX_GRID * WAVES + 3) * TILE + 5

# Knife-edge ReLUs.  A sample is redrawn when a float64 pre-activation of any of the four hidden layers is closer to zero than
# KNIFE = 4 x the largest |z_float32_torch - z_float64| over the test batches.  That figure is measured with the modules alone
# on the host (tests/test_policy_wide_train_host.py::test_knife_is_four_times_the_float32_preactivation_error measures it again,
# the GPU module records the device's figure): 1.61e-6 over BATCHES below, so 4 x is 6.4e-6, rounded up to 7e-6 (the float32 figure moves by a few per cent with the BLAS that computes it).
KNIFE = 7e-6
MAX_REDRAW_SHARE = 0.03


def nets(n_s, n_a=5, seed=5):
    """(actor, critic) on the host with the scales of tests/test_policy_train_gpu.py's _nets, at hidden 512."""
    torch.manual_seed(seed)
    actor, critic = ActorNetwork(n_s, HIDDEN, n_a), CriticNetwork(n_s, n_a, HIDDEN, 1)
    with torch.no_grad():
        for m in (actor.fc1, actor.fc2, critic.fc1, critic.fc2):
            m.bias.uniform_(-0.5, 0.5)
        actor.fc3.bias.uniform_(-1, 1); actor.fc3.weight.mul_(3.0)
        critic.fc3.bias.fill_(0.5); critic.fc3.weight.mul_(2.0)
        critic.fc2.weight[:, HIDDEN:].mul_(3.0)  # the one-hot columns matter as much as a hidden unit
    return actor, critic


@torch.no_grad()
def preactivations(actor, critic, obs, act):
    """The pre-activations of the FOUR hidden layers (both networks) in the modules' dtype."""
    n_a = critic.fc2.weight.shape[1] - HIDDEN
    za1 = actor.fc1(obs)
    za2 = actor.fc2(torch.relu(za1))
    zc1 = critic.fc1(obs)
    zc2 = critic.fc2(torch.cat([torch.relu(zc1), one_hot(act, n_a, obs.dtype)], 1))
    return za1, za2, zc1, zc2


def knife_edges(actor64, critic64, obs64, act):
    close = torch.zeros(obs64.shape[0], dtype=torch.bool)
    for z in preactivations(actor64, critic64, obs64, act):
        close |= z.abs().min(dim=1).values < KNIFE
    return close


def preactivation_error(actor, critic, obs, act):
    """max |z_float32 - z_float64| of the torch modules on a batch (host)."""
    a64, c64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    z32 = preactivations(actor, critic, obs, act)
    z64 = preactivations(a64, c64, obs.double(), act)
    return max(float((x.double() - y).abs().max()) for x, y in zip(z32, z64))


def draw_inputs(actor, critic, n, n_s, n_a, strided, seed, knife_filter=True):
    """The host half of a synthetic batch, stratified as tests/test_policy_train_gpu.py's _batch: a random permutation gives
    every sample a rank k, the action is (k // 2) % n_a.  Returns (obs [n, n_s] dense float32, act int32 [n], noise [n], k,
    redrawn): obs after the knife-edge filter, `redrawn` the number of samples it redrew (at most MAX_REDRAW_SHARE of n)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randperm(n, generator=g)
    act = ((k // 2) % n_a).to(torch.int32)
    if strided:  # (the draws of the other two agent columns are made and dropped: the layout is the caller's)
        obs = (torch.randn(n, 3, n_s, generator=g) * 1.5)[:, 1, :].contiguous()
        noise = torch.randn(n, 3, generator=g)[:, 1].contiguous()
    else:
        obs = torch.randn(n, n_s, generator=g) * 1.5
        noise = torch.randn(n, generator=g)
    noise = noise.abs() * torch.where(k % 2 == 0, -1.0, 1.0)
    a64, c64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    redrawn = 0
    for _ in range(20 if knife_filter else 0):
        close = knife_edges(a64, c64, obs.double(), act)
        if not bool(close.any()):
            break
        redrawn += int(close.sum())
        obs[close] = torch.randn(int(close.sum()), n_s, generator=g) * 1.5
    if knife_filter:
        assert not bool(knife_edges(a64, c64, obs.double(), act).any())
        assert redrawn <= MAX_REDRAW_SHARE * n, (n, redrawn)
    return obs, act, noise, k, redrawn


# the batches of fewer than one tile (strided, as the tests use them): n_s -> seed, chosen so that the filter redraws nobody (one
# sample of 31 is already 3.2 %, over the cap); asserted on the host by test_small_batches_need_no_redraw
SMALL_N = 31
SMALL_SEEDS = {25: 1, 30: 3}


def batch_seed(n, n_s):
    return SMALL_SEEDS[n_s] if n == SMALL_N else 1 + n + n_s


# every (n, n_s, n_a, strided, seed) the GPU module draws with the filter on
BATCHES = ([(SMALL_N, s, 5, True, batch_seed(SMALL_N, s)) for s in (25, 30)]
           + [(1000, s, 5, st, batch_seed(1000, s)) for s in (25, 30) for st in (False, True)]
           + [(N_WRAP, s, 5, True, batch_seed(N_WRAP, s)) for s in (25, 30)]
           + [(1000, 30, 1, True, 12), (1000, 30, 8, True, 19), (1000, 30, 5, True, 21), (N_WRAP, 30, 5, True, 77)])
