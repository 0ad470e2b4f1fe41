"""What the policy-bank tests share (test_policy_bank_host.py without a GPU, test_policy_bank_gpu.py on the MI355X): the members,
the group layouts, one set of 257 observation rows per n_s with every member's float64 log-probabilities on them (computed
once, never modified), and the raw call of mm_policy_bank_act (include/mm_policy_bank.h).  A plain module: no fixtures, nothing
here touches the GPU unless it is handed device tensors.

Members: actor_net(n_s, 5, gain, seed = 100 + k) -- different seeds, so a row computed with the wrong member cannot pass; member
1 has gain 60 (near-deterministic rows, log-probabilities down to -100) and member 2 is member 0 again (an identical pair).
Row i of a layout is base row i % 257, whatever group it falls in."""
import copy
import ctypes
import functools

import numpy as np
import torch

import policy_act_util as U
from marl_mass_amd import _cabi as abi

N_A = 5
NS = (25, 30)
BASE_ROWS = 257
SEED, CTR = U.SEED_A, U.CTR_A
OBS_SEED = {25: 11, 30: 11}  # chosen on the inputs: test_policy_bank_host.py::test_f64_reference_stays_inside_the_band_cap
# group sizes, the smallest shapes at which tiling, lookup or the grid split can go wrong
LAYOUTS = {
    "k1_n1": (1,), "k1_n32": (32,), "k1_n33": (33,), "k1_n257": (257,),
    "k3_off_tile": (1, 31, 33),            # every boundary off a tile edge
    "k5_empty": (0, 40, 0, 24, 0),         # empty first, middle and last
    "k64_by4": (4,) * 64,                  # the table's last slot
    "k2_big": (65541, 7),                  # more tiles than one workgroup's share: persistent stride + grid split
}


def group_start(sizes):
    return [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]


def gain_of(k):
    return 60 if k == 1 else 3


@functools.lru_cache(maxsize=None)
def member(n_s, k):
    return U.actor_net(n_s, N_A, gain_of(k), seed=100 + (0 if k == 2 else k))


@functools.lru_cache(maxsize=None)
def base(n_s):
    """(obs [257, n_s], logp64 [64, 257, 5]): rows on a knife edge of ANY of the 64 members' float64 networks are redrawn."""
    nets64 = [copy.deepcopy(member(n_s, k)).double() for k in range(abi.BANK_MAX_GROUPS)]
    g = torch.Generator().manual_seed(OBS_SEED[n_s])
    obs = torch.randn(BASE_ROWS, n_s, generator=g) * 1.5
    for _ in range(40):
        close = torch.zeros(BASE_ROWS, dtype=torch.bool)
        for net in nets64:
            close |= U.knife_edges("act", net, obs.double())
        if not bool(close.any()):
            break
        obs[close] = torch.randn(int(close.sum()), n_s, generator=g) * 1.5
    assert not bool(close.any())
    with torch.no_grad():
        logp64 = torch.stack([net(obs.double()) for net in nets64])
    return obs.contiguous(), logp64


def rows(n):
    return torch.arange(n) % BASE_ROWS


def obs_of(n_s, n):
    return base(n_s)[0][rows(n)].contiguous()


def group_of(sizes):
    """The member index of every row."""
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def logp64_of(n_s, sizes):
    """The float64 log-probabilities of a layout's rows, gathered from base()."""
    n = int(sum(sizes))
    return base(n_s)[1][group_of(sizes), rows(n)]


def near(n_s, sizes, seed=SEED, ctr=CTR):
    lp = logp64_of(n_s, sizes).numpy()
    return U.near_edge(lp, U.sampler_u(np.arange(lp.shape[0], dtype=np.uint64), ctr, seed))


def actions64(n_s, sizes, seed=SEED, ctr=CTR):
    lp = logp64_of(n_s, sizes).numpy()
    return U.sample_f64(lp, U.sampler_u(np.arange(lp.shape[0], dtype=np.uint64), ctr, seed))


def stack(members, device):
    """The six stacked float32 tensors of the bank, in MMMlpParams order."""
    ms = [(m.fc1, m.fc2, m.fc3) for m in members]
    return [torch.stack([(l[j].weight if w == 0 else l[j].bias).detach() for l in ms]).contiguous().to(device)
            for j in range(3) for w in (0, 1)]


def bank_params(tensors, null=None):
    """MMMlpParams of the stacked tensors (which it keeps alive); null: the index of a base pointer to leave NULL."""
    p = abi.MMMlpParams(*[None if j == null else t.data_ptr() for j, t in enumerate(tensors)])
    p.tensors = tensors
    return p


def c_groups(start):
    return (ctypes.c_int64 * len(start))(*start)


def launch_bank(clib, params, obs, n, n_s, K, start, seed, counter, actions, logp, hidden=128, n_a=N_A):
    """The raw entry: status code out.  params: MMMlpParams or None; start: a ctypes int64 array or None.  The stream is the
    current one of the device the first tensor given lives on."""
    on = next(t for t in (obs, actions, counter, logp) if t is not None)
    return clib.lib.mm_policy_bank_act(U._ptr(obs), n, n_s, None if params is None else ctypes.byref(params), K, start, hidden, n_a,
                                       seed, U._ptr(counter), U._ptr(actions), U._ptr(logp), U._stream(on))


def bank_grid(clib, start):
    """mm_policy_bank_grid's block prefix (host arithmetic only)."""
    K = len(start) - 1
    out = (ctypes.c_int32 * (K + 1))()
    assert clib.lib.mm_policy_bank_grid(K, c_groups(start), out) == abi.MM_OK
    return list(out)
