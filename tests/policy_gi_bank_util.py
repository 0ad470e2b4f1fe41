"""What the shared-policy-bank tests share (test_policy_gi_bank_host.py without a GPU, test_policy_gi_bank_gpu.py on the MI355X):
the members, one set of 257 observation rows per n_s with every member's float64 log-probabilities and values on them (computed
once, never modified), and the raw call of mm_policy_gi_bank_act (include/mm_policy_gi_bank.h).  The group layouts are
policy_bank_util.LAYOUTS.  A plain module: no fixtures, nothing here touches the GPU unless it is handed device tensors.

Members: gi_net(n_s, 5, gain, seed = 100 + k) -- different seeds, so a row computed with the wrong member cannot pass; member 1
has gain 60 (near-deterministic rows) and member 2 is member 0 again (an identical pair).  Row i of a layout is base row i % 257,
whatever group it falls in."""
import copy
import ctypes
import functools

import numpy as np
import torch

import policy_act_util as U
import policy_bank_util as B
from marl_mass_amd import _cabi as abi

N_A = B.N_A
NS = (25, 30)
BASE_ROWS = B.BASE_ROWS
SEED, CTR = U.SEED_A, U.CTR_A
OBS_SEED = 11  # chosen on the inputs: test_policy_gi_bank_host.py::test_f64_reference_stays_inside_the_band_cap
LAYOUTS = B.LAYOUTS
group_start, group_of, rows, c_groups = B.group_start, B.group_of, B.rows, B.c_groups


@functools.lru_cache(maxsize=None)
def member(n_s, k):
    return U.gi_net(n_s, N_A, B.gain_of(k), seed=100 + (0 if k == 2 else k))


@functools.lru_cache(maxsize=None)
def base(n_s):
    """(obs [257, n_s], logp64 [64, 257, 5], value64 [64, 257]): rows on a knife edge of ANY of the 64 members' float64 networks
    are redrawn."""
    nets64 = [copy.deepcopy(member(n_s, k)).double() for k in range(abi.BANK_MAX_GROUPS)]
    g = torch.Generator().manual_seed(OBS_SEED)
    obs = torch.randn(BASE_ROWS, n_s, generator=g) * 1.5
    for _ in range(40):
        close = torch.zeros(BASE_ROWS, dtype=torch.bool)
        for net in nets64:
            close |= U.knife_edges("gi", net, obs.double())
        if not bool(close.any()):
            break
        obs[close] = torch.randn(int(close.sum()), n_s, generator=g) * 1.5
    assert not bool(close.any())
    with torch.no_grad():
        logp64 = torch.stack([net(obs.double()) for net in nets64])
        value64 = torch.stack([net(obs.double(), out_type="v")[:, 0] for net in nets64])
    return obs.contiguous(), logp64, value64


def obs_of(n_s, n):
    return base(n_s)[0][rows(n)].contiguous()


def logp64_of(n_s, sizes):
    """The float64 log-probabilities of a layout's rows, gathered from base()."""
    return base(n_s)[1][group_of(sizes), rows(int(sum(sizes)))]


def value64_of(n_s, sizes):
    return base(n_s)[2][group_of(sizes), rows(int(sum(sizes)))]


def near(n_s, sizes, seed=SEED, ctr=CTR):
    lp = logp64_of(n_s, sizes).numpy()
    return U.near_edge(lp, U.sampler_u(np.arange(lp.shape[0], dtype=np.uint64), ctr, seed))


def actions64(n_s, sizes, seed=SEED, ctr=CTR):
    lp = logp64_of(n_s, sizes).numpy()
    return U.sample_f64(lp, U.sampler_u(np.arange(lp.shape[0], dtype=np.uint64), ctr, seed))


def stack(members, device):
    """The twelve stacked float32 tensors of the bank, in MMGiParams order."""
    ws = [U.weights_of("gi", m) for m in members]
    return [torch.stack([w[j] for w in ws]).contiguous().to(device) for j in range(12)]


def bank_params(tensors, null=None):
    """MMGiParams of the stacked tensors (which it keeps alive); null: the index of a base pointer to leave NULL."""
    p = abi.MMGiParams(*[None if j == null else t.data_ptr() for j, t in enumerate(tensors)])
    p.tensors = tensors
    return p


def launch_bank(clib, params, obs, n, n_s, K, start, seed, counter, actions, logp, value, hidden=128, n_a=N_A):
    """The raw entry: status code out.  params: MMGiParams or None; start: a ctypes int64 array or None.  The stream is the
    current one of the device the first tensor given lives on."""
    on = next(t for t in (obs, actions, counter, logp, value) if t is not None)
    return clib.lib.mm_policy_gi_bank_act(U._ptr(obs), n, n_s, None if params is None else ctypes.byref(params), K, start, hidden,
                                          n_a, seed, U._ptr(counter), U._ptr(actions), U._ptr(logp), U._ptr(value), U._stream(on))
