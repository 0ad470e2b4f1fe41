"""What the tests of the hidden-512 actor share (test_policy_wide_host.py without a GPU, test_policy_wide_gpu.py on the MI355X):
the nets and cases of mm_policy_wide_act, its raw launch, and the n boundaries taken from the constants of
include/mm_policy_wide.h.  The generic pieces -- the numpy Philox, the float64 sampler, the tolerance rule, guarded buffers --
are policy_act_util's; only what hard-codes hidden 128 there has a twin here.  A plain module: no fixtures, nothing here touches
the GPU unless it is handed device tensors."""
import copy
import functools
import os
import re

import numpy as np
import torch

import policy_act_util as U
from policy_act_util import (BAND, BAND_SHARE, CTR_A, CTRS_C, KNIFE, SEED_A, SEEDS_C, U64, Case, compare, counter_tensor,  # noqa: F401
                             counter_value, guarded, knife_edges, near_edge, offset_copy, sample, sample_f64, sampler_u, weights_of)
from marl_mass_amd.rollout import ActorNetwork

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mm_policy_wide.h")
HIDDEN = 512


def header_constants():
    """{name: int} of the header's MM_POLICY_WIDE_* macros: the kernel's own decomposition of a launch."""
    txt = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (MM_POLICY_WIDE_\w+) (\d+)\s*$", txt, re.M)}


_K = header_constants()
TILE, WAVES, MAX_GRID, W2_ALIGN = (_K["MM_POLICY_WIDE_" + k] for k in ("TILE", "WAVES", "MAX_GRID", "W2_ALIGN"))
WG = TILE * WAVES        # agents of one workgroup's trip
GRID = WG * MAX_GRID     # agents of one trip of a full grid of persistent workgroups

NS_A, NA_A, GAINS = (1, 5, 25, 30, 32), (1, 5, 8), (3, 60)
NA_C = (1, 2, 5, 8)
# both sides of one tile, of one workgroup's agents and of one full grid, and once beyond two trips of the persistent loop
N_GRID_B = (1, TILE - 1, TILE, TILE + 1, WG - 1, WG, WG + 1, GRID - 1, GRID, GRID + 1, 2 * GRID + TILE + 1)
# observation seeds chosen on the INPUTS (numpy Philox + float64 network, test_policy_wide_host.py): with them no row of a case
# has its u within BAND of an inner CDF edge under any key the GPU file uses it with.  key: (n_s, n_a, gain); default 11
OBS_SEED = {(25, 5, 3): 12, (30, 8, 3): 12}


def wide_net(n_s, n_a, gain, seed=5):
    """rollout.ActorNetwork(n_s, 512, n_a), torch's default init under a fixed seed, with asymmetric non-zero biases in every
    layer and fc3's weight scaled by `gain` (policy_act_util.actor_net at the other hidden size)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = ActorNetwork(n_s, HIDDEN, n_a)
        with torch.no_grad():
            net.fc1.bias.uniform_(-0.5, 0.5); net.fc2.bias.uniform_(-0.5, 0.5); net.fc3.bias.uniform_(-1, 1)
            net.fc3.weight.mul_(float(gain))
    return net


def filtered_randn(net, n, n_s, seed):
    """randn * 1.5 rows; rows on a knife edge of the float64 network (never the kernel) are redrawn.  Returns (obs, the
    number of redrawn rows, the rounds it took)."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, n_s, generator=g) * 1.5
    net64 = copy.deepcopy(net).double()
    redrawn = rounds = 0
    for _ in range(20):
        close = knife_edges("act", net64, obs.double())
        if not bool(close.any()):
            break
        rounds += 1
        redrawn += int(close.sum())
        obs[close] = torch.randn(int(close.sum()), n_s, generator=g) * 1.5
    return obs, redrawn, rounds


@functools.lru_cache(maxsize=None)
def synthetic_case(n_s, n_a, gain, n=257, obs_seed=None):
    net = wide_net(n_s, n_a, gain)
    seed = OBS_SEED.get((n_s, n_a, gain), 11) if obs_seed is None else obs_seed
    obs, redrawn, rounds = filtered_randn(net, n, n_s, seed)
    case = Case("act", "wide_s%d_a%d_g%d_n%d" % (n_s, n_a, gain, n), net, obs, n_a, redrawn)  # (asserts: no knife-edge row)
    case.rounds = rounds
    return case


def grid_a():
    return [synthetic_case(n_s, n_a, gain) for n_s in NS_A for n_a in NA_A for gain in GAINS]


def case_b(n):
    """Grid B: the 257 rows of the n_s = 30, n_a = 5, gain 3 case, cut or tiled to n rows."""
    return synthetic_case(30, 5, 3).tiled(n)


def case_c(n_a):
    return synthetic_case(30, n_a, 3)


def all_gpu_cases():
    """(case, [(seed, ctr)]) for every launch of test_policy_wide_gpu.py whose actions meet the float64 sampler."""
    a = [(SEED_A, CTR_A)]
    for case in grid_a():
        yield case, a
    for n in N_GRID_B:
        yield case_b(n), a
    for n_a in NA_C:
        yield case_c(n_a), [(s, k) for s in SEEDS_C for k in CTRS_C]


# ---------------------------------------------------------------------------------------------------------------------
# calling the entries
def launch(clib, weights, obs, n, n_s, n_a, seed, counter, actions, logp, hidden=HIDDEN, entry="mm_policy_wide_act"):
    """The raw entry (mm_policy_wide_act, or mm_policy_act with the same arguments): tensors (or None) in, status code out."""
    return getattr(clib.lib, entry)(U._ptr(obs), n, n_s, *[U._ptr(w) for w in weights], hidden, n_a, seed, U._ptr(counter),
                                    U._ptr(actions), U._ptr(logp), U._stream(obs))


def run(clib, weights, obs, n_a, seed, ctr, n=None, entry="mm_policy_wide_act"):
    """One call with fresh sentinel-filled outputs; returns {actions, logp, counter} (counter: the value after)."""
    n = obs.shape[0] if n is None else n
    out = {"actions": torch.full((n,), -1, dtype=torch.int32, device=obs.device),
           "logp": torch.full((n, n_a), float("nan"), dtype=torch.float32, device=obs.device)}
    c = counter_tensor(ctr, obs.device)
    clib.check(launch(clib, weights, obs, n, obs.shape[1], n_a, seed, c, out["actions"], out["logp"], entry=entry))
    out["counter"] = counter_value(c)
    return out


def check_forward(store, clib, case, device, seed=SEED_A, ctr=CTR_A, f64_actions=True):
    """policy_act_util.check_forward for this entry: the rule on the log-probabilities (max|kernel - f64| <= 4 e32 + 1e-6
    max(1, max|f64|), e32 the float32 module on `device`), the row properties, the counter, actions == mm_sample_actions on the
    kernel's own log-probabilities, and (f64_actions) == the float64 inverse CDF under the numpy Philox outside the BAND."""
    net = copy.deepcopy(case.net).to(device)
    obs = case.obs.to(device)
    out = run(clib, weights_of("act", net), obs, case.n_a, seed, ctr)
    with torch.no_grad():
        f32 = {"logp": net(obs)}
    compare(store, case.name, out, f32, {"logp": case.logp64})
    lp = out["logp"]
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()), case.name
    assert float(torch.logsumexp(lp.double(), -1).abs().max()) <= 1e-6, case.name
    assert out["counter"] == ((ctr + 1) & U64), case.name
    a = out["actions"]
    assert bool(((a >= 0) & (a < case.n_a)).all()), case.name
    if case.n_a == 1:
        assert bool((lp == 0.0).all()) and bool((a == 0).all()), case.name
    a_own, _ = sample(clib, lp, seed, ctr)
    assert torch.equal(a, a_own), case.name
    if f64_actions:
        near = case.near(seed, ctr)
        assert np.array_equal(a.cpu().numpy()[~near], case.actions64(seed, ctr)[~near]), case.name
    return out
