"""What the act-side policy tests share (test_policy_act_host.py on the CPU oracle, test_policy_act_gpu.py on the MI355X):
an independent numpy Philox4x32-10, float64 references of mm_policy_act / mm_policy_gi_act / mm_sample_actions /
mm_discount_returns, case builders with fixed seeds, the knife-edge filter of the train-side tests, guarded output buffers
and the tolerance rule.  A plain module: no fixtures, nothing here touches the GPU unless it is handed device tensors.

The rule (tests/test_policy_gi_train_gpu.py::_compare, per output tensor):
    max|kernel - f64| <= 4 * e32 + 1e-6 * max(1, max|f64|),   e32 = max|float32 torch module - f64|
with the float32 module run on the kernel's device.  The factor 4 is the train side's margin for another summation order of the
same float32 products; the floor covers outputs where float32 is exact (n_a = 1)."""
import copy
import ctypes
import functools
import json
import os

import numpy as np
import torch

from golden_util import GOLDEN
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, discount_rewards

# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy, 32-bit words held in uint64
M32 = np.uint64(0xFFFFFFFF)
DOMAIN = 0x53414D50  # the sampler's domain word, xor-ed into the high counter word
U64 = (1 << 64) - 1


def philox4x32_10(counter4, key2):
    """The four output words of Philox4x32-10.  counter4: four arrays (or scalars) of 32-bit words, key2: two scalars."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & M32 for c in counter4])
    k0, k1 = int(key2[0]) & 0xFFFFFFFF, int(key2[1]) & 0xFFFFFFFF
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> sh) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> sh) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0 & M32, p1 & M32, n2 & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u53(w0, w1):
    """53-bit uniform in [0, 1) from two 32-bit words: 27 bits of the first, 26 of the second."""
    w0, w1 = np.asarray(w0, dtype=np.uint64), np.asarray(w1, dtype=np.uint64)
    return ((w0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def sampler_u(idx, ctr, seed):
    """The sampler's uniform of agent idx (include/mm_abi.h mm_sample_actions): counter words (idx low, idx high, ctr low,
    ctr high ^ DOMAIN), key (seed low, seed high); u53 of output words 0 and 1."""
    idx = np.asarray(idx, dtype=np.uint64)
    ctr, seed = int(ctr) & U64, int(seed) & U64
    w = philox4x32_10((idx & M32, idx >> np.uint64(32), ctr & 0xFFFFFFFF, ((ctr >> 32) ^ DOMAIN) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, seed >> 32))
    return u53(w[0], w[1])


# ---------------------------------------------------------------------------------------------------------------------
# float64 sampler: np.random.choice's inverse CDF
BAND = 1e-5      # a row whose u lies closer than this to an inner CDF edge may be drawn either way by a float32 policy
BAND_SHARE = 1e-3  # cap on the share of such rows at large n (the existing tests' cap: a condition on the inputs)


def cdf_f64(logp64):
    cdf = np.cumsum(np.exp(np.asarray(logp64, dtype=np.float64)), axis=-1)
    return cdf / cdf[:, -1:]


def sample_f64(logp64, u):
    """a = min(searchsorted(cdf, u, "right"), n_a - 1) per row (the count of cdf entries <= u of a non-decreasing row)."""
    cdf = cdf_f64(logp64)
    return np.minimum((cdf <= u[:, None]).sum(-1), cdf.shape[1] - 1).astype(np.int32)


def near_edge(logp64, u, band=BAND):
    """Rows whose u is within `band` of an inner CDF edge (the last edge is 1 and is clamped, not searched)."""
    cdf = cdf_f64(logp64)[:, :-1]
    if cdf.shape[1] == 0:
        return np.zeros(len(u), dtype=bool)
    return (np.abs(cdf - u[:, None]) < band).any(-1)


# ---------------------------------------------------------------------------------------------------------------------
# networks and cases
KNIFE = 2e-5  # ~20 x the float32 error of a 160-term dot product of O(1) terms (test_policy_gi_train_gpu.py)
SEED_A, CTR_A = 0x9E3779B97F4A7C15, (1 << 32) + 5  # grids A and B: both high words in use
NS_ACT, NS_GI = (1, 2, 5, 24, 25, 30, 31, 32), (25, 26, 30, 32)
NA_GRID, GAINS = (1, 2, 5, 7, 8), (3, 60)
N_GRID_B = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073)
SEEDS_C, CTRS_C = (99, 1 << 32, 0x9E3779B97F4A7C15), (8, (1 << 32) + 5, (1 << 63) + 1)
NA_C, N_C = (1, 2, 5, 8), (257, 65537)
RECORDED = (("act", "mappo_dropin_mass"), ("act", "mappo_dropin_v0none"), ("gi", "mappo_gi_v1mass"))
# observation seeds of the synthetic cases, chosen on the INPUTS (numpy Philox + float64 network, test_policy_act_host.py):
# with them no row of an n <= 1000 case has its u within BAND of an inner CDF edge.  key: (kind, n_s, n_a, gain)
OBS_SEED = {("act", 5, 7, 3): 12, ("act", 30, 5, 3): 12, ("act", 30, 8, 3): 12, ("gi", 25, 2, 60): 12, ("gi", 25, 8, 3): 12}  # default 11


def actor_net(n_s, n_a, gain, seed=5):
    """rollout.ActorNetwork with asymmetric non-zero biases in every layer; fc3's weight scaled by `gain`."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = ActorNetwork(n_s, 128, n_a)
        with torch.no_grad():
            net.fc1.bias.uniform_(-0.5, 0.5); net.fc2.bias.uniform_(-0.5, 0.5); net.fc3.bias.uniform_(-1, 1)
            net.fc3.weight.mul_(float(gain))
    return net


def gi_net(n_s, n_a, gain, seed=5):
    """rollout.ActorCriticNetwork(state_split=True), the same way; the critic head has scale 4 and bias 2.5."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = ActorCriticNetwork(n_s, n_a, 128, 1, state_split=True)
        with torch.no_grad():
            for m in (net.fc11, net.fc12, net.fc13, net.fc2):
                m.bias.uniform_(-0.5, 0.5)
            net.actor_linear.bias.uniform_(-1, 1); net.actor_linear.weight.mul_(float(gain))
            net.critic_linear.bias.fill_(2.5); net.critic_linear.weight.mul_(4.0)
    return net


def weights_of(kind, net):
    """The network's tensors in the entry's argument order."""
    if kind == "act":
        ms = (net.fc1, net.fc2, net.fc3)
    else:
        ms = (net.fc11, net.fc12, net.fc13, net.fc2, net.actor_linear, net.critic_linear)
    return [t.detach().contiguous() for m in ms for t in (m.weight, m.bias)]


@torch.no_grad()
def knife_edges(kind, net64, obs64):
    """Rows with a float64 pre-activation of either hidden layer within KNIFE of zero: a ReLU there is open in one float32
    implementation and shut in another, and the row's error measures that draw, not the rounding of a sum."""
    if kind == "act":
        z1 = net64.fc1(obs64)
    else:
        s1, s2, s3 = net64.split(obs64)
        z1 = torch.cat([net64.fc11(s1), net64.fc12(s2), net64.fc13(s3)], 1)
    z2 = net64.fc2(torch.relu(z1))
    return (z1.abs().min(dim=1).values < KNIFE) | (z2.abs().min(dim=1).values < KNIFE)


class Case(object):
    """One network + observation set, all on the CPU; logp64 / value64 are the float64 module's outputs."""

    def __init__(self, kind, name, net, obs, n_a, redrawn=0):
        self.kind, self.name, self.net, self.obs, self.n_a, self.redrawn = kind, name, net, obs.contiguous(), n_a, redrawn
        self.n, self.n_s = obs.shape
        self.net64 = copy.deepcopy(net).double()
        assert not bool(knife_edges(kind, self.net64, obs.double()).any()), name
        with torch.no_grad():
            self.logp64 = self.net64(obs.double())
            self.value64 = self.net64(obs.double(), out_type="v")[:, 0] if kind == "gi" else None

    def tiled(self, n):
        """The same rows repeated to n rows (row i = row i % self.n): references are gathered, not recomputed."""
        idx = torch.arange(n) % self.n
        c = object.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name, c.n, c.obs, c.logp64 = "%s_n%d" % (self.name, n), n, self.obs[idx].contiguous(), self.logp64[idx]
        c.value64 = None if self.value64 is None else self.value64[idx]
        return c

    def u(self, seed, ctr):
        return sampler_u(np.arange(self.n, dtype=np.uint64), ctr, seed)

    def near(self, seed, ctr):
        return near_edge(self.logp64.numpy(), self.u(seed, ctr))

    def actions64(self, seed, ctr):
        return sample_f64(self.logp64.numpy(), self.u(seed, ctr))


def _filtered_randn(kind, net, n, n_s, seed):
    """randn * 1.5 rows; rows on a knife edge (float64 network, never the kernel) are redrawn."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, n_s, generator=g) * 1.5
    net64 = copy.deepcopy(net).double()
    redrawn = 0
    for _ in range(20):
        close = knife_edges(kind, net64, obs.double())
        if not bool(close.any()):
            break
        redrawn += int(close.sum())
        obs[close] = torch.randn(int(close.sum()), n_s, generator=g) * 1.5
    return obs, redrawn


@functools.lru_cache(maxsize=None)
def synthetic_case(kind, n_s, n_a, gain, n=257):
    net = actor_net(n_s, n_a, gain) if kind == "act" else gi_net(n_s, n_a, gain)
    seed = OBS_SEED.get((kind, n_s, n_a, gain), 11)
    obs, redrawn = _filtered_randn(kind, net, n, n_s, seed)
    return Case(kind, "%s_s%d_a%d_g%d_n%d" % (kind, n_s, n_a, gain, n), net, obs, n_a, redrawn)


@functools.lru_cache(maxsize=None)
def recorded_case(kind, tag, n=257):
    """The recorded rollout states of a golden file (ro*_states) under the checkpoint stored beside them, knife-edge rows
    left out, tiled to n rows."""
    z = np.load(os.path.join(GOLDEN, tag + ".npz"))
    meta = json.loads(str(z["meta"]))
    if kind == "act":
        net = ActorNetwork(meta["n_s"], 128, meta["n_a"])
        net.load_state_dict({k[len("w_actor."):]: torch.tensor(z[k]) for k in z.files if k.startswith("w_actor.")})
    else:
        net = ActorCriticNetwork(meta["n_s"], meta["n_a"], 128, 1, state_split=True)
        net.load_state_dict({k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w_")})
    rows = np.concatenate([z["ro%d_states" % k].reshape(-1, meta["n_s"]) for k in range(meta["K"])])
    obs = torch.tensor(rows, dtype=torch.float32)
    close = knife_edges(kind, copy.deepcopy(net).double(), obs.double())
    obs = obs[~close]
    assert obs.shape[0] >= 100, tag
    obs = obs[torch.arange(n) % obs.shape[0]].contiguous()
    return Case(kind, "%s_%s_n%d" % (kind, tag, n), net, obs, meta["n_a"], int(close.sum()))


def grid_a(kind):
    return [synthetic_case(kind, n_s, n_a, gain) for n_s in (NS_ACT if kind == "act" else NS_GI) for n_a in NA_GRID for gain in GAINS]


def recorded_cases(kind):
    return [recorded_case(k, tag) for k, tag in RECORDED if k == kind]


def case_b(kind, n):
    """Grid B: the 257 rows of the n_s = 30, n_a = 5, gain 3 case, cut or tiled to n rows."""
    base = synthetic_case(kind, 30, 5, 3)
    return base.tiled(n)


def case_c(kind, n_a, n):
    base = synthetic_case(kind, 30, n_a, 3)
    return base if n == base.n else base.tiled(n)


# ---------------------------------------------------------------------------------------------------------------------
# calling the entries (oracle library with CPU tensors, HIP library with device tensors)
def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if t.is_cuda else None


def _ptr(t):
    return None if t is None else t.data_ptr()


def counter_tensor(value, device):
    value = int(value) & U64
    return torch.tensor([value - (1 << 64) if value >= (1 << 63) else value], dtype=torch.int64, device=device)


def counter_value(t):
    return int(t) & U64


def launch(clib, kind, weights, obs, n, n_s, n_a, seed, counter, actions, logp, value=None):
    """The raw entry: tensors (or None) in, status code out."""
    if kind == "act":
        return clib.lib.mm_policy_act(_ptr(obs), n, n_s, *[_ptr(w) for w in weights], 128, n_a, seed, _ptr(counter), _ptr(actions),
                                      _ptr(logp), _stream(obs))
    return clib.lib.mm_policy_gi_act(_ptr(obs), n, n_s, *[_ptr(w) for w in weights], 128, n_a, seed, _ptr(counter), _ptr(actions),
                                     _ptr(logp), _ptr(value), _stream(obs))


def run(clib, kind, weights, obs, n_a, seed, ctr, n=None):
    """One call with fresh sentinel-filled outputs; returns {actions, logp, value (gi), counter} (counter: the value after)."""
    n = obs.shape[0] if n is None else n
    dev = obs.device
    out = {"actions": torch.full((n,), -1, dtype=torch.int32, device=dev),
           "logp": torch.full((n, n_a), float("nan"), dtype=torch.float32, device=dev),
           "value": torch.full((n,), float("nan"), dtype=torch.float32, device=dev) if kind == "gi" else None}
    c = counter_tensor(ctr, dev)
    clib.check(launch(clib, kind, weights, obs, n, obs.shape[1], n_a, seed, c, out["actions"], out["logp"], out["value"]))
    out["counter"] = counter_value(c)
    return out


def sample(clib, logp, seed, ctr):
    """mm_sample_actions on logp [n, n_a]; returns (actions, counter after)."""
    n, n_a = logp.shape
    logp = logp.contiguous()
    out = torch.full((n,), -1, dtype=torch.int32, device=logp.device)
    c = counter_tensor(ctr, logp.device)
    clib.check(clib.lib.mm_sample_actions(logp.data_ptr(), n, n_a, seed, c.data_ptr(), out.data_ptr(), _stream(logp)))
    return out, counter_value(c)


@torch.no_grad()
def module_outputs(case, net, obs):
    """{logp, value} of a torch module (float32 on the kernel's device, or the float64 copy)."""
    return {"logp": net(obs), "value": net(obs, out_type="v")[:, 0] if case.kind == "gi" else None}


# ---------------------------------------------------------------------------------------------------------------------
# the rule
def compare(store, case, kernel, f32, f64, factor=4.0):
    """kernel / f32 / f64: {output name: tensor or None}.  Prints, records into store[case] and asserts the module
    docstring's rule per output tensor."""
    rec, bad = {}, []
    for name in sorted(f64):
        if f64[name] is None:
            continue
        g64 = f64[name].double().cpu()
        gk, g32 = kernel[name].double().cpu(), f32[name].double().cpu()
        e32 = float((g32 - g64).abs().max())
        err = float((gk - g64).abs().max())
        mx = float(g64.abs().max())
        bound = factor * e32 + 1e-6 * max(1.0, mx)
        rec[name] = {"e32": e32, "kernel_err": err, "max_abs": mx, "bound": bound}
        print("%-36s %-6s e32 %.3e kernel %.3e max %.3e bound %.3e" % (case, name, e32, err, mx, bound))
        if not err <= bound:
            bad.append((name, err, bound))
    store[case] = rec
    assert not bad, (case, bad)
    return rec


def check_forward(store, clib, case, device, seed=SEED_A, ctr=CTR_A, f64_actions=True):
    """One case through its entry on `device`: the rule on log-probabilities (and values), the row properties, the counter,
    actions == mm_sample_actions on the kernel's own log-probabilities, and (f64_actions) == the float64 inverse CDF under
    the numpy Philox outside the BAND.  Returns the kernel's outputs."""
    net = copy.deepcopy(case.net).to(device)
    obs = case.obs.to(device)
    out = run(clib, case.kind, weights_of(case.kind, net), obs, case.n_a, seed, ctr)
    f32 = module_outputs(case, net, obs)
    compare(store, case.name, out, f32, {"logp": case.logp64, "value": case.value64})
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


# equal low words, different high words -- of the counter (bit 32, bit 63) and of the seed
HIGH_PAIRS = (((99, 5), (99, (1 << 32) + 5)), ((99, 1), (99, (1 << 63) + 1)), ((0, 8), (1 << 32, 8)),
              ((0x7F4A7C15, 8), (0x9E3779B97F4A7C15, 8)))


def check_high_words(clib, case, device):
    """Equal low words with different high words must give different action vectors (n >= 257, n_a >= 2)."""
    assert case.n >= 257 and case.n_a >= 2
    w = weights_of(case.kind, copy.deepcopy(case.net).to(device))
    obs = case.obs.to(device)
    for (s0, c0), (s1, c1) in HIGH_PAIRS:
        a0 = run(clib, case.kind, w, obs, case.n_a, s0, c0)["actions"]
        a1 = run(clib, case.kind, w, obs, case.n_a, s1, c1)["actions"]
        assert not torch.equal(a0, a1), (case.name, hex(s1), hex(c1))
        assert np.array_equal(a0.cpu().numpy(), case.actions64(s0, c0)) or case.near(s0, c0).any()


# ---------------------------------------------------------------------------------------------------------------------
# guarded buffers: writes are checked inside ONE allocation, nothing here can fault
def _sentinel(dtype):
    return float("nan") if dtype.is_floating_point else -12345


def guarded(n_elems, dtype, device, pad=64, offset_elems=1):
    """(view, check): a view of n_elems elements that starts pad + offset_elems elements into a sentinel-filled allocation
    (NaN for floats, -12345 for int32) -- 4-byte aligned, not 16-byte aligned -- and a checker that every element outside
    the view still holds the sentinel."""
    lo = pad + offset_elems
    buf = torch.full((lo + n_elems + pad,), _sentinel(dtype), dtype=dtype, device=device)
    view = buf[lo:lo + n_elems]
    assert view.data_ptr() % 4 == 0 and (offset_elems % 4 == 0 or view.data_ptr() % 16 != 0)

    def check():
        outside = torch.cat([buf[:lo], buf[lo + n_elems:]])
        ok = torch.isnan(outside) if dtype.is_floating_point else outside == _sentinel(dtype)
        assert bool(ok.all()), "a write outside [0, n) of a %s output" % dtype

    return view, check


def offset_copy(t, offset_elems=1):
    """A copy of t that starts offset_elems elements into its allocation: 4-byte aligned, not 16-byte aligned."""
    buf = torch.empty(t.numel() + offset_elems + 3, dtype=t.dtype, device=t.device)
    v = buf[offset_elems:offset_elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == 0 and v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------------------------------------
# mm_sample_actions alone: masked and unnormalised rows (oracle and HIP)
def check_sampler_rows(clib, device, n=257, seed=SEEDS_C[2], ctr=CTRS_C[1]):
    for n_a in range(1, 9):
        g = torch.Generator().manual_seed(100 + n_a)
        # one-hot rows made with -inf: the action is the finite index
        hot = torch.arange(n) % n_a
        rows = torch.full((n, n_a), -float("inf"))
        rows[torch.arange(n), hot] = 0.0
        a, c = sample(clib, rows.to(device), seed, ctr)
        assert torch.equal(a.cpu().long(), hot) and c == ctr + 1, n_a
        if n_a >= 3:
            # two or more -inf entries per row (never all): every sampled action has a finite entry, and the draw is the
            # float64 inverse CDF's
            lp = torch.log_softmax(torch.randn(n, n_a, generator=g) * 2, -1)
            masked = torch.rand(n, n_a, generator=g).argsort(-1) < 2 + torch.arange(n)[:, None] % (n_a - 2)
            rows = torch.where(masked, torch.tensor(-float("inf")), lp)
            assert int(masked.sum(-1).min()) >= 2 and int((~masked).sum(-1).min()) >= 1
            a, _ = sample(clib, rows.to(device), seed, ctr)
            a = a.cpu().long()
            assert bool(torch.isfinite(rows[torch.arange(n), a]).all()), n_a
            assert not bool(((a == 0) & masked[:, 0]).any()), n_a
            u = sampler_u(np.arange(n, dtype=np.uint64), ctr, seed)
            near = near_edge(rows.double().numpy(), u)
            assert np.array_equal(a.numpy()[~near], sample_f64(rows.double().numpy(), u)[~near]), n_a
        # unnormalised rows: logp + c draws what logp draws
        lp = torch.log_softmax(torch.randn(n, n_a, generator=g) * 2, -1)
        a0, _ = sample(clib, lp.to(device), seed, ctr)
        u = sampler_u(np.arange(n, dtype=np.uint64), ctr, seed)
        near = near_edge(lp.double().numpy(), u)
        assert np.array_equal(a0.cpu().numpy()[~near], sample_f64(lp.double().numpy(), u)[~near]), n_a
        for shift in (-3.0, 2.0):
            a1, _ = sample(clib, (lp + shift).to(device), seed, ctr)
            differs = (a1 != a0).cpu().numpy()
            assert not differs[~near].any() and differs.sum() <= 1, (n_a, shift)  # (lp + c rounds: a BAND row may move)


# ---------------------------------------------------------------------------------------------------------------------
# mm_discount_returns: the edge list, bit for bit against the torch chain (rollout.discount_rewards)
def discount_edges(shapes):
    """(T, E, N, dones mode, gamma, reward_scale, alias) for every (T, E, N) of `shapes`."""
    out = []
    for T, E, N in shapes:
        for mode in ("random", "all", "none"):
            for gamma in (0.0, 1.0, 0.99):
                for scale in (20.0, 0.0, -1.0):
                    out.append((T, E, N, mode, gamma, scale, False))
        out.append((T, E, N, "random", 0.99, 20.0, True))
    return out


def _bits(t):
    return t.contiguous().view(torch.int64)


def check_discount(clib, device, edge):
    T, E, N, mode, gamma, scale, alias = edge
    g = torch.Generator().manual_seed(1000 * T + 10 * E + N)
    rewards = (torch.rand(T, E, N, dtype=torch.float64, generator=g) - 0.3) * 7
    dones = {"random": (torch.rand(T, E, generator=g) < 0.3), "all": torch.ones(T, E, dtype=torch.bool),
             "none": torch.zeros(T, E, dtype=torch.bool)}[mode].to(torch.uint8)
    final = torch.randn(E, N, dtype=torch.float64, generator=g)
    want = discount_rewards(rewards / scale if scale > 0 else rewards, dones, final, gamma)
    r, d, f = rewards.to(device), dones.to(device), final.to(device)
    if alias:
        got, chk = r, lambda: None
    else:
        got, chk = guarded(T * E * N, torch.float64, device)
    stream = _stream(r)
    assert clib.lib.mm_discount_returns(r.data_ptr(), d.data_ptr(), f.data_ptr(), T, E, N, gamma, scale, got.data_ptr(), stream) == 0
    if r.is_cuda:
        torch.cuda.synchronize()
    chk()
    assert torch.equal(_bits(got.cpu().view(T, E, N)), _bits(want)), edge
    if not alias:
        assert torch.equal(_bits(r.cpu()), _bits(rewards)), edge  # the inputs are read-only


def check_discount_empty(clib, device):
    """T = 0 and n_env = 0: MM_OK, nothing written."""
    r = torch.ones(6, dtype=torch.float64, device=device)
    d = torch.zeros(6, dtype=torch.uint8, device=device)
    f = torch.ones(6, dtype=torch.float64, device=device)
    for T, E in ((0, 2), (3, 0), (0, 0)):
        out = torch.full((6,), float("nan"), dtype=torch.float64, device=device)
        assert clib.lib.mm_discount_returns(r.data_ptr(), d.data_ptr(), f.data_ptr(), T, E, 3, 0.99, 20.0, out.data_ptr(), _stream(r)) == 0
        if r.is_cuda:
            torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), (T, E)
