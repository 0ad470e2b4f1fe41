"""mm_policy_gi_train (include/mm_policy_gi_train.h) and SharedPPOLearner on the MI355X: the loss and the twelve gradients
against torch.autograd in float64, on synthetic batches and on the batches the reference's MAPPO_GI.train() ran on
(tests/golden/gi_train_*.npz); the optimiser steps against the reference's recorded parameters; determinism, graph capture,
degenerate inputs; DeviceRollout.interact() -> train() end to end.

The tolerance is measured, not fixed: in each comparison the float32 torch.autograd gradient is computed too,
e32 = max-abs(grad_f32_torch - grad_f64) per tensor, and the kernel's max-abs error must be <= 4 e32 + 1e-6 max-abs(grad_f64).
Both are float32 sums of n terms in a different order (split-K partial blocks here, rocBLAS there) and either may be the
luckier one, hence the margin of 4; a layout or masking bug shows as an error of the gradient's own size."""
import copy
import ctypes
import json
import os

import pytest
import torch

from gi_train_util import FIXTURES, GRAD_NAMES, fixture_net, load_fixture, loss_and_grads
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import SharedPPOLearner, _params
from marl_mass_amd.rollout import ActorCriticNetwork, DeviceRollout

pytestmark = pytest.mark.gpu

ERRORS = {}  # case -> measured figures; _dump_errors writes their summary when the module is done
LR, RMS_EPS = 1e-4, 1e-8


@pytest.fixture(scope="module", autouse=True)
def _dump_errors(tmp_path_factory):
    """Writes the summary of the measured figures when the module is done: to $MM_GRAD_ERROR_JSON when set (that is how
    profiles/policy_gi_train/grad_error.json is regenerated), else to pytest's temporary directory -- a test run leaves the
    checkout as it found it."""
    yield
    path = os.environ.get("MM_GRAD_ERROR_JSON") or str(tmp_path_factory.mktemp("policy_gi_train") / "grad_error.json")
    with open(path, "w") as f:  # one case per line, three significant digits
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(_rounded(ERRORS[k]), sort_keys=True))
                                   for k in sorted(ERRORS)) + "\n}\n")
    print("measured figures: %s" % path)


def _rounded(x):
    """What is written per case: the tensor closest to its bound -- its name, e32, the kernel's error (or the parameter
    difference of an optimiser-step comparison) and that error as a fraction of the bound."""
    if isinstance(x, dict) and x and all(isinstance(v, dict) for v in x.values()):
        key = "kernel_err" if "kernel_err" in next(iter(x.values())) else "param_diff"
        frac = lambda k: x[k][key] / x[k]["bound"] if x[k]["bound"] > 0 else (0.0 if x[k][key] == 0 else float("inf"))  # noqa: E731
        name = max(x, key=frac)  # (a bound of 0: a gradient that is identically zero, e.g. the actor head with one action)
        return {"worst": name, "of_bound": float("%.3g" % frac(name)), "e32": _rounded(x[name]["e32"]),
                key: _rounded(x[name][key])}
    if isinstance(x, dict):
        return {k: _rounded(v) for k, v in x.items()}
    return float("%.3g" % x) if isinstance(x, float) else x


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _net(n_s, n_a=5, seed=5):
    torch.manual_seed(seed)
    net = ActorCriticNetwork(n_s, n_a, 128, 1, state_split=True).cuda()
    with torch.no_grad():  # asymmetric, non-trivial scales in every layer
        for m in (net.fc11, net.fc12, net.fc13, net.fc2):
            m.bias.uniform_(-0.5, 0.5)
        net.actor_linear.bias.uniform_(-1, 1); net.actor_linear.weight.mul_(3.0)
        net.critic_linear.bias.fill_(0.5); net.critic_linear.weight.mul_(2.0)
    return net


def _grads_of(net):
    named = dict(net.named_parameters())
    return [named[k].grad.detach().clone() for k in GRAD_NAMES]


def _compare(case, kernel, f32, f64):
    """kernel / f32 / f64: (loss [3], [12 gradients]).  Prints, records and asserts the module docstring's rule."""
    rec = {}
    bad = []
    rows = [("loss", kernel[0].double(), f32[0].double(), f64[0])] + [
        (k, kernel[1][i].double(), f32[1][i].double(), f64[1][i]) for i, k in enumerate(GRAD_NAMES)]
    for name, gk, g32, g64 in rows:
        e32 = float((g32 - g64).abs().max())
        err = float((gk - g64).abs().max())
        mx = float(g64.abs().max())
        bound = 4.0 * e32 + 1e-6 * mx
        rec[name] = {"e32": e32, "kernel_err": err, "max_abs": mx, "bound": bound}
        print("%-40s %-22s e32 %.3e kernel %.3e max %.3e bound %.3e" % (case, name, e32, err, mx, bound))
        if not err <= bound:
            bad.append((name, err, bound))
    ERRORS[case] = rec
    assert not bad, (case, bad)
    return rec


KNIFE = 2e-5


@torch.no_grad()
def _knife_edges(net64, obs64):
    """Samples with a pre-activation of either hidden layer within KNIFE of zero (float64 network)."""
    s1, s2, s3 = net64.split(obs64)
    z1 = torch.cat([net64.fc11(s1), net64.fc12(s2), net64.fc13(s3)], 1)
    z2 = net64.fc2(torch.relu(z1))
    return (z1.abs().min(dim=1).values < KNIFE) | (z2.abs().min(dim=1).values < KNIFE)


def _batch(net, n, n_s, ratio, strided, with_valid, seed, n_a=5, knife_filter=True):
    """A synthetic batch; returns (obs, actions, returns, old_logp, valid) with the population checks of the inputs.

    The populations are stratified, not left to chance, so that the checks hold at n = 31 as well as at 524 301: a random
    permutation gives every sample a rank k; the ratio is the k-th point of an even grid over [0.5, 1.6], the advantage noise
    is negative for even k, and the mask drops k % 10 in {2, 5, 8} -- 30 % of the samples, evenly over the ratio grid and
    over both signs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:  # states[:, agent_id, :] of a [B, N, S] tensor, actions / returns[:, agent_id] of [B, N]
        obs = (torch.randn(n, 3, n_s, device="cuda", generator=g) * 1.5)[:, 1, :]
        act = torch.randint(0, n_a, (n, 3), device="cuda", generator=g, dtype=torch.int32)[:, 1]
        noise = torch.randn(n, 3, device="cuda", generator=g)[:, 1]
        assert not obs.is_contiguous() and act.stride(0) == 3
    else:
        obs = (torch.randn(n, n_s, device="cuda", generator=g) * 1.5).contiguous()
        act = torch.randint(0, n_a, (n,), device="cuda", generator=g, dtype=torch.int32)
        noise = torch.randn(n, device="cuda", generator=g)
    k = torch.randperm(n, device="cuda", generator=g)
    noise = noise.abs() * torch.where(k % 2 == 0, -1.0, 1.0)
    net64 = copy.deepcopy(net).double()
    # A ReLU whose pre-activation is within float32 rounding of zero is open in one float32 implementation and shut in
    # another: each such unit moves a gradient by O(1 / B), float32 torch against float64 as much as the kernel, and with
    # 1.5e8 pre-activations at the largest n a handful always exist -- e32 would then measure who drew the shorter straw,
    # not the rounding of a sum.  Like r on a clip edge these points are not differentiable and are not tested: samples with
    # a float64 pre-activation of either hidden layer closer to zero than KNIFE are redrawn (decided on the inputs with the
    # float64 network, never on the kernel).  KNIFE = 2e-5 is ~20 x the float32 error of a 160-term dot product of O(1) terms.
    redrawn = 0
    for _ in range(20 if knife_filter else 0):
        close = _knife_edges(net64, obs.double())
        if not bool(close.any()):
            break
        redrawn += int(close.sum())
        obs[close] = torch.randn(int(close.sum()), n_s, device="cuda", generator=g) * 1.5
    assert not knife_filter or not bool(_knife_edges(net64, obs.double()).any())
    if knife_filter:
        ERRORS.setdefault("knife_redraws", {})["n%d_s%d_%s" % (n, n_s, "strided" if strided else "contig")] = redrawn
    with torch.no_grad():
        logp = net64(obs.double()).gather(1, act.long().unsqueeze(1)).squeeze(1)
        value = net64(obs.double(), out_type="v").squeeze(1)
    # advantages of both signs, |value - return| on both sides of the huber knee.  The offset keeps mean(value - return), the
    # critic bias's one-element gradient, from cancelling to ~1e-5 of its terms: there the 1e-6 max-abs floor vanishes and the
    # test would compare two single random rounding draws.
    ret64 = value + 1.5 * noise.double() + 0.3
    if strided:
        ret = torch.zeros(n, 3, device="cuda")
        ret[:, 1] = ret64.float()
        ret = ret[:, 1]
    else:
        ret = ret64.float()
    if ratio == "one":
        old = logp.float()  # (the kernel's own float32 log-probabilities differ in the last bits: r = 1 +- 1e-6, inside the band)
    else:
        u = 0.5 + 1.1 * (k.double() + 0.5) / n
        # r exactly on 1 +- clip has measure zero and is not tested: move the few samples within 1e-3 of an edge off it, so
        # float32 and float64 put every sample on the same side
        near = ((u - 0.8).abs() < 1e-3) | ((u - 1.2).abs() < 1e-3)
        u = torch.where(near, u + 2.5e-3, u)
        old = (logp - torch.log(u)).float()
    valid = None
    if with_valid:
        valid = (~torch.isin(k % 10, torch.tensor([2, 5, 8], device="cuda"))).to(torch.uint8)
    # population of the INPUTS (float64 network), asserted for every n: both clip sides and the band, both signs of advantage,
    # >= 10 % of the valid samples each and never fewer than 3 samples
    keep = slice(None) if valid is None else valid.bool()
    r = torch.exp(logp - old.double())[keep]
    adv = (ret.double() - value)[keep]
    sets = [adv > 0, adv < 0]
    if ratio == "one":
        assert float((r - 1).abs().max()) < 1e-5
    else:
        sets += [r < 0.8, r > 1.2, (r >= 0.8) & (r <= 1.2)]
        assert float(((r - 0.8).abs() < 1e-4).sum() + ((r - 1.2).abs() < 1e-4).sum()) == 0  # nobody on a clip edge
    for m in sets:
        assert float(m.double().mean()) >= 0.10 and int(m.sum()) >= 3, (n, int(m.sum()), int(m.numel()))
    return obs, act, ret, old, valid


@pytest.mark.parametrize("ratio", ["one", "spread"])
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("with_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("critic_loss", ["mse", "huber"])
@pytest.mark.parametrize("form", ["reference", "flat"])
@pytest.mark.parametrize("n_s", [25, 30])
@pytest.mark.parametrize("n", [31, 1000, 524301])
def test_gradient_matches_autograd(n, n_s, form, critic_loss, with_valid, strided, ratio):
    net = _net(n_s)
    obs, act, ret, old, valid = _batch(net, n, n_s, ratio, strided, with_valid, seed=1 + n + n_s)
    learner = SharedPPOLearner(net, _lib(), critic_loss=critic_loss)
    sums = None
    if form == "reference":  # the same float32 (S+, S-) goes to the kernel and, as a constant, to both torch runs
        sums = learner.advantage_sums(obs, ret, valid)
    for p in net.parameters():
        p.grad.fill_(float("nan"))  # written, not accumulated
    loss, (lp, v, r) = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums, diagnostics=True)
    kernel = (loss.clone(), _grads_of(net))
    net32, net64 = copy.deepcopy(net), copy.deepcopy(net).double()
    args = lambda dt: (obs.to(dt), act, ret.to(dt), old.to(dt), 0.2, critic_loss, form)  # noqa: E731
    f32 = loss_and_grads(net32, *args(torch.float32), adv_sums=sums, valid=valid)
    f64 = loss_and_grads(net64, *args(torch.float64), adv_sums=None if sums is None else sums.double(), valid=valid)
    case = "n%d_s%d_%s_%s_%s_%s_%s" % (n, n_s, form, critic_loss, "valid" if with_valid else "all",
                                     "strided" if strided else "contig", ratio)
    _compare(case, kernel, f32, f64)
    # diagnostics: log-probability, value and ratio per sample (zeros in masked slots)
    with torch.no_grad():
        lp64 = net64(obs.double()).gather(1, act.long().unsqueeze(1)).squeeze(1)
        v64 = net64(obs.double(), out_type="v").squeeze(1)
    keep = torch.ones(n, dtype=torch.bool, device="cuda") if valid is None else valid.bool()
    assert float((lp.double() - lp64)[keep].abs().max()) <= 2e-5
    assert bool(((v.double() - v64).abs() <= 1e-5 * v64.abs().clamp(min=1.0))[keep].all())
    assert float((r.double() - torch.exp(lp64 - old.double()))[keep].abs().max()) <= 1e-4
    if valid is not None:
        assert float(lp[~keep].abs().max()) == 0.0 and float(r[~keep].abs().max()) == 0.0


@pytest.mark.parametrize("form", ["reference", "flat"])
@pytest.mark.parametrize("n_a", [1, 8])
def test_action_counts_and_advantage_sums(n_a, form):
    """The ends of the n_a range (every other case has 5 actions), masked and strided; and learner.advantage_sums with a mask
    against an independent float64 computation on the kept rows."""
    n, n_s = 1000, 30
    net = _net(n_s, n_a=n_a)
    obs, act, ret, old, valid = _batch(net, n, n_s, "spread", True, True, seed=11 + n_a, n_a=n_a)
    learner = SharedPPOLearner(net, _lib(), critic_loss="huber")
    net32, net64 = copy.deepcopy(net), copy.deepcopy(net).double()
    sums = None
    if form == "reference":
        sums = learner.advantage_sums(obs, ret, valid)
        with torch.no_grad():
            adv = (ret.double() - net64(obs.double(), out_type="v").squeeze(1))[valid.bool()]
        ref = torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])
        assert float((sums.double() - ref).abs().max()) <= 1e-5 * float(adv.abs().sum())  # float32 values, float32 sum of 700
    loss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
    kernel = (loss.clone(), _grads_of(net))
    args = lambda dt: (obs.to(dt), act, ret.to(dt), old.to(dt), 0.2, "huber", form)  # noqa: E731
    f32 = loss_and_grads(net32, *args(torch.float32), adv_sums=sums, valid=valid)
    f64 = loss_and_grads(net64, *args(torch.float64), adv_sums=None if sums is None else sums.double(), valid=valid)
    _compare("n_a%d_%s" % (n_a, form), kernel, f32, f64)


def test_unfiltered_batch_figures():
    """What the knife-edge filter of _batch removes, in figures (profiles/policy_gi_train/grad_error.json, "unfiltered_*"):
    the largest batch WITHOUT the filter.  Each ReLU within float32 rounding of zero that one implementation opens and the
    other shuts moves a gradient element by one sample's contribution, O(1 / B) of an O(1) term, so here the float32 torch
    error and the kernel's error are both set by a handful of such units and either can exceed 4 x the other.  Asserted: the
    kernel's error stays of that size -- <= 1e-3 of each tensor's max-abs (reasoning: a flipped unit contributes at most
    |dz| |x| / B ~ 10 / 524 301 = 2e-5 against gradients of 1e-3 .. 1e-2, a few units per tensor; a layout or masking bug
    gives an error of the tensor's own size).  The 4 e32 rule is asserted on the filtered batches and on the fixtures."""
    n, n_s = 524301, 25
    net = _net(n_s)
    obs, act, ret, old, valid = _batch(net, n, n_s, "spread", True, False, seed=1 + n + n_s, knife_filter=False)
    net64 = copy.deepcopy(net).double()
    learner = SharedPPOLearner(net, _lib(), critic_loss="huber")
    loss = learner.loss_and_grad(obs, act, ret, old)
    kernel = (loss.clone(), _grads_of(net))
    args = lambda dt: (obs.to(dt), act, ret.to(dt), old.to(dt), 0.2, "huber", "flat")  # noqa: E731
    f32 = loss_and_grads(copy.deepcopy(net), *args(torch.float32))
    f64 = loss_and_grads(net64, *args(torch.float64))
    rec = {"samples_within_KNIFE": int(_knife_edges(net64, obs.double()).sum())}
    for name, gk, g32, g64 in zip(["loss"] + GRAD_NAMES, [kernel[0]] + kernel[1], [f32[0]] + f32[1], [f64[0]] + f64[1]):
        e32, err, mx = (float((g32.double() - g64).abs().max()), float((gk.double() - g64).abs().max()), float(g64.abs().max()))
        rec[name] = "e32 %.3g kernel %.3g max_abs %.3g" % (e32, err, mx)
        print("unfiltered %-22s %s" % (name, rec[name]))
        assert err <= 1e-3 * mx, (name, err, mx)
    ERRORS["unfiltered_n524301_s25_flat_huber_all_strided_spread"] = rec


def _fixture_step_inputs(z, a, device="cuda"):
    obs = torch.tensor(z["states"], device=device)[:, a, :]  # strided views, as train() takes them
    act = torch.tensor(z["actions"], device=device)[:, a]
    ret = torch.tensor(z["returns"], device=device)[:, a]
    return obs, act, ret


@pytest.mark.parametrize("loss_name,t", FIXTURES)
def test_reference_fixture_gradients(loss_name, t):
    """Losses and pre-clip gradients of every agent step the reference recorded: the kernel against float64 autograd of the
    LITERAL [B, B] expression (same rule), and against the recorded float32 numbers within that bound plus the recorded
    run's own distance from float64 (triangle inequality)."""
    z, meta = load_fixture(loss_name, t)
    target = fixture_net(z, meta, "tp_", device="cuda")
    for a in range(meta["n_agents"]):
        net = fixture_net(z, meta, "p_" if a == 0 else "a%d_q_" % (a - 1), device="cuda")
        learner = SharedPPOLearner(net, _lib(), critic_loss=loss_name, clip_param=meta["clip_param"])
        learner.policy_target.load_state_dict(target.state_dict())
        obs, act, ret = _fixture_step_inputs(z, a)
        old = learner.old_log_probs(obs, act)
        sums = learner.advantage_sums(obs, ret)
        loss = learner.loss_and_grad(obs, act, ret, old, adv_sums=sums)
        kernel = (loss.clone(), _grads_of(net))
        net32, net64 = copy.deepcopy(net), copy.deepcopy(net).double()
        f32 = loss_and_grads(net32, obs, act, ret, old, meta["clip_param"], loss_name, "literal")
        f64 = loss_and_grads(net64, obs.double(), act, ret.double(), old.double(), meta["clip_param"], loss_name, "literal")
        rec = _compare("fixture_%s_t%d_a%d" % (loss_name, t, a), kernel, f32, f64)
        recorded = [torch.tensor(z["a%d_losses" % a], device="cuda")] + [torch.tensor(z["a%d_g_%s" % (a, k)], device="cuda")
                                                                        for k in GRAD_NAMES]
        for name, gk, gr, g64 in zip(["loss"] + GRAD_NAMES, [kernel[0]] + kernel[1], recorded, [f64[0]] + f64[1]):
            slack = float((gr.double() - g64).abs().max())
            assert float((gk.double() - gr.double()).abs().max()) <= rec[name]["bound"] + slack, (a, name)


@pytest.mark.parametrize("loss_name", ["mse", "huber"])
def test_learner_reproduces_the_recorded_optimiser_steps(loss_name):
    """SharedPPOLearner.train(form="reference") from the recorded initial parameters, train 0 then train 1 with the same
    learner (RMSprop's state carries over, no soft update in between, as in the recorded run), against the recorded
    post-step parameters of every agent step.  RMSprop's first step is lr g / (0.1 |g| + eps): an element whose gradient is
    rounding noise around zero moves by up to (lr / eps) dg, so per tensor the bound is (lr / eps) 4 e32 + 1e-7 with e32 the
    float32 torch error on that tensor (max over the agent steps), never the kernel's own."""
    z0, meta0 = load_fixture(loss_name, 0)
    net = fixture_net(z0, meta0, "p_", device="cuda")
    learner = SharedPPOLearner(net, _lib(), lr=meta0["lr"], optimizer_type=meta0["optimizer_type"], critic_loss=loss_name,
                               clip_param=meta0["clip_param"], max_grad_norm=meta0["max_grad_norm"],
                               target_tau=meta0["target_tau"], target_update_steps=meta0["target_update_steps"])
    whole = SharedPPOLearner(copy.deepcopy(net), _lib(), critic_loss=loss_name)
    observed = {}
    for t in (0, 1):
        z, meta = load_fixture(loss_name, t)
        states, actions, returns = (torch.tensor(z[k], device="cuda") for k in ("states", "actions", "returns"))
        e32 = dict.fromkeys(GRAD_NAMES, 0.0)
        for a in range(meta["n_agents"]):
            # e32 of this step: float32 vs float64 autograd at the RECORDED pre-step parameters
            pre = fixture_net(z, meta, "p_" if a == 0 else "a%d_q_" % (a - 1), device="cuda")
            obs, act, ret = _fixture_step_inputs(z, a)
            old = learner.old_log_probs(obs, act)
            g32 = loss_and_grads(pre, obs, act, ret, old, meta["clip_param"], loss_name, "literal")[1]
            g64 = loss_and_grads(copy.deepcopy(pre).double(), obs.double(), act, ret.double(), old.double(), meta["clip_param"],
                                 loss_name, "literal")[1]
            for k, x, y in zip(GRAD_NAMES, g32, g64):
                e32[k] = max(e32[k], float((x.double() - y).abs().max()))
            # one agent step = train() on that agent's column alone
            learner.train(states[:, a:a + 1], actions[:, a:a + 1], returns[:, a:a + 1], n_episodes=meta["n_episodes"])
            named = dict(net.named_parameters())
            for k in GRAD_NAMES:
                diff = float((named[k].detach() - torch.tensor(z["a%d_q_%s" % (a, k)], device="cuda")).abs().max())
                bound = (LR / RMS_EPS) * 4.0 * e32[k] + 1e-7
                observed["t%d_a%d_%s" % (t, a, k)] = {"param_diff": diff, "bound": bound, "e32": e32[k]}
                print("%s t%d a%d %-22s diff %.3e bound %.3e" % (loss_name, t, a, k, diff, bound))
                assert diff <= bound, (t, a, k, diff, bound)
        # the same N steps as ONE train() call: bit-identical to the column-by-column learner
        whole.train(states, actions, returns, n_episodes=meta["n_episodes"])
        for p, q in zip(net.parameters(), whole.policy.parameters()):
            assert torch.equal(p, q)
    ERRORS["learner_steps_%s" % loss_name] = observed


def test_deterministic_and_graph_capturable():
    n, n_s = 70001, 30
    net = _net(n_s)
    obs, act, ret, old, valid = _batch(net, n, n_s, "spread", True, True, seed=77)
    learner = SharedPPOLearner(net, _lib())
    sums = learner.advantage_sums(obs, ret, valid)
    runs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad.fill_(float("nan"))
        loss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        runs.append([loss.clone()] + _grads_of(net))
    for x, y in zip(*runs):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    # capture + replay == eager, bit for bit
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
    for p in net.parameters():
        p.grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(runs[0], [gloss] + _grads_of(net)):
        assert torch.equal(x, y)


def test_degenerate_inputs():
    net = _net(30)
    learner = SharedPPOLearner(net, _lib())
    for p in net.parameters():
        p.grad.fill_(float("nan"))
    e = torch.empty(0, 30, device="cuda")
    loss = learner.loss_and_grad(e, torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, device="cuda"),
                                 torch.empty(0, device="cuda"))
    assert float(loss.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in _grads_of(net))
    obs, act, ret, old, _ = _batch(net, 500, 30, "spread", False, False, seed=3)
    for p in net.parameters():
        p.grad.fill_(float("nan"))
    loss = learner.loss_and_grad(obs, act, ret, old, valid=torch.zeros(500, dtype=torch.uint8, device="cuda"))
    assert float(loss.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in _grads_of(net))
    # masked slots may hold anything: NaN observations / returns and out-of-range actions there change nothing
    valid = torch.ones(500, dtype=torch.uint8, device="cuda")
    valid[::3] = 0
    clean = [learner.loss_and_grad(obs, act, ret, old, valid=valid).clone()] + _grads_of(net)
    obs2, act2, ret2 = obs.clone(), act.clone(), ret.clone()
    obs2[::3] = float("nan"); ret2[::3] = float("nan"); act2[::3] = 1000
    dirty = [learner.loss_and_grad(obs2, act2, ret2, old, valid=valid).clone()] + _grads_of(net)
    for x, y in zip(clean, dirty):
        assert torch.equal(x, y)
    # an out-of-range action in a valid slot is clamped, not read out of bounds
    act3 = act.clone(); act3[0] = 99; act3[1] = -4
    act4 = act.clone(); act4[0] = 4; act4[1] = 0
    a = [learner.loss_and_grad(obs, act3, ret, old).clone()] + _grads_of(net)
    b = [learner.loss_and_grad(obs, act4, ret, old).clone()] + _grads_of(net)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    # invalid arguments -> ValueError through clib.check
    with pytest.raises(ValueError):
        learner.loss_and_grad(torch.randn(8, 24, device="cuda"), act[:8], ret[:8], old[:8])  # n_s < 25
    with pytest.raises(ValueError):
        learner.loss_and_grad(torch.randn(8, 33, device="cuda"), act[:8], ret[:8], old[:8])  # n_s > 32
    small = SharedPPOLearner(net, _lib())
    small._ensure_scratch = lambda n: torch.empty(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        small.loss_and_grad(obs, act, ret, old)  # scratch too small
    bad = SharedPPOLearner(net, _lib())
    bad.clip_param = -0.1
    with pytest.raises(ValueError):
        bad.loss_and_grad(obs, act, ret, old)
    clib = _lib()
    W, G = abi.MMGiParams(), abi.MMGiParams()
    for name, p in zip(abi.GI_PARAMS, _params(net)):
        setattr(W, name, p.detach().data_ptr()); setattr(G, name, p.grad.data_ptr())
    l3 = torch.empty(3, device="cuda")
    scratch = learner._ensure_scratch(500)
    direct = lambda hidden, n_a, crit: clib.check(clib.lib.mm_policy_gi_train(  # noqa: E731
        obs.data_ptr(), 30, 500, 30, act.data_ptr(), 1, ret.data_ptr(), 1, old.data_ptr(), None, ctypes.byref(W), hidden, n_a, 0.2,
        crit, None, ctypes.byref(G), l3.data_ptr(), None, None, None, scratch.data_ptr(), scratch.numel(),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    direct(128, 5, 0)  # the well-formed call goes through
    for hidden, n_a, crit in ((64, 5, 0), (256, 5, 0), (128, 0, 0), (128, 9, 0), (128, 5, 2)):
        with pytest.raises(ValueError):
            direct(hidden, n_a, crit)
    with pytest.raises(ValueError):  # NULL weights / outputs
        clib.check(clib.lib.mm_policy_gi_train(obs.data_ptr(), 30, 500, 30, act.data_ptr(), 1, ret.data_ptr(), 1, old.data_ptr(), None,
                                               None, 128, 5, 0.2, 0, None, None, None, None, None, None, None, 0, None))


def test_rollout_to_train_end_to_end():
    """DeviceRollout(shared) on 256 envs x 4 -> train(form="flat"), three rounds; round one repeated with the gradient taken
    by float32 torch autograd (same optimiser, same rollout tensors): parameters within the per-tensor RMSprop bound."""
    from marl_mass_amd import VecMergeEnv
    E, N, T = 256, 4, 10
    net = _net(30, seed=3)
    start = copy.deepcopy(net)
    env = VecMergeEnv(E, N, seed=9, config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125,
                      qp_solver="exact", cbf_tau=0.5, auto_reset=True)
    ro = DeviceRollout(env, net, roll_out_n_steps=T, sample_seed=4)
    assert ro.shared and ro.fused_policy
    learner = SharedPPOLearner(net, env.clib)
    for rnd in range(3):
        out = ro.interact()
        if rnd == 0:
            kept = {k: out[k].clone() for k in ("states", "actions", "returns")}
        losses = learner.train(out, n_episodes=rnd, form="flat")
        assert len(losses) == 1 and bool(torch.isfinite(losses[0]).all())
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert all(not torch.equal(p, q) for p, q in zip(net.parameters(), start.parameters()))
    # round one again: once with the gradient by float32 torch autograd, once by the kernel, from the same parameters
    obs = kept["states"].reshape(-1, 30).float()
    act, ret = kept["actions"].reshape(-1), kept["returns"].reshape(-1).float()
    twin, again = copy.deepcopy(start), copy.deepcopy(start)
    tw = SharedPPOLearner(twin, env.clib)
    old = tw.old_log_probs(obs, act)
    g32 = loss_and_grads(twin, obs, act, ret, old, 0.2, "mse", "flat")[1]
    g64 = loss_and_grads(copy.deepcopy(twin).double(), obs.double(), act, ret.double(), old.double(), 0.2, "mse", "flat")[1]
    named = dict(twin.named_parameters())
    for k, g in zip(GRAD_NAMES, g32):
        named[k].grad = g.clone()
    tw._step(0)
    SharedPPOLearner(again, env.clib).train(kept, n_episodes=0, form="flat")
    observed = {}
    for k, x32, x64 in zip(GRAD_NAMES, g32, g64):
        e32 = float((x32.double() - x64).abs().max())
        bound = (LR / RMS_EPS) * 4.0 * e32 + 1e-7
        diff = float((dict(again.named_parameters())[k] - named[k]).detach().abs().max())
        moved = float((named[k] - dict(start.named_parameters())[k]).abs().max())
        observed[k] = {"param_diff": diff, "bound": bound, "e32": e32, "step_size": moved}
        print("end-to-end %-22s diff %.3e bound %.3e step %.3e" % (k, diff, bound, moved))
        assert diff <= bound, (k, diff, bound)
    ERRORS["end_to_end_round_one"] = observed
