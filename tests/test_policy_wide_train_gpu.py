"""mm_policy_wide_train / mm_policy_wide_eval (include/mm_policy_wide_train.h) and PPOLearner with hidden-512 networks on the
MI355X: both losses and the twelve gradients against torch.autograd in float64 on synthetic batches, the per-sample
diagnostics and the evaluation against the float64 modules, determinism and graph capture, degenerate and refused calls, the
optimiser steps against a float64 restatement, DeviceRollout.interact() -> train() on the steer_vel env.

There is no recorded reference run at this size (one 512 pair's parameters alone are 2.2 MB): the objective does not depend on
the hidden size and tests/golden/mappo_train_* pin its literal [B, B] form at 128, so float64 autograd on the reference's own
modules (rollout.ActorNetwork / CriticNetwork) is the measure.

The tolerance is measured, not fixed (the rule of tests/test_policy_train_gpu.py): per tensor e32 = max-abs(grad_f32_torch -
grad_f64), and the kernel's max-abs error must be <= 4 e32 + 1e-6 max-abs(grad_f64).  The per-sample outputs follow the same
shape of rule: error <= 4 x the float32 torch module's own max error against float64 on that batch + 1e-6 max(1, |x|)."""
import copy
import ctypes
import json
import os

import pytest
import torch

import policy_wide_train_util as U
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import PPOLearner, _mlp_struct
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout
from policy_train_util import GRAD_NAMES, NAMES, loss_and_grads, one_hot, sums_of

pytestmark = pytest.mark.gpu

ERRORS = {}  # case -> measured figures; _dump_errors writes their summary when the module is done
LR = 1e-4
OPT_EPS = 1e-8  # torch's default eps of RMSprop and of Adam


@pytest.fixture(scope="module", autouse=True)
def _dump_errors(tmp_path_factory):
    """Writes the summary of the measured figures when the module is done: to $MM_GRAD_ERROR_JSON when set (that is how
    profiles/policy_wide_train/grad_error.json is regenerated), else to pytest's temporary directory."""
    yield
    path = os.environ.get("MM_GRAD_ERROR_JSON") or str(tmp_path_factory.mktemp("policy_wide_train") / "grad_error.json")
    ERRORS["knife"] = {"KNIFE": U.KNIFE, "max_redraw_share": U.MAX_REDRAW_SHARE}
    with open(path, "w") as f:  # one case per line, three significant digits
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(_rounded(ERRORS[k]), sort_keys=True))
                                   for k in sorted(ERRORS)) + "\n}\n")
    print("measured figures: %s" % path)


def _rounded(x):
    """What is written per case: the tensor closest to its bound -- its name, e32, the kernel's error (or the parameter
    difference of an optimiser-step comparison) and that error as a fraction of the bound."""
    if isinstance(x, dict) and x and all(isinstance(v, dict) and "bound" in v for v in x.values()):
        key = "kernel_err" if "kernel_err" in next(iter(x.values())) else "param_diff"
        frac = lambda k: x[k][key] / x[k]["bound"] if x[k]["bound"] > 0 else (0.0 if x[k][key] == 0 else float("inf"))  # noqa: E731
        name = max(x, key=frac)
        return {"worst": name, "of_bound": float("%.3g" % frac(name)), "e32": _rounded(x[name]["e32"]),
                key: _rounded(x[name][key])}
    if isinstance(x, dict):
        return {k: _rounded(v) for k, v in x.items()}
    return float("%.3g" % x) if isinstance(x, float) else x


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _nets(n_s, n_a=5, seed=5):
    actor, critic = U.nets(n_s, n_a, seed)
    return actor.cuda(), critic.cuda()


def _learner(actor, critic, **kw):
    """A PPOLearner whose targets have moved away from the networks (as after a few optimiser steps)."""
    learner = PPOLearner(actor, critic, _lib(), **kw)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for p in list(learner.actor_target.parameters()) + list(learner.critic_target.parameters()):
            p.add_(0.01 * torch.randn(p.shape, generator=g).cuda())
    return learner


def _grads_of(actor, critic):
    out = []
    for net in (actor, critic):
        named = dict(net.named_parameters())
        out += [named[k].grad.detach().clone() for k in NAMES]
    return out


def _poison(actor, critic):
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.grad.fill_(float("nan"))  # written, not accumulated


def _compare(case, kernel, f32, f64):
    """kernel / f32 / f64: (loss [2], [12 gradients]).  Prints, records and asserts the module docstring's rule."""
    rec, bad = {}, []
    rows = [("loss", kernel[0].double(), f32[0].double(), f64[0])] + [
        (k, kernel[1][i].double(), f32[1][i].double(), f64[1][i]) for i, k in enumerate(GRAD_NAMES)]
    for name, gk, g32, g64 in rows:
        e32 = float((g32 - g64).abs().max())
        err = float((gk - g64).abs().max())
        mx = float(g64.abs().max())
        bound = 4.0 * e32 + 1e-6 * mx
        rec[name] = {"e32": e32, "kernel_err": err, "max_abs": mx, "bound": bound}
        print("%-44s %-22s e32 %.3e kernel %.3e max %.3e bound %.3e" % (case, name, e32, err, mx, bound))
        if not err <= bound:
            bad.append((name, err, bound))
    ERRORS[case] = rec
    assert not bad, (case, bad)
    return rec


def _batch(learner, n, n_s, ratio, strided, with_valid, seed, n_a=5):
    """A synthetic batch, tests/test_policy_train_gpu.py's _batch with the host half in policy_wide_train_util.draw_inputs;
    returns (obs, actions, returns, old_logp, advantages, valid) after the population checks of the inputs: both clip sides
    and the band, both advantage signs, both sides of the huber knee, every action."""
    host_a, host_c = copy.deepcopy(learner.actor).cpu(), copy.deepcopy(learner.critic).cpu()
    obs_h, act_h, noise_h, k_h, redrawn = U.draw_inputs(host_a, host_c, n, n_s, n_a, strided, seed)
    key = "n%d_s%d_a%d_%s_seed%d" % (n, n_s, n_a, "strided" if strided else "contig", seed)
    ERRORS.setdefault("knife_redraw_share", {})[key] = redrawn / float(n)
    if n == U.SMALL_N:
        assert redrawn == 0
    k, noise = k_h.cuda(), noise_h.cuda()
    if strided:  # states[:, agent_id, :] of a [B, N, S] tensor, actions / returns[:, agent_id] of [B, N]
        g = torch.Generator().manual_seed(seed + 1000)
        full = (torch.randn(n, 3, n_s, generator=g) * 1.5).cuda()
        full[:, 1, :] = obs_h.cuda()
        obs = full[:, 1, :]
        acts = torch.randint(0, n_a, (n, 3), generator=g, dtype=torch.int32).cuda()
        acts[:, 1] = act_h.cuda()
        act = acts[:, 1]
        assert not obs.is_contiguous() and act.stride(0) == 3
    else:
        obs, act = obs_h.cuda(), act_h.cuda()
    a64, c64 = copy.deepcopy(learner.actor).double(), copy.deepcopy(learner.critic).double()
    # the float32 torch modules' own pre-activation error on this batch, on the device: what KNIFE is four times of
    z32 = U.preactivations(learner.actor, learner.critic, obs.contiguous(), act)
    z64 = U.preactivations(a64, c64, obs.double(), act)
    ERRORS.setdefault("preactivation_f32_error", {})[key] = max(float((x.double() - y).abs().max()) for x, y in zip(z32, z64))
    oh = one_hot(act, n_a, torch.float64)
    with torch.no_grad():
        logp = a64(obs.double()).gather(1, act.long().unsqueeze(1)).squeeze(1)
        value = c64(obs.double(), oh).squeeze(1)
        tvalue = copy.deepcopy(learner.critic_target).double()(obs.double(), oh).squeeze(1)
    ret64 = value + 1.5 * noise.double() + 0.3  # |value - return| on both sides of the huber knee, a mean away from zero
    if strided:
        ret = torch.zeros(n, 3, device="cuda")
        ret[:, 1] = ret64.float()
        ret = ret[:, 1]
    else:
        ret = ret64.float()
    if ratio == "one":
        old = logp.float()
    else:
        u = 0.5 + 1.1 * (k.double() + 0.5) / n
        near = ((u - 0.8).abs() < 1e-3) | ((u - 1.2).abs() < 1e-3)  # nobody on a clip edge
        u = torch.where(near, u + 2.5e-3, u)
        old = (logp - torch.log(u)).float()
    valid = None
    if with_valid:
        valid = (~torch.isin(k % 10, torch.tensor([2, 5, 8], device="cuda"))).to(torch.uint8)
    adv = learner.advantages(obs, act, ret, valid)
    keep = slice(None) if valid is None else valid.bool()
    r = torch.exp(logp - old.double())[keep]
    adv64 = (ret.double() - tvalue)[keep]
    assert float((adv.double()[keep] - adv64).abs().max()) <= 1e-4  # the float32 advantages are those of the critic target
    d = (value - ret.double()).abs()[keep]
    sets = [adv64 > 0, adv64 < 0, d < 1.0, d > 1.0]
    if ratio == "one":
        assert float((r - 1).abs().max()) < 1e-5
    else:
        sets += [r < 0.8, r > 1.2, (r >= 0.8) & (r <= 1.2)]
        assert float(((r - 0.8).abs() < 1e-4).sum() + ((r - 1.2).abs() < 1e-4).sum()) == 0
    for m in sets:
        assert float(m.double().mean()) >= 0.10 and int(m.sum()) >= 3, (n, int(m.sum()), int(m.numel()))
    counts = torch.bincount(act[keep].long(), minlength=n_a)
    assert int(counts.numel()) == n_a and float(counts.min()) >= float(counts.sum()) / (2 * n_a)  # every one-hot column is hit
    return obs, act, ret, old, adv, valid


def _torch_sides(learner, obs, act, ret, old, adv, valid, form, sums, critic_loss, clip=0.2):
    actor, critic = learner.actor, learner.critic
    a32, c32, a64, c64 = copy.deepcopy(actor), copy.deepcopy(critic), copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    f32 = loss_and_grads(a32, c32, obs, act, ret, old, clip, critic_loss, form, advantages=adv, adv_sums=sums, valid=valid)
    f64 = loss_and_grads(a64, c64, obs.double(), act, ret.double(), old.double(), clip, critic_loss, form, advantages=adv.double(),
                         adv_sums=None if sums is None else sums.double(), valid=valid)
    return f32, f64


def _launch(learner, obs, act, ret, old, adv, valid, form, diagnostics=False):
    sums = sums_of(adv) if form == "reference" else None
    out = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums, advantages=None if sums is not None else adv,
                                diagnostics=diagnostics)
    return sums, out


def _module_outputs(actor, critic, obs, act, n_a):
    """(logp_taken, value) of the float32 torch modules and of their float64 copies."""
    with torch.no_grad():
        idx = act.long().clamp(0, n_a - 1).unsqueeze(1)
        lp32 = actor(obs).gather(1, idx).squeeze(1)
        v32 = critic(obs, one_hot(idx.squeeze(1), n_a, torch.float32)).squeeze(1)
        lp64 = copy.deepcopy(actor).double()(obs.double()).gather(1, idx).squeeze(1)
        v64 = copy.deepcopy(critic).double()(obs.double(), one_hot(idx.squeeze(1), n_a, torch.float64)).squeeze(1)
    return lp32, v32, lp64, v64


def _check_rows(case, name, mine, t32, t64, keep):
    """The diagnostics rule: |mine - f64| <= 4 max|f32_torch - f64| + 1e-6 max(1, |f64|), on the kept rows."""
    e32 = float((t32.double() - t64)[keep].abs().max())
    err = (mine.double() - t64).abs()[keep]
    bound = 4.0 * e32 + 1e-6 * t64.abs().clamp(min=1.0)[keep]
    ERRORS.setdefault(case, {})[name] = {"e32": e32, "kernel_err": float(err.max()), "bound": float(bound.min())}
    print("%-44s %-22s e32 %.3e kernel %.3e" % (case, name, e32, float(err.max())))
    assert bool((err <= bound).all()), (case, name, float(err.max()), e32)


CROSS = [(1000, n_s, form, cl, v, st, r) for n_s in (25, 30) for form in ("reference", "flat") for cl in ("mse", "huber")
         for v in (False, True) for st in (False, True) for r in ("one", "spread")]
ENDS = [(n, n_s, form, "huber", True, True, "spread") for n in (U.SMALL_N, U.N_WRAP) for n_s in (25, 30) for form in ("reference", "flat")]


@pytest.mark.parametrize("n,n_s,form,critic_loss,with_valid,strided,ratio", ENDS + CROSS)
def test_gradient_matches_autograd(n, n_s, form, critic_loss, with_valid, strided, ratio):
    """n = 31: less than a tile.  N_WRAP: the per-sample launch's persistent loop wraps with a ragged last tile and the
    weight-gradient pass has several slices, the last one shorter (asserted from the header's macros)."""
    if n == U.N_WRAP:
        tiles, per, slices = U.slicing(n)
        assert tiles > U.MAX_GRID * U.WAVES and n % U.TILE != 0 and slices >= 2 and tiles % per != 0
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic, critic_loss=critic_loss)
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, ratio, strided, with_valid, seed=U.batch_seed(n, n_s))
    _poison(actor, critic)
    sums, (loss, (lp, v, r)) = _launch(learner, obs, act, ret, old, adv, valid, form, diagnostics=True)
    kernel = (loss.clone(), _grads_of(actor, critic))
    f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, valid, form, sums, critic_loss)
    case = "n%d_s%d_%s_%s_%s_%s_%s" % (n, n_s, form, critic_loss, "valid" if with_valid else "all",
                                     "strided" if strided else "contig", ratio)
    _compare(case, kernel, f32, f64)
    # diagnostics: log-probability, value and ratio per sample (zeros in masked slots)
    lp32, v32, lp64, v64 = _module_outputs(actor, critic, obs, act, 5)
    keep = torch.ones(n, dtype=torch.bool, device="cuda") if valid is None else valid.bool()
    _check_rows("diag_" + case, "logp", lp, lp32, lp64, keep)
    _check_rows("diag_" + case, "value", v, v32, v64, keep)
    _check_rows("diag_" + case, "ratio", r, torch.exp(lp32 - old), torch.exp(lp64 - old.double()), keep)
    if valid is not None:
        assert float(lp[~keep].abs().max()) == 0.0 and float(r[~keep].abs().max()) == 0.0 and float(v[~keep].abs().max()) == 0.0
    # the diagnostics are the evaluation's outputs, bit for bit
    elp, ev = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    assert torch.equal(elp, lp) and torch.equal(ev, v)


@pytest.mark.parametrize("form", ["reference", "flat"])
@pytest.mark.parametrize("n_a", [1, 8])
def test_action_counts(n_a, form):
    """The ends of the n_a range, masked and strided: the critic's fc2 is [512][513] and [512][520], every one-hot column
    populated (asserted in _batch)."""
    n, n_s = 1000, 30
    actor, critic = _nets(n_s, n_a=n_a)
    assert tuple(critic.fc2.weight.shape) == (512, 512 + n_a)
    learner = _learner(actor, critic, critic_loss="huber")
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, True, seed=11 + n_a, n_a=n_a)
    _poison(actor, critic)
    sums, loss = _launch(learner, obs, act, ret, old, adv, valid, form)
    kernel = (loss.clone(), _grads_of(actor, critic))
    f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, valid, form, sums, "huber")
    _compare("n_a%d_%s" % (n_a, form), kernel, f32, f64)


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_one_network_alone(which):
    """Either network may be left out: the other's gradient and loss are the ones of the joint call, bit for bit, and the
    omitted network's .grad is not touched."""
    n, n_s = 1000, 30
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic)
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, True, seed=21)
    joint = learner.loss_and_grad(obs, act, ret, old, valid=valid, advantages=adv).clone()
    both = _grads_of(actor, critic)
    _poison(actor, critic)
    loss = learner.loss_and_grad(obs, act, ret, old, valid=valid, advantages=adv, networks=which)
    alone = _grads_of(actor, critic)
    mine = slice(0, 6) if which == "actor" else slice(6, 12)
    other = slice(6, 12) if which == "actor" else slice(0, 6)
    assert all(torch.equal(x, y) for x, y in zip(both[mine], alone[mine]))
    assert all(bool(torch.isnan(x).all()) for x in alone[other])
    i = 0 if which == "actor" else 1
    assert float(loss[1 - i]) == 0.0 and float(loss[i]) != 0.0 and float(loss[i]) == float(joint[i])


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("with_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("n,n_s,n_a", [(31, 25, 5), (3001, 30, 5), (1000, 32, 8), (1000, 30, 1)])
def test_eval_matches_the_float64_modules(n, n_s, n_a, with_valid, strided):
    """mm_policy_wide_eval under the diagnostics rule, zeros in masked slots, either network alone equal to the joint call.
    n_a = 5 and 1 read the critic's fc2 with 4-byte loads (rows of 517 and 513 floats), n_a = 8 with 16-byte loads."""
    actor, critic = _nets(n_s, n_a=n_a, seed=8)
    learner = PPOLearner(actor, critic, _lib())
    g = torch.Generator().manual_seed(n + n_s)
    if strided:
        obs = (torch.randn(n, 3, n_s, generator=g) * 1.5).cuda()[:, 2, :]
        act = torch.randint(0, n_a, (n, 3), generator=g, dtype=torch.int32).cuda()[:, 2]
    else:
        obs = (torch.randn(n, n_s, generator=g) * 1.5).cuda()
        act = torch.randint(0, n_a, (n,), generator=g, dtype=torch.int32).cuda()
    valid = (torch.rand(n, generator=g) > 0.3).to(torch.uint8).cuda() if with_valid else None
    keep = torch.ones(n, dtype=torch.bool, device="cuda") if valid is None else valid.bool()
    lp, v = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    lp32, v32, lp64, v64 = _module_outputs(actor, critic, obs, act, n_a)
    case = "eval_n%d_s%d_a%d_%s_%s" % (n, n_s, n_a, "valid" if with_valid else "all", "strided" if strided else "contig")
    _check_rows(case, "logp", lp, lp32, lp64, keep)
    _check_rows(case, "value", v, v32, v64, keep)
    if valid is not None:
        assert float(lp[~keep].abs().max()) == 0.0 and float(v[~keep].abs().max()) == 0.0
    lp1, none = learner.evaluate(obs, act, actor=actor, valid=valid)
    none2, v1 = learner.evaluate(obs, act, critic=critic, valid=valid)
    assert none is None and none2 is None and torch.equal(lp1, lp) and torch.equal(v1, v)
    if not with_valid:  # the learner's wrappers are that call on the targets (fresh targets == the networks)
        assert torch.equal(learner.old_log_probs(obs, act), lp)
        ret = torch.randn(n, generator=g).cuda()
        assert torch.equal(learner.advantages(obs, act, ret), ret - v)


def test_eval_rows_do_not_depend_on_their_place():
    """The same 75 rows first, last and alone in launches of different n: their outputs are the same bits."""
    n_s, m, fill = 30, 75, 70003  # (75 rows: 2 tiles and a ragged third; the long launch wraps the persistent loop)
    actor, critic = _nets(n_s, seed=8)
    learner = PPOLearner(actor, critic, _lib())
    g = torch.Generator().manual_seed(5)
    rows, racts = (torch.randn(m, n_s, generator=g) * 1.5).cuda(), torch.randint(0, 5, (m,), generator=g, dtype=torch.int32).cuda()
    other, oacts = (torch.randn(fill, n_s, generator=g) * 1.5).cuda(), torch.randint(0, 5, (fill,), generator=g, dtype=torch.int32).cuda()
    alone = learner.evaluate(rows, racts, actor=actor, critic=critic)
    first = learner.evaluate(torch.cat([rows, other]), torch.cat([racts, oacts]), actor=actor, critic=critic)
    last = learner.evaluate(torch.cat([other[:1003], rows]), torch.cat([oacts[:1003], racts]), actor=actor, critic=critic)
    for a, f, l in zip(alone, first, last):
        assert torch.equal(a, f[:m]) and torch.equal(a, l[-m:]) and bool(torch.isfinite(a).all())


def test_deterministic_and_graph_capturable():
    n, n_s = U.N_WRAP, 30
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic)
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, True, seed=77)
    sums = sums_of(adv)
    runs = []
    for _ in range(2):
        _poison(actor, critic)
        loss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        runs.append([loss.clone()] + _grads_of(actor, critic))
    for x, y in zip(*runs):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    # capture + replay == eager, bit for bit
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_eval = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        geval = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    _poison(actor, critic)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(runs[0], [gloss] + _grads_of(actor, critic)):
        assert torch.equal(x, y)
    assert torch.equal(eager_eval[0], geval[0]) and torch.equal(eager_eval[1], geval[1])


def _train_batch(B, N, n_s, seed):
    g = torch.Generator().manual_seed(seed)
    states = (torch.randn(B, N, n_s, generator=g) * 1.5).cuda()
    actions = torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32).cuda()
    returns = torch.randn(B, N, generator=g).cuda()
    return states, actions, returns


def _all_params(learner):
    return [p.detach().clone() for net in (learner.actor, learner.critic, learner.actor_target, learner.critic_target)
            for p in net.parameters()]


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
def test_fused_train_in_a_graph(optimizer_type):
    """train() with fused_step=True captured in a graph: the replay leaves the parameters and targets the eager call leaves."""
    states, actions, returns = _train_batch(500, 3, 30, seed=31)
    kw = dict(fused_step=True, optimizer_type=optimizer_type, target_tau=0.5, target_update_steps=2)
    eager = _learner(*_nets(30), **kw)
    captured = _learner(*_nets(30), **kw)
    eager.train(states, actions, returns, n_episodes=2)
    captured._ensure_scratch(500)  # (allocated before the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a twin: the captured learner's state must not move before the replay
        _learner(*_nets(30), **kw).train(states, actions, returns, n_episodes=2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = _all_params(captured)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.train(states, actions, returns, n_episodes=2)
    graph.replay()
    torch.cuda.synchronize()
    after = _all_params(captured)
    for x, y, z in zip(_all_params(eager), after, before):
        assert torch.equal(x, y) and not torch.equal(y, z) and bool(torch.isfinite(y).all())


def test_degenerate_inputs():
    actor, critic = _nets(30)
    learner = _learner(actor, critic)
    zero = lambda loss: float(loss.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in _grads_of(actor, critic))  # noqa: E731
    _poison(actor, critic)
    e = torch.empty(0, 30, device="cuda")
    ei, ef = torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, device="cuda")
    assert zero(learner.loss_and_grad(e, ei, ef, ef, advantages=ef))
    lp, v = learner.evaluate(e, ei, actor=actor, critic=critic)
    assert lp.shape == (0,) and v.shape == (0,)
    obs, act, ret, old, adv, _ = _batch(learner, 1000, 30, "spread", False, False, seed=U.batch_seed(1000, 30))
    obs, act, ret, old, adv = obs[:500], act[:500], ret[:500], old[:500], adv[:500]
    off = torch.zeros(500, dtype=torch.uint8, device="cuda")
    _poison(actor, critic)
    assert zero(learner.loss_and_grad(obs, act, ret, old, advantages=adv, valid=off))
    _poison(actor, critic)
    assert zero(learner.loss_and_grad(obs, act, ret, old, adv_sums=sums_of(adv), valid=off))
    # n == 1: the batch mean over one sample, against float64 autograd under the module's rule
    _poison(actor, critic)
    one = (obs[:1], act[:1], ret[:1], old[:1])
    loss = learner.loss_and_grad(*one, advantages=adv[:1])
    f32, f64 = _torch_sides(learner, *one, adv[:1], None, "flat", None, "mse")
    _compare("n1_flat_mse", (loss.clone(), _grads_of(actor, critic)), f32, f64)
    # masked slots may hold anything: NaN observations / returns / advantages and out-of-range actions there change nothing
    valid = torch.ones(500, dtype=torch.uint8, device="cuda")
    valid[::3] = 0
    clean = [learner.loss_and_grad(obs, act, ret, old, advantages=adv, valid=valid).clone()] + _grads_of(actor, critic)
    clean_eval = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    obs2, act2, ret2, old2, adv2 = obs.clone(), act.clone(), ret.clone(), old.clone(), adv.clone()
    obs2[::3] = float("nan"); ret2[::3] = float("nan"); old2[::3] = float("nan"); adv2[::3] = float("nan"); act2[::3] = 1000
    dirty = [learner.loss_and_grad(obs2, act2, ret2, old2, advantages=adv2, valid=valid).clone()] + _grads_of(actor, critic)
    for x, y in zip(clean, dirty):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    for x, y in zip(clean_eval, learner.evaluate(obs2, act2, actor=actor, critic=critic, valid=valid)):
        assert torch.equal(x, y)
    # an out-of-range action in a valid slot is clamped, not read out of bounds
    act3 = act.clone(); act3[0] = 99; act3[1] = -4
    act4 = act.clone(); act4[0] = 4; act4[1] = 0
    a = [learner.loss_and_grad(obs, act3, ret, old, advantages=adv).clone()] + _grads_of(actor, critic)
    b = [learner.loss_and_grad(obs, act4, ret, old, advantages=adv).clone()] + _grads_of(actor, critic)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    torch.cuda.synchronize()


CANARY = 7.25


def test_refused_calls_write_nothing():
    """Every MM_ERR_INVALID_ARG case of the header: ValueError through clib.check, and the loss, the gradients, the
    diagnostics and the scratch -- each surrounded by canary elements inside its own allocation -- are as they were."""
    n, n_s = 500, 30
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic)
    clib = _lib()
    g = torch.Generator().manual_seed(4)
    obs = (torch.randn(n, n_s, generator=g) * 1.5).cuda()
    act = torch.randint(0, 5, (n,), generator=g, dtype=torch.int32).cuda()
    ret, old, adv = torch.randn(n, generator=g).cuda(), -torch.rand(n, generator=g).cuda() - 1.0, torch.randn(n, generator=g).cuda()
    sums = sums_of(adv)
    Wa, Wc, Ga, Gc = _mlp_struct(actor), _mlp_struct(critic), _mlp_struct(actor, True), _mlp_struct(critic, True)
    need = clib.policy_wide_train_scratch_bytes(n)
    pad = 64
    guarded = torch.full((pad + 2 + pad + n + pad,), CANARY, device="cuda")  # canaries | loss [2] | canaries | probe [n] | canaries
    loss, probe = guarded[pad:pad + 2], guarded[2 * pad + 2:2 * pad + 2 + n]
    arena = torch.full((pad + need + pad,), 0x5A, dtype=torch.uint8, device="cuda")  # canaries | scratch | canaries
    base = arena.data_ptr() + pad
    base += (-base) % 16
    assert base + need <= arena.data_ptr() + arena.numel()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = lambda st: None if st is None else ctypes.byref(st)  # noqa: E731

    def fill():
        guarded.fill_(CANARY)
        arena.fill_(0x5A)
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.grad.fill_(CANARY)

    def untouched():
        torch.cuda.synchronize()
        return (bool((guarded == CANARY).all()) and bool((arena == 0x5A).all())
                and all(bool((p.grad == CANARY).all()) for p in list(actor.parameters()) + list(critic.parameters())))

    def direct(entry="mm_policy_wide_train", hidden=512, n_a=5, crit=0, wa=Wa, wc=Wc, ga=Ga, gc=Gc, sums=None, advp=adv.data_ptr(),
               loss=loss.data_ptr(), value=None, logp=None, ratio=None, n=n, sc=base, sc_bytes=need, n_s=n_s, stride=n_s, clip=0.2,
               obsp=obs.data_ptr(), oldp=old.data_ptr(), retp=ret.data_ptr()):
        clib.check(getattr(clib.lib, entry)(obsp, stride, n, n_s, act.data_ptr(), 1, retp, 1, oldp, None, ref(wa), ref(wc), hidden,
                                            n_a, clip, crit, sums, advp, ref(ga), ref(gc), loss, logp, value, ratio, sc, sc_bytes,
                                            stream))

    hollow = abi.MMMlpParams()
    for name in abi.MLP_PARAMS[:-1]:
        setattr(hollow, name, getattr(Wa, name))  # b3 left NULL
    refused = [dict(hidden=128), dict(hidden=256), dict(hidden=64), dict(sc=None), dict(sc_bytes=need - 1), dict(sc=base + 4),
               dict(sc=base + 8), dict(advp=None), dict(sums=sums.data_ptr()),  # neither / both forms of the advantages
               dict(n_s=24), dict(n_s=33), dict(stride=29), dict(clip=-0.1), dict(clip=float("nan")), dict(n_a=0), dict(n_a=9),
               dict(crit=2), dict(wa=None, wc=None, ga=None, gc=None), dict(ga=None), dict(wc=None), dict(gc=None), dict(loss=None),
               dict(n=-1), dict(n=2 ** 31), dict(wa=hollow), dict(obsp=None), dict(oldp=None), dict(retp=None),
               dict(wa=None, ga=None, advp=None, logp=probe.data_ptr()), dict(wa=None, ga=None, advp=None, ratio=probe.data_ptr()),
               dict(wc=None, gc=None, value=probe.data_ptr()),
               dict(entry="mm_policy_train", hidden=512)]  # the hidden-128 entry still refuses this size
    assert U.M["MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN"] == 16
    for kw in refused:
        fill()
        with pytest.raises(ValueError):
            direct(**kw)
        assert untouched(), kw
    # the evaluation: the other hidden sizes, a network without its output, an output without its network, no network
    ev = lambda *a: clib.check(clib.lib.mm_policy_wide_eval(obs.data_ptr(), n_s, n, n_s, act.data_ptr(), 1, None, *a, stream))  # noqa: E731
    for args in ((ref(Wa), None, 128, 5, probe.data_ptr(), None), (ref(Wa), None, 256, 5, probe.data_ptr(), None),
                 (ref(Wa), None, 512, 5, None, None), (None, None, 512, 5, probe.data_ptr(), None),
                 (None, ref(Wc), 512, 5, probe.data_ptr(), None), (ref(Wa), None, 512, 9, probe.data_ptr(), None)):
        fill()
        with pytest.raises(ValueError):
            ev(*args)
        assert untouched(), args
    with pytest.raises(ValueError):  # and the hidden-128 evaluation refuses 512
        clib.check(clib.lib.mm_policy_eval(obs.data_ptr(), n_s, n, n_s, act.data_ptr(), 1, None, ref(Wa), None, 512, 5,
                                           probe.data_ptr(), None, stream))
    # the well-formed calls go through, stay inside their buffers and agree with the learner's
    fill()
    direct(value=probe.data_ptr())
    direct(wa=None, ga=None, advp=None)  # the critic alone needs no advantages
    torch.cuda.synchronize()
    assert bool((guarded[:pad] == CANARY).all()) and bool((guarded[pad + 2:2 * pad + 2] == CANARY).all())
    assert bool((guarded[-pad:] == CANARY).all())
    lo = base - arena.data_ptr()
    assert bool((arena[:lo] == 0x5A).all()) and bool((arena[lo + need:] == 0x5A).all())
    mine = _grads_of(actor, critic)
    want_loss, (_, want_value, _) = learner.loss_and_grad(obs, act, ret, old, advantages=adv, diagnostics=True)
    assert torch.equal(probe, want_value) and float(loss[1]) == float(want_loss[1]) and float(loss[0]) == 0.0
    assert all(torch.equal(x, y) for x, y in zip(mine, _grads_of(actor, critic)))
    # the learner's own argument errors
    for width in (24, 28, 33):  # not the networks' state size
        with pytest.raises(ValueError):
            learner.loss_and_grad(torch.randn(8, width, device="cuda"), act[:8], ret[:8], old[:8], advantages=adv[:8])
        with pytest.raises(ValueError):
            learner.evaluate(torch.randn(8, width, device="cuda"), act[:8], actor=actor)
    with pytest.raises(ValueError):
        learner.loss_and_grad(obs, act, ret, old)
    with pytest.raises(ValueError):
        learner.loss_and_grad(obs, act, ret, old, advantages=adv, adv_sums=sums)
    torch.cuda.synchronize()


def _named(learner, target=False):
    a, c = (learner.actor_target, learner.critic_target) if target else (learner.actor, learner.critic)
    out = {"actor." + k: v for k, v in a.named_parameters()}
    out.update({"critic." + k: v for k, v in c.named_parameters()})
    return out


def _restated_step(learner, optimizer_type, obs, act, ret, old, adv, states):
    """One agent step in float64 from the learner's own pre-step parameters and optimiser state: autograd of the literal
    [B, B] objective, clip_grad_norm_, torch.optim.  Returns ({name: post-step parameter}, {name: e32})."""
    f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, None, "literal", None, learner.critic_loss, learner.clip_param)
    e32 = {k: float((x.double() - y).abs().max()) for k, x, y in zip(GRAD_NAMES, f32[1], f64[1])}
    out = {}
    for prefix, net, sd, grads in (("actor.", learner.actor, states["actor_optimizer"], f64[1][:6]),
                                   ("critic.", learner.critic, states["critic_optimizer"], f64[1][6:])):
        net64 = copy.deepcopy(net).double()
        opt = (torch.optim.Adam if optimizer_type == "adam" else torch.optim.RMSprop)(net64.parameters(), lr=LR)
        sd = copy.deepcopy(sd)
        for st in sd["state"].values():
            for key in st:
                if key != "step":
                    st[key] = st[key].double()
        opt.load_state_dict(sd)
        named = dict(net64.named_parameters())
        for k, gr in zip(NAMES, grads):
            named[k].grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(net64.parameters(), learner.max_grad_norm)
        opt.step()
        out.update({prefix + k: named[k].detach() for k in NAMES})
    return out, e32


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
def test_learner_steps_match_a_float64_restatement(optimizer_type):
    """PPOLearner.train(form="reference") over N = 3 agents; after every agent step the parameters against a float64 torch
    restatement (literal [B, B] autograd + clip_grad_norm_ + torch.optim) started from the learner's own pre-step parameters
    and optimiser state.  The bound is tests/test_policy_train_gpu.py's, (lr / eps) 4 e32 + 1e-7 per tensor with e32 the
    float32 torch gradient's error on that tensor.  It holds for every RMSprop step: the step lr g / (sqrt(a v + (1 - a) g^2) +
    eps) has |d step / d g| <= lr / (sqrt(..) + eps) <= lr / eps whatever the carried v >= 0 is.  Adam's step lr m^ / (sqrt(v^) +
    eps) has the same first term (d m^ / d g = (1 - b1) / (1 - b1^t) <= 1) and a second one through the denominator,
    |m^| / (sqrt(v^) + eps) . |d sqrt(v^) / d g| / (sqrt(v^) + eps) <= ((1 - b1) / sqrt(1 - b2)) . 1 / eps = 3.17 / eps, so
    Adam's factor is (1 + 3.17) lr / eps.  Then the soft update at n_episodes = target_update_steps."""
    B, N, n_s = 96, 3, 30
    factor = (LR / OPT_EPS) * (1.0 if optimizer_type == "rmsprop" else 1.0 + 0.1 / (1e-3 ** 0.5))
    states, actions, returns = _train_batch(B, N, n_s, seed=41)
    learner = _learner(*_nets(n_s), optimizer_type=optimizer_type, target_tau=0.5, target_update_steps=2)
    targets0 = {k: v.detach().clone() for k, v in _named(learner, True).items()}
    observed = {}
    for rnd in range(2):  # the second round steps from a non-trivial optimiser state
        for a in range(N):
            obs, act, ret = states[:, a, :], actions[:, a], returns[:, a]
            old, adv = learner.old_log_probs(obs, act), learner.advantages(obs, act, ret)
            want, e32 = _restated_step(learner, optimizer_type, obs, act, ret, old, adv, learner.optimizer_state_dict())
            last = rnd == 1 and a == N - 1
            learner.train(states[:, a:a + 1], actions[:, a:a + 1], returns[:, a:a + 1], n_episodes=2 if last else 0)
            for k, p in _named(learner).items():
                diff = float((p.detach().double() - want[k]).abs().max())
                bound = factor * 4.0 * e32[k] + 1e-7
                observed["r%d_a%d_%s" % (rnd, a, k)] = {"param_diff": diff, "bound": bound, "e32": e32[k]}
                print("%s r%d a%d %-22s diff %.3e bound %.3e" % (optimizer_type, rnd, a, k, diff, bound))
                assert diff <= bound, (rnd, a, k, diff, bound)
                assert bool(torch.isfinite(p).all())
            if not last:
                for k, t in _named(learner, True).items():
                    assert torch.equal(t.detach(), targets0[k])
    for k, t in _named(learner, True).items():  # t = (1 - tau) t + tau s, once, in float32
        want = 0.5 * targets0[k].double() + 0.5 * _named(learner)[k].detach().double()
        assert float((t.detach().double() - want).abs().max()) <= 2e-7 * max(1.0, float(want.abs().max())), k
    ERRORS["learner_steps_%s" % optimizer_type] = observed


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
def test_fused_step_against_the_torch_step(optimizer_type):
    """tests/test_opt_step_gpu.py's criterion for the two paths: bit-identical gradients, post-step parameters within 2^-22
    max|p| per tensor, last_grad_norm within 1e-6."""
    states, actions, returns = _train_batch(96, 3, 30, seed=43)
    fused = _learner(*_nets(30), optimizer_type=optimizer_type, fused_step=True)
    plain = _learner(*_nets(30), optimizer_type=optimizer_type)
    start = _all_params(plain)
    col = (states[:, :1], actions[:, :1], returns[:, :1])
    fused.train(*col)
    plain.train(*col)
    nf, npl = fused.last_grad_norm, plain.last_grad_norm
    assert float(((nf - npl).abs() / npl).max()) <= 1e-6
    for x, y, z in zip(_all_params(fused)[:12], _all_params(plain)[:12], start[:12]):
        diff, bound = float((x - y).abs().max()), 2.0 ** -22 * float(y.abs().max())
        assert diff <= bound and not torch.equal(y, z), (diff, bound)


def test_rollout_to_train_end_to_end():
    """DeviceRollout on merge-multi-agent-v1 with lateral_control = steer_vel, 256 envs x 4 agents x 10 steps, 512 actor and
    critic, fused act -> train(): the parameters move, everything is finite, poll_errors() is clean, and the next rollout acts
    with the updated weights."""
    from marl_mass_amd import VecMergeEnv
    E, N, T = 256, 4, 10
    torch.manual_seed(3)
    env = VecMergeEnv(E, N, env_id="merge-multi-agent-v1", seed=9, auto_reset=True,
                      config={"safety_guarantee": "cbf-av", "HEADWAY_TIME": 0.5, "lateral_control": "steer_vel"})
    actor, critic = ActorNetwork(env.n_s, 512, 5).cuda(), CriticNetwork(env.n_s, 5, 512).cuda()
    first_policy = copy.deepcopy(actor)
    start = [p.detach().clone() for p in list(actor.parameters()) + list(critic.parameters())]
    ro = DeviceRollout(env, actor, critic, roll_out_n_steps=T, sample_seed=4)
    assert not ro.shared and ro.fused_policy is True
    learner = PPOLearner(actor, critic, env.clib)
    assert learner.hidden == 512
    out = ro.interact()
    losses = learner.train(out)
    assert len(losses) == N and all(bool(torch.isfinite(x).all()) for x in losses)
    now = list(actor.parameters()) + list(critic.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in now) and all(not torch.equal(p.detach(), q) for p, q in zip(now, start))
    out2 = ro.interact()
    torch.cuda.synchronize()
    env.poll_errors()
    assert all(bool(torch.isfinite(out2[k].float()).all()) for k in ("states", "returns"))
    obs = out2["states"][0].reshape(-1, env.n_s).float().contiguous()
    acts = out2["actions"][0].reshape(-1).to(torch.int32)
    new_lp, _ = learner.evaluate(obs, acts, actor=actor)
    old_lp, _ = learner.evaluate(obs, acts, actor=first_policy)
    assert bool(torch.isfinite(new_lp).all()) and not torch.equal(new_lp, old_lp)
    # the rollout acted with the updated weights: its first step's actions are a draw from them -- every taken action has
    # positive probability under the new policy, and the new policy is the module's
    with torch.no_grad():
        want = actor(obs).gather(1, acts.long().unsqueeze(1)).squeeze(1)
    assert float((new_lp - want).abs().max()) <= 1e-4
