"""mm_opt_step (include/mm_opt_step.h) and the learners' fused_step / soft_update_every on the MI355X.

1. the reference's recorded optimiser steps from its recorded gradients, the optimiser alone;
2. against clip_grad_norm_ + torch.optim in float64 with a MEASURED tolerance: per tensor the kernel's error may be
   4 e32 + K 2^-23 max|p|, e32 the float32 torch.optim error on that tensor (never the kernel's own);
3. bit-exact properties: the blend, determinism, graph replay;
4. the learners: fused against unfused, against the hand-composed sequence, state dicts in both directions, train() in a graph;
5. soft_update_every="agent_step";
6. arguments.
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import gi_train_util as gi
import policy_train_util as pt
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import PPOLearner, SharedPPOLearner, _mlp_params, _params
from opt_step_util import pre_step_prefix_of, recorded_runs, run_lr

pytestmark = pytest.mark.gpu

ERRORS = {}  # case -> measured figures; _dump_errors writes them when the module is done
ULP = 2.0 ** -23
ALPHA, B1, B2, EPS = 0.99, 0.9, 0.999, 1e-8  # torch.optim's defaults


@pytest.fixture(scope="module", autouse=True)
def _dump_errors(tmp_path_factory):
    """Writes the measured figures when the module is done: to $MM_OPT_STEP_ERROR_JSON when set (that is how
    profiles/opt_step/step_error.json is regenerated), else to pytest's temporary directory."""
    yield
    path = os.environ.get("MM_OPT_STEP_ERROR_JSON") or str(tmp_path_factory.mktemp("opt_step") / "step_error.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(ERRORS[k], sort_keys=True)) for k in sorted(ERRORS)) + "\n}\n")
    print("measured figures: %s" % path)


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def make_group(algo, params, grads=None, state1=None, state2=None, targets=None, step=None, lr=1e-4, a=None, b2=B2, eps=EPS,
               max_grad_norm=0.5, tau=1.0, soft_update=False, grad_norm=None):
    """An MMOptGroup over lists of device tensors (None entries: NULL pointers with count 0)."""
    g = abi.MMOptGroup()
    g.algo, g.n_tensors = algo, len(params)
    for i, p in enumerate(params):
        g.count[i] = 0 if p is None else p.numel()
        g.param[i] = _ptr(p)
        for name, lst in (("grad", grads), ("state1", state1), ("state2", state2), ("target", targets)):
            if lst is not None:
                getattr(g, name)[i] = _ptr(lst[i])
    g.step, g.grad_norm = _ptr(step), _ptr(grad_norm)
    g.lr, g.alpha_or_beta1, g.beta2, g.eps = lr, (a if a is not None else (B1 if algo == abi.OPT_ADAM else ALPHA)), b2, eps
    g.max_grad_norm = -1.0 if max_grad_norm is None else max_grad_norm
    g.tau, g.soft_update = tau, int(soft_update)
    return g


def launch(*groups):
    _lib().opt_step(list(groups), _stream())


def dev(x):
    return torch.tensor(np.asarray(x), device="cuda")


def _frac(diff, bound):
    return diff / bound if bound > 0 else (0.0 if diff == 0 else float("inf"))


# ---- 1. the reference's recorded steps ------------------------------------------------------------------------------------
RUNS = recorded_runs()


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_recorded_optimiser_steps(run):
    """Recorded pre-step parameters + recorded gradient -> mm_opt_step (all networks of the run in one launch), RMSprop's
    square_avg carried in the kernel's buffers from zeros through both trains: per tensor within 2^-22 max|q| of the recorded
    post-step parameters (each side rounds the stored parameter once, half an ulp each; the update's own arithmetic
    differences are below 0.01 ulp of the parameter; twice their sum).  grad_norm against the float64 norm of the recorded
    gradients to 1e-6.  The "soft" run's last step carries the soft update: both targets within tau 2^-22 max|q| +
    2^-23 max|t| of the recorded ones; everywhere else the targets stay bit for bit."""
    name, meta0, nets, steps = run
    z0 = steps[0][0]
    v = {n: [torch.zeros_like(dev(z0["p_" + k])) for k in keys] for n, keys in nets.items()}
    tgt = {n: [dev(z0["tp_" + k]) for k in keys] for n, keys in nets.items()}
    norms = torch.zeros(len(nets), device="cuda")
    worst = {"param": 0.0, "norm_rel": 0.0, "target": 0.0}
    for z, meta, a in steps:
        soft = bool(meta.get("soft_update_after_train")) and a == meta["agent_steps"] - 1
        before = {n: [t.clone() for t in tgt[n]] for n in nets}
        p = {n: [dev(z[pre_step_prefix_of(a) + k]) for k in keys] for n, keys in nets.items()}
        g = {n: [dev(z["a%d_g_%s" % (a, k)]) for k in keys] for n, keys in nets.items()}
        launch(*[make_group(abi.OPT_RMSPROP, p[n], g[n], v[n], targets=tgt[n], lr=run_lr(meta, n), max_grad_norm=meta["max_grad_norm"],
                            tau=meta["target_tau"], soft_update=soft, grad_norm=norms[i:i + 1]) for i, n in enumerate(nets)])
        for i, (n, keys) in enumerate(nets.items()):
            want = float(np.sqrt(sum(float(np.sum(z["a%d_g_%s" % (a, k)].astype(np.float64) ** 2)) for k in keys)))
            rel = abs(float(norms[i]) - want) / want
            worst["norm_rel"] = max(worst["norm_rel"], rel)
            assert rel <= 1e-6, (n, a, float(norms[i]), want)
            for j, k in enumerate(keys):
                q = z["a%d_q_%s" % (a, k)]
                diff, bound = float((p[n][j].double() - dev(q).double()).abs().max()), 2.0 ** -22 * float(np.abs(q).max())
                worst["param"] = max(worst["param"], _frac(diff, bound))
                print("%s t%d a%d %-24s diff %.3e bound %.3e" % (name, meta["train_index"], a, k, diff, bound))
                assert diff <= bound, (n, meta["train_index"], a, k, diff, bound)
                assert torch.equal(g[n][j], dev(z["a%d_g_%s" % (a, k)]))  # the gradient is read only
                if soft:
                    t_rec = z["after_tp_" + k]
                    tb = meta["target_tau"] * 2.0 ** -22 * float(np.abs(q).max()) + ULP * float(np.abs(t_rec).max())
                    td = float((tgt[n][j].double() - dev(t_rec).double()).abs().max())
                    worst["target"] = max(worst["target"], _frac(td, tb))
                    assert td <= tb, (n, k, td, tb)
                    assert not torch.equal(tgt[n][j], before[n][j])
                else:
                    assert torch.equal(tgt[n][j], before[n][j])
    softs = sum(bool(meta.get("soft_update_after_train")) for _, meta, a in steps if a == 0)
    assert softs == (1 if name == "mappo_soft" else 0)  # the one soft update the reference ran was exercised
    ERRORS["recorded_%s" % name] = {k: float("%.3g" % x) for k, x in worst.items()}


# ---- 2. torch.optim in float64, measured tolerance -------------------------------------------------------------------------
SIZES = [1, 3, 63, 64, 65, 1025, 4099, 17024]
UNALIGNED, ZERO_GRAD, K_STEPS = 1027, 3, 5  # the unaligned view's size; index (size 64) of the tensor whose gradient is zero


def _synthetic(seed):
    """Parameters (the last real one a view that starts 4 bytes into a larger buffer: the scalar path) and K gradient sets:
    the first large (clipped at 0.5), the third scaled to a total norm of 0.1 (below the bound: coef clamps to 1), tensor
    ZERO_GRAD's gradient zero throughout."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen).cuda() for n in SIZES]
    holder = torch.zeros(UNALIGNED + 8, device="cuda")
    holder[1:1 + UNALIGNED] = torch.randn(UNALIGNED, generator=gen).cuda()
    params.append(holder[1:1 + UNALIGNED])
    assert params[-1].data_ptr() % 16 == 4 and params[0].data_ptr() % 16 == 0
    sets = []
    for k, scale in enumerate([30.0, 1.0, None, 0.02, 1.0][:K_STEPS]):
        g = [torch.randn(p.numel(), generator=gen).cuda() * (scale or 1.0) for p in params]
        g[ZERO_GRAD].zero_()
        if scale is None:
            total = torch.sqrt(sum((x.double() ** 2).sum() for x in g))
            g = [(x * (0.1 / total)).float() for x in g]
        sets.append(g)
    return params, sets


def _torch_run(params, sets, cls, dtype, max_grad_norm):
    ps = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in params]
    opt = cls(ps, lr=1e-3)
    norms = []
    for g in sets:
        for p, x in zip(ps, g):
            p.grad = x.to(dtype).clone()
        if max_grad_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)))
        opt.step()
    return ps, opt, norms


@pytest.mark.parametrize("max_grad_norm", [0.5, None])
@pytest.mark.parametrize("algo", ["rmsprop", "adam"])
def test_matches_torch_optim_float64(algo, max_grad_norm):
    params, sets = _synthetic(11)
    cls = torch.optim.Adam if algo == "adam" else torch.optim.RMSprop
    keys = ("exp_avg", "exp_avg_sq") if algo == "adam" else ("square_avg",)
    p64, o64, n64 = _torch_run(params, sets, cls, torch.float64, max_grad_norm)
    p32, o32, _ = _torch_run(params, sets, cls, torch.float32, max_grad_norm)
    if max_grad_norm is not None:
        assert n64[0] > 100 * max_grad_norm and abs(n64[2] - 0.1) < 1e-6  # clipped hard / below the bound
    # the kernel: the same tensors plus one with count == 0 (NULL pointers), its own state
    mine = [p.clone() for p in params[:-1]]
    holder = torch.zeros(UNALIGNED + 8, device="cuda")
    holder[1:1 + UNALIGNED] = params[-1]
    mine.append(holder[1:1 + UNALIGNED])
    s1 = [torch.zeros_like(p) for p in mine] + [None]
    s2 = ([torch.zeros_like(p) for p in mine] + [None]) if algo == "adam" else None
    step, norm = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    for k, g in enumerate(sets):
        launch(make_group(abi.OPT_ADAM if algo == "adam" else abi.OPT_RMSPROP, mine + [None], list(g) + [None], s1, s2, step=step,
                          lr=1e-3, max_grad_norm=max_grad_norm, grad_norm=norm))
        want = float(torch.sqrt(sum((x.double() ** 2).sum() for x in g)))
        assert abs(float(norm) - want) <= 1e-6 * want
    assert int(step) == K_STEPS
    assert float(holder[0]) == 0.0 and float(holder[1 + UNALIGNED:].abs().max()) == 0.0  # nothing outside the view
    observed = {}
    for i in range(len(mine)):
        rows = [("param", mine[i], p32[i].detach(), p64[i].detach())]
        for key, mine_s in zip(keys, (s1, s2)):
            st32, st64 = o32.state[p32[i]], o64.state[p64[i]]
            rows.append((key, mine_s[i], st32[key], st64[key]))
        for what, x, y32, y64 in rows:
            e32 = float((y32.double() - y64).abs().max())
            err = float((x.double() - y64).abs().max())
            bound = 4.0 * e32 + K_STEPS * ULP * float(y64.abs().max())
            observed["%s_%d" % (what, mine[i].numel())] = {"e32": e32, "kernel_err": err, "bound": bound}
            print("%s clip %s %-10s n %6d e32 %.3e kernel %.3e bound %.3e" % (algo, max_grad_norm, what, mine[i].numel(), e32, err, bound))
            assert err <= bound, (what, mine[i].numel(), err, bound, e32)
    assert torch.equal(mine[ZERO_GRAD], params[ZERO_GRAD])  # a zero gradient moves nothing
    name = max(observed, key=lambda k: _frac(observed[k]["kernel_err"], observed[k]["bound"]))
    ERRORS["torch64_%s_clip_%s" % (algo, max_grad_norm)] = dict(
        worst=name, of_bound=float("%.3g" % _frac(observed[name]["kernel_err"], observed[name]["bound"])),
        e32=float("%.3g" % observed[name]["e32"]), kernel_err=float("%.3g" % observed[name]["kernel_err"]))


# ---- 3. bit-exact properties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 0.5, 0.01])
def test_blend_is_the_torch_expression(tau):
    params, _ = _synthetic(5)
    targets = [torch.randn_like(p) for p in params]
    want = [(1.0 - tau) * t + tau * s for t, s in zip(targets, params)]
    kept = [p.clone() for p in params]
    launch(make_group(abi.OPT_BLEND, params, targets=targets, tau=tau))
    for t, w, p, k in zip(targets, want, params, kept):
        assert torch.equal(t, w) and torch.equal(p, k)


def _two_groups(seed, algo=abi.OPT_ADAM):
    """Two groups (sizes of the actor's and the critic's tensors, the second with targets and the soft update), their tensors."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for sizes in ([3840, 128, 16384, 128, 640, 5], [3840, 128, 17024, 128, 128, 1]):
        t = {"param": [torch.randn(n, generator=gen).cuda() for n in sizes]}
        t["grad"] = [torch.randn(n, generator=gen).cuda() for n in sizes]
        t["state1"] = [torch.zeros(n, device="cuda") for n in sizes]
        t["state2"] = [torch.zeros(n, device="cuda") for n in sizes]
        t["target"] = [torch.randn(n, generator=gen).cuda() for n in sizes]
        t["step"], t["norm"] = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
        out.append(t)
    groups = [make_group(algo, t["param"], t["grad"], t["state1"], t["state2"], t["target"], step=t["step"], lr=1e-3, tau=0.5,
                         soft_update=bool(i), grad_norm=t["norm"]) for i, t in enumerate(out)]
    return out, groups


def _all_tensors(sets):
    return [x for t in sets for k in ("param", "state1", "state2", "target") for x in t[k]] + [t[k] for t in sets for k in ("step", "norm")]


def test_two_calls_on_equal_inputs_are_equal():
    a, ga = _two_groups(21)
    b, gb = _two_groups(21)
    for _ in range(2):
        launch(*ga)
        launch(*gb)
    for x, y in zip(_all_tensors(a), _all_tensors(b)):
        assert torch.equal(x, y) and bool(torch.isfinite(x.float()).all())
    assert int(a[0]["step"]) == 2 and not torch.equal(a[1]["target"][2], _two_groups(21)[0][1]["target"][2])


def test_graph_replay_equals_eager():
    """One captured mm_opt_step (Adam, two groups), the gradient buffers rewritten in place before each of three replays,
    against an eager twin given the same three gradient sets: Adam's step count lives on the device, so the replays take
    steps 1, 2, 3 and parameters, states, targets and counters all agree bit for bit."""
    a, ga = _two_groups(33)
    b, gb = _two_groups(33)
    launch(*_two_groups(1)[1])  # (the kernel is loaded before anything is captured)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(34)
    sets = [[[torch.randn(x.numel(), generator=gen).cuda() for x in t["grad"]] for t in a] for _ in range(3)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(*ga)
    for s in sets:
        for t, u, gs in zip(a, b, s):
            for x, y, g in zip(t["grad"], u["grad"], gs):
                x.copy_(g)
                y.copy_(g)
        graph.replay()
        launch(*gb)
    torch.cuda.synchronize()
    assert int(a[0]["step"]) == 3 and int(b[1]["step"]) == 3
    for x, y in zip(_all_tensors(a), _all_tensors(b)):
        assert torch.equal(x, y)


# ---- 4. the learners -------------------------------------------------------------------------------------------------------
def _ppo(z, meta, prefix, **kw):
    actor, critic = pt.fixture_nets(z, meta, prefix, device="cuda")
    kw.setdefault("target_tau", meta["target_tau"])
    kw.setdefault("target_update_steps", meta["target_update_steps"])
    learner = PPOLearner(actor, critic, _lib(), critic_loss=meta["critic_loss"], clip_param=meta["clip_param"],
                         actor_lr=meta["actor_lr"], critic_lr=meta["critic_lr"], max_grad_norm=meta["max_grad_norm"], **kw)
    ta, tc = pt.fixture_nets(z, meta, "tp_", device="cuda")
    learner.actor_target.load_state_dict(ta.state_dict())
    learner.critic_target.load_state_dict(tc.state_dict())
    return learner


def _shared(z, meta, prefix, **kw):
    learner = SharedPPOLearner(gi.fixture_net(z, meta, prefix, device="cuda"), _lib(), lr=meta["lr"], critic_loss=meta["critic_loss"],
                               clip_param=meta["clip_param"], max_grad_norm=meta["max_grad_norm"], **kw)
    learner.policy_target.load_state_dict(gi.fixture_net(z, meta, "tp_", device="cuda").state_dict())
    return learner


def _make(kind, t=1, **kw):
    """A learner of `kind` on train t's recorded networks (train 1: the targets differ from the networks) + the batch."""
    if kind == "ppo":
        z, meta = pt.load_fixture("soft", t)
        learner = _ppo(z, meta, "p_", **kw)
    else:
        z, meta = gi.load_fixture("mse", t)
        learner = _shared(z, meta, "p_", **kw)
    batch = tuple(dev(z[k]) for k in ("states", "actions", "returns"))
    return learner, batch


def _nets(learner):
    """[(network's parameters, target's parameters)] in the order of the launch's groups."""
    if isinstance(learner, PPOLearner):
        return [(_mlp_params(learner.actor), _mlp_params(learner.actor_target)),
                (_mlp_params(learner.critic), _mlp_params(learner.critic_target))]
    return [(_params(learner.policy), _params(learner.policy_target))]


def _state_dicts(learner):
    sd = learner.optimizer_state_dict()
    return [sd["actor_optimizer"], sd["critic_optimizer"]] if isinstance(learner, PPOLearner) else [sd]


def _assert_same_learners(x, y, state=True):
    for (px, tx), (py, ty) in zip(_nets(x), _nets(y)):
        for a, b in zip(px + tx, py + ty):
            assert torch.equal(a.detach(), b.detach())
    if state:
        for sx, sy in zip(_state_dicts(x), _state_dicts(y)):
            assert list(sx["state"].keys()) == list(sy["state"].keys())
            for i in sx["state"]:
                for k in sx["state"][i]:
                    assert torch.equal(sx["state"][i][k].cpu(), sy["state"][i][k].cpu()), (i, k)


def _column(batch, a):
    return tuple(x[:, a:a + 1] for x in batch)


def _grads_by_hand(learner, batch, a):
    """The agent step's gradient kernels as train(form="reference") calls them; the gradients land in .grad."""
    states, actions, returns = batch[0], batch[1].to(torch.int32), batch[2].float()  # train()'s own conversions, then its views
    obs, act, ret = states[:, a, :], actions[:, a], returns[:, a]
    if isinstance(learner, PPOLearner):
        old, value = learner.evaluate(obs, act, actor=learner.actor_target, critic=learner.critic_target)
        adv = ret - value
        sums = torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])
        return learner.loss_and_grad(obs, act, ret, old, adv_sums=sums)
    dense = obs.contiguous()
    return learner.loss_and_grad(obs, act, ret, learner.old_log_probs(dense, act), adv_sums=learner.advantage_sums(dense, ret))


@pytest.mark.parametrize("kind", ["ppo", "shared"])
def test_fused_step_against_the_torch_step(kind):
    """One agent column from the recorded networks: both paths get bit-identical gradients (the gradient kernels are
    deterministic; the fused path leaves them in .grad unscaled, the torch path leaves coef * g), the post-step parameters
    differ by at most 2^-22 max|p| per tensor (the bound of the recorded steps), last_grad_norm agrees to 1e-6."""
    fused, batch = _make(kind, fused_step=True)
    plain, _ = _make(kind)
    hand, _ = _make(kind)
    assert fused.last_grad_norm is not None and plain.last_grad_norm is None
    fused.train(*_column(batch, 0))
    plain.train(*_column(batch, 0))
    _grads_by_hand(hand, batch, 0)
    nf, npl = fused.last_grad_norm, plain.last_grad_norm
    assert nf.dtype == torch.float32 and nf.shape == npl.shape == (len(_nets(fused)),)
    assert float(((nf - npl).abs() / npl).max()) <= 1e-6
    observed = 0.0
    for i, ((pf, _), (pp, _), (ph, _)) in enumerate(zip(_nets(fused), _nets(plain), _nets(hand))):
        coef = torch.clamp(fused.max_grad_norm / (npl[i] + 1e-6), max=1.0)
        for x, y, h in zip(pf, pp, ph):
            assert torch.equal(x.grad, h.grad)
            assert torch.allclose(y.grad, h.grad * coef, rtol=1e-6, atol=0.0)
            diff, bound = float((x.detach() - y.detach()).abs().max()), 2.0 ** -22 * float(y.detach().abs().max())
            observed = max(observed, _frac(diff, bound))
            assert diff <= bound, (i, diff, bound)
            assert not torch.equal(x.detach(), h.detach())  # a step was taken
    ERRORS["fused_vs_torch_step_%s" % kind] = {"of_bound": float("%.3g" % observed)}


@pytest.mark.parametrize("kind,optimizer_type,n_episodes", [("ppo", "rmsprop", 2), ("ppo", "adam", 1), ("shared", "adam", 2),
                                                            ("shared", "rmsprop", 1)])
def test_fused_train_is_the_hand_composed_sequence(kind, optimizer_type, n_episodes):
    """A whole train() of N = 3 agent steps, with an n_episodes that triggers the soft update (2, target_update_steps 2) and
    with one that does not: bit-identical to evaluate / loss_and_grad / mm_opt_step composed by hand -- parameters, targets
    and optimiser state.  PPOLearner: the soft update rides in the last step's launch; SharedPPOLearner: in every step's."""
    kw = dict(optimizer_type=optimizer_type, target_tau=0.5, target_update_steps=2)
    fused, batch = _make(kind, fused_step=True, **kw)
    hand, _ = _make(kind, **kw)
    N = batch[0].shape[1]
    assert N == 3
    losses = fused.train(*batch, n_episodes=n_episodes)
    adam = optimizer_type == "adam"
    nets = _nets(hand)
    s1 = [[torch.zeros_like(p) for p in ps] for ps, _ in nets]
    s2 = [[torch.zeros_like(p) for p in ps] for ps, _ in nets] if adam else [None] * len(nets)
    steps = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in nets]
    start_targets = [[t.detach().clone() for t in ts] for _, ts in nets]
    for a in range(N):
        loss = _grads_by_hand(hand, batch, a)
        assert torch.equal(loss, losses[a])
        soft = n_episodes == 2 and (kind == "shared" or a == N - 1)
        launch(*[make_group(abi.OPT_ADAM if adam else abi.OPT_RMSPROP, [p.detach() for p in ps], [p.grad for p in ps], s1[i], s2[i],
                            [t.detach() for t in ts], step=steps[i], lr=1e-4, max_grad_norm=hand.max_grad_norm, tau=0.5,
                            soft_update=soft) for i, (ps, ts) in enumerate(nets)])
    _assert_same_learners(fused, hand, state=False)
    for i, sd in enumerate(_state_dicts(fused)):
        assert list(sd["state"].keys()) == list(range(len(nets[i][0])))
        for j in sd["state"]:
            assert float(sd["state"][j]["step"]) == N == int(steps[i])
            assert torch.equal(sd["state"][j]["exp_avg" if adam else "square_avg"], s1[i][j])
            if adam:
                assert torch.equal(sd["state"][j]["exp_avg_sq"], s2[i][j])
    for (_, ts), t0 in zip(nets, start_targets):
        for t, u in zip(ts, t0):
            assert torch.equal(t.detach(), u) == (n_episodes != 2)


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
@pytest.mark.parametrize("first", ["torch", "fused"])
def test_state_dict_moves_between_the_paths(optimizer_type, first):
    """Two steps on one path, its optimizer_state_dict() loaded into a learner of the OTHER path that holds the same
    networks, one more step on each: the results agree under the step bound, 2^-22 max|p| per tensor."""
    one, batch = _make("ppo", fused_step=first == "fused", optimizer_type=optimizer_type)
    for a in (0, 1):
        one.train(*_column(batch, a))
    other = PPOLearner(copy.deepcopy(one.actor), copy.deepcopy(one.critic), _lib(), fused_step=first != "fused",
                       optimizer_type=optimizer_type, critic_loss=one.critic_loss, clip_param=one.clip_param,
                       max_grad_norm=one.max_grad_norm, actor_lr=3e-4)
    other.actor_target.load_state_dict(one.actor_target.state_dict())
    other.critic_target.load_state_dict(one.critic_target.state_dict())
    sd = one.optimizer_state_dict()
    assert float(sd["actor_optimizer"]["state"][0]["step"]) == 2.0 and sd["actor_optimizer"]["state"][0]["step"].dtype == torch.float32
    other.load_optimizer_state_dict(sd)
    assert other.actor_optimizer.param_groups[0]["lr"] == one.actor_optimizer.param_groups[0]["lr"] == 1e-4  # hyperparameters travel
    back = other.optimizer_state_dict()
    for name in sd:
        for i in sd[name]["state"]:
            for k in sd[name]["state"][i]:
                assert torch.equal(sd[name]["state"][i][k].cpu(), back[name]["state"][i][k].cpu())
    before = [p.detach().clone() for p in _nets(one)[0][0]]
    one.train(*_column(batch, 2))
    other.train(*_column(batch, 2))
    for (px, _), (py, _) in zip(_nets(one), _nets(other)):
        for x, y in zip(px, py):
            diff, bound = float((x.detach() - y.detach()).abs().max()), 2.0 ** -22 * float(x.detach().abs().max())
            assert diff <= bound, (diff, bound)
    assert not torch.equal(before[0], _nets(one)[0][0][0].detach())
    assert float(_state_dicts(other)[0]["state"][0]["step"]) == 3.0


@pytest.mark.parametrize("kind", ["ppo", "shared"])
def test_fused_train_in_a_graph(kind):
    """After one eager warm-up call (it sizes the scratch), train() of a fused Adam learner is captured and replayed; an eager
    twin makes the same calls: same losses, parameters, targets and optimiser state, bit for bit."""
    kw = dict(fused_step=True, optimizer_type="adam", target_tau=0.5, target_update_steps=2)
    a, batch = _make(kind, **kw)
    b, _ = _make(kind, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a.train(*batch, n_episodes=2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        la = a.train(*batch, n_episodes=2)
    graph.replay()
    graph.replay()
    for _ in range(2):
        b.train(*batch, n_episodes=2)
    lb = b.train(*batch, n_episodes=2)
    torch.cuda.synchronize()
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    _assert_same_learners(a, b)
    assert float(_state_dicts(a)[0]["state"][0]["step"]) == 9.0


# ---- 5. soft_update_every="agent_step" -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_step", [False, True])
def test_soft_update_every_agent_step(fused_step):
    """MAPPO_GI's non-shared branch: with tau 0.5, N = 3 and n_episodes on a multiple of target_update_steps both targets
    after train() are those of the same learner driven column by column with every call's n_episodes triggering the soft
    update, bit for bit; with n_episodes off the multiple the targets are untouched."""
    kw = dict(fused_step=fused_step, target_tau=0.5, target_update_steps=2)
    whole, batch = _make("ppo", soft_update_every="agent_step", **kw)
    twin, _ = _make("ppo", **kw)
    once, _ = _make("ppo", **kw)
    start = [t.detach().clone() for _, ts in _nets(whole) for t in ts]
    whole.train(*batch, n_episodes=4)
    for a in range(3):
        twin.train(*_column(batch, a), n_episodes=4)
    once.train(*batch, n_episodes=4)
    _assert_same_learners(whole, twin)
    now = [t.detach() for _, ts in _nets(whole) for t in ts]
    assert not any(torch.equal(x, y) for x, y in zip(now, start))
    # (the per-step blend is not the once-per-train one)
    assert not torch.equal(whole.actor_target.fc1.weight.detach(), once.actor_target.fc1.weight.detach())
    off, _ = _make("ppo", soft_update_every="agent_step", **kw)
    off.train(*batch, n_episodes=3)
    for x, y in zip([t.detach() for _, ts in _nets(off) for t in ts], start):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="soft_update_every"):
        _make("ppo", soft_update_every="never")


# ---- 6. arguments -----------------------------------------------------------------------------------------------------------
def _bad(g, field, value, index=None):
    if index is None:
        setattr(g, field, value)
    else:
        getattr(g, field)[index] = value


BAD = [("algo", 7, None), ("algo", -1, None), ("n_tensors", 17, None), ("n_tensors", -1, None), ("count", -1, 1), ("param", None, 0),
       ("grad", None, 1), ("state1", None, 0), ("state2", None, 1), ("step", None, None), ("target", None, 1), ("eps", 0.0, None),
       ("eps", -1e-8, None), ("lr", -1.0, None), ("lr", float("nan"), None), ("alpha_or_beta1", 1.0, None), ("beta2", -0.1, None),
       ("tau", 1.5, None), ("max_grad_norm", float("nan"), None), ("param", "odd", 0)]


@pytest.mark.parametrize("field,value,index", BAD, ids=["%s_%s_%s" % b for b in BAD])
def test_invalid_arguments_raise_and_write_nothing(field, value, index):
    sets, groups = _two_groups(41)
    kept = [x.clone() for x in _all_tensors(sets)]
    if value == "odd":
        value = sets[1]["param"][0].data_ptr() + 2  # not 4-byte aligned
    _bad(groups[1], field, value, index)  # the SECOND group is refused: the first must not have run either
    with pytest.raises(ValueError) as e:
        launch(*groups)
    assert len(str(e.value)) > 10 and "mm_opt_step" in str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(_all_tensors(sets), kept):
        assert torch.equal(x, y)


def test_group_count_and_missing_symbol():
    sets, groups = _two_groups(42)
    lib = _lib()
    for n in (0, 5):
        with pytest.raises(ValueError, match="n_groups"):
            lib.check(lib.lib.mm_opt_step((abi.MMOptGroup * 5)(), n, _stream()))
    with pytest.raises(ValueError, match="NULL"):
        lib.check(lib.lib.mm_opt_step(None, 1, _stream()))
    blend = make_group(abi.OPT_BLEND, sets[0]["param"], tau=0.5)  # a blend without targets
    with pytest.raises(ValueError, match="target"):
        launch(blend)
    launch(make_group(abi.OPT_RMSPROP, []))  # n_tensors == 0: nothing to do, no error
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    launch(make_group(abi.OPT_ADAM, [None], [None], [None], [None], step=step))  # only an empty tensor: the same
    assert int(step) == 0
    without = abi.CLib(lib.path)
    without.has_opt_step = False  # (a library built before mm_opt_step existed)
    z, meta = pt.load_fixture("mse", 0)
    actor, critic = pt.fixture_nets(z, meta, "p_", device="cuda")
    with pytest.raises(NotImplementedError, match="mm_opt_step"):
        PPOLearner(actor, critic, without, fused_step=True)
    zg, mg = gi.load_fixture("mse", 0)
    with pytest.raises(NotImplementedError, match="mm_opt_step"):
        SharedPPOLearner(gi.fixture_net(zg, mg, "p_", device="cuda"), without, fused_step=True)
    PPOLearner(actor, critic, without)  # the default path does not need it
