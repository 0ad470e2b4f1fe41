"""mm_policy_gi_act (include/mm_policy_gi.h) on the MI355X: MAPPO_GI's shared actor-critic + the action sample in one
f32-MFMA launch, against rollout.ActorCriticNetwork in torch, against mm_sample_actions, against the reference's recorded
checkpoint, and inside DeviceRollout's shared mode."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from marl_mass_amd.rollout import ActorCriticNetwork, DeviceRollout
from policy_act_util import sampler_u as _philox_u53  # the numpy Philox, pinned to known answers in test_policy_act_host.py

pytestmark = pytest.mark.gpu

KW = dict(config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5, auto_reset=True)


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
        net.critic_linear.bias.fill_(2.5); net.critic_linear.weight.mul_(4.0)
    return net


def _act(net, obs, seed, counter, actions=True, logp=True, value=True, n_a=5):
    n, S = obs.shape
    dev = obs.device
    a = torch.full((n,), -1, dtype=torch.int32, device=dev) if actions else None
    lp = torch.full((n, n_a), float("nan"), dtype=torch.float32, device=dev) if logp else None
    v = torch.full((n,), float("nan"), dtype=torch.float32, device=dev) if value else None
    p = lambda t: t.detach().contiguous().data_ptr()  # noqa: E731
    o = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    clib = _lib()
    rc = clib.lib.mm_policy_gi_act(obs.data_ptr(), n, S, p(net.fc11.weight), p(net.fc11.bias), p(net.fc12.weight),
                                   p(net.fc12.bias), p(net.fc13.weight), p(net.fc13.bias), p(net.fc2.weight), p(net.fc2.bias),
                                   p(net.actor_linear.weight), p(net.actor_linear.bias), p(net.critic_linear.weight),
                                   p(net.critic_linear.bias), 128, n_a, seed, o(counter), o(a), o(lp), o(v),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    clib.check(rc)
    return a, lp, v


def _sample(logp, seed, counter):
    clib = _lib()
    n, n_a = logp.shape
    out = torch.empty(n, dtype=torch.int32, device=logp.device)
    clib.check(clib.lib.mm_sample_actions(logp.contiguous().data_ptr(), n, n_a, seed, counter.data_ptr(), out.data_ptr(),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


@pytest.mark.parametrize("n", [31, 1000, 65536 * 8 + 13])
@pytest.mark.parametrize("n_s", [25, 30])
def test_kernel_matches_torch_and_sampler(n, n_s):
    net = _net(n_s)
    obs = (torch.randn(n, n_s, device="cuda") * 1.5).contiguous()
    ctr = torch.tensor([8], dtype=torch.int64, device="cuda")
    acts, logp, val = _act(net, obs, 99, ctr)
    with torch.no_grad():
        ref_lp, ref_v = net(obs), net(obs, out_type="v")[:, 0]
    assert float((logp - ref_lp).abs().max()) <= 2e-5
    assert bool(((val - ref_v).abs() <= 1e-5 * ref_v.abs().clamp(min=1.0)).all())
    assert int(ctr) == 9
    # actions == mm_sample_actions on the kernel's own log-probabilities, same seed and counter: bit for bit
    c2 = torch.tensor([8], dtype=torch.int64, device="cuda")
    assert torch.equal(acts, _sample(logp, 99, c2))
    # and == sampling from torch's log-probabilities, except where u falls within 1e-5 of a CDF edge
    u = _philox_u53(np.arange(n, dtype=np.uint64), 8, 99)
    cdf = ref_lp.double().exp().cumsum(-1).cpu().numpy()
    cdf = cdf / cdf[:, -1:]
    a_ref = np.minimum((cdf <= u[:, None]).sum(-1), 4)
    near = (np.abs(cdf - u[:, None]) < 1e-5).any(-1)
    a = acts.cpu().numpy()
    assert np.array_equal(a[~near], a_ref[~near]) and near.mean() < 1e-3
    assert len(np.unique(a)) > 1 or n < 64


def test_counter_and_optional_outputs():
    net = _net(30)
    obs = torch.randn(777, 30, device="cuda").contiguous()
    ctr = torch.tensor([41], dtype=torch.int64, device="cuda")
    a0, lp0, v0 = _act(net, obs, 5, ctr)
    assert int(ctr) == 42
    a1, _, _ = _act(net, obs, 5, ctr, logp=False, value=False)  # counter advanced: fresh draws
    assert int(ctr) == 43 and not torch.equal(a0, a1)
    c = torch.tensor([41], dtype=torch.int64, device="cuda")
    a2, _, _ = _act(net, obs, 5, c, logp=False, value=False)
    assert torch.equal(a2, a0) and int(c) == 42
    # value-only: nothing sampled, counter neither read nor bumped (NULL is accepted)
    _, lp3, v3 = _act(net, obs, 5, ctr, actions=False)
    assert int(ctr) == 43 and torch.equal(lp3, lp0) and torch.equal(v3, v0)
    _, _, v4 = _act(net, obs, 5, None, actions=False, logp=False)
    assert torch.equal(v4, v0)
    _, lp5, _ = _act(net, obs, 5, None, actions=False, value=False)
    assert torch.equal(lp5, lp0)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        _act(net, obs, 5, None)  # actions without a counter
    with pytest.raises(ValueError):
        _act(net, obs, 5, ctr, actions=False, logp=False, value=False)  # no output
    with pytest.raises(ValueError):
        _act(_net(24), torch.randn(8, 24, device="cuda"), 5, ctr)  # n_s < 25


def test_kernel_logprobs_match_reference_checkpoint():
    """On the recorded states of the reference's MAPPO_GI rollout (tests/golden/mappo_gi_v1mass.npz): log-probabilities
    and values of the fixed checkpoint as the reference's ActorCriticNetwork computed them, <= 2e-4."""
    for tag in ("v1mass", "v0prio"):
        z = np.load(os.path.join(GOLDEN, "mappo_gi_%s.npz" % tag))
        meta = json.loads(str(z["meta"]))
        net = ActorCriticNetwork(meta["n_s"], meta["n_a"], 128, 1, state_split=True)
        net.load_state_dict({k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w_")})
        net = net.cuda()
        for k in range(meta["K"]):
            st = torch.tensor(z["ro%d_states" % k], dtype=torch.float32).reshape(-1, meta["n_s"]).cuda().contiguous()
            ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
            _, lp, v = _act(net, st, 1, ctr, n_a=meta["n_a"])
            assert float(np.abs(lp.cpu().numpy() - z["ro%d_logp" % k].reshape(-1, meta["n_a"])).max()) <= 2e-4
            assert float(np.abs(v.cpu().numpy() - z["ro%d_value" % k].reshape(-1)).max()) <= 2e-4


def _shared(E, N, T, seed=9, sample_seed=4, **kw):
    from marl_mass_amd import VecMergeEnv
    torch.manual_seed(3)
    net = _net(30, seed=3)
    return DeviceRollout(VecMergeEnv(E, N, seed=seed, **KW), net, roll_out_n_steps=T, sample_seed=sample_seed, **kw)


def test_shared_rollout_fused_bootstrap():
    """Fused shared mode: one launch per policy step plus one for the bootstrap (T + 1 counter steps), and the bootstrap
    value is policy(final_obs, out_type="v")."""
    E, N, T = 512, 8, 10
    ro = _shared(E, N, T)
    assert ro.shared and ro.fused_policy
    out = ro.interact()
    assert int(ro._sample_counter) == T + 1
    ro0 = _shared(E, N, T, reward_gamma=0.0)
    out0 = ro0.interact()
    assert torch.equal(out["actions"], out0["actions"]) and torch.equal(out["states"], out0["states"])
    with torch.no_grad():
        v = ro.actor(ro.obs.reshape(E * N, 30), out_type="v").view(E, N).double()
    fv = (out["returns"][-1] - out0["returns"][-1]) / 0.99
    live = ~out["dones"][-1].bool()
    assert bool(live.any())
    assert float((fv[live] - v[live]).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max()))


def test_shared_graph_equals_eager():
    E, N, T = 2048, 8, 12
    eager, graph = _shared(E, N, T), _shared(E, N, T, use_graph=True)
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    eager.interact(); eager.interact()
    for _ in range(2):
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for k in ("states", "actions", "returns", "dones", "average_speed", "min_headway"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(eager._sample_counter, graph._sample_counter)


def test_shared_checkpoint_resume_is_bit_identical():
    a = _shared(256, 8, 9)
    a.interact()
    ck = a.state_dict()
    ref = a.interact()
    b = _shared(256, 8, 9)
    b.load_state_dict(ck)
    out = b.interact()
    for k in ("states", "actions", "returns", "dones"):
        assert torch.equal(out[k], ref[k]), k


def test_fused_and_unfused_greedy_rollouts_agree():
    """A policy whose actor head is dominated by its bias draws one action per state with probability ~1 - 1e-12: the
    fused launch and the module's forward + mm_sample_actions must then give the same rollout (values to fp32 rounding)."""
    E, N, T = 512, 8, 12
    fused, plain = _shared(E, N, T), _shared(E, N, T, fused_policy=False)
    for ro in (fused, plain):
        with torch.no_grad():
            ro.actor.actor_linear.weight.mul_(0.01)
            ro.actor.actor_linear.bias.copy_(torch.tensor([0.0, 40.0, 0.0, 0.0, 0.0]))
    assert fused.fused_policy and not plain.fused_policy
    a, b = fused.interact(), plain.interact()
    for k in ("states", "actions", "dones"):
        assert torch.equal(a[k], b[k]), k
    assert float((a["returns"] - b["returns"]).abs().max()) <= 1e-5
    assert torch.equal(fused._sample_counter, plain._sample_counter)


def test_shared_evaluate_leaves_the_training_stream_untouched():
    a, b = _shared(64, 8, 10), _shared(64, 8, 10)
    a.interact(); b.interact()
    before = a.env.state.clone()
    a.evaluate(seeds=list(range(200, 264)))
    assert torch.equal(a.env.state, before)
    assert torch.equal(a.obs, b.obs) and torch.equal(a._sample_counter, b._sample_counter)
    ra, rb = a.interact(), b.interact()
    for k in ("states", "actions", "returns", "dones"):
        assert torch.equal(ra[k], rb[k]), k
