"""The hidden-512 actor's act launch (policy_wide_kernel: mm_policy_wide_act, and mm_policy_act at hidden = 512) on the MI355X.

The tolerance is the rule of both act-side suites (policy_act_util.compare): per output tensor,
    max|kernel - f64| <= 4 * e32 + 1e-6 * max(1, max|f64|),   e32 = max|float32 torch module on the device - f64|.
Nothing is compared with the kernel's own earlier output except where bit identity between two launches of the same kernel is
the claim (grids B, D, E, F, G).  The sampler is checked against the numpy Philox and the float64 inverse CDF; the conditions on
the inputs are asserted in test_policy_wide_host.py, without a GPU.

Grids: A n_s x n_a x gain at n = 257, B the n boundaries of the tile / workgroup / grid / persistent-loop decomposition (from
include/mm_policy_wide.h), C seeds and counters with both high words in use, D guarded, offset and misaligned buffers, E tile
isolation, F the dispatch from mm_policy_act, G DeviceRollout with a 512 actor on the steer_vel env."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import policy_wide_util as W
from marl_mass_amd import _cabi as abi

pytestmark = pytest.mark.gpu

ERRORS = {}  # case -> {output: {e32, kernel_err, max_abs, bound}}
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _dump_errors(tmp_path_factory):
    """Writes the measured figures when the module is done: to $MM_WIDE_ERROR_JSON when set (that is how
    profiles/policy_wide/forward_error.json is regenerated), else to pytest's temporary directory."""
    yield
    path = os.environ.get("MM_WIDE_ERROR_JSON") or str(tmp_path_factory.mktemp("policy_wide") / "forward_error.json")
    sig = lambda v: float("%.3g" % v)  # noqa: E731
    rows = {k: {o: {f: sig(x) for f, x in r.items()} for o, r in ERRORS[k].items()} for k in ERRORS}
    with open(path, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rows[k], sort_keys=True)) for k in sorted(rows)) + "\n}\n")
    print("measured figures: %s" % path)


def _lib():
    from marl_mass_amd import hip_library
    clib = hip_library()
    clib.require_policy_wide()
    return clib


def _on_device(case):
    return W.weights_of("act", copy.deepcopy(case.net).to(DEV)), case.obs.to(DEV)


def _same(a, b, keys=("actions", "logp")):
    """Bit identity of two launches' outputs (NaN-free by construction: compared as integers)."""
    for k in keys:
        assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k


# ---- A: forward against float64
@pytest.mark.parametrize("n_s", W.NS_A)
def test_a_forward_grid(n_s):
    clib = _lib()
    for case in W.grid_a():
        if case.n_s == n_s:
            W.check_forward(ERRORS, clib, case, DEV)


# ---- B: n boundaries
def test_b_n_boundaries():
    """n on both sides of a tile, of a workgroup's agents, of one full grid of persistent workgroups, and once beyond two trips
    of the loop (include/mm_policy_wide.h's constants); the rows are 257 rows repeated, so every row of every launch has a
    bit-exact twin in the launch of the first min(n, 257) rows alone: a row's result may not depend on its tile, wave,
    workgroup, trip of the loop or n."""
    clib = _lib()
    base = W.check_forward(ERRORS, clib, W.case_b(257), DEV)
    for n in W.N_GRID_B:
        case = W.case_b(n)
        out = W.check_forward(ERRORS, clib, case, DEV, f64_actions=n <= 1000)
        idx = torch.arange(n, device=DEV) % 257
        _same({"logp": out["logp"]}, {"logp": base["logp"][idx]}, ("logp",))
        w, obs = _on_device(case)
        m = min(n, 257)
        alone = W.run(clib, w, obs[:m].contiguous(), case.n_a, W.SEED_A, W.CTR_A)
        _same({k: out[k][:m] for k in ("actions", "logp")}, alone)
        if n > 1000:  # (the share of BAND rows is bounded on the host)
            near = case.near(W.SEED_A, W.CTR_A)
            assert np.array_equal(out["actions"].cpu().numpy()[~near], case.actions64(W.SEED_A, W.CTR_A)[~near]), n


# ---- C: the sampler against the independent reference
def test_c_actions_under_every_seed_and_counter():
    clib = _lib()
    for n_a in W.NA_C:
        case = W.case_c(n_a)
        w, obs = _on_device(case)
        for seed in W.SEEDS_C:
            for ctr in W.CTRS_C:
                out = W.run(clib, w, obs, n_a, seed, ctr)
                a_own, c = W.sample(clib, out["logp"], seed, ctr)
                assert torch.equal(out["actions"], a_own), (n_a, hex(seed), hex(ctr))  # no row left out
                assert c == out["counter"] == ((ctr + 1) & W.U64)
                near = case.near(seed, ctr)
                assert np.array_equal(out["actions"].cpu().numpy()[~near], case.actions64(seed, ctr)[~near]), (n_a, hex(seed), hex(ctr))
                if n_a == 1:
                    assert bool((out["actions"] == 0).all())
        if n_a > 1:  # equal low words, different high words of the counter and of the seed: different draws
            for (s0, c0), (s1, c1) in W.U.HIGH_PAIRS:
                a0, a1 = W.run(clib, w, obs, n_a, s0, c0)["actions"], W.run(clib, w, obs, n_a, s1, c1)["actions"]
                assert not torch.equal(a0, a1), (n_a, hex(s1), hex(c1))


# ---- D: memory discipline
def test_d_guarded_outputs_offset_observations_and_alignment():
    """Outputs in sentinel-padded buffers at 4-byte (not 16-byte) aligned addresses, the observations and every weight but
    fc2's offset by one element: the pads stay intact and the outputs equal the aligned run's bit for bit.  logp = NULL gives
    the same actions, n = 0 leaves outputs and counter alone, and fc2's weight off its 16-byte alignment is refused before
    anything is launched."""
    clib = _lib()
    base = W.synthetic_case(30, 5, 3)
    w, obs_all = _on_device(base)
    w_off = [t if i == 2 else W.offset_copy(t) for i, t in enumerate(w)]  # (index 2: fc2.weight, which must stay aligned)
    assert w[2].data_ptr() % W.W2_ALIGN == 0
    for n in (1, 33, 257):
        obs = obs_all[:n].contiguous()
        want = W.run(clib, w, obs, 5, W.SEED_A, W.CTR_A)
        a, chk_a = W.guarded(n, torch.int32, DEV)
        lp, chk_l = W.guarded(n * 5, torch.float32, DEV)
        c = W.counter_tensor(W.CTR_A, DEV)
        clib.check(W.launch(clib, w_off, W.offset_copy(obs), n, 30, 5, W.SEED_A, c, a, lp))
        torch.cuda.synchronize()
        chk_a(); chk_l()
        _same(want, {"actions": a, "logp": lp.view(n, 5)})
        assert W.counter_value(c) == W.CTR_A + 1
        # logp = NULL: the same actions, nothing else written
        a2, chk_a2 = W.guarded(n, torch.int32, DEV)
        c = W.counter_tensor(W.CTR_A, DEV)
        clib.check(W.launch(clib, w, obs, n, 30, 5, W.SEED_A, c, a2, None))
        torch.cuda.synchronize()
        chk_a2()
        assert torch.equal(a2, want["actions"]) and W.counter_value(c) == W.CTR_A + 1
    # n = 0: MM_OK, outputs and counter untouched
    c = W.counter_tensor((1 << 32) - 1, DEV)
    ga, chk_a = W.guarded(8, torch.int32, DEV)
    gl, chk_l = W.guarded(8, torch.float32, DEV)
    ga.fill_(-12345); gl.fill_(float("nan"))
    assert W.launch(clib, w, obs_all, 0, 30, 5, 7, c, ga, gl) == abi.MM_OK
    torch.cuda.synchronize()
    chk_a(); chk_l()
    assert bool((ga == -12345).all()) and bool(torch.isnan(gl).all()) and W.counter_value(c) == (1 << 32) - 1
    # fc2's weight one element (4 bytes) off: an argument error from both entries, and nothing ran
    bad = list(w)
    bad[2] = W.offset_copy(w[2])
    for entry in ("mm_policy_wide_act", "mm_policy_act"):
        assert W.launch(clib, bad, obs_all, 1, 30, 5, 7, c, ga, gl, entry=entry) == abi.MM_ERR_INVALID_ARG, entry
    torch.cuda.synchronize()
    assert bool((ga == -12345).all()) and bool(torch.isnan(gl).all()) and W.counter_value(c) == (1 << 32) - 1


# ---- E: tile isolation
def test_e_a_poisoned_row_reaches_no_other_row():
    """64 rows = two MFMA tiles; row 5 and row 40 poisoned in turn (all-NaN, then +inf in one column): the other 63 rows'
    outputs equal the clean run bit for bit.  Non-finite observations are outside the contract, so of the poisoned row only
    0 <= action < n_a is asserted."""
    clib = _lib()
    case = W.synthetic_case(30, 5, 3)
    w, obs_all = _on_device(case)
    clean_obs = obs_all[:64].contiguous()
    clean = W.run(clib, w, clean_obs, 5, W.SEED_A, W.CTR_A)
    for row in (5, 40):
        for poison in ("nan", "inf"):
            obs = clean_obs.clone()
            if poison == "nan":
                obs[row, :] = float("nan")
            else:
                obs[row, 11] = float("inf")
            a, chk_a = W.guarded(64, torch.int32, DEV)
            lp, chk_l = W.guarded(64 * 5, torch.float32, DEV)
            c = W.counter_tensor(W.CTR_A, DEV)
            clib.check(W.launch(clib, w, obs, 64, 30, 5, W.SEED_A, c, a, lp))
            torch.cuda.synchronize()
            chk_a(); chk_l()
            keep = torch.arange(64, device=DEV) != row
            _same({k: clean[k][keep] for k in ("actions", "logp")}, {"actions": a[keep], "logp": lp.view(64, 5)[keep]})
            assert 0 <= int(a[row]) < 5, (row, poison)


# ---- F: dispatch
def test_f_policy_act_forwards_hidden_512():
    """mm_policy_act(hidden = 512) is mm_policy_wide_act bit for bit; every hidden other than 128 and 512 is refused by
    mm_policy_act, and every hidden other than 512 by mm_policy_wide_act, with nothing written."""
    clib = _lib()
    for n_s, n_a in ((30, 5), (5, 8)):
        case = W.synthetic_case(n_s, n_a, 3)
        w, obs = _on_device(case)
        _same(W.run(clib, w, obs, n_a, W.SEED_A, W.CTR_A), W.run(clib, w, obs, n_a, W.SEED_A, W.CTR_A, entry="mm_policy_act"))
    c = W.counter_tensor(41, DEV)
    ga, chk_a = W.guarded(case.n, torch.int32, DEV)
    for hidden in (64, 256, 1024):
        for entry in ("mm_policy_wide_act", "mm_policy_act"):
            assert W.launch(clib, w, obs, case.n, n_s, n_a, 7, c, ga, None, hidden=hidden, entry=entry) == abi.MM_ERR_INVALID_ARG
    assert W.launch(clib, w, obs, case.n, n_s, n_a, 7, c, ga, None, hidden=128) == abi.MM_ERR_INVALID_ARG  # (wide: 512 only)
    torch.cuda.synchronize()
    chk_a()
    assert bool((ga == -12345).all()) and W.counter_value(c) == 41


# ---- G: the rollout
def _rollouts(use_graph, n=1):
    from marl_mass_amd import VecMergeEnv
    from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout
    E, N, T = 256, 4, 10
    kw = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": "cbf-av", "HEADWAY_TIME": 0.5, "lateral_control": "steer_vel"},
              seed=9, auto_reset=True)
    torch.manual_seed(3)
    env = VecMergeEnv(E, N, **kw)
    # merge-multi-agent-v1 rows are 6 features x 5 vehicles: the actor's input width is the env's
    actor, critic = ActorNetwork(env.n_s, 512, 5).cuda(), CriticNetwork(env.n_s, 5, 512).cuda()
    out = [DeviceRollout(env, actor, critic, roll_out_n_steps=T, sample_seed=4, use_graph=use_graph)]
    for _ in range(n - 1):
        out.append(DeviceRollout(VecMergeEnv(E, N, **kw), actor, critic, roll_out_n_steps=T, sample_seed=4, use_graph=use_graph))
    return out, actor


def test_g_rollout_with_a_512_actor():
    """DeviceRollout with the steer_vel family's networks (actor and critic hidden 512) on 256 envs x 4: the fused path is
    taken, two fresh rollouts with the same seeds are bit-identical, and the first step's actions are the float64 inverse
    CDF of the float64 module under the numpy Philox outside the BAND."""
    (r0, r1), actor = _rollouts(False, 2)
    assert r0.fused_policy is True and r1.fused_policy is True
    obs0 = r0.obs.clone()
    a, b = r0.interact(), r1.interact()
    torch.cuda.synchronize()
    for k in ("states", "actions", "returns", "dones"):
        assert torch.equal(a[k], b[k]), k
    assert int(r0._sample_counter) == 10 + 1  # one sampler step per policy step + the bootstrap's action draw
    assert torch.equal(a["states"][0], obs0)
    rows = obs0.reshape(-1, obs0.shape[-1]).double().cpu()
    with torch.no_grad():
        lp64 = copy.deepcopy(actor).cpu().double()(rows).numpy()
    u = W.sampler_u(np.arange(rows.shape[0], dtype=np.uint64), 0, 4)
    near = W.near_edge(lp64, u)
    assert np.array_equal(a["actions"][0].reshape(-1).cpu().numpy()[~near], W.sample_f64(lp64, u)[~near])


def test_g_graph_captured_rollout_equals_eager():
    """use_graph=True equals eager bit for bit over two replays (the checks of
    test_supervisor_gpu.py::test_graph_captured_rollout_with_priority_equals_eager)."""
    (eager,), _ = _rollouts(False)
    (graph,), _ = _rollouts(True)
    assert eager.fused_policy is True and graph.fused_policy is True
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    eager.interact()
    eager.interact()
    for _ in range(2):
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for k in ("states", "actions", "returns", "dones"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(eager.env.state, graph.env.state)
