"""The "priority" safety supervisor on the MI355X against the reference's prio_* tapes (CAV-only and mixed traffic):
every recorded step teacher-forced with the recorded uniforms (new_action, n_draws, and the step's obs / rewards /
flags), free runs, a ragged batch, the Philox path (shards, resume, graph capture) and the MergeEnvCompat adapter on the
global numpy stream."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from marl_mass_amd import _cabi as abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9
# columns of sub_f / sub_i (tools/gen_golden._veh_snapshot)
SF = {"x": 0, "y": 1, "heading": 2, "speed": 3, "target_speed": 4, "act_steer": 5, "act_acc": 6, "timer": 10}
SI = {"lane": 0, "target_lane": 1, "speed_index": 2, "crashed": 3, "kind": 8}


def _tapes(prefix="prio_v0_"):
    return sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def _load(path):
    z = np.load(path)
    return z, json.loads(str(z["meta"]))


def _env(E, N, ht, n_hdv=0, **kw):
    from marl_mass_amd import VecMergeEnv
    cfg = {"safety_guarantee": "priority", "HEADWAY_TIME": ht, "action_masking": True}
    return VecMergeEnv(E, N, env_id="merge-multi-agent-v0", config=cfg, obs_f64=True, n_hdv=n_hdv, **kw)


def _force(env, sf, si, steps, n_merge):
    """Teacher forcing: the reference's state at the start of a step, one row per env ([E][m] rows, padded slots: kind 0)."""
    dev = env.device
    sf = np.nan_to_num(np.asarray(sf, dtype=np.float64))
    si = np.asarray(si)
    hdv = si[..., SI["kind"]] == 2
    put = lambda plane, v: plane.copy_(torch.as_tensor(np.asarray(v), device=dev).to(plane.dtype))  # noqa: E731
    for name, col in (("X", "x"), ("Y", "y"), ("HEADING", "heading"), ("SPEED", "speed"), ("TARGET_SPEED", "target_speed")):
        put(env.f64[abi.F[name]], sf[..., SF[col]])
    # HDVs keep their last IDM action in the SAFE_* planes and the MOBIL timer in G_VX (mm_abi.h)
    put(env.f64[abi.F["SAFE_STEER"]], np.where(hdv, sf[..., SF["act_steer"]], 0.0))
    put(env.f64[abi.F["SAFE_ACC"]], np.where(hdv, sf[..., SF["act_acc"]], 0.0))
    put(env.f64[abi.F["G_VX"]], np.where(hdv, sf[..., SF["timer"]], np.nan))
    for name in ("LANE", "TARGET_LANE", "SPEED_INDEX", "CRASHED", "KIND"):
        put(env.u8[abi.B[name]], si[..., SI[name.lower()]])
    env.u8[abi.B["HL_ACTION"]].fill_(255)
    env.u8[abi.B["FLAGS"]].zero_()
    env.u8[abi.B["HIST_LEN"]].zero_()
    put(env.env_i32[abi.EP["STEPS"]], steps)
    put(env.env_i32[abi.EP["TIME"]], 3 * np.asarray(steps))
    put(env.env_i32[abi.EP["N_MERGE"]], n_merge)


@pytest.mark.parametrize("path", _tapes(), ids=lambda p: os.path.basename(p)[:-4])
def test_prio_tape_teacher_forced(path):
    """One env per recorded step, all in one launch: new_action and n_draws exactly, then the step itself."""
    z, meta = _load(path)
    T, n = z["actions"].shape
    m = z["sub_f"].shape[1]
    env = _env(T, m, meta["headway_time"], n_hdv=meta["n_hdv"])
    _force(env, z["sub_f"], z["sub_i"], np.arange(T), np.full(T, meta["n_merge"]))
    act = np.ones((T, m), dtype=np.int32)
    act[:, :n] = z["actions"]
    obs, rew, done, info = env.step(torch.as_tensor(act), uniforms=np.nan_to_num(z["uniforms"]))
    got = info["new_action"].cpu().numpy()[:, :n]
    bad = np.nonzero((got != z["new_actions"]).any(axis=1))[0]
    assert len(bad) == 0, "steps %s: device %s, reference %s" % (bad.tolist(), got[bad].tolist(), z["new_actions"][bad].tolist())
    assert np.array_equal(env.n_draws.cpu().numpy(), z["n_draws"])
    assert np.array_equal(done.cpu().numpy(), z["dones"])
    assert np.abs(obs.cpu().numpy()[:, :n] - z["obs"]).max() <= TOL
    assert np.abs(rew.cpu().numpy() - z["rewards"]).max() <= TOL
    assert np.array_equal(info["action_mask"].cpu().numpy()[:, :n], z["action_mask"])


@pytest.mark.parametrize("path", _tapes(), ids=lambda p: os.path.basename(p)[:-4])
def test_prio_tape_free_run(path):
    """From the tape's first state, stepping on its own with the recorded actions and uniforms: the same supervised
    action sequence and the same terminal step."""
    z, meta = _load(path)
    T, n = z["actions"].shape
    m = z["sub_f"].shape[1]
    env = _env(1, m, meta["headway_time"], n_hdv=meta["n_hdv"])
    _force(env, z["sub_f"][:1], z["sub_i"][:1], [0], [meta["n_merge"]])
    for t in range(T):
        act = np.ones((1, m), dtype=np.int32)
        act[0, :n] = z["actions"][t]
        _, _, done, info = env.step(torch.as_tensor(act), uniforms=np.nan_to_num(z["uniforms"][t:t + 1]))
        assert np.array_equal(info["new_action"].cpu().numpy()[0, :n], z["new_actions"][t]), t
        assert bool(done[0]) == bool(z["dones"][t]), t


def test_ragged_batch_density3():
    """Every recorded step of every tape in ONE launch of N = 11 slots, tiled to E = 4096: each row equals the
    reference's answer (and so the E = 1 launches of the tests above)."""
    rows = []
    for p in _tapes():
        z, meta = _load(p)
        for t in range(z["actions"].shape[0]):
            rows.append((z, meta, t))
    N, E = 11, 4096
    sf = np.zeros((E, N, 11))
    si = np.zeros((E, N, 9), dtype=np.int64)
    act = np.ones((E, N), dtype=np.int32)
    U = np.zeros((E, 9 * N))
    ht = np.zeros(E)
    for e in range(E):
        z, meta, t = rows[e % len(rows)]
        m, n = z["sub_f"].shape[1], meta["n"]
        sf[e, :m], si[e, :m], act[e, :n] = z["sub_f"][t], z["sub_i"][t], z["actions"][t]
        U[e, :z["uniforms"].shape[1]] = np.nan_to_num(z["uniforms"][t])
        ht[e] = meta["headway_time"]
    out = {}
    for h in (0.5, 1.2):  # HEADWAY_TIME is a per-handle setting: one launch per value, every row present in both
        env = _env(E, N, h, n_hdv=1)
        _force(env, sf, si, np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64))
        out[h] = [x.cpu().numpy().copy() for x in env.supervise(torch.as_tensor(act), uniforms=U)]
    for e in range(E):
        z, meta, t = rows[e % len(rows)]
        new, nd = out[meta["headway_time"]]
        assert np.array_equal(new[e, :meta["n"]], z["new_actions"][t]), (e, t)
        assert int(nd[e]) == int(z["n_draws"][t])


def test_philox_path_sharding_resume_and_step():
    E, N = 512, 8
    full = _env(E, N, 1.2, seed=7)
    full.reset()
    g = torch.Generator().manual_seed(3)
    acts = [torch.multinomial(torch.tensor([0.15, 0.15, 0.1, 0.5, 0.1]), E * N, True, generator=g).view(E, N).int()
            for _ in range(6)]
    halves = []
    for first, cnt in ((0, E // 2), (E // 2, E - E // 2)):
        h = _env(cnt, N, 1.2, seed=7, first_env=first)
        h.reset()
        halves.append(h)
    snap = None
    news = []
    for t, a in enumerate(acts):
        if t == 3:
            snap = full.state_dict()
        _, _, _, info = full.step(a.cuda())
        news.append(info["new_action"].clone())
        for k, h in enumerate(halves):
            sl = slice(0, E // 2) if k == 0 else slice(E // 2, E)
            _, _, _, ih = h.step(a[sl].cuda())
            assert torch.equal(ih["new_action"], news[-1][sl])
            assert torch.equal(h.f64.nan_to_num(), full.f64[:, sl].nan_to_num())
        assert torch.equal(full.n_draws, (full.u8[abi.B["KIND"]] == 1).sum(1).int())
    assert sum(int((n.cpu() != a).sum()) for n, a in zip(news, acts)) > 0, "no action was ever replaced"
    res = _env(E, N, 1.2, seed=7)  # resume from the snapshot: bit-identical continuation
    res.load_state_dict(snap)
    for t in range(3, 6):
        _, _, _, info = res.step(acts[t].cuda())
        assert torch.equal(info["new_action"], news[t])
    assert torch.equal(res.state, full.state)
    full.poll_errors()


def test_graph_captured_rollout_with_priority_equals_eager():
    from marl_mass_amd import VecMergeEnv
    from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout
    E, N, T = 1024, 8, 10
    kw = dict(env_id="merge-multi-agent-v0", config={"safety_guarantee": "priority", "HEADWAY_TIME": 0.5}, seed=9,
              auto_reset=True, n_hdv=3)
    torch.manual_seed(3)
    actor, critic = ActorNetwork(25, 128, 5).cuda(), CriticNetwork(25, 5, 128).cuda()
    eager = DeviceRollout(VecMergeEnv(E, N, **kw), actor, critic, roll_out_n_steps=T, sample_seed=4)
    graph = DeviceRollout(VecMergeEnv(E, N, **kw), actor, critic, roll_out_n_steps=T, sample_seed=4, use_graph=True)
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    eager.interact()
    eager.interact()
    for _ in range(2):
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for k in ("states", "actions", "returns", "dones"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(eager.env.state, graph.env.state)


def test_compat_reproduces_the_reference_stream():
    """MergeEnvCompat with priority, mixed traffic, seeded like prio_compat_*: the policy's np.random.choice and the
    supervisor share the global stream; new_action and rewards follow the reference's."""
    from marl_mass_amd.compat import MergeEnvCompat
    path = _tapes("prio_compat_")[0]
    z, meta = _load(path)
    n, h = meta["n"], meta["n_hdv"]
    env = MergeEnvCompat("merge-multi-agent-v0", {"safety_guarantee": "priority", "HEADWAY_TIME": meta["headway_time"],
                                                  "action_masking": True, "mixed_traffic": True, "n_step": 6})
    env._num_vehicles = lambda num_CAV=0: (n, h)  # the tape fixes the counts, as tools/gen_golden.make_env does
    env.seed = meta["seed"]
    env.reset()
    for t in range(z["actions"].shape[0]):
        a = tuple(int(x) for x in np.random.choice(5, n, p=meta["p"]))
        assert a == tuple(z["actions"][t]), t
        _, r, d, info = env.step(a)
        assert info["new_action"] == tuple(int(x) for x in z["new_actions"][t]), t
        assert abs(r - z["rewards"][t]) <= TOL and d == bool(z["dones"][t]), t


def test_priority_still_raises_where_unsupported():
    from marl_mass_amd import VecMergeEnv
    v1 = VecMergeEnv(4, 4, env_id="merge-multi-agent-v1", config={"safety_guarantee": "priority"})
    v1.reset()
    with pytest.raises(NotImplementedError):
        v1.step(torch.ones(4, 4, dtype=torch.int32, device="cuda:0"))
    dmc = VecMergeEnv(4, 4, env_id="merge-multi-agent-v0", config={"safety_guarantee": "dmc"})
    dmc.reset()
    with pytest.raises(NotImplementedError):
        dmc.step(torch.ones(4, 4, dtype=torch.int32, device="cuda:0"))
