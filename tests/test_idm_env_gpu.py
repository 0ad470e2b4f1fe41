"""merge-multi-agent-hdv-v1 (the all-HDV IDM baseline, MergeEnvLCHDV) on the MI355X against the reference's idm_* tapes
(tools/gen_golden_hdv.py): teacher-forced steps, free runs from the reference spawn through the compat adapter, the device
reset's count draw in a ragged density-3 batch, graph capture, sharding, resume and the batched eval_idm.py."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from golden_util import SF, SI
from marl_mass_amd import _cabi as abi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENV_ID = "merge-multi-agent-hdv-v1"
TOL = 1e-9
TAPES = sorted(glob.glob(os.path.join(GOLDEN, "idm_*.npz")))


def _load(path):
    z = np.load(path, allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def _env(E, N, ht=1.2, density=1, **kw):
    from marl_mass_amd import VecMergeEnv
    cfg = {"HEADWAY_TIME": ht, "traffic_density": density}
    return VecMergeEnv(E, N, env_id=ENV_ID, config=cfg, obs_f64=True, **kw)


def _spawn(env, z):
    m = z["init_f"].shape[0]
    pad = lambda a, fill: np.concatenate([a, np.full(env.N - m, fill)])[None]  # noqa: E731
    f = z["init_f"]
    return env.set_kinematics(pad(f[:, 0], np.nan), pad(f[:, 1], 0.0), pad(f[:, 2], 0.0), pad(f[:, 3], 0.0),
                              n_merge=np.zeros(1, dtype=np.int32), kind=pad(np.full(m, 2), 0))


def _force(env, z, t, time):
    """Teacher forcing: the reference's state at the end of step t - 1 (every vehicle an HDV: its last IDM action persists in
    the SAFE_* planes, its MOBIL timer in G_VX, include/mm_abi.h)."""
    F, B, EP = abi.F, abi.B, abi.EP
    gf, gi = z["end_f"][t - 1], z["end_i"][t - 1]
    m = gf.shape[0]
    put = lambda plane, v: plane[0, :m].copy_(torch.as_tensor(np.asarray(v)).to(plane.dtype))  # noqa: E731
    for name, col in (("X", "x"), ("Y", "y"), ("HEADING", "heading"), ("SPEED", "speed"), ("TARGET_SPEED", "target_speed"),
                      ("SAFE_STEER", "act_steer"), ("SAFE_ACC", "act_acc"), ("G_VX", "timer")):
        put(env.f64[F[name]], gf[:, SF[col]])
    for name, col in (("LANE", "lane"), ("TARGET_LANE", "target_lane"), ("SPEED_INDEX", "speed_index"), ("CRASHED", "crashed"),
                      ("KIND", "kind")):
        put(env.u8[B[name]], gi[:, SI[col]])
    env.env_i32[EP["STEPS"], 0] = t
    env.env_i32[EP["TIME"], 0] = time
    env.env_i32[EP["N_MERGE"], 0] = 0


def _info_row(info, m):
    return np.array([float(info["crashed"][0, 0]), float(info["average_speed"][0]), float(info["traffic_speed"][0]),
                     float(info["min_headway"][0])])


@pytest.mark.parametrize("path", TAPES, ids=[os.path.basename(p)[:-4] for p in TAPES])
def test_idm_tape_teacher_forced(path):
    """Every step of the tape from the reference's own state at its start."""
    z, meta = _load(path)
    m, K = meta["n_hdv"], meta["K"]
    env = _env(1, m, meta["headway_time"], meta["density"])
    obs, _ = _spawn(env, z)
    assert np.abs(obs[0].cpu().numpy() - z["reset_obs"]).max() <= TOL
    s_at = 0
    for t in range(meta["steps"]):
        if t > 0:
            _force(env, z, t, s_at)
        obs, rew, done, info = env.step(None)
        nsub = int(z["sub_count"][t])
        assert int(env.env_i32[abi.EP["TIME"], 0]) == s_at + nsub, (path, t, "sub-step count")
        assert bool(done[0]) == bool(z["dones"][t]), (path, t)
        ref = z["end_f"][t]
        assert np.array_equal(info["crashed"][0, :m].cpu().numpy(), z["end_i"][t][:, 3]), (path, t)
        for name, col in (("X", "x"), ("Y", "y"), ("SPEED", "speed"), ("HEADING", "heading")):
            assert np.abs(env.f64[abi.F[name], 0, :m].cpu().numpy() - ref[:, SF[col]]).max() <= TOL, (path, t, name)
        assert np.array_equal(env.u8[abi.B["LANE"], 0, :m].cpu().numpy(), z["end_i"][t][:, SI["lane"]]), (path, t)
        if t < K:
            assert np.abs(obs[0].cpu().numpy() - z["obs"][t]).max() <= TOL, (path, t, "obs")
        assert abs(float(rew[0]) - z["rewards"][t]) <= TOL, (path, t, "reward")
        np.testing.assert_allclose(_info_row(info, m), z["info_f"][t, 1:], rtol=0, atol=TOL)
        assert abs(float(env.f64[abi.F["SPEED"], 0, 0]) - z["info_f"][t, 0]) <= TOL
        if done[0]:
            assert float(info["merge_percent"][0]) == 100.0
        s_at += nsub
    env.poll_errors()


@pytest.mark.parametrize("path", TAPES, ids=[os.path.basename(p)[:-4] for p in TAPES])
def test_idm_tape_free_run(path):
    """The whole episode from the reference spawn: through MergeEnvCompat (its own numpy replay of the spawn) where the
    tape comes from a seed, through set_kinematics for the placed scenarios."""
    from marl_mass_amd import compat
    z, meta = _load(path)
    m, T = meta["n_hdv"], meta["steps"]
    if meta["placement"] is None:
        env = compat.make(ENV_ID, config={"HEADWAY_TIME": meta["headway_time"], "traffic_density": meta["density"]})
        obs, avail = env.reset(is_training=False, testing_seeds=meta["seed"])
        assert obs.shape == (m, 30) and np.shape(avail) == (0,)
        assert np.abs(obs - z["reset_obs"]).max() <= TOL
        step = lambda: env.step(None)  # noqa: E731
    else:
        b = _env(1, 12, meta["headway_time"], meta["density"])
        _spawn(b, z)

        def step():
            o, r, d, info = b.step(None)
            out = {"speed": float(b.f64[abi.F["SPEED"], 0, 0]), "crashed": bool(info["crashed"][0, 0]),
                   "average_speed": float(info["average_speed"][0]), "traffic_speed": float(info["traffic_speed"][0]),
                   "min_headway": float(info["min_headway"][0])}
            if d[0]:
                out["merge_percent"] = float(info["merge_percent"][0])
            return o[0, :m].cpu().numpy().reshape(m, 5, 6), float(r[0]), bool(d[0]), out
    for t in range(T):
        o, r, d, info = step()
        assert o.shape == (m, 5, 6)
        if t < meta["K"]:
            assert np.abs(o.reshape(m, 30) - z["obs"][t]).max() <= TOL, (path, t)
        assert abs(r - z["rewards"][t]) <= TOL and d == bool(z["dones"][t]), (path, t)
        got = [info["speed"], float(info["crashed"]), info["average_speed"], info["traffic_speed"], info["min_headway"]]
        np.testing.assert_allclose(got, z["info_f"][t], rtol=0, atol=TOL, err_msg="%s step %d" % (path, t))
        assert ("merge_percent" in info) == d
        assert set(info) <= {"speed", "crashed", "average_speed", "traffic_speed", "min_headway", "merge_percent"}
    if meta["placement"] is None:
        assert env.is_crashed() == meta["eval"]["crashed"]


def test_ragged_density3_device_reset():
    with open(os.path.join(GOLDEN, "idm_reset.json")) as f:
        ref = json.load(f)["3"]["counts"]
    E, N = 4096, 11
    env = _env(E, N, 1.2, 3, draw_counts=True, seed=11)
    obs, _ = env.reset()
    kind = env.u8[abi.B["KIND"]].cpu().numpy()
    assert set(np.unique(kind)) <= {0, 2}
    n = (kind == 2).sum(1)
    assert all(((kind[e, :n[e]] == 2).all() and (kind[e, n[e]:] == 0).all()) for e in range(E))  # occupied slots are a prefix
    cnt = {int(k): int(v) for k, v in zip(*np.unique(n, return_counts=True))}
    assert sorted(cnt) == sorted(int(k) for k in ref)
    for k, w in zip(range(7, 12), (1, 2, 3, 2, 1)):  # sum of two uniform three-way choices
        p = w / 9.0
        assert abs(cnt[k] / E - p) <= 5 * np.sqrt(p * (1 - p) / E), (k, cnt[k])
    o = obs.cpu().numpy()
    assert (o[kind == 0] == 0).all() and (o[kind == 2][:, 0] == 1).all()
    for t in range(env.T):
        obs, rew, done, info = env.step(None)
        for k in ("average_speed", "traffic_speed", "min_headway"):
            assert torch.isfinite(info[k]).all(), (t, k)
        assert torch.isfinite(rew).all() and torch.isfinite(obs).all()
    assert bool(done.all())  # steps >= T at the latest
    env.poll_errors()


def test_graph_capture_equals_eager():
    E, N, T = 1024, 11, 12
    eager = _env(E, N, 0.5, 3, draw_counts=True, seed=5, auto_reset=True)
    graph = _env(E, N, 0.5, 3, draw_counts=True, seed=5, auto_reset=True)
    eager.reset()
    graph.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph.step(None)  # warm-up, outside the capture
        eager.step(None)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph.step(None)
    for _ in range(T):
        g.replay()
        _, r, d, _ = eager.step(None)
        torch.cuda.synchronize()
        assert torch.equal(graph.out["reward"], r) and torch.equal(graph.out["done"], d)
        assert torch.equal(graph.obs, eager.obs)
    assert torch.equal(graph.state, eager.state)


def test_sharding_and_resume():
    E, N = 512, 11
    full = _env(E, N, 1.2, 3, draw_counts=True, seed=7, auto_reset=True)
    full.reset()
    halves = []
    for first, cnt in ((0, E // 2), (E // 2, E - E // 2)):
        h = _env(cnt, N, 1.2, 3, draw_counts=True, seed=7, auto_reset=True, first_env=first)
        h.reset()
        halves.append(h)
    snap, later = None, []
    for t in range(8):
        if t == 4:
            snap = full.state_dict()
        o, r, d, _ = full.step(None)
        if t >= 4:
            later.append((o.clone(), r.clone()))
        for k, h in enumerate(halves):
            sl = slice(0, E // 2) if k == 0 else slice(E // 2, E)
            oh, rh, _, _ = h.step(None)
            assert torch.equal(oh, o[sl]) and torch.equal(rh, r[sl])
            assert torch.equal(h.f64.nan_to_num(), full.f64[:, sl].nan_to_num())
    res = _env(E, N, 1.2, 3, draw_counts=True, seed=7, auto_reset=True)
    res.load_state_dict(snap)
    for t in range(4):
        o, r, _, _ = res.step(None)
        assert torch.equal(o, later[t][0]) and torch.equal(r, later[t][1])
    assert torch.equal(res.state, full.state)


def test_idm_evaluation_matches_the_reference_episodes():
    from marl_mass_amd.rollout import idm_evaluation
    for ht in (1.2, 0.5):
        for density in (1, 2, 3):
            tapes = [_load(p) for p in TAPES]
            tapes = [(z, m) for z, m in tapes if m["placement"] is None and m["headway_time"] == ht and m["density"] == density]
            assert tapes
            env = _env(len(tapes), 12, ht, density)
            ext = idm_evaluation(env, [m["seed"] for _, m in tapes])
            for k, (_, meta) in enumerate(tapes):
                ev = meta["eval"]
                assert ext["steps"][k] == ev["steps"] and ext["crash_count"][k] == ev["crashed"]
                for key, rk in (("avg_speeds", "avg_speed"), ("traffic_speeds", "traffic_speed"), ("min_headways", "min_headway"),
                                ("merge_percents", "merge_percent")):
                    assert abs(ext[key][k] - ev[rk]) <= TOL, (meta["seed"], key, ext[key][k], ev[rk])
            assert ext["step_time"][0] > 0
