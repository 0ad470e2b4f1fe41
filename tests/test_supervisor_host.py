"""The "priority" safety supervisor, host side: dispatch, the library's scratch query, the numpy-stream accounting of
MergeEnvCompat and the integrity of the reference's prio_* tapes.  No GPU needed."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from marl_mass_amd import _cabi as abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HIP_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl-mass_amd", "csrc", "libmm_hip.so")


def prio_tapes():
    return sorted(glob.glob(os.path.join(GOLDEN, "prio_*.npz")))


def test_supervisor_dispatch():
    assert abi.supervisor_id("priority", abi.ENV_V0) == abi.SUP_PRIORITY
    for v in ("none", "cbf-cav", "cbf-avs", None):
        assert abi.supervisor_id(v, abi.ENV_V0) == abi.SUP_NONE
        assert abi.supervisor_id(v, abi.ENV_V1) == abi.SUP_NONE
    with pytest.raises(NotImplementedError):
        abi.supervisor_id("priority", abi.ENV_V1)
    for kind in (abi.ENV_V0, abi.ENV_V1):
        with pytest.raises(NotImplementedError):
            abi.supervisor_id("dmc", kind)
    for v in ("priority", "dmc"):  # the old gate is unchanged
        with pytest.raises(NotImplementedError):
            abi.check_supervisor(v)


def test_scratch_bytes_from_the_hip_library():
    lib = abi.CLib(HIP_SO)  # loads without a GPU, like mm_state_layout
    assert lib.has_supervisor
    E, N, n_step = 1000, 8, 6
    assert lib.supervise_scratch_bytes(E, N, n_step) == 8 * E * N * (10 + 4 * 3 * n_step)
    assert lib.supervise_scratch_bytes(E, N, n_step, sub_steps=15) == 8 * E * N * (10 + 4 * 15 * n_step)
    with pytest.raises(ValueError):
        lib.supervise_scratch_bytes(E, N, 0)
    with pytest.raises(ValueError):
        lib.supervise_scratch_bytes(E, N, 6, sub_steps=0)
    with pytest.raises(ValueError):
        lib.supervise_scratch_bytes(E, abi.MM_MAX_AGENTS + 1, 6)


class _FakeBackend(object):
    """Stands in for VecMergeEnv (E = 1): zero observations, reports n_draws = K per step and keeps the uniforms."""
    K = 5

    def __init__(self, E, N, **kw):
        self.E, self.N, self.device = E, N, torch.device("cpu")
        self.env_i32 = torch.zeros(len(abi.E_PLANES), E, dtype=torch.int32)
        self.n_draws = torch.zeros(E, dtype=torch.int32)
        self.seen = []

    def configure(self, config=None, **kw):
        pass

    def set_kinematics(self, x, y, heading, speed, n_merge=None, env_mask=None, kind=None):
        return torch.zeros(1, self.N, 25, dtype=torch.float64), torch.ones(1, self.N, 5, dtype=torch.uint8)

    def step(self, actions, uniforms=None):
        self.seen.append(None if uniforms is None else uniforms.clone())
        self.n_draws[0] = self.K
        N = self.N
        out = {"reward": torch.zeros(1, dtype=torch.float64), "done": torch.zeros(1, dtype=torch.uint8),
               "agents_rewards": torch.zeros(1, N, dtype=torch.float64), "regional_rewards": torch.zeros(1, N, dtype=torch.float64),
               "agents_dones": torch.zeros(1, N, dtype=torch.uint8), "agents_info": torch.zeros(1, N, 3, dtype=torch.float64),
               "crashed": torch.zeros(1, N, dtype=torch.uint8), "average_speed": torch.zeros(1, dtype=torch.float64),
               "traffic_speed": torch.zeros(1, dtype=torch.float64), "min_headway": torch.zeros(1, dtype=torch.float64),
               "merge_percent": torch.zeros(1, dtype=torch.float64), "action_mask": torch.ones(1, N, 5, dtype=torch.uint8),
               "new_action": actions.view(1, N).clone()}
        return torch.zeros(1, N, 25, dtype=torch.float64), out["reward"], out["done"], out

    def poll_errors(self):
        pass


def test_compat_consumes_what_the_device_used():
    from marl_mass_amd.compat import MergeEnvCompat
    env = MergeEnvCompat("merge-multi-agent-v0", {"safety_guarantee": "priority", "mixed_traffic": False,
                                                  "traffic_density": 1}, backend_factory=_FakeBackend)
    n = len(env.controlled_vehicles)
    np.random.seed(123)
    st = np.random.get_state()
    want = np.random.random_sample(9 * env._b.N)
    np.random.set_state(st)
    env.step((1,) * n)
    u = env._b.seen[-1]
    assert u is not None and np.array_equal(u.numpy().reshape(-1), want)
    # the stream moved by exactly K draws: the next value is the (K+1)-th of the sequence
    np.random.set_state(st)
    np.random.rand(_FakeBackend.K)
    nxt = np.random.rand()
    np.random.set_state(st)
    env.step((1,) * n)  # (re-run from the same state to read the stream right after one step)
    assert np.random.rand() == nxt


def _available(pre_f, pre_i):
    """_get_available_actions (abstract.py:219-240) of one vehicle of the tape."""
    x, y = pre_f[0], pre_f[1]
    lane, sidx = int(pre_i[0]), int(pre_i[2])
    a = {1}
    if lane == 2 and abs(y - 0.0) <= 8.0 and 0 <= x - 320.0 < 105.0:  # bc1 -> bc0 reachable (lane.py:78-90)
        a.add(0)
    if sidx < 4:
        a.add(3)
    if sidx > 0:
        a.add(4)
    return a


def test_prio_tapes_integrity():
    files = prio_tapes()
    assert len(files) >= 20
    with open(os.path.join(GOLDEN, "prio_index.json")) as f:
        index = {r["name"]: r for r in json.load(f)}
    total = to_lc = 0
    mixed = set()
    for p in files:
        z = np.load(p)
        meta = json.loads(str(z["meta"]))
        name = os.path.basename(p)[:-4]
        a, na = z["actions"], z["new_actions"]
        n, m = meta["n"], meta["n"] + meta["n_hdv"]
        assert a.shape == na.shape and a.shape[1] == n and z["uniforms"].shape == (a.shape[0], 9 * m)
        assert np.array_equal(z["n_draws"], (~np.isnan(z["uniforms"])).sum(axis=1))
        # one tie-breaker per controlled vehicle, then two per HDV whose actions a lookahead generates
        assert (z["n_draws"] >= n).all() and ((z["n_draws"] - n) % 2 == 0).all() and (z["n_draws"] <= 9 * n).all()
        if meta["n_hdv"] == 0:
            assert (z["n_draws"] == n).all()
        else:
            mixed.add((meta["n"], meta["n_hdv"]))
        assert z["sub_f"].shape[1] == m and z["obs"].shape == (a.shape[0], n, 25)
        for t, e in zip(*np.nonzero(a != na)):
            assert int(na[t, e]) in _available(z["pre_f"][t, e], z["pre_i"][t, e]), (name, t, e)
        for t in range(a.shape[0]):
            assert sorted(z["order"][t]) == list(range(n))
        repl = int((a != na).sum())
        assert repl >= 1, name
        assert index[name]["replaced"] == repl
        total += repl
        to_lc += int(((a != na) & ((na == 0) | (na == 2))).sum())
        assert os.path.getsize(p) <= 500 * 1024
    assert total >= 150 and to_lc >= 1
    assert {(3, 3), (4, 4), (6, 5)} <= mixed
