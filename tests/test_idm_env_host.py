"""merge-multi-agent-hdv-v1 (the all-HDV IDM baseline, MergeEnvLCHDV), host side: env id to kind and configuration,
supervisor / shield dispatch, the compat adapter's replay of the reference's spawn draws and the integrity of the idm_*
tapes.  No GPU needed."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from marl_mass_amd import _cabi as abi
from marl_mass_amd import compat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENV_ID = "merge-multi-agent-hdv-v1"


def idm_tapes():
    return sorted(glob.glob(os.path.join(GOLDEN, "idm_*.npz")))


def load(path):
    z = np.load(path, allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def test_env_id_kind_and_default_config():
    assert abi.env_kind(ENV_ID) == abi.ENV_HDV_V1 == 2
    assert abi.obs_features(ENV_ID) == 6
    cfg = abi.default_env_config(ENV_ID)
    assert cfg["traffic_type"] == "hdv" and cfg["action_masking"] is False and cfg["lateral_control"] == "steer"
    assert cfg["other_vehicles_type"].endswith("IDMVehicleHist")
    assert cfg["safety_guarantee"] == "priority"  # AbstractEnv's default, never used by this env
    c = abi.make_config(ENV_ID, cfg, draw_counts=True)
    assert c.env_kind == abi.ENV_HDV_V1 and c.shield == abi.SHIELD_NONE and c.mixed_traffic == abi.MIXED_HDV
    assert c.n_hdv == 0 and c.traffic_density == 1
    c = abi.make_config(ENV_ID, dict(cfg, traffic_density=3), draw_counts=True, num_cav=2)
    assert (c.traffic_density, c.num_cav) == (3, 2)
    with pytest.raises(ValueError):
        abi.env_kind("merge-multi-agent-v05")


@pytest.mark.parametrize("sg", ["priority", "dmc", "cbf-cav", "cbf-avs", "none"])
def test_no_supervisor_or_shield(sg):
    assert abi.supervisor_id(sg, abi.ENV_HDV_V1) == abi.SUP_NONE
    assert abi.shield_from_safety_guarantee(sg, abi.ENV_HDV_V1) == abi.SHIELD_NONE
    cfg = dict(abi.default_env_config(ENV_ID), safety_guarantee=sg)
    assert abi.make_config(ENV_ID, cfg).shield == abi.SHIELD_NONE


def test_v1_hdv_traffic_type_still_raises():
    cfg = dict(abi.default_env_config("merge-multi-agent-v1"), traffic_type="hdv")
    with pytest.raises(NotImplementedError):
        abi.make_config("merge-multi-agent-v1", cfg, draw_counts=True)
    with pytest.raises(NotImplementedError):  # and the hdv env does not take another traffic type
        abi.make_config(ENV_ID, dict(abi.default_env_config(ENV_ID), traffic_type="cav"), draw_counts=True)


class _FakeBackend(object):
    """Stands in for VecMergeEnv (E = 1): records the spawn set_kinematics receives, zero observations."""

    def __init__(self, E, N, env_id=None, **kw):
        assert env_id == ENV_ID
        self.E, self.N, self.device = E, N, torch.device("cpu")
        self.env_i32 = torch.zeros(len(abi.E_PLANES), E, dtype=torch.int32)
        self.spawns = []

    def configure(self, config=None, **kw):
        assert kw.get("n_hdv", 0) == 0

    def set_kinematics(self, x, y, heading, speed, n_merge=None, env_mask=None, kind=None):
        self.spawns.append(dict(x=np.asarray(x)[0], y=np.asarray(y)[0], speed=np.asarray(speed)[0], kind=np.asarray(kind)[0],
                                n_merge=int(np.asarray(n_merge)[0])))
        return torch.zeros(1, self.N, 30, dtype=torch.float64), torch.zeros(1, self.N, 5, dtype=torch.uint8)


def test_compat_reset_replays_every_tape_spawn():
    tapes = [p for p in idm_tapes() if load(p)[1]["placement"] is None]
    assert len(tapes) >= 12
    for path in tapes:
        z, meta = load(path)
        env = compat.make(ENV_ID, config={"traffic_density": meta["density"], "HEADWAY_TIME": meta["headway_time"]},
                          backend_factory=_FakeBackend)
        obs, avail = env.reset(is_training=False, testing_seeds=meta["seed"])
        m = meta["n_hdv"]
        assert obs.shape == (m, 30) and np.shape(avail) == (0,)
        sp = env._b.spawns[-1]
        x = sp["x"][:m]
        assert np.isnan(sp["x"][m:]).all() and (sp["kind"][:m] == 2).all() and (sp["kind"][m:] == 0).all()
        np.testing.assert_array_equal(x, z["init_f"][:, 0], err_msg=path)  # the reference's own numpy draws, bit for bit
        np.testing.assert_array_equal(sp["y"][:m], z["init_f"][:, 1])
        np.testing.assert_array_equal(sp["speed"][:m], z["init_f"][:, 3])
        assert sp["n_merge"] == 0 and env.controlled_vehicles == [] and len(env.road.vehicles) == m
        assert env.vehicle is env.road.vehicles[0]


def test_compat_reset_replays_the_spawn_table():
    with open(os.path.join(GOLDEN, "idm_reset.json")) as f:
        table = json.load(f)
    for density, rec in table.items():
        cfg = dict(abi.default_env_config(ENV_ID), traffic_density=int(density))
        for sp in rec["spawns"]:
            x, y, v = compat.hdv_spawn(cfg, sp["seed"])
            assert list(x) == sp["x"] and list(y) == sp["y"] and list(v) == sp["speed"]
        # each total is the sum of two independent uniform three-way choices: counts 1 : 2 : 3 : 2 : 1
        support = sorted(int(k) for k in rec["counts"])
        lo = {1: 2, 2: 4, 3: 7}[int(density)]
        assert support == list(range(lo, lo + 5))


def test_count_code_fold():
    # include/mm_counts.h: mixed_traffic 3 = every drawn vehicle an HDV; the num_CAV override changes the total
    cfg = dict(abi.default_env_config(ENV_ID), traffic_density=3)
    np.random.seed(5)
    totals = {sum(compat.draw_counts(cfg)) for _ in range(200)}
    assert totals == set(range(7, 12))
    np.random.seed(5)
    assert {sum(compat.draw_counts(cfg, num_CAV=1)) for _ in range(200)} == {4, 5, 6}


def test_fixture_integrity():
    with open(os.path.join(GOLDEN, "idm_index.json")) as f:
        index = json.load(f)
    names = {os.path.basename(p)[:-4] for p in idm_tapes()}
    assert {r["name"] for r in index} == names
    seen = set()
    for path in idm_tapes():
        assert os.path.getsize(path) <= 110 * 1024
        z, meta = load(path)
        T, m, K = meta["steps"], meta["n_hdv"], meta["K"]
        assert meta["env_id"] == ENV_ID and meta["n"] == 0 and meta["n_merge"] == 0
        assert z["rewards"].shape == (T,) and z["dones"].shape == (T,) and z["info_f"].shape == (T, 5)
        assert z["dones"][-1] == 1 and not z["dones"][:-1].any()
        assert z["obs"].shape == (K, m, 30) and z["reset_obs"].shape == (m, 30)
        assert z["sub_f"].shape == (int(z["sub_count"][:K].sum()), m, 11)
        assert z["end_f"].shape == (T, m, 11) and z["end_i"].shape == (T, m, 9)
        np.testing.assert_array_equal(z["end_f"][K - 1], z["sub_f"][-1])
        assert (z["sub_i"][:, :, 8] == 2).all()  # every vehicle an HDV
        assert np.isnan(z["merge_percent"][:-1]).all() and z["merge_percent"][-1] == 100.0
        crashed = bool(z["sub_i"][:, :, 3].any()) or meta["eval"]["crashed"]
        if crashed:
            assert T < 100
        seen.add((meta["density"], meta["headway_time"]) if meta["placement"] is None else meta_name(path))
    for d in (1, 2, 3):
        for ht in (1.2, 0.5):
            assert (d, ht) in seen
    assert {"obstacle", "rear_end", "x_neg"} <= seen


def meta_name(path):
    return os.path.basename(path)[:-4].replace("idm_placed_", "")


def test_placed_tapes_cover_the_terminal_rules():
    z, meta = load(os.path.join(GOLDEN, "idm_placed_x_neg.npz"))
    assert z["init_f"][0, 0] < 0 and z["sub_f"][0, 0, 0] < 0 and not z["dones"][0]  # x < 0 ends no episode here
    assert meta["steps"] == 100 and not meta["eval"]["crashed"]
    z, meta = load(os.path.join(GOLDEN, "idm_placed_obstacle.npz"))
    last = z["sub_f"][-1]
    hit = np.flatnonzero(z["sub_i"][-1, :, 3])
    assert meta["eval"]["crashed"] and len(hit) == 1 and abs(last[hit[0], 1] - 4.0) < 1.5 and last[hit[0], 0] > 400
    z, meta = load(os.path.join(GOLDEN, "idm_placed_rear_end.npz"))
    assert meta["eval"]["crashed"] and int(z["sub_i"][-1, :, 3].sum()) == 2
