"""Host side of the per-env shield parameters (include/mm_env_params.h): validation and filling from the config, the oracle
library's refusal, rollout.group_ext_info, and checkpoints without the new key.  No GPU."""
import numpy as np
import pytest
import torch

import env_params_util as U
import oracle_env
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import group_ext_info
from marl_mass_amd.vec_env import ENV_PARAM_KEYS, env_param_planes


def _cfg(safety="cbf-cav", env_id="merge-multi-agent-v1", eta=0.25, tau=0.7, ht=1.2):
    config = abi.default_env_config(env_id)
    config.update({"safety_guarantee": safety, "HEADWAY_TIME": ht})
    return abi.make_config(env_id, config, cbf_eta=eta, cbf_tau=tau)


def test_plane_order_matches_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mm_env_params.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"MM_ENVP_(\w+) = (\d+)", src))
    assert enum == {"ETA": 0, "TAU": 1, "HEADWAY_TIME": 2, "COUNT": 3}
    assert ENV_PARAM_KEYS == ("cbf_eta", "cbf_tau", "HEADWAY_TIME") == U.KEYS


def test_filling_from_the_config_and_broadcast():
    cfg = _cfg()
    p = env_param_planes({}, 5, cfg)
    assert p.dtype == torch.float64 and p.shape == (3, 5)
    assert torch.equal(p, torch.tensor([0.25, 0.7, 1.2], dtype=torch.float64)[:, None].expand(3, 5))
    eta = [0.5, 0.25, 0.125, 0.0625, 0.03125]
    p = env_param_planes({"cbf_eta": eta, "HEADWAY_TIME": 0.5}, 5, cfg)
    assert p[0].tolist() == eta and p[1].tolist() == [0.7] * 5 and p[2].tolist() == [0.5] * 5
    p = env_param_planes({"cbf_tau": np.linspace(0.5, 1.2, 5), "cbf_eta": torch.tensor(-0.5)}, 5, cfg)  # (eta: any finite value)
    assert p[1].tolist() == np.linspace(0.5, 1.2, 5).tolist() and p[0].tolist() == [-0.5] * 5
    for safety in ("cbf-cav", "cbf-avs_cint"):
        env_param_planes({}, 3, _cfg(safety))


@pytest.mark.parametrize("params,match", [
    ({"eta": 0.1}, "unknown env_params key"),
    ({"cbf_eta": [0.1, 0.2]}, "scalar or have shape"),
    ({"cbf_eta": [[0.1] * 5]}, "scalar or have shape"),
    ({"cbf_eta": float("nan")}, "finite"),
    ({"cbf_tau": [0.5, 0.5, float("inf"), 0.5, 0.5]}, "finite"),
    ({"cbf_tau": 0.0}, "> 0"),
    ({"cbf_tau": [0.5, 0.5, -1.0, 0.5, 0.5]}, "> 0"),
    ({"HEADWAY_TIME": 0.0}, "> 0"),
    ({"HEADWAY_TIME": -1.2}, "> 0"),
])
def test_validation_errors(params, match):
    with pytest.raises(ValueError, match=match):
        env_param_planes(params, 5, _cfg())


@pytest.mark.parametrize("safety,env_id", [("none", "merge-multi-agent-v1"), ("cbf-cav", "merge-multi-agent-v0"),
                                            ("none", "merge-multi-agent-hdv-v1")])
def test_scope_is_the_shielded_v1_env(safety, env_id):
    with pytest.raises(ValueError, match="merge-multi-agent-v1"):
        env_param_planes({}, 5, _cfg(safety, env_id))


def test_oracle_library_refuses():
    """The CPU oracle's envs are uniform: env_params= and set_env_params raise NotImplementedError there, before anything
    else; the library reports the symbol as absent and CLib.SYMBOLS does not list it."""
    clib = oracle_env.library()
    assert not clib.has_env_params and "mm_set_env_params" not in abi.CLib.SYMBOLS
    with pytest.raises(NotImplementedError, match="mm_set_env_params"):
        clib.require_env_params()
    kw = U.env_kw(U.CASES[0])
    with pytest.raises(NotImplementedError, match="mm_set_env_params"):
        oracle_env.OracleEnv(4, 4, env_params={"cbf_eta": 0.5}, **kw)
    env = oracle_env.OracleEnv(4, 4, **kw)
    assert env.env_params is None
    with pytest.raises(NotImplementedError, match="mm_set_env_params"):
        env.set_env_params(cbf_eta=0.5)
    env.clear_env_params()  # nothing set: nothing to do
    env.close()


def test_state_dict_without_the_key():
    """An env without planes writes no "env_params" key, and such a dict -- every checkpoint from before -- loads."""
    kw = U.env_kw(U.CASES[0])
    env = oracle_env.OracleEnv(4, 4, **kw)
    env.reset()
    for a in U.tape(4, 4, 3):
        env.step(a)
    d = env.state_dict()
    assert "env_params" not in d
    other = oracle_env.OracleEnv(4, 4, **kw)
    other.load_state_dict(d)
    a = U.tape(4, 4, 4)[3]
    assert torch.equal(env.step(a)[0], other.step(a)[0]) and torch.equal(env.state, other.state)
    env.close(); other.close()


def test_group_ext_info_against_numpy():
    g = torch.Generator().manual_seed(0)
    E = 60
    groups = torch.randint(0, 12, (E,), generator=g)
    ext = {"steps": torch.randint(1, 101, (E,), generator=g, dtype=torch.int32), "avg_speeds": torch.rand(E, generator=g, dtype=torch.float64) * 30,
           "crash_count": torch.rand(E, generator=g) < 0.3, "min_headway": 0.25,
           "traffic_speeds": torch.rand(E, generator=g, dtype=torch.float64) * 30, "merge_percents": torch.rand(E, generator=g, dtype=torch.float64) * 100}
    got = group_ext_info(ext, groups)
    want = U.group_ext_info_numpy({"steps": ext["steps"].numpy(), "avg_speeds": ext["avg_speeds"].numpy(),
                                   "crash_rate": ext["crash_count"].numpy(), "traffic_speeds": ext["traffic_speeds"].numpy(),
                                   "merge_percents": ext["merge_percents"].numpy()}, groups.numpy())
    assert sorted(got) == sorted(want)
    assert got["count"].tolist() == want["count"].tolist() and int(got["count"].sum()) == E
    for k in want:
        if k != "count":
            # (a mean of <= 60 float64 values in another summation order: a few ulp)
            np.testing.assert_allclose(got[k].numpy(), want[k], rtol=1e-13, atol=0, err_msg=k)
    # a group without envs: count 0, NaN means; an index outside the groups: refused
    got = group_ext_info(ext, groups, n_groups=14)
    assert got["count"][12:].tolist() == [0, 0] and bool(torch.isnan(got["steps"][12:]).all())
    with pytest.raises(ValueError):
        group_ext_info(ext, groups, n_groups=3)
    with pytest.raises(ValueError):
        group_ext_info(ext, groups[:-1])
