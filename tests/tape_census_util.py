"""Shared by tests/test_tape_census_host.py and tests/test_tape_census_gpu.py: the placed coverage tapes (cv_* / ipm_cv_*),
their index and allow-list, and the free run of a tape's action script on two backends."""
import glob
import json
import os

import numpy as np
import torch

from golden_util import GOLDEN, SI, env_kwargs, load_episode
from marl_mass_amd import _cabi as abi



def cv_files():
    """The placed coverage tapes: cv_* and their interior-point twins ipm_cv_*."""
    return sorted(glob.glob(os.path.join(GOLDEN, "cv_*.npz")) + glob.glob(os.path.join(GOLDEN, "ipm_cv_*.npz")))


def tape_name(path):
    return os.path.basename(path)[:-4]


def cv_index():
    with open(os.path.join(GOLDEN, "cv_index.json")) as f:
        return json.load(f)


def cv_unreached():
    with open(os.path.join(GOLDEN, "cv_unreached.json")) as f:
        return json.load(f)


def free_run_pair(make_a, make_b, path):
    """The tape's own action script free-running from its placed initial state on two backends, for the tape's length:
    every state plane, observation and output must be the same bits."""
    z, meta = load_episode(path)
    n = meta["n"] + meta.get("n_hdv", 0)
    kw = env_kwargs(meta)
    f0, i0 = z["init_f"], z["init_i"]
    envs = [mk(E=1, N=n, **kw) for mk in (make_a, make_b)]
    first = [e.set_kinematics(f0[None, :, 0], f0[None, :, 1], f0[None, :, 2], f0[None, :, 3], n_merge=np.array([meta["n_merge"]]),
                              kind=i0[None, :, SI["kind"]]) for e in envs]
    def same(a, b):  # NaN marks "nothing here" in planes and outputs: equal to itself, everything else by value
        a, b = a.cpu(), b.cpu()
        return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) if a.is_floating_point() else torch.equal(a, b)

    assert same(first[0][0], first[1][0]) and same(first[0][1], first[1][1]), (path, "reset obs / mask")
    for t in range(meta["steps"]):
        act = np.ones((1, n), dtype=np.int32)
        act[0, :meta["n"]] = z["actions"][t]
        res = [e.step(torch.tensor(act, dtype=torch.int32, device=e.device)) for e in envs]
        (oa, ra, da, outa), (ob, rb, db, outb) = res
        assert same(oa, ob) and same(ra, rb) and same(da, db), (path, t, "obs / reward / done")
        for k in outa:
            assert same(outa[k], outb[k]), (path, t, k)
        assert same(envs[0].u8, envs[1].u8) and same(envs[0].env_i32, envs[1].env_i32), (path, t, "discrete state")
        assert same(envs[0].f64, envs[1].f64), (path, t, "float state planes")
        for plane in ("QP_ROWS", "QP_D", "STATUS", "SAFE_ACC", "SAFE_STEER", "LC_MARGIN", "HEADWAY"):  # what the shield decided
            k = abi.T[plane]
            assert same(envs[0].trace[:, k], envs[1].trace[:, k]), (path, t, plane)
        if bool(da[0]):
            break
    for e in envs:
        e.poll_errors()
        e.close()
