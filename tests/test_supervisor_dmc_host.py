"""The "dmc" safety supervisor, host side: the library's exports and scratch query, the opt-in dispatch, the numpy-stream
accounting of MergeEnvCompat and the integrity, knife-edge share and census of the reference's dmc_* tapes.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmc_util as D
from marl_mass_amd import _cabi as abi
from test_supervisor_host import _FakeBackend

HIP_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl-mass_amd", "csrc", "libmm_hip.so")


def test_library_exports_dmc_and_the_abi_list_is_unchanged():
    lib = abi.CLib(HIP_SO)
    assert lib.has_supervisor_dmc and lib.has_supervisor
    raw = C.CDLL(HIP_SO)
    for sym in ("mm_supervise_dmc", "mm_supervise_dmc_scratch_bytes", "mm_supervise", "mm_supervise_scratch_bytes"):
        getattr(raw, sym)
    assert not any("dmc" in s or "supervise" in s for s in abi.CLib.SYMBOLS)  # optional exports, as every entry after the v6 list
    assert (abi.SUP_NONE, abi.SUP_PRIORITY, abi.SUP_DMC, abi.DMC_LITERAL, abi.DMC_TRACE_DOUBLES) == (0, 1, 2, 1, D.TRACE)


def test_dmc_scratch_bytes():
    lib = abi.CLib(HIP_SO)

    def want(E, N, n_points):  # [n_points][4] trajectory + 20 trace + 1 order planes of E N doubles, 5 E N + 1 int32 rounded up
        return 8 * (E * N * (4 * n_points + 20 + 1) + (5 * E * N + 2) // 2)
    assert lib.supervise_dmc_scratch_bytes(1000, 8, 6) == want(1000, 8, 18)
    assert lib.supervise_dmc_scratch_bytes(1, 1, 1) == want(1, 1, 3)
    assert lib.supervise_dmc_scratch_bytes(63, 11, 2, sub_steps=5) == want(63, 11, 10)
    assert lib.supervise_dmc_scratch_bytes(4096, 16, 42) == want(4096, 16, 126)
    for bad in ((1000, 8, 0, 3), (1000, 8, 6, 0), (1000, abi.MM_MAX_AGENTS + 1, 6, 3), (0, 8, 6, 3), (1000, 0, 6, 3),
                (1000, 8, 43, 3),          # more than 128 points
                (1 << 26, 8, 6, 3)):       # E * N * 8 does not fit the work list's int32 items
        with pytest.raises(ValueError):
            lib.supervise_dmc_scratch_bytes(bad[0], bad[1], bad[2], sub_steps=bad[3])
    # the priority entry's answer did not move
    assert lib.supervise_scratch_bytes(1000, 8, 6) == 8 * 1000 * 8 * (10 + 4 * 18)


def test_dispatch_is_opt_in():
    assert abi.supervisor_id("dmc", abi.ENV_V0, dmc=True) == abi.SUP_DMC
    assert abi.supervisor_id("dmc", abi.ENV_V0, True) == abi.SUP_DMC  # the new LAST positional argument
    with pytest.raises(NotImplementedError):
        abi.supervisor_id("dmc", abi.ENV_V1, dmc=True)
    assert abi.supervisor_id("dmc", abi.ENV_HDV_V1, dmc=True) == abi.SUP_NONE
    for flag in (False, True):  # everything else is what it was
        assert abi.supervisor_id("priority", abi.ENV_V0, dmc=flag) == abi.SUP_PRIORITY
        for v in ("none", "cbf-cav", "cbf-avs", None):
            assert abi.supervisor_id(v, abi.ENV_V0, dmc=flag) == abi.SUP_NONE
            assert abi.supervisor_id(v, abi.ENV_V1, dmc=flag) == abi.SUP_NONE
        with pytest.raises(NotImplementedError):
            abi.supervisor_id("priority", abi.ENV_V1, dmc=flag)
    for kind in (abi.ENV_V0, abi.ENV_V1):  # the default still refuses
        with pytest.raises(NotImplementedError):
            abi.supervisor_id("dmc", kind)
    with pytest.raises(NotImplementedError):
        abi.check_supervisor("dmc")


class _Backend(_FakeBackend):
    K = 7

    def __init__(self, E, N, enable_dmc=False, **kw):
        super().__init__(E, N, **kw)
        self.enable_dmc = enable_dmc


def test_compat_hands_dmc_2n_draws_and_consumes_what_the_device_used():
    from marl_mass_amd.compat import MergeEnvCompat
    cfg = {"safety_guarantee": "dmc", "mixed_traffic": False, "traffic_density": 1}
    env = MergeEnvCompat("merge-multi-agent-v0", cfg, backend_factory=_Backend, enable_dmc=True)
    assert env._b.enable_dmc is True
    n = len(env.controlled_vehicles)
    np.random.seed(321)
    st = np.random.get_state()
    want = np.random.random_sample(2 * env._b.N)
    np.random.set_state(st)
    env.step((1,) * n)
    u = env._b.seen[-1]
    assert u is not None and np.array_equal(u.numpy().reshape(-1), want)
    np.random.set_state(st)
    np.random.rand(_Backend.K)
    nxt = np.random.rand()
    np.random.set_state(st)
    env.step((1,) * n)
    assert np.random.rand() == nxt
    # without the opt-in the adapter refuses, as before
    plain = MergeEnvCompat("merge-multi-agent-v0", cfg, backend_factory=_Backend)
    with pytest.raises(NotImplementedError):
        plain.step((1,) * len(plain.controlled_vehicles))


def test_dmc_tapes_integrity_and_census():
    files = D.tapes()
    idx = D.index()
    by_name = {r["name"]: r for r in idx["tapes"]}
    assert len(files) == len(by_name) and len(D.natural_tapes()) >= 12 and len(D.tapes("dmc_placed_")) >= 10 and len(D.tapes("dmc_compat_")) == 1
    parts, size, shapes, horizons = [], 0, set(), set()
    for p in files:
        z, meta = D.load(p)
        name = os.path.basename(p)[:-4]
        r = by_name[name]
        T, n = z["actions"].shape
        m = n + meta["n_hdv"]
        assert n == meta["n"] and 1 <= T <= 4096 and T == r["kept"]
        assert z["sub_f"].shape == (T, m, 11) and z["trace"].shape == (T, m, D.TRACE) and z["uniforms"].shape == (T, 2 * m)
        assert np.array_equal(z["n_draws"], (~np.isnan(z["uniforms"])).sum(axis=1))
        assert (z["n_draws"] == n + 2 * meta["n_hdv"]).all()  # an env always draws n_cav + 2 n_hdv values
        for t in range(T):
            assert sorted(z["order"][t]) == list(range(n))
            assert np.array_equal(z["trace"][t, z["order"][t], D.T_POS], np.arange(n))
        crashed = z["trace"][:, :n, D.T_CRASH] >= 0
        assert np.array_equal(z["actions"] != z["new_actions"], crashed & (z["actions"] != z["new_actions"]))  # no replacement without a crash
        avail = z["trace"][:, :n, D.T_MASK].astype(int)
        assert ((avail >> z["new_actions"]) & 1)[crashed].all()  # a replacement is an available action
        assert r["dropped"] <= D.MAX_DROP * (r["kept"] + r["dropped"]), name
        c = D.census(z, meta)
        assert c == r["census"], name  # the index cannot drift from the tapes
        parts.append(c)
        assert os.path.getsize(p) <= 1024 * 1024
        size += os.path.getsize(p)
        shapes.add((n, meta["n_hdv"]))
        horizons.add((meta["n_step"], meta["simulation_frequency"]))
    assert size < 6 * 1024 * 1024
    assert {(4, 0), (6, 0), (8, 0), (3, 3), (4, 4), (6, 5)} <= shapes
    assert {(6, 15), (1, 15), (2, 15), (6, 25)} <= horizons
    assert idx["dropped"] <= D.MAX_DROP * (idx["kept"] + idx["dropped"])
    assert D.total_census(parts) == idx["census"]


def test_dmc_census_reaches_every_required_branch():
    """Every required census entry, recomputed from the tape fields, is at least CENSUS_MIN = 20.  Replacement by FASTER comes
    from the dmc_placed_faster_wins_* tape alone (dmc_util.faster_wins_scenes says why no other state reaches it)."""
    total = D.total_census(D.census(*D.load(p)) for p in D.tapes())
    short = {k: total[k] for k in D.CENSUS_REQUIRED if total[k] < D.CENSUS_MIN}
    assert not short, "branches the tapes reach fewer than %d times: %s" % (D.CENSUS_MIN, short)


def test_plain_dmc_config_still_raises_without_a_gpu():
    """The refusal is decided on the host: the dispatch a VecMergeEnv built without enable_dmc uses."""
    from marl_mass_amd import vec_env
    import inspect
    sig = inspect.signature(vec_env.BatchedMergeEnv.__init__)
    assert sig.parameters["enable_dmc"].default is False
    with pytest.raises(NotImplementedError):
        abi.supervisor_id("dmc", abi.ENV_V0, dmc=sig.parameters["enable_dmc"].default)
