"""Which branches and states of the step do the reference's tapes reach?  The oracle (oracle/mm_oracle.c) counts them
(orc_step_census) while every step tape is replayed teacher-forced: a name nobody reaches is a place where the oracle is
not pinned to the reference, and where the HIP kernels, pinned to the oracle bit for bit, would copy its mistake.  Every
name must be reached by a tape or stand, with the reason, in tests/golden/cv_unreached.json; the placed cv_* / ipm_cv_*
tapes (tools/gen_golden.py, section 11) are there for what the other tapes miss.  No GPU needed.

The IDM env's tapes (idm_*) are not replayed here: the oracle has no merge-multi-agent-hdv-v1 (mm_create refuses the env
kind), that env is pinned tape-to-kernel directly in tests/test_idm_env_gpu.py."""
import os

import numpy as np
import pytest

import oracle_env
from golden_util import GOLDEN, episode_files, replay
from tape_census_util import cv_files, cv_index, cv_unreached, tape_name

CV = cv_files()
# The mm_math_* names exist only under include/mm_math.h (math mode 1: the device arithmetic of the bicycle step); they are
# counted in a second pass over every tape in that mode (where the older tapes may hold up to 6 knife-edges, as in
# tests/test_oracle_golden.py; the cv tapes none, test_cv_tape_alone).


def _census_of(paths, mode=0, max_knife_edges=0):
    oracle_env.set_math_mode(mode)
    oracle_env.step_census_reset(True)
    try:
        for path in paths:
            replay(oracle_env.OracleEnv, path, tol=1e-9, max_knife_edges=max_knife_edges)
        return oracle_env.step_census()
    finally:
        oracle_env.step_census_reset(False)
        oracle_env.set_math_mode(0)


@pytest.fixture(scope="module")
def census():
    """One pass over every step tape on the -O2 oracle under libm (math mode 0); the committed tapes hold no knife-edge there.
    Plus the mm_math_* names from a pass over every tape under include/mm_math.h."""
    got = _census_of(episode_files())
    assert not any(v for k, v in got.items() if k.startswith("mm_math_"))
    got.update({k: v for k, v in _census_of(episode_files(), mode=1, max_knife_edges=6).items() if k.startswith("mm_math_")})
    return got


def test_every_name_is_reached_or_explained(census):
    unreached = cv_unreached()
    assert set(unreached) <= set(census), sorted(set(unreached) - set(census))  # no stale names
    for name, why in unreached.items():
        assert len(why) > 40 and ".py" in why, name  # a sentence that cites the reference (or its stand-in solver)
    never = sorted(k for k, v in census.items() if v == 0)
    assert never == sorted(unreached), {"no tape reaches": sorted(set(never) - set(unreached)),
                                        "listed as unreachable, yet reached": sorted(set(unreached) - set(never))}
    assert len(census) >= 80


def test_index_and_tapes_agree(census):
    index = cv_index()
    assert sorted(index) == [tape_name(p) for p in CV]  # a missing or an unlisted tape fails here, by name
    for name, reach in index.items():
        assert reach and set(reach) <= set(census), name
        assert name.startswith(("cv_", "ipm_cv_")) and os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 64 * 1024
    # every name the cv tapes are there for is reached by them alone (counts add up: all tapes minus the cv tapes)
    alone = [_census_of([p]) for p in CV]
    alone_mm = _census_of(CV, mode=1)
    mine = sorted({n for reach in index.values() for n in reach})
    assert [n for n in mine if not n.startswith("mm_math_") and census[n] != sum(c[n] for c in alone)] == [], "reached without the cv tapes"
    assert [n for n in mine if n.startswith("mm_math_") and census[n] != alone_mm[n]] == [], "reached without the cv tapes"


@pytest.mark.parametrize("mode", [0, 1], ids=["libm", "mm_math"])
@pytest.mark.parametrize("path", CV, ids=tape_name)
def test_cv_tape_alone(path, mode):
    """Each placed tape by itself: within 1e-9 of the reference with every discrete quantity exact and NO knife-edge, under
    libm and under include/mm_math.h (so the GPU replay can demand zero too), reaching each name cv_index.json gives it."""
    z = np.load(path, allow_pickle=False)
    assert 2 <= z["init_f"].shape[0] <= 6 and len(z["actions"]) <= 40
    got = _census_of([path], mode=mode, max_knife_edges=0)
    for name in cv_index()[tape_name(path)]:
        if name.startswith("mm_math_") == (mode == 1):  # (the mm_math_* names: under include/mm_math.h, the others under libm)
            assert got[name] > 0, (tape_name(path), name)


def test_census_is_exact_under_the_env_loop():
    """The counters are atomic adds: a batch of E copies of one tape's start, stepped by the OpenMP loop over envs, counts
    exactly E times what one env counts."""
    from golden_util import SI, env_kwargs, load_episode
    import torch
    path = os.path.join(GOLDEN, "cv_v1_reverse_mass.npz")
    z, meta = load_episode(path)
    f0, i0, n = z["init_f"], z["init_i"], meta["n"] + meta["n_hdv"]
    counts = []
    for E in (1, 257):
        env = oracle_env.OracleEnv(E=E, N=n, **env_kwargs(meta))
        rep = lambda a: np.repeat(a[None], E, 0)  # noqa: E731
        oracle_env.step_census_reset(True)
        env.set_kinematics(rep(f0[:, 0]), rep(f0[:, 1]), rep(f0[:, 2]), rep(f0[:, 3]), n_merge=np.full(E, meta["n_merge"]),
                           kind=rep(i0[:, SI["kind"]]))
        for t in range(meta["steps"]):
            act = np.ones(n, dtype=np.int32)  # (the HDV's slot takes no action)
            act[:meta["n"]] = z["actions"][t]
            env.step(torch.tensor(rep(act), dtype=torch.int32))
        counts.append(oracle_env.step_census())
        oracle_env.step_census_reset(False)
        env.close()
    assert counts[0]["clip_speed_below_minus_max"] == 2 and sum(counts[0].values()) > 500
    assert counts[1] == {k: 257 * v for k, v in counts[0].items()}


def test_census_is_off_by_default():
    oracle_env.step_census_reset(False)
    replay(oracle_env.OracleEnv, CV[0], tol=1e-9)
    assert not any(oracle_env.step_census().values())


def test_failed_kkt_factorisations_through_the_qp_entry():
    """cvqp.npz: QPs of get_G's form on which the reference-side coneqp fails to factor its KKT matrix -- the first one (no
    iterate: NaN) and a later one (the iterate stands, status "unknown").  No state of the env gets there (cv_unreached.json),
    so the oracle's interior point is pinned on them through mm_shield_qp: same d and slack bit for bit (NaN where the
    reference has none), same status and iteration count."""
    z = np.load(os.path.join(GOLDEN, "cvqp.npz"))
    env = oracle_env.OracleEnv(1, 2, config={"safety_guarantee": "none"})
    oracle_env.step_census_reset(True)
    try:
        u, st, it = env.shield_qp(z["G"], z["h"], z["rows"], solver="ipm", with_iters=True)
        got = oracle_env.step_census()
    finally:
        oracle_env.step_census_reset(False)
    assert got["qp_first_factor_failed"] == 2 and got["qp_later_factor_failed"] == len(z["rows"]) - 2
    u = u.numpy()
    for col in (0, 2):
        assert np.array_equal(u[:, col], z["x"][:, col], equal_nan=True), (col, u[:, col], z["x"][:, col])
    assert np.isnan(z["x"][:2]).all() and not z["status"].any()
    assert np.array_equal(st.numpy(), z["status"]) and np.array_equal(it.numpy(), z["iters"])
    env.close()
