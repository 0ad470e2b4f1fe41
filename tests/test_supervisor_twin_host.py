"""The CPU twin of the "priority" supervisor (oracle/mm_oracle.c mm_supervise) against the reference, on the build machine:
every prio_v0_* tape, the adapter's tape and the placed sup_placed_* tapes replayed through OracleEnv.step, in both math
modes; free runs; the Philox path against an outside implementation; the documented refusals; the integrity and the census
of the placed tapes.  No GPU needed.  (At volume the twin is compared with the reference by tools/supervisor_ref_fuzz.py,
whose result is profiles/supervisor_twin/ref_fuzz.json.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import supervisor_twin_util as U
from marl_mass_amd import _cabi as abi

ENV_ID = "merge-multi-agent-v0"
TOL = U.TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def math_mode():
    oe = U.oracle()
    yield oe.set_math_mode
    oe.set_math_mode(0)


def _env(E, N, meta, **kw):
    return U.oracle().OracleEnv(E, N, env_id=ENV_ID, config=U.tape_config(meta), obs_f64=True, n_hdv=min(meta["n_hdv"], N - 1), **kw)


def _ids(p):
    return os.path.basename(p)[:-4]


def test_tapes_present():
    assert len(U.tapes("prio_v0_")) >= 20 and len(U.tapes("prio_compat_")) == 1 and len(U.tapes("sup_placed_")) >= 10


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("path", U.replay_tapes(), ids=_ids)
def test_tape_teacher_forced(path, mode, math_mode):
    """One env per recorded step, each forced to the reference's state and fed its uniforms.  Math mode 0 (libm, the
    reference's arithmetic): new_action, n_draws, the priority order, dones and the action mask exactly, obs and rewards within
    TOL.  Math mode 1 (the device arithmetic): the discrete results exactly."""
    z, meta = U.load_tape(path)
    T, n = z["actions"].shape
    m = z["sub_f"].shape[1]
    math_mode(mode)
    env = _env(T, m, meta)
    U.put_state(env, U.tape_state(z), steps=np.arange(T), n_merge=meta["n_merge"])
    act = np.ones((T, m), dtype=np.int32)
    act[:, :n] = z["actions"]
    n_points = meta.get("n_step", 6) * (meta.get("simulation_frequency", 15) // 5)
    with U.Trace(T, m, n_points) as tr:
        obs, rew, done, info = env.step(torch.as_tensor(act), uniforms=np.nan_to_num(z["uniforms"]))
        order = tr.parse()["order"][:, :n]
    got = info["new_action"].numpy()[:, :n]
    bad = np.nonzero((got != z["new_actions"]).any(axis=1))[0]
    assert len(bad) == 0, "steps %s: twin %s, reference %s" % (bad.tolist(), got[bad].tolist(), z["new_actions"][bad].tolist())
    assert np.array_equal(env.n_draws.numpy(), z["n_draws"])
    assert np.array_equal(order, z["order"])
    assert np.array_equal(done.numpy(), z["dones"])
    assert np.array_equal(info["action_mask"].numpy()[:, :n], z["action_mask"])
    if mode == 0:
        assert np.abs(obs.numpy()[:, :n] - z["obs"]).max() <= TOL
        assert np.abs(rew.numpy() - z["rewards"]).max() <= TOL


@pytest.mark.parametrize("path", U.replay_tapes(), ids=_ids)
def test_tape_free_run(path):
    """From the tape's first state, stepping on its own with the recorded actions and uniforms: the same supervised action
    sequence and the same terminal step."""
    z, meta = U.load_tape(path)
    T, n = z["actions"].shape
    m = z["sub_f"].shape[1]
    env = _env(1, m, meta)
    U.put_state(env, U.tape_state(z, slice(0, 1)), steps=0, n_merge=meta["n_merge"])
    for t in range(T):
        act = np.ones((1, m), dtype=np.int32)
        act[0, :n] = z["actions"][t]
        _, _, done, info = env.step(torch.as_tensor(act), uniforms=np.nan_to_num(z["uniforms"][t:t + 1]))
        assert np.array_equal(info["new_action"].numpy()[0, :n], z["new_actions"][t]), t
        assert bool(done[0]) == bool(z["dones"][t]), t
    assert bool(z["dones"][-1]) or T >= 8


def test_placed_tapes_integrity_and_census():
    """The sup_placed_* fixtures: small, consistent with their index, and together with the natural tapes they reach every
    required census entry (counted by the twin while it reproduces the reference's answers)."""
    with open(os.path.join(U.GOLDEN, "sup_placed_index.json")) as f:
        index = {r["name"]: r for r in json.load(f)}
    files = U.tapes("sup_placed_")
    assert sorted(index) == [_ids(p) for p in files]
    total = {}
    for p in U.replay_tapes():
        z, meta = U.load_tape(p)
        assert os.path.getsize(p) <= 500 * 1024
        T, n = z["actions"].shape
        m = z["sub_f"].shape[1]
        assert z["uniforms"].shape == (T, 9 * m) and np.array_equal(z["n_draws"], (~np.isnan(z["uniforms"])).sum(axis=1))
        env = _env(T, m, meta)
        U.put_state(env, U.tape_state(z), steps=np.arange(T), n_merge=meta["n_merge"])
        act = np.ones((T, m), dtype=np.int32)
        act[:, :n] = z["actions"]
        new, _ = env.supervise(torch.as_tensor(act), uniforms=np.nan_to_num(z["uniforms"]))
        assert np.array_equal(new.numpy()[:, :n], z["new_actions"])
        cen = U.census()
        if _ids(p) in index:
            assert {k: v for k, v in cen.items() if v} == index[_ids(p)]["census"], _ids(p)
            assert index[_ids(p)]["replaced"] == int((z["actions"] != z["new_actions"]).sum())
        U.add_census(total, cen)
    missing = [k for k in U.CENSUS_REQUIRED if total.get(k, 0) < 1]
    assert not missing, missing
    assert set(U.CENSUS_REQUIRED) <= set(U.census_names()) and "replaced_by_2" in U.census_names()


def test_placed_generator_is_deterministic_and_reaches_the_census():
    """The placed states the GPU tests regenerate from a seed: the same on every run, and alone they already reach every
    required entry at least CENSUS_MIN times under the default horizon."""
    a, b = U.placed_scenes(20261019), U.placed_scenes(20261019)
    assert a == b and len(a) == 40 * len(U.FAMILIES)
    N = 11
    st, act = U.scenes_to_state(a, N)
    total = {}
    for n_step, sim in ((6, 15), (1, 15), (6, 5)):
        env = U.oracle().OracleEnv(act.shape[0], N, env_id=ENV_ID, obs_f64=True, n_hdv=1,
                                   config={"safety_guarantee": "priority", "HEADWAY_TIME": 1.2, "n_step": n_step, "simulation_frequency": sim})
        U.put_state(env, st)
        new, nd = env.supervise(torch.as_tensor(act))
        U.add_census(total, U.census())
        ctrl = st["kind"] == 1
        assert np.array_equal(new.numpy()[~ctrl], act[~ctrl]) and (nd.numpy()[~ctrl.any(1)] == 0).all()
    assert not [k for k in U.CENSUS_REQUIRED if total[k] < U.CENSUS_MIN]
    assert total["replaced_by_2"] == 0


@pytest.mark.parametrize("mode", (0, 1))
def test_philox_against_numpy(mode, math_mode):
    """uniforms=None draws what include/mm_supervisor.h documents: feeding the twin the values of an outside Philox (numpy,
    policy_act_util, pinned to published known answers) reproduces new_action, n_draws and the whole trace."""
    E, N = 128, 8
    st, act = U.scenes_to_state([s for s in U.placed_scenes(7, 20) if len(s[1]) <= N][:E - 3], N)
    assert act.shape[0] == E
    steps, episode = np.arange(E) % 97, 1 + np.arange(E) % 5
    math_mode(mode)
    env = U.oracle().OracleEnv(E, N, env_id=ENV_ID, obs_f64=True, n_hdv=3, seed=0xC0FFEE12345, first_env=5,
                               config={"safety_guarantee": "priority", "HEADWAY_TIME": 0.5})
    U.put_state(env, st, steps=steps, episode=episode)
    Uh = U.philox_uniforms(env.seeds.numpy().astype(np.uint64), episode, steps, 9 * N)
    assert Uh.min() >= 0 and Uh.max() < 1 and len(np.unique(Uh)) == Uh.size
    out = []
    for uniforms in (None, Uh):
        with U.Trace(E, N, 18) as tr:
            new, nd = env.supervise(torch.as_tensor(act), uniforms=uniforms)
            out.append((new.clone(), nd.clone(), tr.parse()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) 
    assert bool((out[0][1].numpy() > (st["kind"] == 1).sum(1)).any())  # (HDV draws happened, not only the tie-breakers)
    for k in ("order", "key", "len", "live", "points"):
        assert U.same_bits(out[0][2][k], out[1][2][k]).all(), k
    # and a wrong stream is noticed: the keys carry the first draws
    with U.Trace(E, N, 18) as tr:
        env.supervise(torch.as_tensor(act), uniforms=np.roll(Uh, 1, axis=1))
        assert not U.same_bits(tr.parse()["key"], out[0][2]["key"]).all()


def test_refusals_and_contracts():
    """The twin returns the device library's error codes and writes nothing when it refuses; a valid call leaves the state
    unchanged and honours n_draws = NULL and a scratch of exactly mm_supervise_scratch_bytes."""
    E, N = 5, 8
    oe = U.oracle()
    lib = oe.library()
    assert lib.has_supervisor
    assert lib.supervise_scratch_bytes(E, N, 6) == 8 * E * N * (10 + 4 * 18)
    assert lib.supervise_scratch_bytes(E, N, 2, sub_steps=15) == 8 * E * N * (10 + 4 * 30)
    for bad in ((E, N, 0, 3), (E, N, 6, 0), (E, abi.MM_MAX_AGENTS + 1, 6, 3), (0, N, 6, 3)):
        with pytest.raises(ValueError):
            lib.supervise_scratch_bytes(bad[0], bad[1], bad[2], sub_steps=bad[3])
    env = oe.OracleEnv(E, N, env_id=ENV_ID, obs_f64=True, n_hdv=2, seed=3, config={"safety_guarantee": "priority", "HEADWAY_TIME": 1.2})
    env.reset()
    v1 = oe.OracleEnv(E, N, env_id="merge-multi-agent-v1", config={"safety_guarantee": "none"})
    v1.reset()
    need = lib.supervise_scratch_bytes(E, N, 6)
    act = torch.ones(E, N, dtype=torch.int32)
    uni = torch.zeros(E, 9 * N, dtype=torch.float64)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def buffers(misalign=0):
        raw = torch.full((need + 64,), 0xFF, dtype=torch.uint8)
        off = (-raw.data_ptr()) % 8 + 8 + misalign
        return raw, raw[off: off + need], torch.full((E, N), 0x11111111, dtype=torch.int32), torch.full((E,), 0x11111111, dtype=torch.int32)

    def call(h=env, kind=abi.SUP_PRIORITY, n_step=6, a=act, u=None, stride=0, scratch="own", nbytes=need, new="own", nd="own", misalign=0):
        raw, scr, new_, nd_ = buffers(misalign)
        rc = lib.lib.mm_supervise(h._h, kind, n_step, p(a), p(u), stride, p(scr if scratch == "own" else None), nbytes,
                                  p(new_ if new == "own" else None), p(nd_ if nd == "own" else None), None)
        return rc, raw, new_, nd_

    cases = {"v1 handle": dict(h=v1), "unknown kind": dict(kind=7), "n_step 0": dict(n_step=0), "n_step -2": dict(n_step=-2),
             "stride < 9 N": dict(u=uni, stride=9 * N - 1), "scratch one byte short": dict(nbytes=need - 1),
             "scratch misaligned by 4": dict(misalign=4), "NULL actions": dict(a=None), "NULL new_actions": dict(new=None),
             "NULL scratch": dict(scratch=None)}
    for name, kw in cases.items():
        rc, raw, new_, nd_ = call(**kw)
        assert rc == -1, (name, rc)  # MM_ERR_INVALID_ARG
        assert bool((raw == 0xFF).all()) and bool((new_ == 0x11111111).all()) and bool((nd_ == 0x11111111).all()), name
    before = env.state.clone()
    rc, raw, new_, nd_ = call()
    rc2, _, new2, nd2 = call(nd=None)
    assert rc == 0 and rc2 == 0 and torch.equal(env.state, before)
    assert torch.equal(new_, new2) and bool((nd2 == 0x11111111).all()) and bool((nd_ >= 0).all()) and int(nd_.max()) >= 1
    assert bool((raw == 0xFF).all())  # (the twin keeps its lookahead copy in memory of its own)
    rc, _, new3, _ = call(u=uni, stride=9 * N)
    assert rc == 0


def test_oracle_env_steps_through_the_twin():
    """has_supervisor is true for the oracle, so OracleEnv(..., safety_guarantee="priority") steps through the twin; v1 and dmc
    still raise."""
    oe = U.oracle()
    env = oe.OracleEnv(64, 8, env_id=ENV_ID, obs_f64=True, auto_reset=True, seed=2, n_hdv=3,
                       config={"safety_guarantee": "priority", "HEADWAY_TIME": 0.5})
    env.reset()
    g = torch.Generator().manual_seed(1)
    replaced = 0
    for _ in range(12):
        a = torch.multinomial(torch.tensor([0.2, 0.1, 0.1, 0.5, 0.1]), 64 * 8, True, generator=g).view(64, 8).int()
        _, _, _, info = env.step(a)
        replaced += int((info["new_action"] != a).sum())
        assert bool(((info["new_action"] >= 0) & (info["new_action"] <= 4)).all())
    assert replaced > 0
    env.poll_errors()
    for env_id, sg in (("merge-multi-agent-v1", "priority"), (ENV_ID, "dmc")):
        bad = oe.OracleEnv(4, 4, env_id=env_id, config={"safety_guarantee": sg})
        bad.reset()
        with pytest.raises(NotImplementedError):
            bad.step(torch.ones(4, 4, dtype=torch.int32))


def test_profiles_record_the_fuzz_and_the_census():
    """profiles/supervisor_twin: the reference-against-twin fuzz found nothing on at least 20 000 states, and the recorded census
    of the committed GPU-test inputs meets the conditions the GPU test asserts."""
    with open(os.path.join(ROOT, "profiles", "supervisor_twin", "ref_fuzz.json")) as f:
        fz = json.load(f)
    assert fz["states"] >= 20000 and fz["decision_differences"] == 0 and fz["worst_trace_deviation"] <= TOL and not fz["census_missing"]
    with open(os.path.join(ROOT, "profiles", "supervisor_twin", "census.json")) as f:
        cen = json.load(f)
    assert not [k for k in U.CENSUS_REQUIRED if cen["union"][k] < U.CENSUS_MIN]
    assert cen["free_run"]["replaced_actions"] >= U.FREE_RUN_MIN_REPLACED
