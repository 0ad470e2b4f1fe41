"""The "priority" supervisor kernel (mm_supervisor.hip) against its CPU twin (oracle/mm_oracle.c mm_supervise) on the MI355X:
bit for bit in math mode 1, at volume and at the edges no recorded tape reaches.  The twin itself is pinned to the reference
on the build machine (test_supervisor_twin_host.py, tools/supervisor_ref_fuzz.py).  Compared are new_action, n_draws, the
whole state after the step, and the kernel's lookahead copy (read back from its scratch buffer) against the twin's trace.

The tests must not pass by never reaching the hard branches: test_census_conditions asserts, from the TWIN's census of the
very inputs used here (counted on the CPU, never by the kernel), that every entry of supervisor_twin_util.CENSUS_REQUIRED
occurred at least 20 times over the free-run and placed inputs, and that the free runs replaced at least 500 actions.

Limits of the handle, asserted in test_handle_limits: mm_create refuses N > 12 (the road has 6 + 6 spawn points, the
reference cannot hold more vehicles) and simulation_frequency // policy_frequency > 3, in both libraries.  No handle exists on
which the supervisor could run N = 16 or 15 sub-steps per policy step, so the grids below stop at N = 12 and run the
30-point horizon -- the scratch size of (n_step 2, 15 sub-steps) -- as (n_step 10, 3 sub-steps).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import supervisor_twin_util as U
from marl_mass_amd import _cabi as abi

pytestmark = pytest.mark.gpu
ENV_ID = "merge-multi-agent-v0"
E_FREE, T_FREE = 1024, 25
WEIGHTS = [0.2, 0.1, 0.1, 0.5, 0.1]  # skewed to FASTER and LANE_LEFT: lookaheads crash
# lock-step free runs: N, HEADWAY_TIME, fixed HDV count or a per-episode count draw (traffic density, mixed traffic)
FREE_RUNS = {
    "N4_cav_ht05": dict(N=4, ht=0.5, n_hdv=0),
    "N4_mixed_ht12": dict(N=4, ht=1.2, n_hdv=2),
    "N6_d1_mixed_ht05": dict(N=6, ht=0.5, density=1, mixed=True),
    "N8_cav_ht12": dict(N=8, ht=1.2, n_hdv=0),
    "N8_d2_mixed_ht05": dict(N=8, ht=0.5, density=2, mixed=True),
    "N12_d3_cav_ht05": dict(N=12, ht=0.5, density=3, mixed=False),
    "N12_d3_mixed_ht12": dict(N=12, ht=1.2, density=3, mixed=True),
}
# placed-state grid: (n_step, simulation_frequency // policy_frequency), one launch per horizon and N
HORIZONS = ((1, 3), (6, 3), (8, 3), (6, 1), (10, 3))
PLACED_SEED = 20261019
_CENSUS = {}  # name of the input -> the twin's census of it


def _make(backend, E, N, ht, n_step=6, sub_steps=3, **kw):
    cfg = {"safety_guarantee": "priority", "HEADWAY_TIME": ht, "action_masking": True, "n_step": n_step,
           "simulation_frequency": 5 * sub_steps, "policy_frequency": 5}
    if "density" in kw:
        mixed = kw.pop("mixed")
        cfg.update({"traffic_density": kw.pop("density"), "mixed_traffic": mixed, "traffic_type": "mixed" if mixed else "cav"})
        kw["draw_counts"] = True
    if backend == "hip":
        from marl_mass_amd import VecMergeEnv
        return VecMergeEnv(E, N, env_id=ENV_ID, config=cfg, obs_f64=True, **kw)
    return U.oracle().OracleEnv(E, N, env_id=ENV_ID, config=cfg, obs_f64=True, **kw)


def _free_actions(name, N):
    g = torch.Generator().manual_seed(1000 + sorted(FREE_RUNS).index(name))
    return [torch.multinomial(torch.tensor(WEIGHTS), E_FREE * N, True, generator=g).view(E_FREE, N).int() for _ in range(T_FREE)]


def _free_run(name, dev_env=None):
    """The twin's free run `name`; with dev_env the device env is stepped alongside and compared after every step."""
    kw = dict(FREE_RUNS[name])
    N, ht = kw.pop("N"), kw.pop("ht")
    U.oracle().set_math_mode(1)
    try:
        tw = _make("oracle", E_FREE, N, ht, seed=31, auto_reset=True, **kw)
        tw.reset()
        if dev_env is not None:
            dev_env.reset()
            assert torch.equal(dev_env.f64.cpu().nan_to_num(), tw.f64.nan_to_num()) and torch.equal(dev_env.u8.cpu(), tw.u8), "the two resets differ"
        cen, checked = {}, 0
        with U.Trace(E_FREE, N, 18) as tr:
            for t, a in enumerate(_free_actions(name, N)):
                _, _, _, ti = tw.step(a)
                U.add_census(cen, U.census())
                if dev_env is None:
                    continue
                _, _, _, di = dev_env.step(a.to(dev_env.device))
                # (the scratch is read after the step: nothing but the supervisor writes it)
                assert torch.equal(di["new_action"].cpu(), ti["new_action"]), (name, t)
                assert torch.equal(dev_env.n_draws.cpu(), tw.n_draws), (name, t)
                assert torch.equal(dev_env.f64.cpu().nan_to_num(), tw.f64.nan_to_num()), (name, t)
                assert torch.equal(dev_env.u8.cpu(), tw.u8) and torch.equal(dev_env.env_i32.cpu(), tw.env_i32), (name, t)
                checked += U.assert_copy_equal(tr.parse(), U.scratch_copy(dev_env._sup_scratch, E_FREE, N, 18), "%s step %d" % (name, t))
        _CENSUS["free:" + name] = cen
        return cen, checked
    finally:
        U.oracle().set_math_mode(0)


def _placed(N):
    st, act = U.scenes_to_state(U.placed_scenes(PLACED_SEED), N)
    return st, act


def _supervise_pair(tw, dev, st, act, n_points, uniforms=None, what="", **put):
    """One supervise() call on the twin and (if given) the device env from the same forced state; returns the twin's results."""
    U.put_state(tw, st, **put)
    E, N = act.shape
    with U.Trace(E, N, n_points) as tr:
        tn, td = [x.clone() for x in tw.supervise(torch.as_tensor(act), uniforms=uniforms)]
        trace = tr.parse()
    cen = U.census()
    if dev is not None:
        U.put_state(dev, st, **put)
        before = dev.state.clone()
        dn, dd = dev.supervise(torch.as_tensor(act), uniforms=uniforms)
        assert torch.equal(dn.cpu(), tn), what + ": new_action differs in envs %s" % (torch.nonzero((dn.cpu() != tn).any(1)).flatten()[:8].tolist(),)
        assert torch.equal(dd.cpu(), td), what + ": n_draws"
        U.assert_copy_equal(trace, U.scratch_copy(dev._sup_scratch, E, N, n_points), what)
        assert torch.equal(dev.state, before), what + ": the state buffer changed"
    return tn, td, trace, cen


def _tape_batch(N):
    """Every recorded step of the sup_placed_* tapes of one horizon as rows of N slots: {(n_step, sub_steps, ht): (state, actions,
    uniforms, expected new_action, expected n_draws, n)}."""
    groups = {}
    for p in U.tapes("sup_placed_"):
        z, meta = U.load_tape(p)
        key = (meta["n_step"], meta["simulation_frequency"] // 5, meta["headway_time"])
        groups.setdefault(key, []).append((z, meta))
    out = {}
    for key, items in groups.items():
        sts, acts, us, news, nds, ns = [], [], [], [], [], []
        for z, meta in items:
            T, n = z["actions"].shape
            sts.append(U.pad_state(U.tape_state(z), N))
            a = np.ones((T, N), dtype=np.int32)
            a[:, :n] = z["actions"]
            u = np.zeros((T, 9 * N))
            u[:, :z["uniforms"].shape[1]] = np.nan_to_num(z["uniforms"])
            acts.append(a), us.append(u), nds.append(z["n_draws"])
            news += [z["new_actions"][t] for t in range(T)]
        out[key] = (U.cat_states(sts), np.concatenate(acts), np.concatenate(us), news, np.concatenate(nds))
    return out


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FREE_RUNS))
def test_lock_step_free_run(name):
    """E = 1024 envs, auto-reset, 25 steps on Philox draws and seeded skewed actions, the device env and the twin side by side:
    after every step new_action, n_draws, the whole state and the lookahead copy are equal."""
    kw = dict(FREE_RUNS[name])
    dev = _make("hip", E_FREE, kw.pop("N"), kw.pop("ht"), seed=31, auto_reset=True, **kw)
    cen, checked = _free_run(name, dev)
    dev.poll_errors()
    assert checked > 10 * E_FREE and cen["replaced_actions"] > 0


@pytest.mark.parametrize("N", (11, 12))
def test_placed_grid(N):
    """The placed rare-branch states (regenerated from a seed, ragged rows, rows with no controlled vehicle, action codes outside
    0..4) under every horizon, one launch each; then the sup_placed_* tapes of the reference in the same launches' shapes."""
    st, act = _placed(N)
    E = act.shape[0]
    U.oracle().set_math_mode(1)
    try:
        for k, (n_step, sub) in enumerate(HORIZONS):
            ht = (0.5, 1.2)[k % 2]
            tw, dev = _make("oracle", E, N, ht, n_step, sub, n_hdv=1, seed=5), _make("hip", E, N, ht, n_step, sub, n_hdv=1, seed=5)
            tn, td, _, cen = _supervise_pair(tw, dev, st, act, n_step * sub, what="placed N=%d horizon %s" % (N, (n_step, sub)))
            _CENSUS["placed:N%d:%d:%d" % (N, n_step, sub)] = cen
            # rows with no controlled vehicle and slots that are absent or not controlled pass through; so do foreign codes
            ctrl = torch.as_tensor(st["kind"] == 1)
            assert torch.equal(tn[~ctrl], torch.as_tensor(act)[~ctrl]) and (td[~ctrl.any(1)] == 0).all()
            foreign = torch.as_tensor((act < 0) | (act > 4)) & ctrl
            assert foreign.any() and ((tn == torch.as_tensor(act)) | ((tn >= 0) & (tn <= 4)))[foreign].all()
        for (n_step, sub, ht), (tst, tact, tu, news, nds) in _tape_batch(N).items():
            tw, dev = _make("oracle", len(tact), N, ht, n_step, sub, n_hdv=1), _make("hip", len(tact), N, ht, n_step, sub, n_hdv=1)
            tn, td, _, _ = _supervise_pair(tw, dev, tst, tact, n_step * sub, uniforms=tu, what="tapes %s" % ((n_step, sub, ht),))
            for e, new in enumerate(news):  # and both equal the reference's answer
                assert np.array_equal(tn[e, :len(new)].numpy(), new), e
            assert np.array_equal(td.numpy(), nds)
    finally:
        U.oracle().set_math_mode(0)


def _guarded(n_bytes, dtype, fill, misalign=0):
    """A device buffer of n_bytes between two 256-byte canaries; returns (whole buffer, the view between the canaries)."""
    raw = torch.full((512 + n_bytes + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    body = raw[256 + misalign: 256 + misalign + n_bytes]
    body.view(torch.uint8).fill_(fill)
    return raw, body.view(dtype)


def _canaries_intact(raw, n_bytes, misalign=0):
    return bool((raw[:256 + misalign] == 0xA5).all()) and bool((raw[256 + misalign + n_bytes:] == 0xA5).all())


def _direct(env, act, scratch, scratch_bytes, new, nd, kind=abi.SUP_PRIORITY, n_step=6, uniforms=None, stride=0):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    return env.clib.lib.mm_supervise(env._h, kind, n_step, p(act), p(uniforms), stride, p(scratch), scratch_bytes, p(new), p(nd), env._stream())


def test_tile_and_buffer_edges():
    """mm_supervise called directly with caller-owned buffers: E around the 64-lane block, the scratch exactly
    mm_supervise_scratch_bytes long, scratch and both outputs between canaries, one run without n_draws.  Row e of every launch
    equals row e of the twin (and so of every other launch that contains it); canaries intact, state unchanged."""
    N, n_points = 8, 18
    scenes = U.placed_scenes(PLACED_SEED + 1, 26)
    st_all, act_all = U.scenes_to_state([s for s in scenes if len(s[1]) <= N], N)
    assert act_all.shape[0] >= 257
    U.oracle().set_math_mode(1)
    try:
        tw = _make("oracle", 257, N, 1.2, n_hdv=1, seed=9)
        tn, td, trace, _ = _supervise_pair(tw, None, {k: v[:257] for k, v in st_all.items()}, act_all[:257], n_points)
    finally:
        U.oracle().set_math_mode(0)
    for E, with_nd in ((1, True), (63, True), (64, False), (65, True), (257, True)):
        env = _make("hip", E, N, 1.2, n_hdv=1, seed=9)
        U.put_state(env, {k: v[:E] for k, v in st_all.items()})
        before = env.state.clone()
        need = env.clib.supervise_scratch_bytes(E, N, 6, 3)
        assert need == 8 * E * N * (10 + 4 * n_points)
        sraw, scr = _guarded(need, torch.float64, 0xFF)
        nraw, new = _guarded(4 * E * N, torch.int32, 0x11)
        draw, nd = _guarded(4 * E, torch.int32, 0x11)
        act = torch.as_tensor(act_all[:E]).cuda().contiguous()
        assert _direct(env, act, scr, need, new, nd if with_nd else None) == 0  # MM_OK
        torch.cuda.synchronize()
        assert _canaries_intact(sraw, need) and _canaries_intact(nraw, 4 * E * N) and _canaries_intact(draw, 4 * E), E
        assert torch.equal(env.state, before), E
        assert torch.equal(new.view(E, N).cpu(), tn[:E]), E
        if with_nd:
            assert torch.equal(nd.cpu(), td[:E]), E
        else:
            assert bool((nd == 0x11111111).all()), "n_draws = NULL was written"
        sub = {k: v[:E] for k, v in trace.items()}
        U.assert_copy_equal(sub, U.scratch_copy(scr, E, N, n_points), "E=%d" % E)


def test_philox_against_numpy():
    """uniforms=None draws what include/mm_supervisor.h documents: the same call fed the values of an outside Philox (numpy,
    policy_act_util) reproduces new_action, n_draws and the lookahead copy -- on the device and on the twin."""
    E, N = 256, 8
    st, act = U.scenes_to_state([s for s in U.placed_scenes(PLACED_SEED + 2, 30) if len(s[1]) <= N][:E - 3], N)
    assert act.shape[0] == E
    steps, episode = np.arange(E) % 97, 1 + np.arange(E) % 5
    U.oracle().set_math_mode(1)
    try:
        tw, dev = _make("oracle", E, N, 0.5, n_hdv=3, seed=0xC0FFEE12345), _make("hip", E, N, 0.5, n_hdv=3, seed=0xC0FFEE12345)
        seeds = tw.seeds.numpy().astype(np.uint64)
        assert np.array_equal(seeds, dev.seeds.cpu().numpy().astype(np.uint64))
        Uh = U.philox_uniforms(seeds, episode, steps, 9 * N)
        a = _supervise_pair(tw, dev, st, act, 18, what="philox", steps=steps, episode=episode)
        b = _supervise_pair(tw, dev, st, act, 18, uniforms=Uh, what="numpy philox", steps=steps, episode=episode)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) 
        assert bool((a[1].numpy() > (st["kind"] == 1).sum(1)).any())  # (HDV draws happened, not only the tie-breakers)
        for k in ("len", "live", "points", "key"):
            assert U.same_bits(a[2][k], b[2][k]).all(), k
    finally:
        U.oracle().set_math_mode(0)


def test_refusals():
    """Every documented refusal returns MM_ERR_INVALID_ARG and writes nothing: outputs and scratch sit between canaries."""
    from marl_mass_amd import VecMergeEnv
    E, N = 65, 8
    env = _make("hip", E, N, 1.2, n_hdv=1)
    env.reset()
    v1 = VecMergeEnv(E, N, env_id="merge-multi-agent-v1", config={"safety_guarantee": "none"})
    v1.reset()
    need = env.clib.supervise_scratch_bytes(E, N, 6, 3)
    act = torch.ones(E, N, dtype=torch.int32, device="cuda")
    uni = torch.zeros(E, 9 * N, dtype=torch.float64, device="cuda")
    cases = {
        "v1 handle": dict(env=v1), "unknown kind": dict(kind=7), "n_step 0": dict(n_step=0), "n_step -1": dict(n_step=-1),
        "stride < 9 N": dict(uniforms=uni, stride=9 * N - 1), "scratch one byte short": dict(scratch_bytes=need - 1),
        "scratch misaligned by 4": dict(misalign=4), "NULL actions": dict(act=None), "NULL new_actions": dict(new=None),
        "NULL scratch": dict(scratch=None),
    }
    for name, c in cases.items():
        mis = c.get("misalign", 0)
        sraw, scr = _guarded(need, torch.uint8, 0xFF, misalign=mis)
        nraw, new = _guarded(4 * E * N, torch.int32, 0x11)
        draw, nd = _guarded(4 * E, torch.int32, 0x11)
        rc = _direct(c.get("env", env), c.get("act", act), c.get("scratch", scr), c.get("scratch_bytes", need), c.get("new", new), nd,
                     kind=c.get("kind", abi.SUP_PRIORITY), n_step=c.get("n_step", 6), uniforms=c.get("uniforms"), stride=c.get("stride", 0))
        torch.cuda.synchronize()
        assert rc == -1, (name, rc)  # MM_ERR_INVALID_ARG
        assert bool((new == 0x11111111).all()) and bool((nd == 0x11111111).all()) and bool((scr == 0xFF).all()), name
        assert _canaries_intact(sraw, need, mis) and _canaries_intact(nraw, 4 * E * N) and _canaries_intact(draw, 4 * E), name


def test_handle_limits():
    """Why the grids stop at N = 12 and 3 sub-steps: no handle can be created beyond (see the module docstring).  If either
    limit is lifted, the grids above must grow with it."""
    for backend in ("hip", "oracle"):
        with pytest.raises(ValueError):
            _make(backend, 4, 16, 1.2, n_hdv=0)
        with pytest.raises(ValueError):
            _make(backend, 4, 8, 1.2, n_step=2, sub_steps=15, n_hdv=0)


def test_census_conditions():
    """The condition on the inputs (not a measurement of the kernel): the twin's census of the free-run and placed inputs of this
    module.  Inputs whose test did not run in this session are counted here by the twin alone."""
    for name in sorted(FREE_RUNS):
        if "free:" + name not in _CENSUS:
            _free_run(name)
    U.oracle().set_math_mode(1)
    try:
        for N in (11, 12):
            st, act = _placed(N)
            for k, (n_step, sub) in enumerate(HORIZONS):
                key = "placed:N%d:%d:%d" % (N, n_step, sub)
                if key not in _CENSUS:
                    tw = _make("oracle", act.shape[0], N, (0.5, 1.2)[k % 2], n_step, sub, n_hdv=1, seed=5)
                    _CENSUS[key] = _supervise_pair(tw, None, st, act, n_step * sub)[3]
    finally:
        U.oracle().set_math_mode(0)
    total, free = {}, {}
    for key, c in _CENSUS.items():
        U.add_census(total, c)
        if key.startswith("free:"):
            U.add_census(free, c)
    missing = {k: total.get(k, 0) for k in U.CENSUS_REQUIRED if total.get(k, 0) < U.CENSUS_MIN}
    assert not missing, "census entries below %d: %s" % (U.CENSUS_MIN, missing)
    assert free["replaced_actions"] >= U.FREE_RUN_MIN_REPLACED, free["replaced_actions"]
    assert total["replaced_by_2"] == 0  # (unreachable: see supervisor_twin_util.CENSUS_REQUIRED)
