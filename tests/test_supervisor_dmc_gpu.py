"""The "dmc" safety supervisor on the MI355X against the reference's dmc_* tapes: every recorded state teacher-forced with
the recorded uniforms in both forms (new_action, n_draws, the per-stage trace, then the env step), free runs, the two
forms against each other on states no tape holds, a ragged batch, the Philox path (shards, resume, graph capture), tile and
buffer edges with canaries, the MergeEnvCompat adapter on the global numpy stream, and the priority supervisor after the
helper move."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import dmc_util as D
from marl_mass_amd import _cabi as abi

pytestmark = pytest.mark.gpu
FASTER = [0.05, 0.1, 0.05, 0.75, 0.05]


def _ids(p):
    return os.path.basename(p)[:-4]


def _acts(z, rows, m):
    act = np.ones((len(rows), m), dtype=np.int32)
    act[:, :z["actions"].shape[1]] = z["actions"][rows]
    return torch.as_tensor(act)


@pytest.mark.parametrize("path", D.tapes(), ids=_ids)
def test_dmc_tape_teacher_forced(path):
    """One env per recorded state, one launch per form: new_action, n_draws and the trace integers exactly, the trace floats
    within TOL; then the step's obs / rewards / dones as the reference's."""
    z, meta = D.load(path)
    T, n = z["actions"].shape
    m = z["sub_f"].shape[1]
    env = D.tape_env(T, m, meta)
    D.force(env, z["sub_f"], z["sub_i"], z["step"], np.full(T, meta["n_merge"]))
    act, U = _acts(z, np.arange(T), m), np.nan_to_num(z["uniforms"])
    outs = []
    for literal in (True, False):
        new, nd = env.supervise(act, uniforms=U, literal=literal, trace=True)
        got = new.cpu().numpy()[:, :n]
        bad = np.nonzero((got != z["new_actions"]).any(axis=1))[0]
        what = "literal" if literal else "default"
        tr = env.dmc_trace.cpu().numpy()
        D.assert_trace(tr, z["trace"], what)  # (first: a failing stage says more than a failing action)
        assert len(bad) == 0, "%s, states %s: device %s, reference %s" % (what, bad.tolist(), got[bad].tolist(), z["new_actions"][bad].tolist())
        assert np.array_equal(nd.cpu().numpy(), z["n_draws"])
        outs.append((new.clone(), nd.clone(), env.dmc_trace.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and D.same_bits(outs[0][2], outs[1][2])
    obs, rew, done, info = env.step(act, uniforms=U)
    assert np.array_equal(info["new_action"].cpu().numpy()[:, :n], z["new_actions"])
    assert np.array_equal(done.cpu().numpy(), z["dones"])
    assert np.abs(obs.cpu().numpy()[:, :n] - z["obs"]).max() <= D.TOL
    assert np.abs(rew.cpu().numpy() - z["rewards"]).max() <= D.TOL
    assert np.array_equal(info["action_mask"].cpu().numpy()[:, :n], z["action_mask"])


@pytest.mark.parametrize("path", D.natural_tapes(), ids=_ids)
def test_dmc_tape_free_run(path):
    """From the tape's first state, stepping on its own with the recorded actions and uniforms through the first episode
    (up to a dropped knife-edge state, if it has one): the same supervised actions and the same terminal step."""
    z, meta = D.load(path)
    n, m = z["actions"].shape[1], z["sub_f"].shape[1]
    steps = z["step"]
    assert steps[0] == 0
    env = D.tape_env(1, m, meta)
    D.force(env, z["sub_f"][:1], z["sub_i"][:1], [0], [meta["n_merge"]])
    t = 0
    while t < len(steps) and steps[t] == t:
        _, _, done, info = env.step(_acts(z, [t], m), uniforms=np.nan_to_num(z["uniforms"][t:t + 1]))
        assert np.array_equal(info["new_action"].cpu().numpy()[0, :n], z["new_actions"][t]), t
        assert bool(done[0]) == bool(z["dones"][t]), t
        t += 1
    assert t >= 5


def _reset_with_absent_slot(E, n_hdv, seed):
    """A device-reset batch of 11 vehicles per env in 12 slots: the last slot absent (kind 0, every plane zero)."""
    src = D.make_env(E, 11, 0.5, n_hdv=n_hdv, seed=seed)
    src.reset()
    env = D.make_env(E, 12, 0.5, n_hdv=n_hdv, seed=seed)  # (a new env's state buffer is all zero)
    env.f64[:, :, :11] = src.f64
    env.u8[:, :, :11] = src.u8
    env.env_i32.copy_(src.env_i32)
    env.seeds.copy_(src.seeds)
    return env


@pytest.mark.parametrize("N", [8, 12])
def test_forms_agree_bit_for_bit_on_fresh_states(N):
    E = 2048
    if N == 8:
        env = D.make_env(E, 8, 0.5, n_hdv=4, seed=11)
        env.reset()
    else:
        env = _reset_with_absent_slot(E, 5, 12)
    g = torch.Generator().manual_seed(5)
    replaced = 0
    # 12 compared steps saw 65 replacements from a fresh reset (vehicles spawn apart): the FASTER bias runs 12 supervised
    # steps longer first, then the 12 steps are compared (measured: 2 189 replacements at N = 8, 4 298 at N = 12)
    for t in range(24):
        a = torch.multinomial(torch.tensor(FASTER), E * N, True, generator=g).view(E, N).int().cuda()
        if t < 12:
            env.step(a)
            continue
        new, nd = env.supervise(a, literal=True, trace=True)
        lit = (new.clone(), nd.clone(), env.dmc_trace.clone())
        new, nd = env.supervise(a, trace=True)
        assert torch.equal(new, lit[0]), t
        assert torch.equal(nd, lit[1]), t
        assert D.same_bits(env.dmc_trace, lit[2]), t
        kind = env.u8[abi.B["KIND"]]
        assert torch.equal(nd, ((kind == 1).sum(1) + 2 * (kind == 2).sum(1)).int())
        assert torch.equal(new[kind != 1], a[kind != 1])  # absent and uncontrolled slots are copied through
        replaced += int((new != a).sum())
        env.step(a)
    env.poll_errors()
    assert replaced >= 500, replaced


def test_ragged_batch_density3():
    """Every recorded state of every default-horizon tape in ONE launch of N = 11 slots, tiled to E = 4096, one launch per
    HEADWAY_TIME: each row equals the reference's answer in both forms."""
    rows = []
    for p in D.tapes():
        z, meta = D.load(p)
        if (meta["n_step"], meta["simulation_frequency"]) == (6, 15):
            rows += [(z, meta, t) for t in range(z["actions"].shape[0])]
    N, E = 11, 4096
    sf = np.zeros((E, N, 11))
    si = np.zeros((E, N, 9), dtype=np.int64)
    act = np.ones((E, N), dtype=np.int32)
    U = np.zeros((E, 2 * N))
    for e in range(E):
        z, meta, t = rows[e % len(rows)]
        m, n = z["sub_f"].shape[1], meta["n"]
        sf[e, :m], si[e, :m], act[e, :n] = z["sub_f"][t], z["sub_i"][t], z["actions"][t]
        U[e, :z["uniforms"].shape[1]] = np.nan_to_num(z["uniforms"][t])
    out = {}
    for h in (0.5, 1.2):
        env = D.make_env(E, N, h, n_hdv=1)
        D.force(env, sf, si, np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64))
        for literal in (False, True):
            out[h, literal] = [x.cpu().numpy().copy() for x in env.supervise(torch.as_tensor(act), uniforms=U, literal=literal)]
    for e in range(E):
        z, meta, t = rows[e % len(rows)]
        for literal in (False, True):
            new, nd = out[meta["headway_time"], literal]
            assert np.array_equal(new[e, :meta["n"]], z["new_actions"][t]), (e, t, literal)
            assert int(nd[e]) == int(z["n_draws"][t])


def test_philox_path_sharding_and_resume():
    E, N = 512, 8
    kw = dict(n_hdv=3, seed=7)
    full = D.make_env(E, N, 0.5, **kw)
    full.reset()
    g = torch.Generator().manual_seed(3)
    acts = [torch.multinomial(torch.tensor(FASTER), E * N, True, generator=g).view(E, N).int() for _ in range(6)]
    halves = []
    for first, cnt in ((0, E // 2), (E // 2, E - E // 2)):
        h = D.make_env(cnt, N, 0.5, first_env=first, **kw)
        h.reset()
        halves.append(h)
    snap, news = None, []
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
    assert sum(int((n.cpu() != a).sum()) for n, a in zip(news, acts)) > 0, "no action was ever replaced"
    res = D.make_env(E, N, 0.5, **kw)
    res.load_state_dict(snap)
    for t in range(3, 6):
        _, _, _, info = res.step(acts[t].cuda())
        assert torch.equal(info["new_action"], news[t])
    assert torch.equal(res.state, full.state)
    full.poll_errors()


def test_graph_captured_rollout_with_dmc_equals_eager():
    from marl_mass_amd import VecMergeEnv
    from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout
    E, N, T = 1024, 8, 10
    kw = dict(env_id="merge-multi-agent-v0", config={"safety_guarantee": "dmc", "HEADWAY_TIME": 0.5}, seed=9,
              auto_reset=True, n_hdv=3, enable_dmc=True)
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


CANARY = 0x5A


def _guarded(nbytes, align=256):
    """nbytes of device memory between two canary zones: (whole buffer, the guarded slice)."""
    pad = 1024
    buf = torch.full((nbytes + 2 * pad + align,), CANARY, dtype=torch.uint8, device="cuda")
    off = pad + (-(buf.data_ptr() + pad)) % align
    return buf, buf[off:off + nbytes], off


def _intact(buf, off, nbytes):
    return bool((buf[:off] == CANARY).all()) and bool((buf[off + nbytes:] == CANARY).all())


@pytest.mark.parametrize("E", [1, 63, 64, 65])
def test_tile_and_buffer_edges(E):
    """Batches around the 64-lane tile with canaries before and after every buffer the entry writes; the guarded call
    equals the env's own; every refused call leaves everything untouched."""
    N = 8
    env = D.make_env(E, N, 0.5, n_hdv=4, seed=21)
    env.reset()
    g = torch.Generator().manual_seed(E)
    a = torch.multinomial(torch.tensor(FASTER), E * N, True, generator=g).view(E, N).int().cuda()
    for _ in range(4):  # a few steps in, so that lookaheads crash
        env.step(a)
    lib, clib = env.clib.lib, env.clib
    need = clib.supervise_dmc_scratch_bytes(E, N, env.n_step)
    sizes = dict(scr=need, new=4 * E * N, nd=4 * E, tr=8 * E * N * D.TRACE)
    for literal in (False, True):
        want_new, want_nd = [x.clone() for x in env.supervise(a, literal=literal, trace=True)]
        want_tr = env.dmc_trace.clone()
        G = {k: _guarded(v) for k, v in sizes.items()}

        def call(flags=abi.DMC_LITERAL if literal else 0, n_step=env.n_step, actions=a, scratch=None, scratch_bytes=need, new=True,
                 uniforms=None, stride=0):
            sp = G["scr"][1].data_ptr() if scratch is None else scratch
            return lib.mm_supervise_dmc(env._h, n_step, flags, C.c_void_p(actions.data_ptr()) if actions is not None else None,
                                        uniforms, stride, C.c_void_p(sp), scratch_bytes,
                                        C.c_void_p(G["new"][1].data_ptr()) if new else None, C.c_void_p(G["nd"][1].data_ptr()),
                                        C.c_void_p(G["tr"][1].data_ptr()), None)
        u = torch.zeros(E, 2 * N, dtype=torch.float64, device="cuda")
        refused = [call(flags=2), call(flags=abi.DMC_LITERAL | 4), call(n_step=0), call(actions=None), call(new=False),
                   call(scratch_bytes=need - 8), call(scratch=G["scr"][1].data_ptr() + 4),
                   call(uniforms=C.c_void_p(u.data_ptr()), stride=2 * N - 1), call(n_step=43)]
        torch.cuda.synchronize()
        assert refused == [abi.MM_ERR_INVALID_ARG] * len(refused)
        for k in G:  # nothing was written, inside or outside
            assert bool((G[k][0] == CANARY).all()), k
        assert call() == 0
        torch.cuda.synchronize()
        for k, v in sizes.items():
            assert _intact(G[k][0], G[k][2], v), k
        assert torch.equal(G["new"][1].view(torch.int32).view(E, N), want_new)
        assert torch.equal(G["nd"][1].view(torch.int32), want_nd)
        assert D.same_bits(G["tr"][1].view(torch.float64).view(E, N, D.TRACE), want_tr)
    # a v1 handle is refused too
    from marl_mass_amd import VecMergeEnv
    v1 = VecMergeEnv(E, N, env_id="merge-multi-agent-v1", config={"safety_guarantee": "none"})
    v1.reset()
    G = {k: _guarded(v) for k, v in sizes.items()}
    rc = lib.mm_supervise_dmc(v1._h, 6, 0, C.c_void_p(a.data_ptr()), None, 0, C.c_void_p(G["scr"][1].data_ptr()), need,
                              C.c_void_p(G["new"][1].data_ptr()), C.c_void_p(G["nd"][1].data_ptr()), C.c_void_p(G["tr"][1].data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == abi.MM_ERR_INVALID_ARG and all(bool((G[k][0] == CANARY).all()) for k in G)


def test_compat_reproduces_the_reference_stream():
    """MergeEnvCompat(enable_dmc=True), mixed traffic, seeded like dmc_compat_*: the policy's np.random.choice and the
    supervisor share the global stream; new_action and rewards follow the reference's at every kept step."""
    from marl_mass_amd.compat import MergeEnvCompat
    z, meta = D.load(D.tapes("dmc_compat_")[0])
    n, h = meta["n"], meta["n_hdv"]
    env = MergeEnvCompat("merge-multi-agent-v0", {"safety_guarantee": "dmc", "HEADWAY_TIME": meta["headway_time"],
                                                  "action_masking": True, "mixed_traffic": True, "n_step": 6}, enable_dmc=True)
    env._num_vehicles = lambda num_CAV=0: (n, h)  # the tape fixes the counts, as tools/gen_golden.make_env does
    env.seed = meta["seed"]
    env.reset()
    row = {int(s): k for k, s in enumerate(z["step"])}
    for t in range(int(z["step"].max()) + 1):
        a = tuple(int(x) for x in np.random.choice(5, n, p=meta["p"]))
        _, r, d, info = env.step(a)
        if t in row:
            k = row[t]
            assert a == tuple(z["actions"][k]), t
            assert info["new_action"] == tuple(int(x) for x in z["new_actions"][k]), t
            assert abs(r - z["rewards"][k]) <= D.TOL and d == bool(z["dones"][k]), t


def test_priority_answers_did_not_move():
    """mm_supervise after its helpers moved to mm_supervisor_dev.h: one prio tape, teacher-forced."""
    from test_supervisor_gpu import _env, _force, _load
    path = sorted(glob.glob(os.path.join(D.GOLDEN, "prio_v0_6c5h_*.npz")))[0]
    z, meta = _load(path)
    T, n = z["actions"].shape
    m = z["sub_f"].shape[1]
    env = _env(T, m, meta["headway_time"], n_hdv=meta["n_hdv"])
    _force(env, z["sub_f"], z["sub_i"], np.arange(T), np.full(T, meta["n_merge"]))
    act = np.ones((T, m), dtype=np.int32)
    act[:, :n] = z["actions"]
    new, nd = env.supervise(torch.as_tensor(act), uniforms=np.nan_to_num(z["uniforms"]))
    assert np.array_equal(new.cpu().numpy()[:, :n], z["new_actions"])
    assert np.array_equal(nd.cpu().numpy(), z["n_draws"])
    with pytest.raises(ValueError):
        env.supervise(torch.as_tensor(act), literal=True)
