"""The default mode (qp_solver = "ipm") AROUND the step, on the GPU: test_hip_parity.py compares the interior-point step's
arithmetic with the oracle on one handle stepped from reset() with every output requested; here the same step -- in both of
its forms, the fused kernel (debug_flags bit2) and the split step (bit3: nsub + 1 phase launches with a sweep launch between
them, handing off through handle-owned planes that no state_dict() carries) -- is resumed from a checkpoint, sharded,
switched on and off on a live handle, folded into the rollout metrics, asked for fewer outputs / caller-owned slots / float32
observations, captured into a hipGraph under DeviceRollout, and given a bad action.  Bit equality against the oracle or
between two runs of the library everywhere; rtol = 1e-12 only for the re-associated metric sums."""
import pytest
import torch

import oracle_env
import default_step_util as U
from marl_mass_amd import VecMergeEnv, _cabi as abi
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout

pytestmark = pytest.mark.gpu

FORM_IDS = sorted(U.FORMS)


@pytest.fixture(autouse=True)
def _portable_math():
    """The oracle evaluates include/mm_math.h (as the kernels do): HIP-vs-oracle must be bit-equal."""
    oracle_env.set_math_mode(1)
    yield
    oracle_env.set_math_mode(0)


def _gpu(E, case, form, **over):
    safety, N, n_hdv = case
    return VecMergeEnv(E, N, device="cuda:0", debug_flags=U.FORMS[form], **U.env_kw(safety, n_hdv, **over))


# ---- 1. checkpoint / resume ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("case,E,trace", [(U.CASES[0], 200, True), (U.CASES[1], 100, False), (U.CASES[2], 100, True), (U.CASES[3], 100, False)],
                         ids=lambda v: U.case_id(v) if isinstance(v, tuple) else str(v))
def test_checkpoint_resume_on_the_hip_backend(case, E, trace, form):
    """A steps 0..T with a state_dict() after step k; a FRESH handle B (urgent = 0, zeroed hand-off planes) loaded with it
    steps k..T on the same actions: every step of B is A's, bit for bit (state, obs, reward, done, the QP planes of the
    trace), and so is a fresh handle of the OTHER form (split resumed from a fused snapshot and the reverse).  A itself is
    the oracle's run.  Episodes end and re-spawn after the snapshot and (trace cases) QPs run to the iteration cap."""
    k, T = 25, 50
    N = case[1]
    acts = U.tape(E, N, T)
    a = _gpu(E, case, form, trace=trace)
    head = U.run(a, acts[:k], trace)
    ck = a.state_dict()
    ref = U.run(a, acts[k:], trace, fresh=False)
    assert U.respawns(head[-1], ref[-1]) > 0, "no episode ended after the snapshot"
    if trace:
        assert sum(U.capped_qps(r) for r in ref) > 0, "no QP ran to the iteration cap after the snapshot"
    for t, (got, want) in enumerate(zip(head + ref, U.oracle_run(case, E, T, 1))):
        U.assert_same(got, want, ("vs oracle", t))
    other = [f for f in FORM_IDS if f != form][0]
    for name, b in (("same form", _gpu(E, case, form, trace=trace)), ("other form", _gpu(E, case, other, trace=trace))):
        b.load_state_dict(ck)
        assert torch.equal(b.state, ck["state"]) and torch.equal(b.obs, ck["obs"])
        for t, (got, want) in enumerate(zip(U.run(b, acts[k:], trace, fresh=False), ref)):
            U.assert_same(got, want, (name, "resumed", k + t))
        b.poll_errors()
    a.poll_errors()


# ---- 2. shards against the whole batch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_shards_equal_the_whole_batch_in_one_process(case, form):
    """Handles first_env = 0 / count 72 and first_env = 72 / count 128 against the whole E = 200: a shard puts an env into
    another lane and another wave (other company for the sweep's gating, speculation and verification queue) -- after every
    step each shard's planes, observations, rewards, dones and QP trace planes are the whole batch's slice; the whole batch
    is the oracle's run; the shards' metrics add up to the whole batch's (sums to rtol 1e-12, counts and the min exactly)."""
    E, T, N = 200, 40, case[1]
    acts = U.tape(E, N, T)
    parts = []
    for first, count in ((0, 72), (72, 128)):
        env = _gpu(count, case, form, first_env=first, trace=True)
        m = env.enable_metrics()
        parts.append((slice(first, first + count), U.run(env, [a[first:first + count].contiguous() for a in acts], True, first_env=first), m, env))
    whole = _gpu(E, case, form, trace=True)
    mw = whole.enable_metrics()
    ref = U.run(whole, acts, True)
    assert U.respawns(ref[0], ref[-1]) > 0 and sum(U.capped_qps(r) for r in ref) > 0
    for sl, recs, _, _ in parts:
        for t, got in enumerate(recs):
            U.assert_same(got, ref[t], ("shard", sl.start, t), sl)
    for t, (got, want) in enumerate(zip(ref, U.oracle_run(case, E, T, 1))):
        U.assert_same(got, want, ("whole vs oracle", t))
    for _, _, _, env in parts:
        env.poll_errors()
    whole.poll_errors()
    total = parts[0][2].cpu().clone()
    total[:7] += parts[1][2].cpu()[:7]
    total[7] = min(float(total[7]), float(parts[1][2][7]))
    U.assert_metrics(total, mw, "shards vs whole")
    assert float(mw[4]) == E * T and float(mw[6]) > 0


# ---- 3. configure(qp_solver=...) on a live handle -----------------------------------------------------------------------
@pytest.mark.parametrize("plan", sorted(U.SWITCH_PLANS))
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_mode_switches_on_a_live_handle(case, plan):
    """debug_flags bit3, so "ipm" is the split step at this size.  exact -> ipm: the hand-off planes are allocated by the
    switch, not by mm_create; ipm -> exact -> ipm: the planes of the first ipm leg are kept and are STALE when the second
    one starts.  The oracle twin gets the same configure calls at the same steps: every step equal, bit for bit; and a third
    handle built "ipm" and loaded with the state at the last switch (fresh planes) continues exactly as the live one."""
    E, N = 100, case[1]
    legs = U.SWITCH_PLANS[plan]
    T = sum(n for _, n in legs)
    acts = U.tape(E, N, T)
    live = _gpu(E, case, "split", qp_solver=legs[0][0], trace=True)
    recs, snaps = U.switch_run(live, legs, acts, True)
    twin = oracle_env.OracleEnv(E, N, trace=True, **U.env_kw(case[0], case[2], qp_solver=legs[0][0]))
    want, _ = U.switch_run(twin, legs, acts, True)
    for t, (g, w) in enumerate(zip(recs, want)):
        U.assert_same(g, w, (plan, "vs oracle twin", t))
    n_last = legs[-1][1]
    assert sum(U.capped_qps(r) for r in recs[T - n_last:]) > 0, "no QP ran to the iteration cap after the last switch"
    assert sum(r["_commits_b"] for r in recs[T - n_last:]) > 0, "no candidate-B commit after the last switch"
    fresh = _gpu(E, case, "split", trace=True)
    fresh.load_state_dict(snaps[-1])
    for i, got in enumerate(U.run(fresh, acts[T - n_last:], True, fresh=False)):
        U.assert_same(got, recs[T - n_last + i], (plan, "fresh planes vs the live handle's", T - n_last + i))
    live.poll_errors(); twin.poll_errors(); fresh.poll_errors()


# ---- 4. rollout metrics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("case", [U.CASES[0], U.CASES[3]], ids=U.case_id)
def test_metrics_in_the_default_mode(case, form):
    """The metrics block behind the interior-point step (split form: only the last phase launch reaches it; 6-lane
    layout: the partial buffer is sized for the power-of-two layout and indexed by the running layout's waves), per-step
    fold and deferred, against the HOST: the per-step outputs accumulated in float64 with math.fsum.  Counts and the min
    exactly, sums to rtol 1e-12.  Deferred: nothing visible before a flush, a second flush adds nothing, a state_dict()
    contains the pending sums.  111 steps: every episode reaches T = 100 and re-spawns."""
    E, N, T = 100, case[1], 111
    acts = U.tape(E, N, T, seed=9)
    per_step, deferred = _gpu(E, case, form), _gpu(E, case, form)
    mp, md = per_step.enable_metrics(), deferred.enable_metrics(deferred=True)
    per_step.reset(); deferred.reset()
    keys = ("reward", "done", "crashed", "average_speed", "traffic_speed", "merge_percent", "min_headway")
    outs = []
    for t, a in enumerate(acts):
        a = a.cuda()
        info = per_step.step(a)[3]
        deferred.step(a)
        outs.append({k: info[k].cpu().clone() for k in keys})
        if t in (50, T - 2):
            torch.cuda.synchronize()
            U.assert_metrics(mp, U.host_metric_sums(outs), ("per-step fold", t))
        if t == 50:
            assert float(md[4]) == 0.0 and float(md[7]) == float("inf") and not bool(md[:7].any()), "deferred sums visible before a flush"
            deferred.flush_metrics(); deferred.flush_metrics()  # (the second flush has nothing left to add)
            torch.cuda.synchronize()
            U.assert_metrics(md, U.host_metric_sums(outs), ("deferred, flushed twice", t))
        if t == T - 2:
            # a snapshot taken in deferred mode contains the pending sums
            U.assert_metrics(deferred.state_dict()["metrics"], U.host_metric_sums(outs), ("deferred, state_dict", t))
    want = U.host_metric_sums(outs)
    assert float(want[6]) >= E and float(want[4]) == E * T, "every episode must have finished once"
    per_step.poll_errors(); deferred.poll_errors()  # (the poll flushes, then synchronises)
    U.assert_metrics(mp, want, "per-step fold, end")
    U.assert_metrics(md, want, "deferred, end")


# ---- 5. outputs ---------------------------------------------------------------------------------------------------------
def _same_info(a, b, where):
    for k in b:
        assert torch.equal(a[k].nan_to_num(), b[k].nan_to_num()), (where, k)


@pytest.mark.parametrize("form", FORM_IDS)
def test_skipped_outputs_in_the_default_mode(form):
    """skip_outputs: NULL MMStepOut pointers through every phase launch; state and every remaining output are the full call's."""
    E, T, case = 200, 30, U.CASES[0]
    full, lean = _gpu(E, case, form), _gpu(E, case, form, skip_outputs=("agents_info", "action_mask", "crashed"))
    U.start(full); U.start(lean)
    for t, a in enumerate(U.tape(E, case[1], T)):
        of, rf, df, inf_ = full.step(a.cuda())
        ol, rl, dl, inl = lean.step(a.cuda())
        assert torch.equal(full.state, lean.state) and torch.equal(of, ol) and torch.equal(rf, rl) and torch.equal(df, dl), t
        assert set(inf_) - set(inl) == {"agents_info", "action_mask", "crashed"}
        _same_info(inf_, inl, t)
    U.assert_same(U.record(lean), U.oracle_run(case, E, T, 1)[-1], "lean vs oracle")
    full.poll_errors(); lean.poll_errors()


@pytest.mark.parametrize("form", FORM_IDS)
def test_caller_slots_in_the_default_mode(form):
    """step(obs_out=..., out={...}): every output of the step lands in the caller's tensors with the bits a twin writes into
    its own buffers, the env-owned buffers are left alone -- and are written again by a step that passes neither argument."""
    E, T, case = 200, 30, U.CASES[0]
    own, slots = _gpu(E, case, form), _gpu(E, case, form)
    U.start(own); U.start(slots)
    acts = U.tape(E, case[1], T)
    for t, a in enumerate(acts[:-1]):
        obs_out = torch.full_like(slots.obs, -9.0)
        out = {k: torch.full_like(v, 7) for k, v in slots.out.items()}
        kept_obs, kept = slots.obs.clone(), {k: v.clone() for k, v in slots.out.items()}
        oa, ra, da, ia = own.step(a.cuda())
        ob, rb, db, ib = slots.step(a.cuda(), obs_out=obs_out, out=out)
        assert ob.data_ptr() == obs_out.data_ptr() and all(ib[k].data_ptr() == out[k].data_ptr() for k in out)
        assert torch.equal(ob, oa) and torch.equal(own.state, slots.state), t
        _same_info(ib, ia, t)
        assert torch.equal(slots.obs, kept_obs), "the env's own observation buffer was written although a slot was given"
        for k in kept:
            assert torch.equal(slots.out[k].nan_to_num(), kept[k].nan_to_num()), ("env-owned buffer written although a slot was given", k)
    oa, _, _, ia = own.step(acts[-1].cuda())
    ob, _, _, ib = slots.step(acts[-1].cuda())
    assert ob.data_ptr() == slots.obs.data_ptr() and all(ib[k].data_ptr() == slots.out[k].data_ptr() for k in ib)
    assert torch.equal(ob, oa)
    _same_info(ib, ia, "after the slots")
    U.assert_same(U.record(slots), U.oracle_run(case, E, T, 1)[-1], "slots vs oracle")
    own.poll_errors(); slots.poll_errors()


@pytest.mark.parametrize("form", FORM_IDS)
def test_float32_observations_in_the_default_mode(form):
    """obs_f64 = False: the observation is the float64 run's, rounded once; nothing else changes."""
    E, T, case = 200, 30, U.CASES[0]
    e32, e64 = _gpu(E, case, form, obs_f64=False), _gpu(E, case, form)
    U.start(e32); U.start(e64)
    assert e32.obs.dtype == torch.float32 and torch.equal(e32.obs, e64.obs.float())
    for t, a in enumerate(U.tape(E, case[1], T)):
        o32, r32, d32, i32 = e32.step(a.cuda())
        o64, r64, d64, i64 = e64.step(a.cuda())
        assert o32.dtype == torch.float32 and torch.equal(o32, o64.float()), t
        assert torch.equal(e32.state, e64.state) and torch.equal(r32, r64) and torch.equal(d32, d64), t
        _same_info(i32, i64, t)
    e32.poll_errors(); e64.poll_errors()


# ---- 6. DeviceRollout, eager and hipGraph -------------------------------------------------------------------------------
def test_device_rollout_graph_equals_eager_in_the_default_mode():
    """The split step (2 nsub + 1 launches per env step) under DeviceRollout with the fused Philox policy launch: the
    hipGraph replay gives the eager loop's tensors over two compared rollouts and the same final state; the eager run's
    recorded actions, replayed from reset() on the oracle, end in the same state bits; a DeviceRollout.state_dict() taken
    between rollouts and loaded into a FRESH graph-mode rollout reproduces the eager stream.  26 steps per rollout: the 100th
    step of every episode (done, re-spawn) falls into the fourth rollout, the second of the compared ones."""
    E, T, case = 256, 26, U.CASES[0]
    kw = U.env_kw(case[0], obs_f64=False, debug_flags=U.FORMS["split"])  # (the fused policy launch reads float32 observations)
    torch.manual_seed(3)
    actor, critic = ActorNetwork(30, 128, 5).cuda(), CriticNetwork(30, 5, 128).cuda()
    make = lambda **k: DeviceRollout(VecMergeEnv(E, case[1], device="cuda:0", **kw), actor, critic, roll_out_n_steps=T, sample_seed=4, **k)  # noqa: E731
    eager, graph, resumed = make(), make(use_graph=True), make(use_graph=True)
    assert eager.fused_policy and eager.obs.dtype == torch.float32 and eager.env.qp_solver == "ipm"
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    actions = [eager.interact()["actions"].clone(), eager.interact()["actions"].clone()]
    ck = eager.state_dict()
    keys = ("states", "actions", "returns", "dones")
    dones, last = 0, None
    for i in range(2):
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for k in keys + ("average_speed", "min_headway"):
            assert torch.equal(a[k], b[k]), (i, k)
        actions.append(a["actions"].clone())
        dones += int(a["dones"].sum())
        last = {k: a[k].clone() for k in keys}
    assert dones > 0, "no episode ended inside the compared rollouts"
    assert len(torch.unique(torch.cat(actions))) == 5
    assert torch.equal(eager.env.state, graph.env.state)
    # a fresh graph-mode rollout: its first interact() is two rollouts of the stream (warm-up outside capture, then the
    # replay whose tensors it returns) -- the second one after the snapshot, i.e. the eager run's last
    resumed.load_state_dict(ck)
    c = resumed.interact()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(c[k], last[k]), ("resumed", k)
    assert torch.equal(resumed.env.state, eager.env.state)
    twin = oracle_env.OracleEnv(E, case[1], **U.env_kw(case[0], obs_f64=False))
    twin.reset()
    for a in torch.cat(actions).cpu():
        twin.step(a.contiguous())
    assert int(twin.env_i32[abi.EP["EPISODE"]].min()) >= 2, "the replayed stream must contain the re-spawn"
    assert torch.equal(eager.env.state.cpu(), twin.state), "the recorded actions end in another state on the oracle"
    for ro in (eager, graph, resumed):
        ro.env.poll_errors()
    twin.poll_errors()


# ---- 7. bad action latch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_IDS)
def test_bad_action_latch_in_the_default_mode(form):
    """Action 7 in one slot for one step: poll_errors raises ValueError once (split form: latched by the first phase
    launch only, rewritten to IDLE in every one), the step acted as IDLE (a twin given 1 in that slot has the same state),
    and the next step and poll are clean."""
    E, case = 64, U.CASES[0]
    bad, twin = _gpu(E, case, form), _gpu(E, case, form)
    acts = U.tape(E, case[1], 16)
    for env in (bad, twin):
        U.run(env, acts[:14])
        env.poll_errors()
    a_bad, a_idle = acts[14].clone(), acts[14].clone()
    a_bad[37, 5], a_idle[37, 5] = 7, 1
    rb, rt = bad.step(a_bad.cuda()), twin.step(a_idle.cuda())
    with pytest.raises(ValueError):
        bad.poll_errors()
    bad.poll_errors()  # raised once: the latch was cleared by the poll that reported it
    twin.poll_errors()
    assert torch.equal(bad.state, twin.state) and torch.equal(rb[0], rt[0]) and torch.equal(rb[1], rt[1])
    rb, rt = bad.step(acts[15].cuda()), twin.step(acts[15].cuda())
    bad.poll_errors(); twin.poll_errors()
    assert torch.equal(bad.state, twin.state) and torch.equal(rb[0], rt[0])
