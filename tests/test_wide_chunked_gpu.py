"""mm_policy_wide_train_chunked (include/mm_policy_wide_train.h) and PPOLearner's scratch budget at hidden 512 on the MI355X.

What the design promises is asserted as stated (tests/test_train_chunked_gpu.py's plan at the other hidden size): with
chunk >= n the chunked entry IS the unchunked one, bit for bit; for any chunk the losses and the per-sample diagnostics are the
unchunked entry's bits (same tiles, same count, same loss tree) and every gradient is within the project's rule against float64
autograd, 4 e32 + 1e-6 max|g64| with e32 the float32 torch error on the same tensor on the device -- a different slicing of the
sample sum is one more float32 summation order, which is what that rule covers.  The batches, the networks, the knife-edge
filter, the float64 references and the comparison are tests/test_policy_wide_train_gpu.py's (policy_wide_train_util); the
6 208-sample batches' input conditions are asserted on the host in tests/test_wide_chunked_host.py."""
import copy
import ctypes as C

import pytest
import torch

import policy_wide_train_util as U
import test_policy_wide_train_gpu as wt_t
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import PPOLearner, _mlp_struct
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout
from policy_train_util import GRAD_NAMES, sums_of
from test_train_chunked_gpu import shared_refusals

pytestmark = pytest.mark.gpu

LR, RMS_EPS = 1e-4, 1e-8
NAN = float("nan")
FORMS = ("reference", "flat")


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _opt(t):
    return None if t is None else t.data_ptr()


class Case(object):
    """One hidden-512 learner and one batch: the unchunked call (through the learner), the chunked call (straight through the
    binding: the test chooses chunk and scratch) and the two torch sides."""

    def __init__(self, learner, obs, act, ret, old, adv, valid, critic_loss, clip=0.2):
        self.learner, self.critic_loss, self.clip = learner, critic_loss, clip
        self.obs, self.act, self.ret, self.old, self.adv, self.valid = obs, act, ret, old, adv, valid

    # -- construction
    @staticmethod
    def synthetic(n, n_s=30, n_a=5, critic_loss="mse", strided=True, with_valid=True):
        """The unchunked module's batch of n samples (its seeds: batch_seed(n, n_s), 11 + n_a at the ends of the action range)."""
        seed = U.batch_seed(n, n_s) if n_a == 5 or n_s != 30 else 11 + n_a
        learner = wt_t._learner(*wt_t._nets(n_s, n_a=n_a), critic_loss=critic_loss)
        obs, act, ret, old, adv, valid = wt_t._batch(learner, n, n_s, "spread", strided, with_valid, seed=seed, n_a=n_a)
        return Case(learner, obs, act, ret, old, adv, valid, critic_loss)

    def prefix(self, m):
        """The first m samples (the strides stay): every per-sample property of the batch holds for a prefix."""
        cut = lambda t: None if t is None else t[:m]  # noqa: E731
        return Case(self.learner, self.obs[:m], self.act[:m], self.ret[:m], cut(self.old).contiguous(), cut(self.adv),
                    None if self.valid is None else self.valid[:m].contiguous(), self.critic_loss, self.clip)

    def masked(self, valid):
        """The same samples under another mask (the advantages are zero in masked slots)."""
        adv = self.learner.advantages(self.obs, self.act, self.ret, valid)
        return Case(self.learner, self.obs, self.act, self.ret, self.old, adv, valid, self.critic_loss, self.clip)

    # -- pieces
    @property
    def n(self):
        return self.obs.shape[0]

    def nets(self):
        return [self.learner.actor, self.learner.critic]

    def grads(self):
        return wt_t._grads_of(*self.nets())

    def fill_grads(self, value):
        for net in self.nets():
            for p in net.parameters():
                p.grad.fill_(value)

    def sums(self, form):
        """The float32 (S+, S-) that goes to the kernel and, as a constant, to both torch runs; None for the per-sample form."""
        return sums_of(self.adv) if form == "reference" else None

    def chunked_bytes(self, chunk):
        return self.learner.clib.policy_wide_train_chunked_scratch_bytes(self.n, chunk)

    # -- the calls: [loss] + the twelve gradients + (logp_taken, value, ratio)
    def unchunked(self, form, networks="both"):
        self.fill_grads(NAN)
        kw = dict(valid=self.valid, adv_sums=self.sums(form), diagnostics=True, networks=networks)
        if form != "reference":
            kw["advantages"] = self.adv
        loss, diag = self.learner.loss_and_grad(self.obs, self.act, self.ret, self.old, **kw)
        return [loss.clone()] + self.grads() + list(diag)

    def chunked_rc(self, form, chunk, scratch=None, scratch_ptr=None, scratch_bytes=None, sums=None, hidden=512, networks="both",
                   loss=None, null_inputs=False, clip=None, critic_loss=None, both_adv=False, stray=None):
        """(status, [loss] + gradients + diagnostics) of the chunked entry; the gradients are read whatever the status.
        scratch: a uint8 tensor (default: one of the queried size); scratch_ptr / scratch_bytes override what is passed.
        clip .. stray: the arguments of test_train_chunked_gpu.shared_refusals (critic_loss: the raw code)."""
        clip = self.clip if clip is None else clip
        code = abi.PT_CRITIC_LOSS[self.critic_loss] if critic_loss is None else critic_loss
        L, clib, n, S = self.learner, self.learner.clib, self.n, self.obs.shape[1]
        sums = self.sums(form) if sums is None else sums
        loss = torch.full((2,), NAN, device="cuda") if loss is None else loss
        with_a, with_c = networks != "critic", networks != "actor"
        diag = [torch.full((n,), NAN, device="cuda") if on or stray == i else None for i, on in enumerate((with_a, with_c, with_a))]
        if scratch is None and scratch_ptr is None:
            scratch = torch.empty(self.chunked_bytes(chunk), dtype=torch.uint8, device="cuda")
        ptr = scratch.data_ptr() if scratch_ptr is None else (scratch_ptr or None)
        nbytes = scratch.numel() if scratch_bytes is None else scratch_bytes
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        obs, act, ret = self.obs, self.act, self.ret
        if null_inputs:
            head = (None, S, n, S, None, 1, None, 1, None, None)
        else:
            head = (obs.data_ptr(), obs.stride(0) if n else S, n, S, act.data_ptr(), act.stride(0) if n else 1, ret.data_ptr(),
                    ret.stride(0) if n else 1, self.old.data_ptr(), _opt(self.valid))
        ref = lambda on, st: C.byref(st) if on else None  # noqa: E731
        W = [_mlp_struct(L.actor), _mlp_struct(L.critic)]
        G = [_mlp_struct(L.actor, True), _mlp_struct(L.critic, True)]
        adv = None if ((sums is not None and not both_adv) or null_inputs) else self.adv
        rc = clib.lib.mm_policy_wide_train_chunked(
            *head, ref(with_a, W[0]), ref(with_c, W[1]), hidden, L.n_a, clip, code,
            _opt(sums) if with_a else None, _opt(adv) if with_a else None, ref(with_a, G[0]), ref(with_c, G[1]), loss.data_ptr(),
            _opt(diag[0]), _opt(diag[1]), _opt(diag[2]), ptr, nbytes, stream, chunk)
        return rc, [loss] + self.grads() + diag

    def chunked(self, form, chunk, **kw):
        self.fill_grads(NAN)
        rc, out = self.chunked_rc(form, chunk, **kw)
        assert rc == abi.MM_OK
        return out

    def torch_sides(self, form, sums):
        """(float32, float64) torch.autograd on the device: (losses, the twelve gradients) each."""
        return wt_t._torch_sides(self.learner, self.obs, self.act, self.ret, self.old, self.adv, self.valid, form, sums,
                                 self.critic_loss, self.clip)

    def compare(self, case, out, f32, f64):
        """The rule of the unchunked module on [loss] + gradients: prints every figure, then asserts."""
        return wt_t._compare("wide_chunked_%s" % case, (out[0], out[1:13]), f32, f64)


def _bit_equal(xs, ys, what):
    assert len(xs) == len(ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert (x is None) == (y is None), (what, i)
        if x is not None:
            assert torch.equal(x, y), (what, i, float((x.double() - y.double()).abs().max()))


def _rest(out):
    """The losses and the diagnostics of [loss] + gradients + diagnostics."""
    return out[:1] + out[13:]


_BASE = {}


def _base(n, **kw):
    """One batch per configuration, shared by the tests that read it; nothing writes into it."""
    key = (n,) + tuple(sorted(kw.items()))
    if key not in _BASE:
        _BASE[key] = Case.synthetic(n, **kw)
    return _BASE[key]


# ---- identity: chunk >= n is the unchunked entry
@pytest.mark.parametrize("n,chunk", [(31, 64), (31, 1024), (1000, 1024)])
def test_one_pass_is_the_unchunked_entry(n, chunk):
    case = _base(n)
    for form in FORMS:
        want = case.unchunked(form)
        got = case.chunked(form, chunk)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        _bit_equal(got, want, (form, "losses, gradients and diagnostics"))


# ---- several passes
# (n, chunk, the configuration).  n = 129 is the first 129 samples of the n = 1000 batch.  n_a = 8: the critic's fc2 rows (520
# floats) take 16-byte loads in place; n_a = 5 and 1 (517, 513): the copy at pitch 512 that prep wrote.  6208 = 194 tiles at
# chunk 3136 = 98 tiles: a full pass of 33 slices of 3 tiles, then a last pass of 3072 samples that cuts 48 slices of 2.
MULTI = [
    (1000, 64, dict(form="reference", critic_loss="mse", strided=True, with_valid=True)),    # 16 passes, the last one 40 samples
    (1000, 192, dict(form="flat", critic_loss="huber", strided=True, with_valid=True, n_a=8)),
    (1000, 960, dict(form="reference", critic_loss="huber", strided=True, with_valid=True, n_a=1)),
    (129, 64, dict(form="flat", critic_loss="mse", strided=True, with_valid=True)),          # the last pass holds one sample
    (6208, 3136, dict(form="reference", critic_loss="huber", strided=True, with_valid=True)),
    (6208, 3136, dict(form="flat", critic_loss="mse", strided=False, with_valid=False)),
    (6208, 3136, dict(form="flat", critic_loss="huber", strided=True, with_valid=True, n_s=25, n_a=8)),
]


@pytest.mark.parametrize("n,chunk,cfg", MULTI, ids=["%d_%d_%s_a%d" % (n, c, k["form"], k.get("n_a", 5)) for n, c, k in MULTI])
def test_passes_sum_to_the_whole_batch(n, chunk, cfg):
    cfg = dict(cfg)
    form = cfg.pop("form")
    case = _base(1000, **cfg).prefix(n) if n == 129 else _base(n, **cfg)
    assert (n + chunk - 1) // chunk > 1
    if n == 6208:
        last = n % chunk
        assert (U.slicing(chunk)[2], U.slicing(last)[2]) == (33, 48) and last == 3072
    want = case.unchunked(form)
    got = case.chunked(form, chunk)
    _bit_equal(_rest(got), _rest(want), "losses and diagnostics")
    f32, f64 = case.torch_sides(form, case.sums(form))
    case.compare("n%d_c%d_%s_a%d" % (n, chunk, form, case.learner.n_a), got, f32, f64)


# ---- masks
def test_a_pass_without_a_valid_sample():
    base = _base(1000)
    valid = base.valid.clone()
    valid[64:128] = 0  # the whole second pass at chunk 64
    case = base.masked(valid)
    for form in FORMS:
        got = case.chunked(form, 64)
        _bit_equal(_rest(got), _rest(case.unchunked(form)), "losses and diagnostics")
        f32, f64 = case.torch_sides(form, case.sums(form))
        case.compare("masked_pass_%s" % form, got, f32, f64)


def test_nothing_valid_and_nothing_at_all():
    base = _base(1000)
    none = base.masked(torch.zeros(1000, dtype=torch.uint8, device="cuda"))
    for form in FORMS:
        for t in none.chunked(form, 192):
            assert float(t.abs().max()) == 0.0
    empty = base.prefix(0)
    empty.valid = None
    tiny = torch.empty(16, dtype=torch.uint8, device="cuda")
    for form in FORMS:  # n == 0: the inputs, adv_sums / advantages and the scratch are not looked at
        out = empty.chunked(form, 64, scratch=tiny, null_inputs=True)
        for t in out[:13]:
            assert float(t.abs().max()) == 0.0
        out = empty.chunked(form, 64, scratch_ptr=0, scratch_bytes=0, null_inputs=True)
        for t in out[:13]:
            assert float(t.abs().max()) == 0.0


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_one_network_alone(which):
    """Either network may be left out: over several passes the other's gradient, loss and diagnostics are the joint chunked
    call's bits (and the unchunked single-network call's loss and diagnostics); the omitted network's .grad is not touched."""
    case = _base(1000)
    mine = slice(1, 7) if which == "actor" else slice(7, 13)
    other = slice(7, 13) if which == "actor" else slice(1, 7)
    i = 0 if which == "actor" else 1
    for form in FORMS:
        joint = case.chunked(form, 192)
        alone = case.chunked(form, 192, networks=which)
        _bit_equal(alone[mine], joint[mine], (form, which, "gradients"))
        assert all(bool(torch.isnan(g).all()) for g in alone[other])
        assert float(alone[0][1 - i]) == 0.0 and float(alone[0][i]) == float(joint[0][i]) != 0.0
        want = case.unchunked(form, networks=which)
        _bit_equal(_rest(alone), _rest(want), (form, which, "losses and diagnostics"))
        _bit_equal(case.chunked(form, 1024, networks=which)[mine], want[mine], (form, which, "one pass"))


# ---- the scratch is written before it is read; two calls give the same bits
def test_scratch_contents_do_not_matter():
    """NaN-filled (every byte 0xFF: NaN as float and as double) against zero-filled scratch, and the same scratch twice.  The
    actor's kernel B never writes the one-hot tile of dW2 (columns 512..543 of the partial block's rows): the accumulate kernel
    sums what the scratch held there, NaN in the first run, and no result depends on it."""
    case = _base(1000)
    scratch = torch.empty(case.chunked_bytes(192), dtype=torch.uint8, device="cuda")
    for form in FORMS:
        runs = []
        for fill in (0xFF, 0x00, None):
            if fill is not None:
                scratch.fill_(fill)
            runs.append(case.chunked(form, 192, scratch=scratch))
        assert all(bool(torch.isfinite(t).all()) for t in runs[0])
        _bit_equal(runs[0], runs[1], "NaN-filled against zero-filled")
        _bit_equal(runs[1], runs[2], "the second call on the same scratch")


# ---- graph capture
def test_graph_capturable():
    case = _base(1000)
    chunk = 192  # 6 passes, the last one 40 samples
    sums = case.sums("reference")
    scratch = torch.empty(case.chunked_bytes(chunk), dtype=torch.uint8, device="cuda")
    eager = [t.clone() for t in case.chunked("reference", chunk, scratch=scratch, sums=sums)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        case.chunked("reference", chunk, scratch=scratch, sums=sums)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc, captured = case.chunked_rc("reference", chunk, scratch=scratch, sums=sums)
    assert rc == abi.MM_OK
    for _ in range(2):
        case.fill_grads(NAN)
        scratch.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        _bit_equal([captured[0]] + case.grads() + captured[13:], eager, "replay against the eager call")


# ---- refusals enqueue nothing
CANARY = 7.25


def test_refusals_between_canaries():
    """Every refusal the chunk adds to mm_policy_wide_train's, and hidden 128: MM_ERR_INVALID_ARG, and the losses, the
    gradients and the scratch -- between canary bytes inside its own allocation -- are as they were."""
    case = _base(1000)
    need = case.chunked_bytes(64)
    pad = 64
    arena = torch.full((pad + need + pad,), 0x5A, dtype=torch.uint8, device="cuda")  # canaries | scratch | canaries
    base = arena.data_ptr() + pad
    base += (-base) % 16
    assert base + need <= arena.data_ptr() + arena.numel()
    guarded = torch.full((pad + 2 + pad,), CANARY, device="cuda")  # canaries | loss [2] | canaries
    loss = guarded[pad:pad + 2]
    sums = case.sums("reference")

    def untouched():
        torch.cuda.synchronize()
        return (bool((guarded == CANARY).all()) and bool((arena == 0x5A).all())
                and all(bool((g == CANARY).all()) for g in case.grads()))

    refused = [dict(chunk=0), dict(chunk=32), dict(chunk=100), dict(chunk=-64), dict(chunk=64, scratch_bytes=need - 1),
               dict(chunk=64, scratch_ptr=base + 4), dict(chunk=64, scratch_ptr=base + 8), dict(chunk=64, scratch_ptr=0),
               dict(chunk=64, hidden=128), dict(chunk=128)]  # (chunk 128: the scratch of chunk 64 is too small for it)
    for kw in refused:
        kw = dict(kw)
        case.fill_grads(CANARY)
        rc, _ = case.chunked_rc("reference", kw.pop("chunk"), scratch_ptr=kw.pop("scratch_ptr", base),
                                scratch_bytes=kw.pop("scratch_bytes", need), sums=sums, loss=loss, **kw)
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert untouched(), kw
    for kw in shared_refusals(True, (64, 128)):  # what the small helpers shared with the hidden-128 entries refuse
        case.fill_grads(CANARY)
        rc, out = case.chunked_rc("reference", 64, scratch_ptr=base, scratch_bytes=need, sums=sums, loss=loss, **kw)
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert untouched(), kw
        assert all(bool(torch.isnan(d).all()) for d in out[13:] if d is not None), kw  # the diagnostics were not written either
    with pytest.raises(ValueError):  # the hidden-128 chunked entry refuses this size
        lib = case.learner.clib
        W, G = [_mlp_struct(n) for n in case.nets()], [_mlp_struct(n, True) for n in case.nets()]
        lib.check(lib.lib.mm_policy_train_chunked(
            case.obs.data_ptr(), case.obs.stride(0), case.n, 30, case.act.data_ptr(), case.act.stride(0), case.ret.data_ptr(),
            case.ret.stride(0), case.old.data_ptr(), None, C.byref(W[0]), C.byref(W[1]), 512, 5, 0.2, 0, sums.data_ptr(), None,
            C.byref(G[0]), C.byref(G[1]), loss.data_ptr(), None, None, None, base, need,
            C.c_void_p(torch.cuda.current_stream().cuda_stream), 64))
    assert untouched()
    q = case.learner.clib.policy_wide_train_chunked_scratch_bytes
    for chunk in (0, 32, 100, -64):
        with pytest.raises(ValueError):
            q(1000, chunk)
    # the well-formed call goes through, stays inside its scratch and gives the bits of the call on a scratch of its own
    case.fill_grads(CANARY)
    rc, out = case.chunked_rc("reference", 64, scratch_ptr=base, scratch_bytes=need, sums=sums, loss=loss)
    torch.cuda.synchronize()
    assert rc == abi.MM_OK
    lo = base - arena.data_ptr()
    assert bool((arena[:lo] == 0x5A).all()) and bool((arena[lo + need:] == 0x5A).all())
    assert bool((guarded[:pad] == CANARY).all()) and bool((guarded[pad + 2:] == CANARY).all())
    mine = [loss.clone()] + out[1:]
    _bit_equal(mine, case.chunked("reference", 64, sums=sums), "inside the arena against a scratch of its own")


# ---- the learner under a budget
def _rollout_like(B, N, S, n_a, seed):
    g = torch.Generator().manual_seed(seed)
    states = (torch.randn(B, N, S, generator=g) * 1.5).cuda()
    actions = torch.randint(0, n_a, (B, N), generator=g, dtype=torch.int32).cuda()
    returns = (torch.randn(B, N, generator=g) * 1.5 + 0.3).cuda()
    return states, actions, returns


def _named(learner):
    named = {"actor." + k: v for k, v in learner.actor.named_parameters()}
    named.update({"critic." + k: v for k, v in learner.critic.named_parameters()})
    return named


@pytest.mark.parametrize("fused", [False, True], ids=["torch_tail", "fused_tail"])
def test_learner_under_a_budget(fused):
    """B = 200 samples per agent step under the budget of the wide query at (B, 64) -- room for 64-sample passes only, less than
    the unchunked scratch of B -- against a twin without a budget: three train(form="reference") calls, one agent's column
    each, then three train(form="flat") calls on the same columns.  RMSprop moves an element whose gradient is rounding noise
    around zero by up to (lr / eps) dg, so per tensor the bound is (lr / eps) 4 e32 + 1e-7 with e32 the float32 torch error on
    that tensor at the twin's pre-step parameters (max over the steps so far): tests/test_train_chunked_gpu.py's."""
    B, N, S, n_a = 200, 3, 30, 5
    clib = _lib()
    states, actions, returns = _rollout_like(B, N, S, n_a, seed=21)
    actor, critic = wt_t._nets(S)
    budget = clib.policy_wide_train_chunked_scratch_bytes(B, 64)
    assert budget < clib.policy_wide_train_chunked_scratch_bytes(B, 128) and budget < clib.policy_wide_train_scratch_bytes(B)
    twin = wt_t._learner(copy.deepcopy(actor), copy.deepcopy(critic), fused_step=fused)
    small = wt_t._learner(actor, critic, fused_step=fused, scratch_budget_bytes=budget)
    assert small.hidden == 512 and small.scratch_budget_bytes == budget
    e32 = dict.fromkeys(GRAD_NAMES, 0.0)

    def measure(obs, act, ret, form):
        """e32 of the step the twin is about to take."""
        old, value = twin.evaluate(obs, act, actor=twin.actor_target, critic=twin.critic_target)
        adv = ret - value
        sums = sums_of(adv) if form == "reference" else None
        f32, f64 = Case(twin, obs, act, ret, old, adv, None, "mse").torch_sides(form, sums)
        for k, x, y in zip(GRAD_NAMES, f32[1], f64[1]):
            e32[k] = max(e32[k], float((x.double() - y).abs().max()))

    def check(step):
        a, b = _named(small), _named(twin)
        for k in GRAD_NAMES:
            diff = float((a[k].detach() - b[k].detach()).abs().max())
            bound = (LR / RMS_EPS) * 4.0 * e32[k] + 1e-7
            print("%s %-10s %-22s diff %.3e bound %.3e" % ("fused" if fused else "torch", step, k, diff, bound))
            assert diff <= bound, (step, k, diff, bound)
        assert small._scratch.numel() <= budget and small._chunks[B] == (64, budget)

    start = {k: v.detach().clone() for k, v in _named(small).items()}
    for form in FORMS:
        for a in range(N):
            obs, act, ret = states[:, a, :], actions[:, a], returns[:, a]
            measure(obs if form == "reference" else obs.contiguous(), act, ret, form)
            for learner in (twin, small):  # one agent step = train() on that agent's column alone
                learner.train(states[:, a:a + 1], actions[:, a:a + 1], returns[:, a:a + 1], form=form)
            check("%s%d" % (form, a))
    assert all(not torch.equal(v.detach(), start[k]) for k, v in _named(small).items())
    assert all(bool(torch.isfinite(v).all()) for v in _named(small).values())
    assert small._scratch.numel() <= budget < twin._scratch.numel()


def test_rollout_to_train_under_a_budget():
    """DeviceRollout.interact() on the steer_vel env, 16 envs x 4 agents x 16 steps, into PPOLearner.train() under the budget
    of the wide query at (256, 64): the unchunked scratch of 256 samples does not fit and neither do passes of 128, so every
    agent step runs four passes of 64.  The losses are finite and the parameters move."""
    from marl_mass_amd import VecMergeEnv
    E, N, T = 16, 4, 16
    torch.manual_seed(3)
    env = VecMergeEnv(E, N, env_id="merge-multi-agent-v1", seed=9, auto_reset=True,
                      config={"safety_guarantee": "cbf-av", "HEADWAY_TIME": 0.5, "lateral_control": "steer_vel"})
    actor, critic = ActorNetwork(env.n_s, 512, 5).cuda(), CriticNetwork(env.n_s, 5, 512).cuda()
    start = [p.detach().clone() for p in list(actor.parameters()) + list(critic.parameters())]
    ro = DeviceRollout(env, actor, critic, roll_out_n_steps=T, sample_seed=4)
    clib = env.clib
    budget = clib.policy_wide_train_chunked_scratch_bytes(E * T, 64)
    assert budget < clib.policy_wide_train_scratch_bytes(E * T) and budget < clib.policy_wide_train_chunked_scratch_bytes(E * T, 128)
    learner = PPOLearner(actor, critic, clib, scratch_budget_bytes=budget)
    out = ro.interact()
    assert out["states"].reshape(-1, N, env.n_s).shape[0] == E * T
    losses = learner.train(out)
    torch.cuda.synchronize()
    env.poll_errors()
    assert len(losses) == N and all(bool(torch.isfinite(x).all()) for x in losses)
    assert learner._chunks == {E * T: (64, budget)} and learner._scratch.numel() == budget
    now = list(actor.parameters()) + list(critic.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in now) and all(not torch.equal(p.detach(), q) for p, q in zip(now, start))
