"""mm_policy_gi_train_chunked / mm_policy_train_chunked (include/mm_policy_gi_train.h, include/mm_policy_train.h) and the
learners' scratch budget on the MI355X.

What the design promises is asserted as stated: with chunk >= n the chunked entry IS the unchunked one, bit for bit; for any
chunk the losses and the per-sample diagnostics are the unchunked entry's bits (same tiles, same count, same loss tree) and
every gradient is within the project's rule against float64 autograd, 4 e32 + 1e-6 max|g64| with e32 the float32 torch error
on the same tensor -- a different slicing of the sample sum is one more float32 summation order, which is what that rule
covers.  The batches, the networks, the float64 references and the comparison are those of the two unchunked test modules
(the synthetic batches with their knife-edge filter live there, the objectives in gi_train_util / policy_train_util)."""
import copy
import ctypes as C

import pytest
import torch

import gi_train_util
import policy_train_util
import test_policy_gi_train_gpu as gi_t
import test_policy_train_gpu as pt_t
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import PPOLearner, SharedPPOLearner, _mlp_struct, _params

pytestmark = pytest.mark.gpu

ENTRIES = ("gi", "pt")  # the shared actor-critic's entry, the separate actor's and critic's
LR, RMS_EPS = 1e-4, 1e-8
NAN = float("nan")


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _opt(t):
    return None if t is None else t.data_ptr()


class Case(object):
    """One learner and one batch, for either entry: the unchunked call (through the learner), the chunked call (straight
    through the binding: the test chooses chunk and scratch) and the two torch sides."""

    def __init__(self, kind, learner, obs, act, ret, old, adv, valid, critic_loss, clip=0.2):
        self.kind, self.learner, self.critic_loss, self.clip = kind, learner, critic_loss, clip
        self.obs, self.act, self.ret, self.old, self.adv, self.valid = obs, act, ret, old, adv, valid

    # -- construction
    @staticmethod
    def synthetic(kind, n, n_s=30, n_a=5, critic_loss="mse", strided=True, with_valid=True, seed=None):
        """The unchunked modules' batch of n samples (their seeds: 1 + n + n_s, 11 + n_a at the ends of the action range)."""
        if seed is None:
            seed = 1 + n + n_s if n_a == 5 else 11 + n_a
        if kind == "gi":
            net = gi_t._net(n_s, n_a=n_a)
            learner = SharedPPOLearner(net, _lib(), critic_loss=critic_loss)
            obs, act, ret, old, valid = gi_t._batch(net, n, n_s, "spread", strided, with_valid, seed=seed, n_a=n_a)
            adv = None
        else:
            learner = pt_t._learner(*pt_t._nets(n_s, n_a=n_a), critic_loss=critic_loss)
            obs, act, ret, old, adv, valid = pt_t._batch(learner, n, n_s, "spread", strided, with_valid, seed=seed, n_a=n_a)
        return Case(kind, learner, obs, act, ret, old, adv, valid, critic_loss)

    def prefix(self, m):
        """The first m samples (the strides stay): every per-sample property of the batch holds for a prefix."""
        cut = lambda t: None if t is None else t[:m]  # noqa: E731
        return Case(self.kind, self.learner, self.obs[:m], self.act[:m], self.ret[:m], cut(self.old).contiguous(), cut(self.adv),
                    None if self.valid is None else self.valid[:m].contiguous(), self.critic_loss, self.clip)

    def masked(self, valid):
        """The same samples under another mask (the advantages of the separate networks are zero in masked slots)."""
        adv = None if self.kind == "gi" else self.learner.advantages(self.obs, self.act, self.ret, valid)
        return Case(self.kind, self.learner, self.obs, self.act, self.ret, self.old, adv, valid, self.critic_loss, self.clip)

    # -- pieces
    @property
    def n(self):
        return self.obs.shape[0]

    @property
    def n_a(self):
        return self.learner.n_a

    def nets(self):
        return [self.learner.policy] if self.kind == "gi" else [self.learner.actor, self.learner.critic]

    def grads(self):
        return gi_t._grads_of(*self.nets()) if self.kind == "gi" else pt_t._grads_of(*self.nets())

    def fill_grads(self, value):
        for net in self.nets():
            for p in net.parameters():
                p.grad.fill_(value)

    def sums(self, form):
        """The float32 (S+, S-) that goes to the kernel and, as a constant, to both torch runs; None for the per-sample form."""
        if form != "reference":
            return None
        if self.kind == "gi":
            return self.learner.advantage_sums(self.obs, self.ret, self.valid)
        return policy_train_util.sums_of(self.adv)

    def chunked_bytes(self, chunk):
        q = self.learner.clib.policy_gi_train_chunked_scratch_bytes if self.kind == "gi" else self.learner.clib.policy_train_chunked_scratch_bytes
        return q(self.n, chunk)

    # -- the calls: [loss] + the twelve gradients + (logp_taken, value, ratio)
    def unchunked(self, form):
        self.fill_grads(NAN)
        kw = dict(valid=self.valid, adv_sums=self.sums(form), diagnostics=True)
        if self.kind == "pt" and form != "reference":
            kw["advantages"] = self.adv
        loss, diag = self.learner.loss_and_grad(self.obs, self.act, self.ret, self.old, **kw)
        return [loss.clone()] + self.grads() + list(diag)

    def chunked_rc(self, form, chunk, scratch=None, scratch_bytes=None, sums=None, hidden=128, clip=None, critic_loss=None,
                   networks="both", both_adv=False, stray=None):
        """(status, [loss] + gradients + diagnostics) of the chunked entry; the gradients are read whatever the status.
        hidden .. stray: the arguments of SHARED_REFUSALS below (critic_loss: the raw code)."""
        clip = self.clip if clip is None else clip
        L, clib, n, S = self.learner, self.learner.clib, self.n, self.obs.shape[1]
        sums = self.sums(form) if sums is None else sums
        loss = torch.full((3 if self.kind == "gi" else 2,), NAN, device="cuda")
        diag = [torch.full((n,), NAN, device="cuda") for _ in range(3)]
        if scratch is None:
            scratch = torch.empty(self.chunked_bytes(chunk), dtype=torch.uint8, device="cuda")
        nbytes = scratch.numel() if scratch_bytes is None else scratch_bytes
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        obs, act, ret = self.obs, self.act, self.ret
        head = (obs.data_ptr(), obs.stride(0) if n else S, n, S, act.data_ptr(), act.stride(0) if n else 1, ret.data_ptr(),
                ret.stride(0) if n else 1, self.old.data_ptr(), _opt(self.valid))
        with_a, with_c = networks != "critic", networks != "actor"
        given = [diag[i].data_ptr() if on or stray == i else None for i, on in enumerate((with_a, with_c, with_a))]
        tail = (loss.data_ptr(), given[0], given[1], given[2], scratch.data_ptr(), nbytes, stream, chunk)
        if self.kind == "gi":
            W, G = abi.MMGiParams(), abi.MMGiParams()
            for name, p in zip(abi.GI_PARAMS, _params(L.policy)):
                setattr(W, name, p.detach().data_ptr())
                setattr(G, name, p.grad.data_ptr())
            code = abi.GI_CRITIC_LOSS[self.critic_loss] if critic_loss is None else critic_loss
            rc = clib.lib.mm_policy_gi_train_chunked(*head, C.byref(W), hidden, self.n_a, clip, code, _opt(sums), C.byref(G), *tail)
        else:
            ref = lambda on, st: C.byref(st) if on else None  # noqa: E731
            W = [_mlp_struct(L.actor), _mlp_struct(L.critic)]
            G = [_mlp_struct(L.actor, True), _mlp_struct(L.critic, True)]
            adv = self.adv if (sums is None or both_adv) else None
            code = abi.PT_CRITIC_LOSS[self.critic_loss] if critic_loss is None else critic_loss
            rc = clib.lib.mm_policy_train_chunked(*head, ref(with_a, W[0]), ref(with_c, W[1]), hidden, self.n_a, clip, code,
                                                  _opt(sums) if with_a else None, _opt(adv) if with_a else None, ref(with_a, G[0]),
                                                  ref(with_c, G[1]), *tail)
        return rc, [loss] + self.grads() + diag

    def chunked(self, form, chunk, **kw):
        self.fill_grads(NAN)
        rc, out = self.chunked_rc(form, chunk, **kw)
        assert rc == abi.MM_OK
        return out

    def torch_sides(self, form, sums):
        """(float32, float64) torch.autograd: (losses, the twelve gradients) each."""
        obs, act, ret, old, valid = self.obs, self.act, self.ret, self.old, self.valid
        if self.kind == "pt":
            return pt_t._torch_sides(self.learner, obs, act, ret, old, self.adv, valid, form, sums, self.critic_loss, self.clip)
        net = self.learner.policy
        args = lambda dt: (obs.to(dt), act, ret.to(dt), old.to(dt), self.clip, self.critic_loss, form)  # noqa: E731
        f32 = gi_train_util.loss_and_grads(copy.deepcopy(net), *args(torch.float32), adv_sums=sums, valid=valid)
        f64 = gi_train_util.loss_and_grads(copy.deepcopy(net).double(), *args(torch.float64),
                                           adv_sums=None if sums is None else sums.double(), valid=valid)
        return f32, f64

    def compare(self, case, out, f32, f64):
        """The rule of the unchunked modules on [loss] + gradients: prints every figure, then asserts."""
        mod = gi_t if self.kind == "gi" else pt_t
        return mod._compare("chunked_%s_%s" % (self.kind, case), (out[0], out[1:13]), f32, f64)


def _bit_equal(xs, ys, what):
    assert len(xs) == len(ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(x, y), (what, i, float((x.double() - y.double()).abs().max()))


_BASE = {}


def _base(kind, n, **kw):
    """One batch per (entry, configuration), shared by the tests that read it; nothing writes into it."""
    key = (kind, n) + tuple(sorted(kw.items()))
    if key not in _BASE:
        _BASE[key] = Case.synthetic(kind, n, **kw)
    return _BASE[key]


# ---- identity: chunk >= n is the unchunked entry
@pytest.mark.parametrize("n,chunk", [(31, 64), (31, 1024), (1000, 1024)])
@pytest.mark.parametrize("kind", ENTRIES)
def test_one_pass_is_the_unchunked_entry(kind, n, chunk):
    case = _base(kind, n)
    for form in ("reference", "flat"):
        want = case.unchunked(form)
        got = case.chunked(form, chunk)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        _bit_equal(got, want, (form, "losses, gradients and diagnostics"))


# ---- several passes
# (n, chunk, the configuration): both forms, both critic losses, strided and contiguous inputs, masked and not, the ends of
# the action range once each.  n = 129 is the first 129 samples of the n = 1000 batch.
MULTI = [
    (1000, 64, dict(form="reference", critic_loss="mse", strided=True, with_valid=True)),    # 16 passes, the last one 40 samples
    (1000, 192, dict(form="flat", critic_loss="huber", strided=True, with_valid=True, n_a=8)),  # 3 slices per pass
    (1000, 960, dict(form="reference", critic_loss="huber", strided=True, with_valid=True, n_a=1)),
    (129, 64, dict(form="flat", critic_loss="mse", strided=True, with_valid=True)),          # the last pass holds one sample
    (70001, 16384, dict(form="reference", critic_loss="huber", strided=True, with_valid=True)),  # 256 slices per pass, 5 passes
    (70001, 16384, dict(form="flat", critic_loss="mse", strided=False, with_valid=False)),
]


@pytest.mark.parametrize("n,chunk,cfg", MULTI, ids=["%d_%d_%s" % (n, c, k["form"]) for n, c, k in MULTI])
@pytest.mark.parametrize("kind", ENTRIES)
def test_passes_sum_to_the_whole_batch(kind, n, chunk, cfg):
    cfg = dict(cfg)
    form = cfg.pop("form")
    case = _base(kind, 1000, **cfg).prefix(n) if n == 129 else _base(kind, n, seed=77 if n == 70001 else None, **cfg)
    assert (n + chunk - 1) // chunk > 1
    want = case.unchunked(form)
    got = case.chunked(form, chunk)
    _bit_equal(got[:1] + got[13:], want[:1] + want[13:], "losses and diagnostics")
    sums = case.sums(form)
    f32, f64 = case.torch_sides(form, sums)
    case.compare("n%d_c%d_%s" % (n, chunk, form), got, f32, f64)


# ---- masks
@pytest.mark.parametrize("kind", ENTRIES)
def test_a_pass_without_a_valid_sample(kind):
    base = _base(kind, 1000)
    valid = base.valid.clone()
    valid[64:128] = 0  # the whole second pass at chunk 64
    case = base.masked(valid)
    for form in ("reference", "flat"):
        got = case.chunked(form, 64)
        _bit_equal(got[:1] + got[13:], [x for i, x in enumerate(case.unchunked(form)) if i == 0 or i >= 13], "losses and diagnostics")
        f32, f64 = case.torch_sides(form, case.sums(form))
        case.compare("masked_pass_%s" % form, got, f32, f64)


@pytest.mark.parametrize("kind", ENTRIES)
def test_nothing_valid_and_nothing_at_all(kind):
    base = _base(kind, 1000)
    none = base.masked(torch.zeros(1000, dtype=torch.uint8, device="cuda"))
    for form in ("reference", "flat"):
        for t in none.chunked(form, 192):
            assert float(t.abs().max()) == 0.0
    empty = base.prefix(0)
    empty.valid = None
    sums = torch.zeros(2, device="cuda")
    for form in ("reference", "flat"):
        out = empty.chunked(form, 64, scratch=torch.empty(16, dtype=torch.uint8, device="cuda"), sums=sums if form == "reference" else None)
        for t in out[:13]:
            assert float(t.abs().max()) == 0.0


# ---- the scratch is written before it is read; two calls give the same bits
@pytest.mark.parametrize("kind", ENTRIES)
def test_scratch_contents_do_not_matter(kind):
    case = _base(kind, 1000)
    scratch = torch.empty(case.chunked_bytes(192), dtype=torch.uint8, device="cuda")
    runs = []
    for fill in (0xFF, 0x00):
        scratch.fill_(fill)
        runs.append(case.chunked("reference", 192, scratch=scratch))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    _bit_equal(runs[0], runs[1], "0xFF against zeros")


# ---- graph capture
@pytest.mark.parametrize("kind", ENTRIES)
def test_graph_capturable(kind):
    case = _base(kind, 1000)
    chunk = 384  # 3 passes
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
def shared_refusals(separate, wrong_hidden):
    """What the chunked and the partial entry of a family refuse through one shared check, as keyword arguments of the modules'
    *_rc calls.  Only arguments that would be memory-safe if a broken check let them through: clip_param negative and NaN, an
    unknown critic_loss, a hidden size the entry is not built for (the networks keep their own), and for the separate networks
    adv_sums together with advantages and a diagnostic (0 logp_taken, 1 value, 2 ratio) without its network."""
    table = [dict(clip=-0.125), dict(clip=NAN), dict(critic_loss=2), dict(critic_loss=-1)] + [dict(hidden=h) for h in wrong_hidden]
    if separate:
        table += [dict(both_adv=True), dict(networks="critic", stray=0), dict(networks="critic", stray=2),
                  dict(networks="actor", stray=1)]
    return table


@pytest.mark.parametrize("kind", ENTRIES)
def test_refusals_leave_the_gradients_alone(kind):
    case = _base(kind, 1000)
    need = case.chunked_bytes(64)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    sums = case.sums("reference")
    torch.cuda.synchronize()
    refused = [dict(chunk=0), dict(chunk=32), dict(chunk=100), dict(chunk=64, scratch_bytes=need - 1)]
    for kw in refused:
        case.fill_grads(-7.0)
        rc, out = case.chunked_rc("reference", kw["chunk"], scratch=scratch, scratch_bytes=kw.get("scratch_bytes"), sums=sums)
        torch.cuda.synchronize()
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        for g in out[1:13]:
            assert bool((g == -7.0).all()), kw
        assert bool(torch.isnan(out[0]).all())  # the losses were not written either
    for kw in shared_refusals(kind == "pt", (64, 512)):
        case.fill_grads(-7.0)
        rc, out = case.chunked_rc("reference", 64, scratch=scratch, sums=sums, **kw)
        torch.cuda.synchronize()
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert all(bool((g == -7.0).all()) for g in out[1:13]), kw
        assert all(bool(torch.isnan(t).all()) for t in out[:1] + out[13:]), kw  # neither losses nor diagnostics were written
    q = case.learner.clib
    for query in (q.policy_gi_train_chunked_scratch_bytes, q.policy_train_chunked_scratch_bytes):
        for chunk in (0, 32, 100, -64):
            with pytest.raises(ValueError):
                query(1000, chunk)
    assert case.chunked_rc("reference", 64, scratch=scratch, sums=sums)[0] == abi.MM_OK  # the well-formed call goes through


# ---- the batches the reference ran on: 2 passes at chunk 64
@pytest.mark.parametrize("loss_name,t", gi_train_util.FIXTURES)
def test_reference_fixture_gradients_gi(loss_name, t):
    z, meta = gi_train_util.load_fixture(loss_name, t)
    target = gi_train_util.fixture_net(z, meta, "tp_", device="cuda")
    for a in range(meta["n_agents"]):
        net = gi_train_util.fixture_net(z, meta, "p_" if a == 0 else "a%d_q_" % (a - 1), device="cuda")
        learner = SharedPPOLearner(net, _lib(), critic_loss=loss_name, clip_param=meta["clip_param"])
        learner.policy_target.load_state_dict(target.state_dict())
        obs, act, ret = gi_t._fixture_step_inputs(z, a)
        assert 64 < obs.shape[0] <= 128
        case = Case("gi", learner, obs, act, ret, learner.old_log_probs(obs, act), None, None, loss_name, meta["clip_param"])
        got = case.chunked("reference", 64)
        f32, f64 = case.torch_sides("literal", None)
        rec = case.compare("fixture_%s_t%d_a%d" % (loss_name, t, a), got, f32, f64)
        recorded = [torch.tensor(z["a%d_losses" % a], device="cuda")] + [torch.tensor(z["a%d_g_%s" % (a, k)], device="cuda")
                                                                        for k in gi_train_util.GRAD_NAMES]
        for name, gk, gr, g64 in zip(["loss"] + gi_train_util.GRAD_NAMES, got[:13], recorded, [f64[0]] + f64[1]):
            slack = float((gr.double() - g64).abs().max())
            assert float((gk.double() - gr.double()).abs().max()) <= rec[name]["bound"] + slack, (a, name)


@pytest.mark.parametrize("run,t", policy_train_util.FIXTURES)
def test_reference_fixture_gradients_pt(run, t):
    z, meta = policy_train_util.load_fixture(run, t)
    for a in range(meta["n_agents"]):
        learner = pt_t._fixture_learner(z, meta, policy_train_util.pre_step_prefix(a))
        obs, act, ret = pt_t._fixture_step_inputs(z, a)
        assert 64 < obs.shape[0] <= 128
        old, adv = learner.old_log_probs(obs, act), learner.advantages(obs, act, ret)
        case = Case("pt", learner, obs, act, ret, old, adv, None, meta["critic_loss"], meta["clip_param"])
        got = case.chunked("reference", 64)
        f32, f64 = case.torch_sides("literal", None)
        rec = case.compare("fixture_%s_t%d_a%d" % (run, t, a), got, f32, f64)
        recorded = [torch.tensor(z["a%d_losses" % a], device="cuda")] + [torch.tensor(z["a%d_g_%s" % (a, k)], device="cuda")
                                                                        for k in policy_train_util.GRAD_NAMES]
        for name, gk, gr, g64 in zip(pt_t.LOSS_AND_GRADS, got[:13], recorded, [f64[0]] + f64[1]):
            slack = float((gr.double() - g64).abs().max())
            assert float((gk.double() - gr.double()).abs().max()) <= rec[name]["bound"] + slack, (a, name)


# ---- the learners under a budget
def _rollout_like(B, N, S, n_a, seed):
    g = torch.Generator().manual_seed(seed)
    states = (torch.randn(B, N, S, generator=g) * 1.5).cuda()
    actions = torch.randint(0, n_a, (B, N), generator=g, dtype=torch.int32).cuda()
    returns = (torch.randn(B, N, generator=g) * 1.5 + 0.3).cuda()
    return states, actions, returns


def _named(learner, kind):
    if kind == "gi":
        return dict(learner.policy.named_parameters())
    named = {"actor." + k: v for k, v in learner.actor.named_parameters()}
    named.update({"critic." + k: v for k, v in learner.critic.named_parameters()})
    return named


@pytest.mark.parametrize("fused", [False, True], ids=["torch_tail", "fused_tail"])
@pytest.mark.parametrize("kind", ENTRIES)
def test_learner_under_a_budget(kind, fused):
    """B = 200, N = 3 under a budget that leaves room for 64-sample passes only, against a twin without a budget: the three
    agent steps of train(form="reference"), then one train(form="flat") on all 600 samples.  RMSprop moves an element whose
    gradient is rounding noise around zero by up to (lr / eps) dg, so per tensor the bound is (lr / eps) 4 e32 + 1e-7 with e32
    the float32 torch error on that tensor at the twin's pre-step parameters (max over the steps so far)."""
    B, N, S, n_a = 200, 3, 30, 5
    clib = _lib()
    states, actions, returns = _rollout_like(B, N, S, n_a, seed=21)
    if kind == "gi":
        net = gi_t._net(S)
        budget = clib.policy_gi_train_chunked_scratch_bytes(B * N, 64)
        assert budget < clib.policy_gi_train_chunked_scratch_bytes(B, 128) and budget < clib.policy_gi_train_scratch_bytes(B)
        twin = SharedPPOLearner(copy.deepcopy(net), clib, fused_step=fused)
        small = SharedPPOLearner(net, clib, fused_step=fused, scratch_budget_bytes=budget)
        names = gi_train_util.GRAD_NAMES
    else:
        actor, critic = pt_t._nets(S)
        budget = clib.policy_train_chunked_scratch_bytes(B * N, 64)
        assert budget < clib.policy_train_chunked_scratch_bytes(B, 128) and budget < clib.policy_train_scratch_bytes(B)
        twin = pt_t._learner(copy.deepcopy(actor), copy.deepcopy(critic), fused_step=fused)
        small = pt_t._learner(actor, critic, fused_step=fused, scratch_budget_bytes=budget)
        names = policy_train_util.GRAD_NAMES
    e32 = dict.fromkeys(names, 0.0)

    def measure(obs, act, ret, form):
        """e32 of the step the twin is about to take."""
        if kind == "gi":
            dense = obs.contiguous()
            old = twin.old_log_probs(dense, act)
            sums = twin.advantage_sums(dense, ret) if form == "reference" else None
            case = Case("gi", twin, obs, act, ret, old, None, None, "mse")
        else:
            old, value = twin.evaluate(obs, act, actor=twin.actor_target, critic=twin.critic_target)
            adv = ret - value
            sums = policy_train_util.sums_of(adv) if form == "reference" else None
            case = Case("pt", twin, obs, act, ret, old, adv, None, "mse")
        f32, f64 = case.torch_sides(form, sums)
        for k, x, y in zip(names, f32[1], f64[1]):
            e32[k] = max(e32[k], float((x.double() - y).abs().max()))

    def check(step):
        a, b = _named(small, kind), _named(twin, kind)
        for k in names:
            diff = float((a[k].detach() - b[k].detach()).abs().max())
            bound = (LR / RMS_EPS) * 4.0 * e32[k] + 1e-7
            print("%s %s %-8s %-22s diff %.3e bound %.3e" % (kind, "fused" if fused else "torch", step, k, diff, bound))
            assert diff <= bound, (step, k, diff, bound)

    start = {k: v.detach().clone() for k, v in _named(small, kind).items()}
    for a in range(N):
        measure(states[:, a, :], actions[:, a], returns[:, a], "reference")
        for learner in (twin, small):  # one agent step = train() on that agent's column alone
            learner.train(states[:, a:a + 1], actions[:, a:a + 1], returns[:, a:a + 1], form="reference")
        check("agent%d" % a)
    measure(states.reshape(-1, S), actions.reshape(-1), returns.reshape(-1), "flat")
    for learner in (twin, small):
        learner.train(states, actions, returns, form="flat")
    check("flat")
    assert all(not torch.equal(v.detach(), start[k]) for k, v in _named(small, kind).items())
    assert small._scratch.numel() <= budget < twin._scratch.numel()
