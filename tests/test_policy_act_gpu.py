"""The act-side policy kernels on the MI355X against float64 on their whole accepted domain: policy_kernel (mm_policy_act),
policy_gi_kernel (mm_policy_gi_act), sample_kernel (mm_sample_actions) and discount_kernel (mm_discount_returns).

The tolerance is the train side's rule (policy_act_util.compare): per output tensor,
    max|kernel - f64| <= 4 * e32 + 1e-6 * max(1, max|f64|),   e32 = max|float32 torch module on the device - f64|.
Nothing is compared with the kernel's own earlier output except where bit identity between two launches of the same kernel is
the claim (grids B, D, E).  The sampler is checked against a numpy Philox pinned to published known answers
(test_policy_act_host.py) and a float64 inverse CDF; the conditions on the inputs are asserted there, without a GPU.

Grids: A n_s x n_a x gain at n = 257 (gain 60: log-probabilities down to -100, beyond float32's expf range), B the n boundaries of
the tile / wave / workgroup / persistent-loop decomposition, C seeds and counters with both high words in use, D guarded and
misaligned buffers, E tile isolation, F act against eval, G mm_discount_returns' edges."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import policy_act_util as U
from marl_mass_amd import _cabi as abi

pytestmark = pytest.mark.gpu

ERRORS = {}   # case -> {output: {e32, kernel_err, max_abs, bound}}
FIGURES = {}  # figures that are recorded, not asserted
KINDS = ("act", "gi")
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _dump_errors(tmp_path_factory):
    """Writes the measured figures when the module is done: to $MM_ACT_ERROR_JSON when set (that is how
    profiles/policy_act/forward_error.json is regenerated), else to pytest's temporary directory."""
    yield
    path = os.environ.get("MM_ACT_ERROR_JSON") or str(tmp_path_factory.mktemp("policy_act") / "forward_error.json")
    sig = lambda v: float("%.3g" % v)  # noqa: E731
    rows = {k: {o: {f: sig(x) for f, x in r.items()} for o, r in ERRORS[k].items()} for k in ERRORS}
    rows["figures"] = {k: sig(v) for k, v in FIGURES.items()}
    with open(path, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rows[k], sort_keys=True)) for k in sorted(rows)) + "\n}\n")
    print("measured figures: %s" % path)


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _on_device(case):
    net = copy.deepcopy(case.net).to(DEV)
    return U.weights_of(case.kind, net), case.obs.to(DEV)


def _same(a, b, keys=("actions", "logp", "value")):
    """Bit identity of two launches' outputs (NaN-free by construction: compared as integers)."""
    for k in keys:
        if a.get(k) is None:
            assert b.get(k) is None
            continue
        assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k


# ---- A: forward against float64 over the accepted domain
@pytest.mark.parametrize("kind,n_s", [("act", s) for s in U.NS_ACT] + [("gi", s) for s in U.NS_GI])
def test_a_forward_grid(kind, n_s):
    clib = _lib()
    for case in U.grid_a(kind):
        if case.n_s == n_s:
            U.check_forward(ERRORS, clib, case, DEV)


@pytest.mark.parametrize("kind,tag", U.RECORDED)
def test_a_recorded_states(kind, tag):
    U.check_forward(ERRORS, _lib(), U.recorded_case(kind, tag), DEV)


# ---- B: n boundaries
@pytest.mark.parametrize("kind", KINDS)
def test_b_n_boundaries(kind):
    """n on both sides of a tile (32), a workgroup (256), one tile per wave at 256 workgroups (65536) and the persistent loop
    beyond; the rows are 257 rows repeated, so every row of every launch has a bit-exact twin in the launch of the first
    min(n, 257) rows alone: a row's result may not depend on its tile, wave or trip of the loop."""
    clib = _lib()
    base = U.check_forward(ERRORS, clib, U.case_b(kind, 257), DEV)
    for n in U.N_GRID_B:
        case = U.case_b(kind, n)
        out = U.check_forward(ERRORS, clib, case, DEV, f64_actions=n <= 1000)
        idx = torch.arange(n, device=DEV) % 257
        _same({"logp": out["logp"], "value": out["value"]},
              {"logp": base["logp"][idx], "value": None if base["value"] is None else base["value"][idx]}, ("logp", "value"))
        w, obs = _on_device(case)
        m = min(n, 257)
        alone = U.run(clib, kind, w, obs[:m].contiguous(), case.n_a, U.SEED_A, U.CTR_A)
        _same({k: None if out[k] is None else out[k][:m] for k in ("actions", "logp", "value")}, alone)
        if n > 1000:  # (the share of BAND rows is bounded on the host)
            near = case.near(U.SEED_A, U.CTR_A)
            assert np.array_equal(out["actions"].cpu().numpy()[~near], case.actions64(U.SEED_A, U.CTR_A)[~near]), n


# ---- C: the sampler against the independent reference
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", U.N_C)
def test_c_actions_under_every_seed_and_counter(kind, n):
    clib = _lib()
    for n_a in U.NA_C:
        case = U.case_c(kind, n_a, n)
        w, obs = _on_device(case)
        for seed in U.SEEDS_C:
            for ctr in U.CTRS_C:
                out = U.run(clib, kind, w, obs, n_a, seed, ctr)
                a_own, c = U.sample(clib, out["logp"], seed, ctr)
                assert torch.equal(out["actions"], a_own), (n_a, hex(seed), hex(ctr))  # no row left out
                assert c == out["counter"] == ((ctr + 1) & U.U64)
                near = case.near(seed, ctr)
                assert np.array_equal(out["actions"].cpu().numpy()[~near], case.actions64(seed, ctr)[~near]), (n_a, hex(seed), hex(ctr))
                if n_a == 1:
                    assert bool((out["actions"] == 0).all())
        if n_a > 1 and n == 257:
            U.check_high_words(clib, case, DEV)


def test_c_sampler_masked_and_unnormalised_rows():
    U.check_sampler_rows(_lib(), DEV)


def test_c_sampler_high_words():
    """mm_sample_actions alone: equal low words with different high words, of the seed or of the counter, draw differently,
    and each draw is the float64 inverse CDF's under the numpy Philox."""
    clib = _lib()
    for n in U.N_C:
        lp = torch.log_softmax(torch.randn(n, 5, generator=torch.Generator().manual_seed(n)) * 2, -1)
        dev = lp.to(DEV)
        idx = np.arange(n, dtype=np.uint64)
        for (s0, c0), (s1, c1) in U.HIGH_PAIRS:
            a0, a1 = U.sample(clib, dev, s0, c0)[0], U.sample(clib, dev, s1, c1)[0]
            assert not torch.equal(a0, a1), (hex(s1), hex(c1))
            for a, s, c in ((a0, s0, c0), (a1, s1, c1)):
                u = U.sampler_u(idx, c, s)
                near = U.near_edge(lp.double().numpy(), u)
                assert near.mean() <= U.BAND_SHARE
                assert np.array_equal(a.cpu().numpy()[~near], U.sample_f64(lp.double().numpy(), u)[~near]), (hex(s), hex(c))


def test_c_counter_steps_and_empty_batch():
    """The counter advances by exactly one per call that samples and by nothing for a value-only or logp-only
    mm_policy_gi_act call; n = 0 returns MM_OK, enqueues nothing and leaves the counter unchanged (the headers say so)."""
    clib = _lib()
    for kind in KINDS:
        case = U.synthetic_case(kind, 30, 5, 3)
        w, obs = _on_device(case)
        c = U.counter_tensor((1 << 32) - 1, DEV)  # the step carries into the high word
        a = torch.full((case.n,), -1, dtype=torch.int32, device=DEV)
        lp = torch.full((case.n, 5), float("nan"), device=DEV)
        v = torch.full((case.n,), float("nan"), device=DEV) if kind == "gi" else None
        for step in range(1, 4):
            clib.check(U.launch(clib, kind, w, obs, case.n, 30, 5, 7, c, a, lp, v))
            assert U.counter_value(c) == (1 << 32) - 1 + step
        ref = U.run(clib, kind, w, obs, 5, 7, (1 << 32) + 1)  # the third call's counter
        assert torch.equal(ref["actions"], a)
        if kind == "gi":
            before = U.counter_value(c)
            for outs in ((None, lp, v), (None, None, v), (None, lp, None)):
                clib.check(U.launch(clib, kind, w, obs, case.n, 30, 5, 7, c, *outs))
                assert U.counter_value(c) == before
            clib.check(U.launch(clib, kind, w, obs, case.n, 30, 5, 7, None, None, lp, v))  # (no counter needed)
        # n = 0: outputs and counter untouched
        before = U.counter_value(c)
        ga, chk_a = U.guarded(8, torch.int32, DEV)
        gl, chk_l = U.guarded(8, torch.float32, DEV)
        ga.fill_(-12345); gl.fill_(float("nan"))
        assert U.launch(clib, kind, w, obs, 0, 30, 5, 7, c, ga, gl, None if kind == "act" else gl) == abi.MM_OK
        torch.cuda.synchronize()
        chk_a(); chk_l()
        assert bool((ga == -12345).all()) and bool(torch.isnan(gl).all()) and U.counter_value(c) == before
    c = U.counter_tensor(41, DEV)
    lp = torch.zeros(8, 5, device=DEV)
    ga, chk_a = U.guarded(8, torch.int32, DEV)
    ga.fill_(-12345)
    assert clib.lib.mm_sample_actions(lp.data_ptr(), 0, 5, 7, c.data_ptr(), ga.data_ptr(), None) == abi.MM_OK
    torch.cuda.synchronize()
    chk_a()
    assert bool((ga == -12345).all()) and U.counter_value(c) == 41


# ---- D: memory discipline
@pytest.mark.parametrize("kind", KINDS)
def test_d_guarded_outputs_and_misaligned_pointers(kind):
    """Outputs in sentinel-padded buffers, every input and output pointer 4-byte but not 16-byte aligned: the pads stay
    intact and the outputs equal the aligned run's bit for bit."""
    clib = _lib()
    base = U.synthetic_case(kind, 30, 5, 3)
    w, obs_all = _on_device(base)
    w_off = [U.offset_copy(t) for t in w]
    for n in (1, 33, 257):
        obs = obs_all[:n].contiguous()
        want = U.run(clib, kind, w, obs, 5, U.SEED_A, U.CTR_A)
        a, chk_a = U.guarded(n, torch.int32, DEV)
        lp, chk_l = U.guarded(n * 5, torch.float32, DEV)
        v, chk_v = U.guarded(n, torch.float32, DEV) if kind == "gi" else (None, lambda: None)
        c = U.counter_tensor(U.CTR_A, DEV)
        clib.check(U.launch(clib, kind, w_off, U.offset_copy(obs), n, 30, 5, U.SEED_A, c, a, lp, v))
        torch.cuda.synchronize()
        chk_a(); chk_l(); chk_v()
        _same(want, {"actions": a, "logp": lp.view(n, 5), "value": v})
        # mm_sample_actions from and into offset buffers
        a2, chk_a2 = U.guarded(n, torch.int32, DEV)
        c = U.counter_tensor(U.CTR_A, DEV)
        clib.check(clib.lib.mm_sample_actions(lp.data_ptr(), n, 5, U.SEED_A, c.data_ptr(), a2.data_ptr(), None))
        torch.cuda.synchronize()
        chk_a2()
        assert torch.equal(a2, want["actions"])
        if kind == "gi":  # each optional output alone writes only itself
            for outs in ((None, None, v), (None, lp, None), (a, None, None)):
                for t in (a, lp, v):
                    t.fill_(U._sentinel(t.dtype))
                c = U.counter_tensor(U.CTR_A, DEV)
                clib.check(U.launch(clib, kind, w_off, U.offset_copy(obs), n, 30, 5, U.SEED_A, c, *outs))
                torch.cuda.synchronize()
                chk_a(); chk_l(); chk_v()
                got = {"actions": a, "logp": lp.view(n, 5), "value": v}
                for k, t in zip(("actions", "logp", "value"), outs):
                    if t is None:
                        s = got[k]
                        assert bool((torch.isnan(s) if s.dtype.is_floating_point else s == -12345).all()), k
                    else:
                        _same({k: want[k]}, {k: got[k]}, (k,))


@pytest.mark.parametrize("n_s", [26, 30, 32])
def test_d_gi_split_never_reads_columns_past_24(n_s):
    """rollout.SPLIT_COLS: the state split reads columns 0..24 whatever n_s is; NaN in columns 25..n_s-1 changes no bit."""
    clib = _lib()
    case = U.synthetic_case("gi", n_s, 5, 3)
    w, obs = _on_device(case)
    want = U.run(clib, "gi", w, obs, 5, U.SEED_A, U.CTR_A)
    obs = obs.clone()
    obs[:, 25:] = float("nan")
    _same(want, U.run(clib, "gi", w, obs, 5, U.SEED_A, U.CTR_A))


# ---- E: tile isolation
@pytest.mark.parametrize("kind", KINDS)
def test_e_a_poisoned_row_reaches_no_other_row(kind):
    """64 rows = two MFMA tiles; row 5 and row 40 poisoned in turn (all-NaN, then +inf in one column): the other 63 rows'
    outputs equal the clean run bit for bit.  Non-finite observations are outside the contract (fmaxf drops a NaN
    pre-activation where torch's relu keeps it), so of the poisoned row only 0 <= action < n_a is asserted."""
    clib = _lib()
    case = U.synthetic_case(kind, 30, 5, 3)
    w, obs_all = _on_device(case)
    clean_obs = obs_all[:64].contiguous()
    clean = U.run(clib, kind, w, clean_obs, 5, U.SEED_A, U.CTR_A)
    for row in (5, 40):
        for poison in ("nan", "inf"):
            obs = clean_obs.clone()
            if poison == "nan":
                obs[row, :] = float("nan")
            else:
                obs[row, 11] = float("inf")
            a, chk_a = U.guarded(64, torch.int32, DEV)
            lp, chk_l = U.guarded(64 * 5, torch.float32, DEV)
            v, chk_v = U.guarded(64, torch.float32, DEV) if kind == "gi" else (None, lambda: None)
            c = U.counter_tensor(U.CTR_A, DEV)
            clib.check(U.launch(clib, kind, w, obs, 64, 30, 5, U.SEED_A, c, a, lp, v))
            torch.cuda.synchronize()
            chk_a(); chk_l(); chk_v()
            keep = torch.arange(64, device=DEV) != row
            got = {"actions": a[keep], "logp": lp.view(64, 5)[keep], "value": None if v is None else v[keep]}
            _same({k: None if clean[k] is None else clean[k][keep] for k in ("actions", "logp", "value")}, got)
            assert 0 <= int(a[row]) < 5, (row, poison)


# ---- F: act against eval
def test_f_act_and_eval_agree_with_float64():
    """mm_policy_act's logp[j, a_j] and mm_policy_eval's logp_taken of the same actor on 1000 rows: each within the rule of
    float64; their largest mutual difference is recorded, not asserted."""
    import ctypes as C
    from marl_mass_amd.learner import _mlp_struct
    clib = _lib()
    case = U.synthetic_case("act", 30, 5, 3, 1000)
    net = copy.deepcopy(case.net).to(DEV)
    obs = case.obs.to(DEV)
    out = U.run(clib, "act", U.weights_of("act", net), obs, 5, U.SEED_A, U.CTR_A)
    acts = out["actions"]
    taken = lambda lp: lp.gather(1, acts.long().to(lp.device).unsqueeze(1)).squeeze(1)  # noqa: E731
    ev = torch.full((1000,), float("nan"), device=DEV)
    clib.check(clib.lib.mm_policy_eval(obs.data_ptr(), 30, 1000, 30, acts.data_ptr(), 1, None, C.byref(_mlp_struct(net)), None, 128, 5,
                                       ev.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    with torch.no_grad():
        f32 = taken(net(obs))
    f64 = taken(case.logp64)
    U.compare(ERRORS, "f_act_taken_n1000", {"logp": taken(out["logp"])}, {"logp": f32}, {"logp": f64})
    U.compare(ERRORS, "f_eval_taken_n1000", {"logp": ev}, {"logp": f32}, {"logp": f64})
    FIGURES["act_vs_eval_max_abs_diff"] = float((taken(out["logp"]) - ev).abs().max())


# ---- G: mm_discount_returns
@pytest.mark.parametrize("T", [1, 7])
def test_g_discount_returns_edges(T):
    clib = _lib()
    for edge in U.discount_edges([(T, 257, 3), (T, 257, 1)]):
        U.check_discount(clib, DEV, edge)
    U.check_discount_empty(clib, DEV)
