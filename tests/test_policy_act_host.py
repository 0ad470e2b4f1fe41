"""The act-side policy entries without a GPU: the numpy Philox of policy_act_util.py against published known answers, the
oracle build's mm_policy_act / mm_sample_actions / mm_discount_returns over the grid that test_policy_act_gpu.py runs on the
device (the CPU twin has the same contract), and the conditions on the INPUTS of every case of that grid -- computed with the
numpy Philox and the float64 network, never with code under test."""
import numpy as np
import pytest
import torch

import oracle_env
import policy_act_util as U

ERRORS = {}


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: zeros, and the digits of pi."""
    got = U.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(w) for w in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = U.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert [int(w) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # vectorised == element by element, and the sampler's word layout
    idx = np.array([0, 1, 77, (1 << 32) + 3], dtype=np.uint64)
    ctr, seed = (1 << 63) + 1, 0x9E3779B97F4A7C15
    u = U.sampler_u(idx, ctr, seed)
    for i, x in enumerate(idx.tolist()):
        w = U.philox4x32_10((x & 0xFFFFFFFF, x >> 32, ctr & 0xFFFFFFFF, (ctr >> 32) ^ U.DOMAIN), (seed & 0xFFFFFFFF, seed >> 32))
        assert u[i] == ((int(w[0]) >> 5) * 67108864 + (int(w[1]) >> 6)) / 9007199254740992.0
    assert 0.0 <= u.min() and u.max() < 1.0


@pytest.mark.parametrize("n_s", U.NS_ACT)
def test_oracle_policy_act_grid_a(n_s):
    clib = oracle_env.library()
    for case in U.grid_a("act"):
        if case.n_s == n_s:
            U.check_forward(ERRORS, clib, case, "cpu")


def test_oracle_policy_act_recorded_and_grid_b():
    clib = oracle_env.library()
    for case in U.recorded_cases("act"):
        U.check_forward(ERRORS, clib, case, "cpu")
    base = U.check_forward(ERRORS, clib, U.case_b("act", 257), "cpu")
    for n in U.N_GRID_B:
        case = U.case_b("act", n)
        out = U.check_forward(ERRORS, clib, case, "cpu", f64_actions=n <= 1000)
        idx = torch.arange(n) % 257
        assert torch.equal(out["logp"], base["logp"][idx]), n
        if n > 1000:
            near = case.near(U.SEED_A, U.CTR_A)
            assert np.array_equal(out["actions"].numpy()[~near], case.actions64(U.SEED_A, U.CTR_A)[~near]), n


def test_oracle_sampler_grid_c():
    """Grid C on the oracle: the actions of mm_policy_act and of mm_sample_actions under every seed and counter, and that
    the high words of both reach the draw."""
    clib = oracle_env.library()
    for n_a in U.NA_C:
        case = U.case_c("act", n_a, 257)
        w = U.weights_of("act", case.net)
        for seed in U.SEEDS_C:
            for ctr in U.CTRS_C:
                out = U.run(clib, "act", w, case.obs, n_a, seed, ctr)
                a_own, c = U.sample(clib, out["logp"], seed, ctr)
                assert torch.equal(out["actions"], a_own) and c == out["counter"] == ((ctr + 1) & U.U64)
                near = case.near(seed, ctr)
                assert np.array_equal(out["actions"].numpy()[~near], case.actions64(seed, ctr)[~near]), (n_a, seed, ctr)
        if n_a > 1:
            U.check_high_words(clib, case, "cpu")
    U.check_sampler_rows(clib, "cpu")


def test_high_words_reach_the_uniform():
    """Equal low words with different high words, of the seed or of the counter, give different uniforms (numpy Philox):
    what the device test asserts of the action vectors is a property of the inputs."""
    idx = np.arange(257, dtype=np.uint64)
    for lo in (5, 99):
        assert not np.array_equal(U.sampler_u(idx, lo, 7), U.sampler_u(idx, (1 << 32) + lo, 7))
        assert not np.array_equal(U.sampler_u(idx, 7, lo), U.sampler_u(idx, 7, (1 << 32) + lo))
        assert not np.array_equal(U.sampler_u(idx, lo, 7), U.sampler_u(idx, (1 << 63) + lo, 7))


def _all_gpu_cases():
    """(case, [(seed, ctr)]) for every forward launch of test_policy_act_gpu.py whose actions meet the float64 sampler."""
    a = [(U.SEED_A, U.CTR_A)]
    c = [(s, k) for s in U.SEEDS_C for k in U.CTRS_C]
    for kind in ("act", "gi"):
        for case in U.grid_a(kind) + U.recorded_cases(kind):
            yield case, a
        for n in U.N_GRID_B:
            yield U.case_b(kind, n), a
        for n_a in U.NA_C:
            for n in U.N_C:
                yield U.case_c(kind, n_a, n), c


def test_input_conditions_of_the_gpu_grid():
    """No u within BAND of an inner CDF edge for n <= 1000, a share of at most BAND_SHARE beyond; no knife-edge row (asserted
    when a Case is built); and on the recorded state sets the float32 module's CDF meets the same condition."""
    worst = 0.0
    for case, keys in _all_gpu_cases():
        for seed, ctr in keys:
            near = case.near(seed, ctr)
            if case.n <= 1000:
                assert not near.any(), (case.name, hex(seed), hex(ctr), np.nonzero(near)[0])
            else:
                worst = max(worst, float(near.mean()))
                assert near.mean() <= U.BAND_SHARE, (case.name, hex(seed), hex(ctr))
    print("largest share of rows within %g of a CDF edge at n > 1000: %.3g" % (U.BAND, worst))
    for kind, tag in U.RECORDED:
        case = U.recorded_case(kind, tag)
        with torch.no_grad():
            lp32 = case.net(case.obs).double().numpy()
        assert not U.near_edge(lp32, case.u(U.SEED_A, U.CTR_A)).any(), tag
        assert np.array_equal(U.sample_f64(lp32, case.u(U.SEED_A, U.CTR_A)), case.actions64(U.SEED_A, U.CTR_A)), tag


def test_oracle_discount_returns_edges():
    clib = oracle_env.library()
    for edge in U.discount_edges([(1, 9, 5), (37, 9, 5), (1, 257, 1), (7, 257, 1), (7, 257, 3)]):
        U.check_discount(clib, "cpu", edge)
    U.check_discount_empty(clib, "cpu")
