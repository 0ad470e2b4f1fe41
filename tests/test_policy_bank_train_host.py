"""The policy bank's training half without a GPU: the headers' constants against _cabi, the entries' presence in the HIP library
and their absence from the oracle, BankPPOLearner's refusals that need no device, the scratch query against the sum of the
per-group needs and its monotonic growth, host-side refusals of the raw entries, and the new objects' kernel resources."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import oracle_env
import policy_bank_train_util as U
from policy_act_util import gi_net
from marl_mass_amd import _cabi as abi, hip_library
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(text, name):
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


def test_header_constants_match_cabi():
    text = open(os.path.join(REPO, "include", "mm_policy_bank_train.h")).read()
    assert _define(text, "MM_PT_FORM_REFERENCE") == abi.PT_FORM["reference"] == 0
    assert _define(text, "MM_PT_FORM_PER_SAMPLE") == abi.PT_FORM["per_sample"] == 1
    for name, value in (("HEADER", abi.PBT_HEADER_BYTES), ("MEMBER", abi.PBT_MEMBER_BYTES), ("SAMPLE", abi.PBT_SAMPLE_BYTES),
                        ("TILE", abi.PBT_TILE_BYTES), ("PARTIAL", abi.PBT_PARTIAL_BYTES)):
        assert _define(text, "MM_PBT_%s_BYTES" % name) == value
    bank = open(os.path.join(REPO, "include", "mm_policy_bank.h")).read()
    assert _define(bank, "MM_BANK_MAX_GROUPS") == abi.BANK_MAX_GROUPS
    assert "mm_opt_step_bank" in open(os.path.join(REPO, "include", "mm_opt_step.h")).read()


def test_hip_library_has_the_entries_and_the_learner_imports():
    hip = hip_library()  # loading the library needs no GPU
    assert hip.has_policy_bank_train
    hip.require_policy_bank_train()
    from marl_mass_amd.learner import BankPPOLearner  # noqa: F401


def test_oracle_library_lacks_the_entries():
    lib = oracle_env.library()
    assert not lib.has_policy_bank_train
    with pytest.raises(NotImplementedError, match="mm_policy_bank_train"):
        lib.require_policy_bank_train()
    with pytest.raises(NotImplementedError, match="mm_policy_bank_train"):
        lib.policy_bank_train_scratch_bytes(1, 1, [0, 1])


def test_learner_refusals_without_a_device():
    from marl_mass_amd.learner import BankPPOLearner
    hip = hip_library()
    a, c = ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1)
    with pytest.raises(ValueError, match="at most 64"):
        BankPPOLearner([a] * 65, [c] * 65, hip, [1] * 65)
    with pytest.raises(ValueError, match="one critic per actor"):
        BankPPOLearner([a, a], [c], hip, [1, 1])
    with pytest.raises(ValueError, match="one shape"):
        BankPPOLearner([a, ActorNetwork(25, 128, 5)], [c, CriticNetwork(25, 5, 128, 1)], hip, [1, 1])
    with pytest.raises(ValueError, match="one shape"):
        BankPPOLearner([a, ActorNetwork(30, 128, 4)], [c, CriticNetwork(30, 4, 128, 1)], hip, [1, 1])
    with pytest.raises(ValueError, match="hidden-128"):
        BankPPOLearner([ActorNetwork(30, 512, 5)], [CriticNetwork(30, 5, 512, 1)], hip, [1])
    gi = gi_net(30, 5, 3)
    assert isinstance(gi, ActorCriticNetwork)
    with pytest.raises(ValueError, match="ActorCriticNetwork"):
        BankPPOLearner([gi], [gi], hip, [1])
    with pytest.raises(ValueError, match="on the device"):
        BankPPOLearner([a], [c], hip, [1])  # (CPU modules)
    with pytest.raises(ValueError, match="ActorNetwork and rollout.CriticNetwork"):
        BankPPOLearner([c], [a], hip, [1])


@pytest.mark.parametrize("name", sorted(U.LAYOUTS))
def test_scratch_query_is_the_sum_of_the_group_needs(name):
    rows, row_len, cols = U.LAYOUTS[name][:3]
    got = hip_library().policy_bank_train_scratch_bytes(rows, row_len, list(cols))
    assert got == U.scratch_need(rows, cols)
    # a group's rows and tiles are those of mm_policy_train on its n_k samples; only the partial blocks are a bound
    hip = hip_library()
    for k in range(len(cols) - 1):
        n_k = rows * (cols[k + 1] - cols[k])
        if n_k:
            t = U.tiles(n_k)
            per = max(2, -(-t // 512))
            own = 4 * 64 + abi.PBT_MEMBER_BYTES + 32 * t * abi.PBT_SAMPLE_BYTES + 8 * t + -(-t // per) * abi.PBT_PARTIAL_BYTES
            assert hip.policy_train_scratch_bytes(n_k) == own
            assert U.group_need(n_k) >= own - 4 * 64 - abi.PBT_MEMBER_BYTES


def test_scratch_query_grows_with_every_width():
    hip = hip_library()
    q = lambda rows, widths: hip.policy_bank_train_scratch_bytes(rows, sum(widths), [sum(widths[:k]) for k in range(len(widths) + 1)])  # noqa: E731
    for rows in (1, 7, 41):
        for base in ([0, 5, 1, 17], [64, 32], [800, 1], [1] * 64):
            for k in range(len(base)):
                last = q(rows, base)
                for extra in (1, 2, 31, 32, 33, 799, 800, 801, 1 << 14):  # across the 1 024-tile edge where the slicing changes
                    w = list(base)
                    w[k] += extra
                    now = q(rows, w)
                    assert now >= last, (rows, base, k, extra)
                    last = now
    # one width step by step across 1 024 -> 1 025 tiles (32 768 -> 32 800 samples)
    sizes = [q(1, [n]) for n in range(32 * 1020, 32 * 1030 + 1, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))


def test_raw_entries_refuse_on_the_host():
    """Refused calls enqueue nothing and dereference nothing: host arrays stand in for device memory."""
    hip = hip_library()
    lib = hip.lib
    out = C.c_uint64()
    cs = U.c_cols
    assert lib.mm_policy_bank_train_scratch_bytes(2, 5, 2, cs([0, 2, 5]), C.byref(out)) == abi.MM_OK
    for rows, row_len, K, cols in ((2, 5, 2, [1, 2, 5]), (2, 5, 2, [0, 3, 2]), (2, 5, 2, [0, 2, 4]), (-1, 5, 2, [0, 2, 5]),
                                   (2, 5, 0, [0, 2, 5]), (2, 5, 65, [0] * 65 + [5]), (1 << 20, 1 << 12, 1, [0, 1 << 12])):
        assert lib.mm_policy_bank_train_scratch_bytes(rows, row_len, K, cs(cols), C.byref(out)) == abi.MM_ERR_INVALID_ARG
    assert lib.mm_policy_bank_train_scratch_bytes(2, 5, 2, cs([0, 2, 5]), None) == abi.MM_ERR_INVALID_ARG
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    w = abi.MMMlpParams(p, p, p, p, p, p)
    ok = [p, 30, 2, 5, 30, p, 1, None, C.byref(w), C.byref(w), 2, cs([0, 2, 5]), 128, 5, p, p, None]
    for i, bad in ((4, 24), (4, 33), (12, 512), (13, 0), (13, 9), (10, 0), (10, 65), (1, 29), (0, None), (5, None), (14, None),
                   (15, None), (11, cs([0, 6, 5])), (11, None)):
        args = list(ok)
        args[i] = bad
        assert lib.mm_policy_bank_eval(*args) == abi.MM_ERR_INVALID_ARG, (i, bad)
    g = abi.MMOptGroup()
    g.algo, g.n_tensors = abi.OPT_RMSPROP, 1
    g.count[0], g.param[0], g.grad[0], g.state1[0] = 4, p, p, p
    g.lr, g.alpha_or_beta1, g.eps, g.max_grad_norm = 1e-3, 0.99, 1e-8, 0.5
    arr = (abi.MMOptGroup * 1)(g)
    for K in (0, 65):
        assert lib.mm_opt_step_bank(arr, 1, K, 0, None) == abi.MM_ERR_INVALID_ARG
        assert b"K" in lib.mm_last_error(None)
    assert lib.mm_opt_step_bank(arr, 0, 2, 0, None) == abi.MM_ERR_INVALID_ARG
    assert lib.mm_opt_step_bank(None, 1, 2, 0, None) == abi.MM_ERR_INVALID_ARG
    assert lib.mm_opt_step_bank(arr, 1, 2, 0b10, None) == abi.MM_ERR_INVALID_ARG  # a member blends and there is no target
    assert b"target" in lib.mm_last_error(None)


def test_kernel_resources(tmp_path):
    """The cross-compile gate of the new objects: zero VGPR spills, zero scratch, LDS within 160 KB, and
    profiles/policy_bank_train/kernel_resources.json records what the build gives."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_bank_train.o", "mm_opt_step_bank.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "bank", "--json", path,
                           os.path.join(csrc, "mm_policy_bank_train.o"), os.path.join(csrc, "mm_opt_step_bank.o")],
                          stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    sample = "mm::mfma::mlp_sample_kernel<%s, mm::bank_train::Group, mm::bank_train::SampleArgs, mm::bank_train::Tables>"  # kernel A
    assert set(now) == {"mm::bank_train::bank_frag_kernel", "mm::bank_train::bank_stats_kernel", "mm::bank_train::bank_stats_fold_kernel",
                        "mm::bank_train::bank_fold_kernel", sample % "false, false", sample % "true, false", sample % "false, true",
                        sample % "true, true", "mm::bank_train::bank_wgrad_kernel<false>",
                        "mm::bank_train::bank_wgrad_kernel<true>", "mm::opt::opt_step_bank_kernel"}
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0 and r["lds_B"] <= 160 * 1024, r
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_bank_train", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)
