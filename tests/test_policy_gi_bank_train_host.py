"""The shared actor-critic bank's training half without a GPU: the header's constants against _cabi, the entries' presence in the
HIP library and their absence from the oracle, SharedBankPPOLearner's refusals that need no device, the scratch query against the
sum of the per-group needs and its monotonic growth, host-side refusals of the raw entries, and the new object's kernel
resources."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import oracle_env
import policy_gi_bank_train_util as U
from marl_mass_amd import _cabi as abi, hip_library
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mm_policy_gi_bank_eval", "mm_policy_gi_bank_train_scratch_bytes", "mm_policy_gi_bank_train")


def _define(text, name):
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


def test_header_constants_match_cabi():
    text = open(os.path.join(REPO, "include", "mm_policy_gi_bank_train.h")).read()
    for name, value, want in (("HEADER", abi.GBT_HEADER_BYTES, 1024), ("MEMBER", abi.GBT_MEMBER_BYTES, 5 * 4 * 4 * 64 * 16),
                              ("SAMPLE", abi.GBT_SAMPLE_BYTES, 4 * (2 * 160 + 2 * 128 + 16 + 32)), ("TILE", abi.GBT_TILE_BYTES, 8 * (2 + 3)),
                              ("PARTIAL", abi.GBT_PARTIAL_BYTES, 4 * 27952)):
        assert _define(text, "MM_GBT_%s_BYTES" % name) == value == want
    assert '#include "mm_policy_bank_train.h"' in text  # MM_PT_FORM_*
    for s in SYMBOLS:
        assert s + "(" in text


def test_hip_library_has_the_entries_and_the_learner_imports():
    raw = C.CDLL(os.path.join(REPO, "marl-mass_amd", "csrc", "libmm_hip.so"))
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert s not in abi.CLib.SYMBOLS  # not part of include/mm_abi.h's symbol list
    hip = hip_library()  # loading the library needs no GPU
    assert hip.has_policy_gi_bank_train and hip.has_policy_gi_train and hip.has_policy_gi_bank
    hip.require_policy_gi_bank_train()
    from marl_mass_amd.learner import SharedBankPPOLearner  # noqa: F401


def test_oracle_library_lacks_the_entries():
    lib = oracle_env.library()
    assert not lib.has_policy_gi_bank_train
    with pytest.raises(NotImplementedError, match="mm_policy_gi_bank_train"):
        lib.require_policy_gi_bank_train()
    with pytest.raises(NotImplementedError, match="mm_policy_gi_bank_train"):
        lib.policy_gi_bank_train_scratch_bytes(1, 1, [0, 1])


def test_learner_refusals_without_a_device():
    from marl_mass_amd.learner import BankPPOLearner, SharedBankPPOLearner
    hip = hip_library()
    one = ActorCriticNetwork(30, 5, 128, 1, state_split=True)
    with pytest.raises(ValueError, match="at least one member"):
        SharedBankPPOLearner([], hip, [])
    with pytest.raises(ValueError, match="at most 64"):
        SharedBankPPOLearner([one] * 65, hip, [1] * 65)
    with pytest.raises(ValueError, match="one shape"):
        SharedBankPPOLearner([one, ActorCriticNetwork(30, 4, 128, 1, state_split=True)], hip, [1, 1])
    for other in (ActorCriticNetwork(30, 5, 128, 1, state_split=False), ActorCriticNetwork(30, 5, 256, 1, state_split=True),
                  ActorNetwork(30, 128, 5)):
        with pytest.raises(ValueError, match=r"ActorCriticNetwork\(state_split=True\) members with hidden size 128"):
            SharedBankPPOLearner([one, other], hip, [1, 1])
    with pytest.raises(ValueError, match="on the device"):
        SharedBankPPOLearner([one], hip, [1])  # (a CPU module)
    with pytest.raises(ValueError, match="on the device"):
        SharedBankPPOLearner([ActorCriticNetwork(30, 5, 128, 1, state_split=True).double()], hip, [1])
    # BankPPOLearner points the caller here
    with pytest.raises(ValueError, match="ActorCriticNetwork.*SharedBankPPOLearner"):
        BankPPOLearner([one], [one], hip, [1])


@pytest.mark.parametrize("name", sorted(U.LAYOUTS))
def test_scratch_query_is_the_sum_of_the_group_needs(name):
    rows, row_len, cols = U.LAYOUTS[name][:3]
    hip = hip_library()
    assert hip.policy_gi_bank_train_scratch_bytes(rows, row_len, list(cols)) == U.scratch_need(rows, cols)
    # a group's rows and loss partials are those of mm_policy_gi_train on its n_k samples; the statistics (three fp64 per tile)
    # are the bank's own and the partial blocks a bound on that call's slices
    for k in range(len(cols) - 1):
        n_k = rows * (cols[k + 1] - cols[k])
        if n_k:
            t = U.tiles(n_k)
            per = max(2, -(-t // 512))
            slices = -(-t // per)
            own = 4 * 64 + abi.GBT_MEMBER_BYTES + 32 * t * abi.GBT_SAMPLE_BYTES + 16 * t + slices * abi.GBT_PARTIAL_BYTES
            assert hip.policy_gi_train_scratch_bytes(n_k) == own
            cap = min((t + 1) // 2, 512)
            assert cap >= slices
            assert U.group_need(n_k) - 24 * t - (cap - slices) * abi.GBT_PARTIAL_BYTES == own - 4 * 64 - abi.GBT_MEMBER_BYTES


def test_scratch_query_grows_with_every_width():
    hip = hip_library()
    q = lambda rows, widths: hip.policy_gi_bank_train_scratch_bytes(rows, sum(widths), [sum(widths[:k]) for k in range(len(widths) + 1)])  # noqa: E731
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
    """Refused calls enqueue nothing and dereference nothing: host arrays stand in for device memory, one bad argument at a
    time."""
    lib = hip_library().lib
    out = C.c_uint64()
    cs = U.c_cols
    assert lib.mm_policy_gi_bank_train_scratch_bytes(2, 5, 2, cs([0, 2, 5]), C.byref(out)) == abi.MM_OK
    assert out.value == U.scratch_need(2, [0, 2, 5])
    for rows, row_len, K, cols in ((2, 5, 2, [1, 2, 5]), (2, 5, 2, [0, 3, 2]), (2, 5, 2, [0, 2, 4]), (-1, 5, 2, [0, 2, 5]),
                                   (2, 5, 0, [0, 2, 5]), (2, 5, 65, [0] * 65 + [5]), (1 << 20, 1 << 12, 1, [0, 1 << 12])):
        assert lib.mm_policy_gi_bank_train_scratch_bytes(rows, row_len, K, cs(cols), C.byref(out)) == abi.MM_ERR_INVALID_ARG
    assert lib.mm_policy_gi_bank_train_scratch_bytes(2, 5, 2, cs([0, 2, 5]), None) == abi.MM_ERR_INVALID_ARG
    assert lib.mm_policy_gi_bank_train_scratch_bytes(2, 5, 2, None, C.byref(out)) == abi.MM_ERR_INVALID_ARG
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    w = abi.MMGiParams(*[p] * 12)
    holes = [abi.MMGiParams(*[None if i == j else p for i in range(12)]) for j in range(12)]
    # ---- eval: obs, obs_stride, rows, row_len, n_s, actions, act_stride, valid, bank, K, col_start, hidden, n_a, logp, value, stream
    ok = [p, 30, 2, 5, 30, p, 1, None, C.byref(w), 2, cs([0, 2, 5]), 128, 5, p, p, None]
    bad = [(4, 24), (4, 33), (11, 512), (12, 0), (12, 9), (9, 0), (9, 65), (1, 29), (0, None), (5, None), (8, None),
           (10, cs([0, 6, 5])), (10, cs([1, 2, 5])), (10, cs([0, 2, 4])), (10, None), (2, -1), (2, 1 << 31)]
    bad += [(8, C.byref(h)) for h in holes]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert lib.mm_policy_gi_bank_eval(*args) == abi.MM_ERR_INVALID_ARG, (i, v)
    args = list(ok)
    args[13] = args[14] = None  # no output
    assert lib.mm_policy_gi_bank_eval(*args) == abi.MM_ERR_INVALID_ARG
    args = list(ok)
    args[0], args[2], args[5] = None, 0, None  # n == 0: nothing is looked at, nothing is enqueued
    assert lib.mm_policy_gi_bank_eval(*args) == abi.MM_OK
    # ---- train: obs, obs_stride, rows, row_len, n_s, actions, act_stride, returns, ret_stride, old_logp, valid, bank, K, col_start,
    # hidden, n_a, clip, critic_loss, form, value_now, grads, loss, adv_sums, logp, value, ratio, scratch, scratch_bytes, stream
    big = (C.c_char * (U.scratch_need(2, [0, 2, 5]) + 16))()
    sp = (C.cast(big, C.c_void_p).value + 15) & ~15
    need = U.scratch_need(2, [0, 2, 5])
    ok = [p, 30, 2, 5, 30, p, 1, p, 1, p, None, C.byref(w), 2, cs([0, 2, 5]), 128, 5, 0.2, 0, 0, p, C.byref(w), p, None, None, None,
          None, sp, need, None]
    bad = [(4, 24), (4, 33), (14, 512), (15, 0), (15, 9), (12, 0), (12, 65), (1, 29), (0, None), (5, None), (7, None), (9, None),
           (11, None), (20, None), (21, None), (13, cs([0, 6, 5])), (13, None), (2, 1 << 31), (16, -0.5), (16, float("nan")), (17, 2),
           (17, -1), (18, 2), (18, -1), (19, None), (26, None), (26, sp + 4), (27, need - 1)]
    bad += [(11, C.byref(h)) for h in holes] + [(20, C.byref(h)) for h in holes]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert lib.mm_policy_gi_bank_train(*args) == abi.MM_ERR_INVALID_ARG, (i, v)
    args = list(ok)
    args[18] = abi.PT_FORM["per_sample"]  # value_now given in the per-sample form
    assert lib.mm_policy_gi_bank_train(*args) == abi.MM_ERR_INVALID_ARG


def test_kernel_resources(tmp_path):
    """The cross-compile gate of the new object: zero VGPR spills, zero scratch, LDS within 160 KB, and
    profiles/policy_gi_bank_train/kernel_resources.json records what the build gives."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_gi_bank_train.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(csrc, "mm_policy_gi_bank_train.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    ns = "mm::gi_bank_train::"
    assert set(now) == {ns + "gi_bank_frag_kernel", ns + "gi_bank_stats_kernel", ns + "gi_bank_stats_fold_kernel",
                        ns + "gi_bank_sample_kernel<false>", ns + "gi_bank_sample_kernel<true>", ns + "gi_bank_wgrad_kernel",
                        ns + "gi_bank_fold_kernel"}
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0 and r["lds_B"] <= 160 * 1024, r
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_gi_bank_train", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)
