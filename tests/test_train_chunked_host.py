"""The chunked gradient entries without a GPU: the exported symbols and the binding, the scratch layout restated on the host,
the resources of the new kernels, and the learners' refusal of a budget that no call can meet."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import oracle_env
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mm_policy_gi_train_chunked_scratch_bytes", "mm_policy_gi_train_chunked", "mm_policy_train_chunked_scratch_bytes",
           "mm_policy_train_chunked")

HDR = 64             # floats: the header, [0] the count of valid samples
MAX_SLICES = 512
# (floats of W2^T fragments, floats per sample row set, doubles of loss partial per tile, floats of a partial block, networks)
GI = dict(frag=5 * 4 * 4 * 64 * 4, row=2 * 160 + 2 * 128 + 16 + 32, sums=2, part=27952, nets=1)
PT = dict(frag=2 * 4 * 4 * 4 * 64 * 4, row=4 * 128 + 16 + 32, sums=2, part=26896, nets=2)  # (one loss partial per network)


def _hip():
    from marl_mass_amd import hip_library
    return hip_library()  # loading the library needs no GPU


def _layout_bytes(k, n, chunk):
    """include/mm_policy_*_train.h: header, fragments, the rows of `chunk` samples, the fp64 loss partials of ALL tiles, the
    partial blocks of one pass (2 tiles per slice up to 1024 tiles, at most 512), one fp64 accumulator block per network."""
    tiles_c = chunk // 32
    blocks = (tiles_c + 1) // 2 if tiles_c <= 2 * MAX_SLICES else MAX_SLICES
    floats = HDR + k["frag"] + chunk * k["row"] + 2 * k["sums"] * ((n + 31) // 32) + blocks * k["part"] + 2 * k["nets"] * k["part"]
    return 4 * floats


def test_exports_and_binding():
    raw = ctypes.CDLL(os.path.join(REPO, "marl-mass_amd", "csrc", "libmm_hip.so"))
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert s not in abi.CLib.SYMBOLS  # like the unchunked entries: not part of mm_abi.h's list or version
    hip = _hip()
    assert hip.has_policy_gi_train_chunked and hip.has_policy_train_chunked
    hip.require_policy_gi_train_chunked()
    hip.require_policy_train_chunked()
    # the unchunked entry's arguments, then the chunk
    assert hip.lib.mm_policy_gi_train_chunked.argtypes == list(hip.lib.mm_policy_gi_train.argtypes) + [ctypes.c_int64]
    assert hip.lib.mm_policy_train_chunked.argtypes == list(hip.lib.mm_policy_train.argtypes) + [ctypes.c_int64]
    ora = oracle_env.library()  # the oracle has no twin
    assert not ora.has_policy_gi_train_chunked and not ora.has_policy_train_chunked
    for call in (ora.require_policy_gi_train_chunked, ora.require_policy_train_chunked,
                 lambda: ora.policy_gi_train_chunked_scratch_bytes(64, 64), lambda: ora.policy_train_chunked_scratch_bytes(64, 64)):
        with pytest.raises(NotImplementedError):
            call()


@pytest.mark.parametrize("which", ["gi", "pt"])
def test_scratch_query(which):
    hip = _hip()
    k = GI if which == "gi" else PT
    query = hip.policy_gi_train_chunked_scratch_bytes if which == "gi" else hip.policy_train_chunked_scratch_bytes
    whole = hip.policy_gi_train_scratch_bytes if which == "gi" else hip.policy_train_scratch_bytes
    assert k["part"] == {"gi": 27952, "pt": 26896}[which] and 4 * k["row"] == {"gi": 2496, "pt": 2240}[which]
    for n in (0, 1, 31, 1000, 70001, 6553600, 2 ** 31 - 1):
        for chunk in (64, 128, 192, 1024, 16384, 32768, 32832, 65536, 524288):
            assert query(n, chunk) == _layout_bytes(k, n, chunk), (n, chunk)
    # monotone in the chunk (what the learner's search for the largest chunk under a budget relies on) and in n
    n = 6553600
    sizes = [query(n, 64 * m) for m in list(range(1, 40)) + [500, 511, 512, 513, 514, 1023, 1024, 1025, 1026, 2048, 8192, n // 64]]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert query(1000, 64) < query(70001, 64) < query(n, 64)
    # one agent step of the project's own workload (65 536 envs x 100 steps): the rows of a 524 288-sample pass instead of all
    assert whole(n) > 14e9 and query(n, 524288) < whole(n) / 10 and query(n, 64) < 5e6
    assert query(n, 524288) - query(524288, 524288) == 16 * (n - 524288) // 32  # all that grows with n: the loss partials
    for bad in ((1000, 0), (1000, 32), (1000, 100), (1000, -64), (-1, 64), (2 ** 31, 64), (1000, 2 ** 31)):
        with pytest.raises(ValueError):
            query(*bad)


def test_kernel_resources(tmp_path):
    """mm_policy_chunked.o holds the one accumulate kernel and one finish kernel per entry (the separate networks' as one
    template, instantiated for hidden 128 and 512), none spills or uses scratch memory, and
    profiles/train_chunked/kernel_resources.json records what the build gives.  (That the training objects still hold exactly
    their recorded kernels is test_kernel_resources of tests/test_policy_train_host.py and tests/test_policy_wide_train_host.py.)"""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_chunked.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(csrc, "mm_policy_chunked.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    assert sorted(now) == ["mm::chunked::policy_gi_train_chunked_finish_kernel",
                           "mm::chunked::policy_train_chunked_finish_kernel<mm::chunked::Pt128>",
                           "mm::chunked::policy_train_chunked_finish_kernel<mm::chunked::Pt512>",
                           "mm::chunked::train_chunked_accumulate_kernel"]
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_B"] == 0 and r["vgpr"] <= 64, r
        assert r["lds_B"] <= 2 * 256 * 8  # the loss tree of the finish kernels
    for name in now:
        if "policy_train_chunked_finish_kernel" in name:
            assert now[name]["lds_B"] <= 256 * 8  # one network's loss tree
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "train_chunked", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        assert rec[name]["object"] == "mm_policy_chunked.o"
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)


def test_learners_refuse_a_budget_below_one_pass():
    """The smallest pass is 64 samples; a budget below its scratch is refused when the learner is built -- before anything
    else is looked at, so the refusal needs no device."""
    from marl_mass_amd.learner import PPOLearner, SharedPPOLearner
    hip = _hip()
    gi_least, pt_least = hip.policy_gi_train_chunked_scratch_bytes(64, 64), hip.policy_train_chunked_scratch_bytes(64, 64)
    shared = ActorCriticNetwork(30, 5, 128, 1, state_split=True)
    actor, critic = ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1)
    for budget in (0, 1000, gi_least - 1):
        with pytest.raises(ValueError, match="scratch_budget_bytes"):
            SharedPPOLearner(shared, hip, scratch_budget_bytes=budget)
    for budget in (0, 1000, pt_least - 1):
        with pytest.raises(ValueError, match="scratch_budget_bytes"):
            PPOLearner(actor, critic, hip, scratch_budget_bytes=budget)
    # at the minimum the budget passes (what refuses these host-side networks then is that they are not on the device)
    with pytest.raises(ValueError, match="on the device"):
        SharedPPOLearner(shared, hip, scratch_budget_bytes=gi_least)
    with pytest.raises(ValueError, match="on the device"):
        PPOLearner(actor, critic, hip, scratch_budget_bytes=pt_least)
    with pytest.raises(NotImplementedError):  # a library without the chunked entries cannot serve a budget
        SharedPPOLearner(shared, oracle_env.library(), scratch_budget_bytes=gi_least)
