"""mm_policy_wide_train_chunked (include/mm_policy_wide_train.h) without a GPU: the exported symbols and the binding, the size
query against a restatement of the header's sum, the header as C, the resources of the entry's two kernels, the learner's budget
floor at hidden 512, and the input conditions of the 6 208-sample batches of the GPU module (host generators: they are
properties of the seeds)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import oracle_env
import policy_wide_train_util as U
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork

REPO = U.REPO
CSRC = os.path.join(REPO, "marl-mass_amd", "csrc")
SYMBOLS = ("mm_policy_wide_train_chunked_scratch_bytes", "mm_policy_wide_train_chunked")

LOSS_BYTES = 16                    # per tile: one fp64 loss partial per network
ACC_BYTES = 2 * U.PARTIAL_BYTES    # one network's accumulator block: a double per float of a partial block

# (n, n_s, n_a, strided, seed) of the GPU module's batches that policy_wide_train_util.BATCHES does not list
BIG = [(6208, 30, 5, True, 6239), (6208, 30, 5, False, 6239), (6208, 25, 8, True, 6234)]


def _hip():
    from marl_mass_amd import hip_library
    return hip_library()  # loading the library needs no GPU


def blocks(chunk):
    """The partial blocks of the chunked scratch: the most slices any pass of at most `chunk` samples cuts."""
    return min(U.MAX_SLICES, chunk // 64)


def layout_bytes(n, chunk):
    """The header's sum: the fixed part, the rows of `chunk` samples, the loss partials of ALL tiles of both networks, the
    partial blocks of one pass, two accumulator blocks."""
    tiles = (n + U.TILE - 1) // U.TILE
    return U.FIXED_BYTES + chunk * U.ROW_BYTES + LOSS_BYTES * tiles + blocks(chunk) * U.PARTIAL_BYTES + 2 * ACC_BYTES


def test_exports_and_binding():
    raw = ctypes.CDLL(os.path.join(CSRC, "libmm_hip.so"))
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert s not in abi.CLib.SYMBOLS  # like the unchunked entry: not part of mm_abi.h's list or version
    hip = _hip()
    assert hip.has_policy_wide_train_chunked
    hip.require_policy_wide_train_chunked()
    # the unchunked entry's arguments, then the chunk
    assert hip.lib.mm_policy_wide_train_chunked.argtypes == list(hip.lib.mm_policy_wide_train.argtypes) + [ctypes.c_int64]
    assert hip.lib.mm_policy_wide_train_chunked_scratch_bytes.argtypes == list(hip.lib.mm_policy_train_chunked_scratch_bytes.argtypes)
    ora = oracle_env.library()  # the oracle has no twin
    assert not ora.has_policy_wide_train_chunked
    for call in (ora.require_policy_wide_train_chunked, lambda: ora.policy_wide_train_chunked_scratch_bytes(64, 64)):
        with pytest.raises(NotImplementedError):
            call()


def test_the_partial_region_holds_any_pass():
    """A pass of t tiles cuts slicing(32 t) slices; the region of `chunk` holds the most of any t <= chunk / 32 -- which is not
    always the full pass's: chunk 3136 cuts 33 slices, its possible last pass of 3072 samples cuts 48."""
    assert U.slicing(3136)[2] == 33 and U.slicing(3072)[2] == 48 and blocks(3136) == 48
    for chunk in list(range(64, 64 * 130, 64)) + [16384, 524288]:
        most = max(U.slicing(32 * t)[2] for t in range(1, min(chunk // 32, 4096) + 1))
        assert most <= blocks(chunk), chunk
        if chunk <= 64 * 130:
            assert most == blocks(chunk), chunk  # and no block more than that


def test_scratch_query():
    hip = _hip()
    query, whole = hip.policy_wide_train_chunked_scratch_bytes, hip.policy_wide_train_scratch_bytes
    assert U.ROW_BYTES == 8384 and U.PARTIAL_BYTES == 4 * 304144
    for n in (0, 1, 31, 1000, 6208, 6553600, 2 ** 31 - 1):
        for chunk in (64, 128, 3072, 3136, 16384, 524288):
            assert query(n, chunk) == layout_bytes(n, chunk), (n, chunk)
    # strictly monotone in the chunk (what the learner's search for the largest chunk under a budget relies on) and in n
    n = 6553600
    sizes = [query(n, 64 * m) for m in list(range(1, 60)) + [96, 97, 98, 99, 256, 8192, n // 64]]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert query(0, 64) < query(1, 64) < query(1000, 64) < query(6208, 64) < query(n, 64) < query(2 ** 31 - 1, 64)
    assert 10.7e6 < query(64, 64) < 10.9e6  # the smallest call: the fixed part and the two accumulators dominate
    # one agent step of the project's own workload (65 536 envs x 100 steps): the rows of a 524 288-sample pass instead of all
    assert whole(n) > 54e9 and query(n, 524288) < whole(n) / 10
    assert query(n, 524288) - query(524288, 524288) == LOSS_BYTES * (n - 524288) // 32  # all that grows with n: the loss partials
    for bad in ((1000, 0), (1000, 32), (1000, 100), (1000, -64), (-1, 64), (2 ** 31, 64), (1000, 2 ** 31)):
        with pytest.raises(ValueError):
            query(*bad)


def test_header_compiles_as_c_and_states_the_sum(tmp_path):
    cc = [os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "mm_policy_wide_train.h"\ntypedef void (*fn)(void);\n'
                    "fn entries[2] = {(fn)mm_policy_wide_train_chunked, (fn)mm_policy_wide_train_chunked_scratch_bytes};\n")
    subprocess.check_call(cc + ["-c", "-o", str(tmp_path / "decl.o"), str(decl)])
    pairs = [(0, 64), (64, 64), (6208, 3136), (6208, 3072), (6553600, 524288), (2 ** 31 - 1, 16384)]
    src = tmp_path / "sum.c"
    src.write_text('#include <stdio.h>\n#include "mm_policy_wide_train.h"\nint main(void) {\n'
                   '  printf("%lld %lld\\n", (long long)MM_POLICY_WIDE_TRAIN_CHUNKED_LOSS_BYTES, (long long)MM_POLICY_WIDE_TRAIN_ACC_BYTES);\n'
                   + "".join('  printf("%%llu\\n", (unsigned long long)MM_POLICY_WIDE_TRAIN_CHUNKED_BYTES(%dLL, %dLL));\n' % p for p in pairs)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "sum")
    subprocess.check_call(cc + ["-o", exe, str(src)])
    lines = subprocess.check_output([exe]).decode().split("\n")
    assert [int(x) for x in lines[0].split()] == [LOSS_BYTES, ACC_BYTES]
    hip = _hip()
    for (n, chunk), line in zip(pairs, lines[1:]):
        assert int(line) == layout_bytes(n, chunk) == hip.policy_wide_train_chunked_scratch_bytes(n, chunk), (n, chunk)


def test_kernel_resources(tmp_path):
    """The hidden-512 entry's kernels in mm_policy_chunked.o -- the accumulate kernel it shares with the hidden-128 entries and
    the Pt512 instantiation of the separate networks' finish kernel -- neither spills or uses scratch memory, and
    profiles/train_chunked/kernel_resources.json records what the build gives.  (The object's whole kernel list:
    tests/test_train_chunked_host.py::test_kernel_resources; that mm_policy_wide_train.o still holds exactly its recorded
    kernels: tests/test_policy_wide_train_host.py::test_kernel_resources.)"""
    subprocess.check_call(["make", "-C", CSRC, "mm_policy_chunked.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(CSRC, "mm_policy_chunked.o")], stdout=subprocess.DEVNULL)
    mine = ["mm::chunked::policy_train_chunked_finish_kernel<mm::chunked::Pt512>", "mm::chunked::train_chunked_accumulate_kernel"]
    now = {r["kernel"]: r for r in json.load(open(path))}
    assert sorted(k for k in now if "Pt512" in k or "accumulate" in k) == mine
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "train_chunked", "kernel_resources.json")))}
    for name in mine:
        r = now[name]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_B"] == 0 and r["vgpr"] <= 64, r
        assert r["lds_B"] <= 256 * 8  # the loss tree of the finish kernel
        assert rec[name]["object"] == "mm_policy_chunked.o"
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert r[k] == rec[name][k], (name, k)


def test_learner_budget_floor_at_512():
    """The smallest pass is 64 samples: a budget below the WIDE entry's scratch for it is refused by name when a hidden-512
    learner is built, before any device check -- also a budget the hidden-128 entry could serve.  At the floor what refuses
    these host-side networks is that they are not on the device, and the message says so about the argument."""
    from marl_mass_amd.learner import PPOLearner
    hip = _hip()
    wide_least, pt_least = hip.policy_wide_train_chunked_scratch_bytes(64, 64), hip.policy_train_chunked_scratch_bytes(64, 64)
    assert pt_least < wide_least
    pair = lambda: (ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 512, 1))  # noqa: E731
    for budget in (0, 1000, pt_least, (pt_least + wide_least) // 2, wide_least - 1):
        with pytest.raises(ValueError, match="scratch_budget_bytes=%d is below" % budget):
            PPOLearner(*pair(), hip, scratch_budget_bytes=budget)
    for budget in (wide_least, 1 << 30):
        with pytest.raises(ValueError, match="scratch_budget_bytes.*on the device"):
            PPOLearner(*pair(), hip, scratch_budget_bytes=budget)
    with pytest.raises(ValueError, match="^PPOLearner needs float32 networks on the device$"):  # without a budget: as before
        PPOLearner(*pair(), hip)
    with pytest.raises(NotImplementedError):  # a library without the chunked entry cannot serve a budget
        PPOLearner(*pair(), oracle_env.library(), scratch_budget_bytes=wide_least)


@pytest.mark.parametrize("n,n_s,n_a,strided,seed", BIG)
def test_big_batches_meet_the_filters_conditions(n, n_s, n_a, strided, seed):
    """The 6 208-sample batches are not in policy_wide_train_util.BATCHES: the filter stays under its cap on them (asserted in
    draw_inputs, again here) and KNIFE is at least four times their float32 pre-activation error."""
    assert seed == U.batch_seed(n, n_s)
    actor, critic = U.nets(n_s, n_a)
    obs, act, _, _, redrawn = U.draw_inputs(actor, critic, n, n_s, n_a, strided, seed)
    err = U.preactivation_error(actor, critic, obs, act)
    print("n %d n_s %d n_a %d %s: redraw share %.4f, 4 x float32 pre-activation error %.3e, KNIFE %.3e"
          % (n, n_s, n_a, "strided" if strided else "dense", redrawn / float(n), 4.0 * err, U.KNIFE))
    assert redrawn <= U.MAX_REDRAW_SHARE * n and U.MAX_REDRAW_SHARE == 0.03
    assert 4.0 * err <= U.KNIFE == 7e-6
