"""mm_policy_wide_train_partial / mm_policy_wide_train_finish (include/mm_policy_wide_train.h) without a GPU: the exported
symbols and the binding, the shard block's size against the public header as C, the resources of the entries' two kernels, and
what a hidden-512 learner with a shard group refuses."""
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
SYMBOLS = ("mm_policy_wide_train_shard_bytes", "mm_policy_wide_train_partial", "mm_policy_wide_train_finish")
SHARD_DOUBLES = 608294


def _hip():
    from marl_mass_amd import hip_library
    return hip_library()  # loading the library needs no GPU


def test_exports_and_binding():
    raw = ctypes.CDLL(os.path.join(CSRC, "libmm_hip.so"))
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert s not in abi.CLib.SYMBOLS  # optional, like the chunked entry: not part of mm_abi.h's list or version
    hip = _hip()
    assert hip.has_policy_wide_train_sharded
    hip.require_policy_wide_train_sharded()
    # the argument lists of the hidden-128 entries
    assert hip.lib.mm_policy_wide_train_partial.argtypes == list(hip.lib.mm_policy_train_partial.argtypes)
    assert hip.lib.mm_policy_wide_train_finish.argtypes == list(hip.lib.mm_policy_train_finish.argtypes)
    assert hip.lib.mm_policy_wide_train_shard_bytes.argtypes == list(hip.lib.mm_policy_train_shard_bytes.argtypes)
    # partial: the chunked entry's arguments with (count, shard) in place of the gradients and the loss
    vp = ctypes.c_void_p
    a = list(hip.lib.mm_policy_wide_train_chunked.argtypes)
    assert hip.lib.mm_policy_wide_train_partial.argtypes == a[:18] + [vp, vp] + a[21:]
    ora = oracle_env.library()  # the oracle has no twin
    assert not ora.has_policy_wide_train_sharded
    for call in (ora.require_policy_wide_train_sharded, ora.policy_wide_train_shard_doubles):
        with pytest.raises(NotImplementedError):
            call()


def test_block_size_is_the_headers(tmp_path):
    hip = _hip()
    assert U.PARTIAL_BYTES == 4 * 304144
    assert hip.policy_wide_train_shard_doubles() == 6 + 2 * U.PARTIAL_BYTES // 4 == SHARD_DOUBLES
    b = ctypes.c_uint64()
    assert hip.lib.mm_policy_wide_train_shard_bytes(ctypes.byref(b)) == abi.MM_OK and b.value == 8 * SHARD_DOUBLES == 4866352
    assert hip.lib.mm_policy_wide_train_shard_bytes(None) == abi.MM_ERR_INVALID_ARG
    # the header as C99: the three declarations, and the macro against the partial block it is made of
    cc = [os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "mm_policy_wide_train.h"\ntypedef void (*fn)(void);\n'
                    "fn entries[3] = {(fn)mm_policy_wide_train_shard_bytes, (fn)mm_policy_wide_train_partial, "
                    "(fn)mm_policy_wide_train_finish};\n")
    subprocess.check_call(cc + ["-c", "-o", str(tmp_path / "decl.o"), str(decl)])
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "mm_policy_wide_train.h"\nint main(void) {\n'
                   '  printf("%lld %lld\\n", (long long)MM_PW_SHARD_DOUBLES, (long long)(6 + 2 * (MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES / 4)));\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(cc + ["-o", exe, str(src)])
    assert [int(x) for x in subprocess.check_output([exe]).decode().split()] == [SHARD_DOUBLES, SHARD_DOUBLES]


def test_kernel_resources(tmp_path):
    """The hidden-512 entries' kernels in mm_policy_sharded.o -- the Pt512 instantiations of the tail kernel of `partial` and of
    the finish kernel -- neither spills or uses scratch memory, both fit 64 VGPRs, the only LDS is the tail's loss tree (one
    network per workgroup), and profiles/train_sharded/kernel_resources.json records what the build gives.  (The object's whole
    kernel list and its source: tests/test_train_sharded_host.py::test_kernel_resources.)"""
    subprocess.check_call(["make", "-C", CSRC, "mm_policy_sharded.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(CSRC, "mm_policy_sharded.o")], stdout=subprocess.DEVNULL)
    finish, tail = ("mm::sharded::train_shard_%s_kernel<mm::chunked::Pt512>" % k for k in ("finish", "tail"))
    now = {r["kernel"]: r for r in json.load(open(path))}
    assert sorted(k for k in now if "Pt512" in k) == [finish, tail]
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "train_sharded", "kernel_resources.json")))}
    for name in (finish, tail):
        r = now[name]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_B"] == 0 and r["vgpr"] <= 64, r
        assert r["lds_B"] <= 2 * 256 * 8  # the loss trees, 256 x 8 B per network
        assert rec[name]["object"] == "mm_policy_sharded.o"
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert r[k] == rec[name][k], (name, k)
    assert now[finish]["lds_B"] == 0
    source = open(os.path.join(CSRC, "mm_policy_sharded.hip")).read()
    assert "atomicAdd" not in source


def test_learner_construction():
    """A hidden-512 learner takes a shard group: what refuses these host-side networks is that they are not on the device, and
    the message says so about the argument; a library without the entries cannot serve a shard group."""
    from marl_mass_amd.learner import PPOLearner
    hip = _hip()
    pair = lambda: (ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 512, 1))  # noqa: E731
    with pytest.raises(ValueError, match="shard_group.*on the device"):
        PPOLearner(*pair(), hip, shard_group="world")
    least = hip.policy_wide_train_chunked_scratch_bytes(64, 64)
    with pytest.raises(ValueError, match="scratch_budget_bytes.*shard_group.*on the device"):
        PPOLearner(*pair(), hip, shard_group="world", scratch_budget_bytes=least)
    with pytest.raises(ValueError, match="^PPOLearner needs float32 networks on the device$"):  # with neither: as before
        PPOLearner(*pair(), hip)
    with pytest.raises(NotImplementedError):
        PPOLearner(*pair(), oracle_env.library(), shard_group="world")
