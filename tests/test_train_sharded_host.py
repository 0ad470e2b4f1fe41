"""The rank-sharded gradient entries without a GPU: the exported symbols and the binding, the shard block's size against the
public headers, the resources of the kernels of mm_policy_sharded.o, the rank-ordered gather over two gloo ranks, and the learners' refusals."""
import ctypes
import datetime
import json
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle_env
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mm_policy_gi_train_shard_bytes", "mm_policy_gi_train_partial", "mm_policy_gi_train_finish",
           "mm_policy_train_shard_bytes", "mm_policy_train_partial", "mm_policy_train_finish")


def _hip():
    from marl_mass_amd import hip_library
    return hip_library()  # loading the library needs no GPU


def _define(header, name):
    text = open(os.path.join(REPO, "include", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_exports_and_binding():
    raw = ctypes.CDLL(os.path.join(REPO, "marl-mass_amd", "csrc", "libmm_hip.so"))
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert s not in abi.CLib.SYMBOLS  # optional, like the chunked entries: not part of mm_abi.h's list or version
    hip = _hip()
    assert hip.has_policy_gi_train_sharded and hip.has_policy_train_sharded
    hip.require_policy_gi_train_sharded()
    hip.require_policy_train_sharded()
    # partial: the chunked entry's arguments with (count, shard) in place of the gradients and the loss
    vp = ctypes.c_void_p
    a = list(hip.lib.mm_policy_gi_train_chunked.argtypes)
    assert hip.lib.mm_policy_gi_train_partial.argtypes == a[:16] + [vp, vp] + a[18:]
    a = list(hip.lib.mm_policy_train_chunked.argtypes)
    assert hip.lib.mm_policy_train_partial.argtypes == a[:18] + [vp, vp] + a[21:]
    ora = oracle_env.library()  # the oracle has no twin
    assert not ora.has_policy_gi_train_sharded and not ora.has_policy_train_sharded
    for call in (ora.require_policy_gi_train_sharded, ora.require_policy_train_sharded, ora.policy_gi_train_shard_doubles,
                 ora.policy_train_shard_doubles):
        with pytest.raises(NotImplementedError):
            call()


def test_block_sizes_are_the_headers():
    hip = _hip()
    gi, pt = _define("mm_policy_gi_train.h", "MM_GI_SHARD_DOUBLES"), _define("mm_policy_train.h", "MM_PT_SHARD_DOUBLES")
    assert gi == 4 + 2 + 27952 and pt == 4 + 2 + 2 * 26896  # header, loss sums, PartialBlock<5> | two PartialBlock<4>
    assert hip.policy_gi_train_shard_doubles() == gi and hip.policy_train_shard_doubles() == pt
    b = ctypes.c_uint64()
    assert hip.lib.mm_policy_gi_train_shard_bytes(ctypes.byref(b)) == abi.MM_OK and b.value == 8 * gi
    assert hip.lib.mm_policy_train_shard_bytes(ctypes.byref(b)) == abi.MM_OK and b.value == 8 * pt
    assert hip.lib.mm_policy_gi_train_shard_bytes(None) == abi.MM_ERR_INVALID_ARG
    assert hip.lib.mm_policy_train_shard_bytes(None) == abi.MM_ERR_INVALID_ARG


def test_kernel_resources(tmp_path):
    """mm_policy_sharded.o holds the shared network's header kernel, the separate networks' tail kernel at both hidden sizes and
    the finish kernel of the three families, none spills or uses scratch memory, all fit 64 VGPRs and are built for 256-thread
    workgroups, the only LDS is the loss trees of the header and tail kernels, and
    profiles/train_sharded/kernel_resources.json records what the build gives."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_sharded.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(csrc, "mm_policy_sharded.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    finish = ["mm::sharded::train_shard_finish_kernel<mm::%s>" % f for f in ("chunked::Pt128", "chunked::Pt512", "sharded::Gi")]
    assert sorted(now) == finish + ["mm::sharded::train_shard_header_kernel", "mm::sharded::train_shard_tail_kernel<mm::chunked::Pt128>",
                                    "mm::sharded::train_shard_tail_kernel<mm::chunked::Pt512>"]
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_B"] == 0 and r["vgpr"] <= 64, r
        assert r["lds_B"] <= 2 * 256 * 8  # the loss tree of the header kernel
    for name in now:
        if "tail_kernel" in name:
            assert now[name]["lds_B"] <= 256 * 8  # one network per workgroup
    for name in finish:
        assert now[name]["lds_B"] == 0
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "train_sharded", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        assert rec[name]["object"] == "mm_policy_sharded.o"
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)
    source = open(os.path.join(csrc, "mm_policy_sharded.hip")).read()
    assert source.count("__global__ __launch_bounds__(256)") == 3 and "atomicAdd" not in source  # header, tail<F>, finish<F>


def _gather_worker(rank, world, port, out_dir):
    sys.path.insert(0, REPO)
    from marl_mass_amd.learner import fold_rank_sums, gather_in_rank_order
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        block = torch.arange(7, dtype=torch.float64) + 100.0 * rank  # rank r's "block"
        packed = torch.tensor([[1e8, -3.0, 5.0], [1.0, -1e8, 7.0]], dtype=torch.float64)[rank]
        sub = dist.new_group([0, 1])
        out = {"blocks": gather_in_rank_order(block), "packed": gather_in_rank_order(packed, sub),
               "ints": gather_in_rank_order(torch.tensor([rank + 1], dtype=torch.int64)),
               "strided": gather_in_rank_order(torch.arange(12, dtype=torch.float64).reshape(3, 4)[:, rank])}
        out["sums"], out["count"] = fold_rank_sums(out["packed"], True)
        out["count_only"] = fold_rank_sums(out["packed"], False)
        torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gather_in_rank_order(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    want = torch.stack([torch.arange(7, dtype=torch.float64), torch.arange(7, dtype=torch.float64) + 100.0])
    assert torch.equal(a["blocks"], want) and a["blocks"].dtype == torch.float64  # row r is rank r's
    assert torch.equal(a["ints"], torch.tensor([[1], [2]])) and a["ints"].dtype == torch.int64
    assert torch.equal(a["strided"], torch.tensor([[0.0, 4.0, 8.0], [1.0, 5.0, 9.0]], dtype=torch.float64))
    for k in ("blocks", "packed", "ints", "strided", "sums", "count"):
        assert torch.equal(a[k], b[k]), k  # identical on both ranks
    # the float32 sums are added in rank order, the count is exact
    assert a["sums"].dtype == torch.float32 and a["count"].dtype == torch.int32 and int(a["count"]) == 12
    f = torch.float32
    assert torch.equal(a["sums"], torch.tensor([1e8, -3.0], dtype=f) + torch.tensor([1.0, -1e8], dtype=f))
    assert a["count_only"][0] is None and int(a["count_only"][1]) == 12


def test_learners_refuse_what_is_not_there():
    from marl_mass_amd.learner import PPOLearner, SharedPPOLearner
    hip = _hip()
    wide = ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 512, 1)
    with pytest.raises(ValueError, match="shard_group"):  # the wide entries are not sharded: refused before anything else
        PPOLearner(wide[0], wide[1], hip, shard_group="world")
    with pytest.raises(ValueError, match="on the device"):  # (without it, what refuses host-side networks is the device check)
        PPOLearner(wide[0], wide[1], hip)
    # a library without the entries cannot serve a shard group
    from marl_mass_amd.rollout import ActorCriticNetwork
    ora = oracle_env.library()
    with pytest.raises(NotImplementedError):
        SharedPPOLearner(ActorCriticNetwork(30, 5, 128, 1, state_split=True), ora, shard_group="world")
    with pytest.raises(NotImplementedError):
        PPOLearner(ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1), ora, shard_group="world")
