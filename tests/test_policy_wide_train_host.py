"""mm_policy_wide_train / mm_policy_wide_eval / PPOLearner at hidden 512 without a GPU: the binding surface and the scratch
arithmetic against the header's stated bytes, which networks the learner takes, the kernels' resources, the header as C, and
the input conditions of the GPU file's batches (host generators: they are properties of the seeds)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import oracle_env
import policy_wide_train_util as U
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork

REPO = U.REPO
CSRC = os.path.join(REPO, "marl-mass_amd", "csrc")
SYMBOLS = ("mm_policy_wide_train", "mm_policy_wide_eval", "mm_policy_wide_train_scratch_bytes")


def _hip():
    from marl_mass_amd import hip_library
    return hip_library()  # loading the library needs no GPU


def test_binding_surface():
    ora = oracle_env.library()
    assert not ora.has_policy_wide_train  # the oracle has no twin
    with pytest.raises(NotImplementedError):
        ora.require_policy_wide_train()
    with pytest.raises(NotImplementedError):
        ora.policy_wide_train_scratch_bytes(64)
    hip = _hip()
    assert hip.has_policy_wide_train and all(hasattr(hip.lib, s) for s in SYMBOLS)
    hip.require_policy_wide_train()
    assert not any(s in abi.CLib.SYMBOLS for s in SYMBOLS)
    # the hidden-128 entries' argument types: the two contracts differ in the hidden size alone
    assert list(hip.lib.mm_policy_wide_train.argtypes) == list(hip.lib.mm_policy_train.argtypes)
    assert list(hip.lib.mm_policy_wide_eval.argtypes) == list(hip.lib.mm_policy_eval.argtypes)
    assert list(hip.lib.mm_policy_wide_train_scratch_bytes.argtypes) == list(hip.lib.mm_policy_train_scratch_bytes.argtypes)
    with pytest.raises(ValueError):
        hip.policy_wide_train_scratch_bytes(-1)


def test_scratch_bytes_are_the_headers():
    """0 < b(0) < b(1000) < b(N); the per-sample part is the header's bytes per sample (of n rounded up to whole tiles, plus
    the 8-byte loss partial per tile), the partial blocks follow the header's slicing rule and stay within its bound."""
    hip = _hip()
    sizes = (0, 1, 31, 32, 33, 1000, U.N_WRAP, 524288, 2 ** 31 - 1)
    b = [hip.policy_wide_train_scratch_bytes(n) for n in sizes]
    assert 0 < b[0] and all(x <= y for x, y in zip(b, b[1:])) and b[0] < b[5] < b[6] < b[7]
    for n, got in zip(sizes, b):
        tiles, per, slices = U.slicing(n)
        assert slices <= U.MAX_SLICES
        assert got == U.FIXED_BYTES + tiles * U.TILE * U.ROW_BYTES + 8 * tiles + slices * U.PARTIAL_BYTES, n
        assert got - U.FIXED_BYTES - tiles * (U.TILE * U.ROW_BYTES + 8) <= U.MAX_SLICES * U.PARTIAL_BYTES
    assert U.ROW_BYTES == 8384 and U.PARTIAL_BYTES == 4 * 304144
    # whole-tile slices, the last one shorter, at the wrap size; its persistent loop wraps with a ragged last tile
    tiles, per, slices = U.slicing(U.N_WRAP)
    assert tiles > U.MAX_GRID * U.WAVES and U.N_WRAP % U.TILE and slices >= 2 and tiles % per


def test_header_compiles_as_c_and_states_the_constants(tmp_path):
    names = ["TILE", "WAVES", "MAX_GRID", "MAX_SLICES", "MIN_SLICE_TILES", "FIXED_BYTES", "ROW_BYTES", "PARTIAL_BYTES",
             "PARTIAL_MAX_BYTES", "SCRATCH_ALIGN"]
    cc = [os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include")]
    # the declarations, used (compiled, not linked: the entries live in libmm_hip.so)
    decl = tmp_path / "decl.c"
    decl.write_text('#include "mm_policy_wide_train.h"\ntypedef void (*fn)(void);\n'
                    "fn entries[3] = {(fn)mm_policy_wide_train, (fn)mm_policy_wide_eval, (fn)mm_policy_wide_train_scratch_bytes};\n")
    subprocess.check_call(cc + ["-c", "-o", str(tmp_path / "decl.o"), str(decl)])
    # the macros, through a host program
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "mm_policy_wide_train.h"\nint main(void) {\n'
                   + "".join('  printf("%s %%lld\\n", (long long)MM_POLICY_WIDE_TRAIN_%s);\n' % (k, k) for k in names)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "consts")
    subprocess.check_call(cc + ["-o", exe, str(src)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe]).decode().splitlines())}
    assert (got["TILE"], got["WAVES"], got["MAX_GRID"]) == (U.TILE, U.WAVES, U.MAX_GRID)
    assert (got["MAX_SLICES"], got["MIN_SLICE_TILES"], got["SCRATCH_ALIGN"]) == (U.MAX_SLICES, U.MIN_SLICE_TILES, 16)
    assert (got["FIXED_BYTES"], got["ROW_BYTES"], got["PARTIAL_BYTES"]) == (U.FIXED_BYTES, U.ROW_BYTES, U.PARTIAL_BYTES)
    assert got["PARTIAL_MAX_BYTES"] == U.MAX_SLICES * U.PARTIAL_BYTES


def test_learner_accepts_512_pairs_and_refuses_the_rest():
    """Device-free: a well-formed pair on the host gets as far as the device check (its shapes were accepted), every other
    pair is refused on its shapes."""
    from marl_mass_amd.learner import PPOLearner
    hip = _hip()
    for n_s, n_a in ((30, 5), (25, 1), (32, 8)):
        with pytest.raises(ValueError, match="on the device"):
            PPOLearner(ActorNetwork(n_s, 512, n_a), CriticNetwork(n_s, n_a, 512, 1), hip)
    with pytest.raises(ValueError, match="on the device"):  # and hidden 128 as before
        PPOLearner(ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1), hip)
    bad = [(ActorNetwork(30, 256, 5), CriticNetwork(30, 5, 256, 1)),    # hidden 256
           (ActorNetwork(30, 64, 5), CriticNetwork(30, 5, 64, 1)),      # hidden 64
           (ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 128, 1)),    # a 512 actor with a 128 critic
           (ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 512, 1)),    # and the reverse
           (ActorNetwork(30, 512, 5), CriticNetwork(30, 4, 512, 1)),    # different action counts
           (ActorNetwork(30, 512, 5), CriticNetwork(28, 5, 512, 1)),    # different state sizes
           (ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 512, 2))]    # two critic outputs
    for actor, critic in bad:
        with pytest.raises(ValueError, match="hidden size 128 or 512"):
            PPOLearner(actor, critic, hip)
    for actor, critic in ((ActorNetwork(30, 512, 9), CriticNetwork(30, 9, 512, 1)), (ActorNetwork(24, 512, 5), CriticNetwork(24, 5, 512, 1))):
        with pytest.raises(ValueError, match="state columns"):
            PPOLearner(actor, critic, hip)
    # the chunked entries are hidden-128 only
    with pytest.raises(ValueError, match="scratch_budget_bytes"):
        PPOLearner(ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 512, 1), hip, scratch_budget_bytes=1 << 30)
    with pytest.raises(ValueError, match="on the device"):  # (128 with a budget gets as far as the device check)
        PPOLearner(ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1), hip, scratch_budget_bytes=1 << 30)
    with pytest.raises(NotImplementedError):  # the oracle cannot serve it
        oracle_env.library().require_policy_wide_train()


def test_kernel_resources(tmp_path):
    """Every kernel of mm_policy_wide_train.o: zero VGPR spills, zero scratch, LDS within a CU's 160 KiB, and what
    profiles/policy_wide_train/kernel_resources.json records is what the build gives."""
    subprocess.check_call(["make", "-C", CSRC, "mm_policy_wide_train.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(CSRC, "mm_policy_wide_train.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    # prep, fold, sample x {actor, critic} x {train, eval} x {16-byte, 4-byte loads of fc2}, wgrad x {actor, critic}
    assert len(now) == 12 and all(k.startswith("mm::wt::policy_wide_") or "mm::wt::policy_wide_" in k for k in now), sorted(now)
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0, r
        assert r["lds_B"] <= 160 * 1024
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_wide_train", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)


def test_small_batches_need_no_redraw():
    """At n = 31 one redrawn sample is 3.2 %, over the cap: the seeds of those batches are chosen so that nobody is redrawn."""
    for n_s, seed in sorted(U.SMALL_SEEDS.items()):
        actor, critic = U.nets(n_s)
        assert U.batch_seed(U.SMALL_N, n_s) == seed
        assert U.draw_inputs(actor, critic, U.SMALL_N, n_s, 5, True, seed)[4] == 0


def test_knife_is_four_times_the_float32_preactivation_error():
    """KNIFE = 4 x the largest |z_float32_torch - z_float64| over the GPU file's batches, measured with the modules alone; the
    filter stays under its cap of 3 % on every one of them (asserted in draw_inputs)."""
    worst = 0.0
    for n, n_s, n_a, strided, seed in U.BATCHES:
        actor, critic = U.nets(n_s, n_a)
        obs, act, _, _, redrawn = U.draw_inputs(actor, critic, n, n_s, n_a, strided, seed)
        assert redrawn <= U.MAX_REDRAW_SHARE * n
        worst = max(worst, U.preactivation_error(actor, critic, obs, act))
    print("largest float32 pre-activation error %.3e, KNIFE %.3e" % (worst, U.KNIFE))
    assert 4.0 * worst <= U.KNIFE <= 4.0 * worst * 1.5 and U.MAX_REDRAW_SHARE == 0.03
    assert U.KNIFE < 1e-5  # (between the 5e-6 and 1e-5 rows of the share table: 1.2 % .. 2.6 % of the samples)
