"""The relation word of a pose code (MM_RELATION_WORD, marl-mass_amd/csrc/mm_relation.h) and the placed batch of
tests/test_relation_word_gpu.py (CPU only).

Part 1 compiles mm_relation.h with the host compiler -- the header the kernels include, so the table is the one they use, not a
copy -- and compares, for all 8 x 8 (reader pair, owner pair) cases, the two bits the owner publishes for that reader with
is_adj_lane restated in Python as the oracle states it (oracle/mm_oracle.c, decentral_layer.py:23-39):

  adj_any   is_adj_lane(ego, other.lane) != 0 or is_adj_lane(other, ego.lane) != 0
  csel      is_adj_lane(ego, other.lane) == -1 or is_adj_lane(other, ego.lane) == 1     (which front corner of `other` counts)

and pair_index / the owner's select form (pose_relw) against the table.

Part 2 is the placed batch: 16 envs whose vehicles are put on every (lane, next lane) pair, once with both front corners on
their lane and once with a corner off it, so that every one of the 64 combinations occurs as (ego, neighbour within the
perception distance) with and without a corner bit in the neighbour's pose code.  The count is taken from the oracle's state
planes at the step that follows the caller's edit, with next_lane and the corner test restated here.
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_env
import test_scan_selects_host as H
from marl_mass_amd import _cabi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB, BC0, BC1, CD0, JK, KB0 = 0, 1, 2, 3, 4, 5
# the eight pairs next_lane admits, in the order of pair_index
PAIRS = ((AB, BC0), (BC0, CD0), (BC1, CD0), (CD0, CD0), (JK, KB0), (KB0, BC0), (AB, BC1), (KB0, BC1))

SHIM = r"""
#include "mm_relation.h"
extern "C" {
int rw_pairs(void) { return kRelPairs; }
int rw_shift(void) { return kRelShift; }
unsigned rw_word(int o) { return kRelTable.w[o]; }
int rw_pair_index(int lane, int nl) { return pair_index(lane, nl); }
int rw_pose_relw(int lane, int nl) { return pose_relw(lane, nl); }
int rw_pair_lane(int k) { return kRelPairLane[k]; }
int rw_pair_next(int k) { return kRelPairNext[k]; }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("relation_word")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O1", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "marl-mass_amd", "csrc"), "-shared", "-o", str(so), str(src)])
    return C.CDLL(str(so))


# ---- part 1: the table ----------------------------------------------------------------------------------------------------------
def lane_road(l):
    return 0 if l == AB else (1 if l <= BC1 else l - 1)


def lane_id(l):
    return 1 if l == BC1 else 0


def is_adj_lane(lane, nl, lane2):
    """oracle/mm_oracle.c is_adj_lane with the vehicle's next lane given."""
    if lane_road(lane) == lane_road(lane2) and abs(lane_id(lane) - lane_id(lane2)) == 1:
        return lane_id(lane) - lane_id(lane2)
    if lane_road(nl) == lane_road(lane2) and abs(lane_id(nl) - lane_id(lane2)) == 1:
        return lane_id(nl) - lane_id(lane2)
    return 0


def test_pair_index_numbers_the_eight_pairs(lib):
    assert lib.rw_pairs() == 8 and lib.rw_shift() == 11
    for k, (lane, nl) in enumerate(PAIRS):
        assert (lib.rw_pair_lane(k), lib.rw_pair_next(k)) == (lane, nl)
        assert lib.rw_pair_index(lane, nl) == k
    assert sorted(lib.rw_pair_index(lane, nl) for lane, nl in PAIRS) == list(range(8))


def test_table_against_is_adj_lane(lib):
    seen = set()
    for o, (olane, onl) in enumerate(PAIRS):
        word = lib.rw_word(o)
        assert word < 1 << 16
        for e, (elane, enl) in enumerate(PAIRS):
            v_a, a_v = is_adj_lane(elane, enl, olane), is_adj_lane(olane, onl, elane)
            want = (1 if (v_a != 0 or a_v != 0) else 0) | (2 if (v_a == -1 or a_v == 1) else 0)
            assert (word >> (2 * e)) & 3 == want, (e, o)
            seen.add(want)
        # the owner's select form gives the same word at its place in the pose code, and touches no other bit of it
        assert lib.rw_pose_relw(olane, onl) == word << 11
        assert lib.rw_pose_relw(olane, onl) & 0x7FF == 0 and lib.rw_pose_relw(olane, onl) >> 27 == 0
    assert seen == {0, 1, 3}  # nothing adjacent, adjacent with the right corner, adjacent with the left corner


# ---- part 2: the placed batch ---------------------------------------------------------------------------------------------------
CASES = {"E16_N8_mass": (16, 8, "mass"), "E16_N8_hss": (16, 8, "hss"), "E16_N4_mass": (16, 4, "mass"), "E16_N4_hss": (16, 4, "hss"),
         "E16_N2_mass": (16, 2, "mass"), "E16_N2_hss": (16, 2, "hss")}
STEPS, SCRIPT_AT, TAPE_SEED = 5, 2, 61
P_ACT = torch.tensor([0.15, 0.4, 0.15, 0.2, 0.1])  # LEFT, IDLE, RIGHT, FASTER, SLOWER

# pose of a vehicle on pair k with both front corners on its lane: (x, y, heading).  ab0 heading for bc1 (y > 2) and kb0 heading
# for bc0 (y <= 2) are off their lane's centre line by more than half a width, so they are turned until both corners are back
# on the lane.
ON_LANE = {0: (300.0, 0.0, 0.0), 1: (340.0, 0.0, 0.0), 2: (350.0, 4.0, 0.0), 3: (422.0, 0.0, 0.0), 4: (214.0, 10.5, 0.0),
           5: (317.0, 1.9, -0.9), 6: (290.0, 2.1, 0.9), 7: (270.0, 7.25, 0.0)}
# ... and with a front corner off the lane
OFF_LANE = {0: (300.0, -1.5, 0.0), 1: (340.0, -1.5, 0.0), 2: (350.0, 5.5, 0.0), 3: (422.0, -1.5, 0.0), 4: (214.0, 12.0, 0.0),
            5: (317.0, 1.0, 0.0), 6: (290.0, 3.5, 0.0), 7: (270.0, 9.0, 0.0)}
# cd0 begins 200 m behind the end of jk0: for the two to be neighbours one of them stands where its lane is not (x moved; its own
# corners are then off), once each way
MOVED = {"cd0": {3: 392.0}, "jk0": {4: 250.0}}


def _rows():
    """Per env of the first eight: (pairs by slot, poses, moved).  env 0 / 1: one vehicle per pair (the 56 combinations of two
    different pairs), env 2: the even pairs twice, env 3: the odd pairs twice (the 8 combinations of a pair with itself);
    envs 4 .. 7: the same with a corner off the lane.  Envs 8 .. 15 repeat 0 .. 7 with the slots in reverse order."""
    base = [([v for v in range(8)], "cd0"), ([v for v in range(8)], "jk0"), ([(2 * v) % 8 for v in range(8)], None),
            ([(2 * v + 1) % 8 for v in range(8)], None)]
    rows = [(p, ON_LANE, m) for p, m in base] + [(p, OFF_LANE, m) for p, m in base]
    return rows + [(p[::-1], poses, m) for p, poses, m in rows]


def scenes(N):
    """(env, vehicle, x, y, heading, lane) of the caller's edit for envs of N vehicles (the first N slots of each row)."""
    out = []
    for e, (pairs, poses, moved) in enumerate(_rows()):
        seen = {}
        for v, k in enumerate(pairs[:N]):
            x, y, h = poses[k]
            if moved is not None:
                x = MOVED[moved].get(k, x)
            x -= 7.0 * seen.get(k, 0)  # the second vehicle of a pair: 7 m behind the first
            seen[k] = seen.get(k, 0) + 1
            out.append((e, v, x, y, h, PAIRS[k][0]))
    return out


def script(env):
    F, B = abi.F, abi.B
    for e, v, x, y, h, lane in scenes(env.f64.shape[2]):
        env.f64[F["X"], e, v] = x
        env.f64[F["Y"], e, v] = y
        env.f64[F["HEADING"], e, v] = h
        env.f64[F["SPEED"], e, v] = 15.0
        env.f64[F["TARGET_SPEED"], e, v] = 15.0
        env.u8[B["LANE"], e, v] = lane
        env.u8[B["TARGET_LANE"], e, v] = lane
        env.u8[B["CRASHED"], e, v] = 0


def kw(name, **more):
    d = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": H.SHIELDS[CASES[name][2]], "HEADWAY_TIME": 0.5},
             cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=False, auto_reset=True, seed=1618)
    d.update(more)
    return d


def actions(E, N):
    g = torch.Generator().manual_seed(TAPE_SEED)
    return [torch.multinomial(P_ACT, E * N, True, generator=g).view(E, N).int() for _ in range(STEPS)]


def run(env, E, N, edit=script):
    """Per step: the planes before it and the record after it."""
    env.reset()
    tape = []
    for t, a in enumerate(actions(E, N)):
        if t == SCRIPT_AT:
            edit(env)
        pre = {"u8": env.u8.detach().cpu().clone(), "f64": env.f64.detach().cpu().clone()}
        tape.append({"pre": pre, "rec": H.snap(env, env.step(a.to(env.device)))})
    return tape


@functools.lru_cache(maxsize=None)
def oracle_tape(name):
    """The oracle's run of a case, once (shared by the tests of both files; nothing changes it afterwards)."""
    E, N, _ = CASES[name]
    oracle_env.set_math_mode(1)
    try:
        return run(oracle_env.OracleEnv(E, N, **kw(name)), E, N)
    finally:
        oracle_env.set_math_mode(0)


SX = {AB: 0.0, BC0: 320.0, BC1: 320.0, CD0: 420.0, JK: 0.0, KB0: 220.0}
SY = {AB: 0.0, BC0: 0.0, BC1: 4.0, CD0: 0.0, JK: 10.5, KB0: 7.25}
LEN = {AB: 320.0, BC0: 100.0, BC1: 100.0, CD0: 1000.0, JK: 220.0, KB0: 100.0}


def next_lane(lane, x, y):
    """road.py:67-109 as mm_device.h states it."""
    if lane in (AB, KB0):
        d = [abs(y - SY[l]) + max(x - 320.0 - 100.0, 0.0) + max(320.0 - x, 0.0) for l in (BC0, BC1)]
        return BC0 if d[0] <= d[1] else BC1
    return KB0 if lane == JK else CD0


def corner_bits(lane, x, y, h):
    """controller.py:257-267 + lane.on_lane of the two front corners: bit 0 the left one is off `lane`, bit 1 the right one."""
    clen, alpha = math.sqrt(1.0 + 6.25) + 0.0075, math.atan(2.0 / 5.0)
    cx = x + clen * math.cos(alpha + h)
    cyl, cyr = y - clen * math.sin(alpha + h) + 0.01, y - clen * math.sin(-alpha + h) + 0.01
    s = cx - SX[lane]
    off = 3.25 * math.sin(math.pi / 100.0 * s + math.pi / 2) if lane == KB0 else 0.0
    lon = -5.0 <= s < LEN[lane] + 5.0
    return (0 if (abs(cyl - SY[lane] - off) <= 2.0 and lon) else 1) | (0 if (abs(cyr - SY[lane] - off) <= 2.0 and lon) else 2)


def count_combinations(pre):
    """{(reader pair, owner pair, owner has a corner bit)}: ordered pairs of present vehicles of an env within 180 m."""
    F, B = abi.F, abi.B
    u8, f64 = pre["u8"], pre["f64"]
    E, N = u8.shape[1], u8.shape[2]
    seen = set()
    for e in range(E):
        veh = []
        for v in range(N):
            if int(u8[B["KIND"], e, v]) == 0:
                continue
            lane, x, y, h = int(u8[B["LANE"], e, v]), float(f64[F["X"], e, v]), float(f64[F["Y"], e, v]), float(f64[F["HEADING"], e, v])
            pair = (lane, next_lane(lane, x, y))
            assert pair in PAIRS, (e, v, pair)
            veh.append((PAIRS.index(pair), x, y, corner_bits(lane, x, y, h) != 0))
        for a, (ka, xa, ya, _) in enumerate(veh):
            for b, (kb, xb, yb, cb) in enumerate(veh):
                if a != b and (xb - xa) ** 2 + (yb - ya) ** 2 < 180.0 ** 2:
                    seen.add((ka, kb, cb))
    return seen


def test_the_placed_batch_holds_every_combination():
    for name in ("E16_N8_mass", "E16_N8_hss"):
        tape = oracle_tape(name)
        seen = count_combinations(tape[SCRIPT_AT]["pre"])
        missing = [(e, o, c) for e in range(8) for o in range(8) for c in (False, True) if (e, o, c) not in seen]
        assert not missing, (name, missing)
    # the smaller groups hold the first slots of the same rows: fewer combinations, with and without a corner bit, and in the
    # 4-lane groups the adjacent pair bc0 / bc1 both ways
    for name, least in (("E16_N4_mass", 24), ("E16_N2_mass", 8)):
        seen = count_combinations(oracle_tape(name)[SCRIPT_AT]["pre"])
        print(name, len(seen))
        assert len(seen) >= least, (name, len(seen))
        assert any(c for _, _, c in seen) and any(not c for _, _, c in seen), name
    seen = count_combinations(oracle_tape("E16_N4_mass")[SCRIPT_AT]["pre"])
    assert {(1, 2), (2, 1)} <= {(e, o) for e, o, _ in seen}


def test_the_shield_ran_on_the_placed_vehicles():
    """The classification that reads the word runs for vehicles with two history records: the edit comes after two steps, and
    the placed batch stays alive (no env of the first eight ended at the edit's step for want of vehicles)."""
    tape = oracle_tape("E16_N8_mass")
    B = abi.B
    assert int((tape[SCRIPT_AT]["pre"]["u8"][B["KIND"]] == 1).sum()) == 16 * 8
    for st in tape:
        assert torch.isfinite(st["rec"]["reward"]).all()
