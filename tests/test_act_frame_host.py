"""The act selects, the pose-code heading bits and the placed batch of tests/test_act_frame_gpu.py (CPU, oracle only).

Part 1 restates, statement for statement, the two code shapes that marl-mass_amd/csrc/mm_kernels.hip chooses between and
compares their results bit for bit:

  * MM_ACT_FRAME (kActSel): hl_act + controlled_act behind their `live` guards, and the same calls on a copy with `live`
    selecting the five fields they write -- every action on every lane, x at and either side of each hand-over point, y at the
    reach of bc0 / bc1, speeds on the rounding points of speed_to_index and a NaN, live and dead lanes, first and later sub-step;
  * MM_POSE_HBITS: relate()'s heading predicate read from the heading, and read from the two bits the owner of the pose put into
    its pose code (pose_hbits) -- h = + / - 0.037, their neighbours on either side, + / - 0, infinities and a NaN, for dy < 0,
    dy > 0, dy == + / - 0 and a NaN dy -- and against the reference's condition written out in Python.

The sine-frame block that gave the switch its name measured slower and is not in the tree, so there is
no frame to compile here; the oracle comparison of the act phase is the GPU test's.

Part 2 is the placed batch (the one of tests/test_combined_forms_host.py, in more shapes and with two more vehicles): what it
must hold is counted from the oracle's own planes, so that the GPU test cannot pass on a batch that lost a case:

  kb0          controlled vehicles whose target lane is the sine lane
  kb0_handover ... and that are past its end minus half a length (follow_road hands them on)
  off_kb0      controlled vehicles in the same env as a kb0 vehicle but on another lane
  dy_neg / dy_pos / dy_zero   ordered pairs of present vehicles by the sign of the partner's y minus the ego's
  h_pos / h_neg               vehicles whose heading is beyond + 0.037 / - 0.037 ...
  h_in_pos / h_in_neg         ... and inside (0, 0.037] / [- 0.037, 0)
  h_on_pos / h_on_neg         ... and exactly on + 0.037 / - 0.037
  h_carried    vehicles beyond either threshold at a step the caller did not edit (the carried pose code re-derives its bits)
  respawn      envs whose episode counter moves in the step after an edit
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_env
import test_combined_forms_host as P
import test_scan_selects_host as H
from marl_mass_amd import _cabi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <math.h>
/* marl-mass_amd/csrc/mm_device.h, mm_kernels.hip */
#define kVehLength 5.0
#define kLaneWidth 4.0
#define kTauA 0.6
enum { MM_LANE_AB0 = 0, MM_LANE_BC0, MM_LANE_BC1, MM_LANE_CD0, MM_LANE_JK0, MM_LANE_KB0 };
static double lane_sx(int l) { return l == 0 ? 0.0 : (l <= 2 ? 320.0 : (l == 3 ? 420.0 : (l == 4 ? 0.0 : 220.0))); }
static double lane_sy(int l) { return l == 2 ? 4.0 : (l == 4 ? 10.5 : (l == 5 ? 7.25 : 0.0)); }
static double lane_len(int l) { return l == 0 ? 320.0 : (l == 3 ? 1000.0 : (l == 4 ? 220.0 : 100.0)); }
static int lane_forbidden(int l) { return l == 2 || l >= 4; }
static int lane_road(int l) { return l == 0 ? 0 : (l <= 2 ? 1 : l - 1); }
static double clipd(double x, double a, double b) { return fmin(fmax(x, a), b); }
static int lane_reachable(int l, double x, double y) {
  if (lane_forbidden(l)) return 0;
  double s = x - lane_sx(l), r = y - lane_sy(l);
  return fabs(r) <= 2 * kLaneWidth && (0 <= s && s < lane_len(l) + kVehLength);
}
static int lane_after_end(int l, double x) { return (x - lane_sx(l)) > lane_len(l) - kVehLength / 2; }
static double lane_distance_straight(int l, double x, double y) { /* lane_distance for bc0 / bc1 (no sine) */
  double s = x - lane_sx(l), r = y - lane_sy(l);
  return fabs(r) + fmax(s - lane_len(l), 0.0) + fmax(0.0 - s, 0.0);
}
static int next_lane(int l, double x, double y) {
  if (l == MM_LANE_AB0 || l == MM_LANE_KB0)
    return lane_distance_straight(MM_LANE_BC0, x, y) <= lane_distance_straight(MM_LANE_BC1, x, y) ? MM_LANE_BC0 : MM_LANE_BC1;
  if (l == MM_LANE_JK0) return MM_LANE_KB0;
  return MM_LANE_CD0;
}
static int speed_to_index(double speed) {
  double x = (speed - 10) / 20.0;
  return (int)clipd(rint(x * (5 - 1)), 0, 5 - 1);
}
static double index_to_speed(int i) { return 10 + i * (30.0 - 10) / (5 - 1); }
typedef struct { double x, y, v, tspeed, act_acc; int tlane, sidx, hl; } Veh;
static void hl_act(Veh *v, int action) { /* KIND == MM_ENV_V1 */
  if (action >= 0) v->hl = action;
  if (action == 3 || action == 4) {
    int si = speed_to_index(v->v) + (action == 3 ? 1 : -1);
    v->sidx = si < 0 ? 0 : (si > 4 ? 4 : si);
    v->tspeed = index_to_speed(v->sidx);
  }
  if (lane_after_end(v->tlane, v->x)) v->tlane = next_lane(v->tlane, v->x, v->y);
  if (action == 2 || action == 0) {
    int cand = v->tlane;
    if (lane_road(v->tlane) == 1) cand = (action == 2) ? MM_LANE_BC1 : MM_LANE_BC0;
    if (lane_reachable(cand, v->x, v->y)) v->tlane = cand;
  }
}
static void controlled_act(Veh *v, int action) { /* STEER = false */
  if (lane_after_end(v->tlane, v->x)) v->tlane = next_lane(v->tlane, v->x, v->y);
  if (action == 2 || action == 0) {
    int cand = v->tlane;
    if (lane_road(v->tlane) == 1) cand = (action == 2) ? MM_LANE_BC1 : MM_LANE_BC0;
    if (lane_reachable(cand, v->x, v->y)) v->tlane = cand;
  }
  v->act_acc = (1 / kTauA) * (v->tspeed - v->v);
}
/* step_kernel's act phase in the kPrimary kernels: the guarded calls, and kActSel's copy + selects.
 * in: x, y, v, tspeed, act_acc; ints: tlane, sidx, hl, action, live, first sub-step; out: tspeed, act_acc, tlane, sidx, hl per form */
void af_act(const double *in, const int *ii, double *out, long n) {
  for (long i = 0; i < n; i++) {
    const int action = ii[6 * i + 3], live = ii[6 * i + 4], first = ii[6 * i + 5];
    for (int f = 0; f < 2; f++) {
      Veh v = {in[5 * i], in[5 * i + 1], in[5 * i + 2], in[5 * i + 3], in[5 * i + 4], ii[6 * i], ii[6 * i + 1], ii[6 * i + 2]};
      if (f == 0) {
        if (live) { if (first) hl_act(&v, action); }
        if (live) controlled_act(&v, -1);
      } else {
        Veh w = v;
        if (first) hl_act(&w, action);
        controlled_act(&w, -1);
        v.hl = live ? w.hl : v.hl; v.sidx = live ? w.sidx : v.sidx; v.tspeed = live ? w.tspeed : v.tspeed;
        v.tlane = live ? w.tlane : v.tlane; v.act_acc = live ? w.act_acc : v.act_acc;
      }
      double *o = out + 10 * i + 5 * f;
      o[0] = v.tspeed; o[1] = v.act_acc; o[2] = v.tlane; o[3] = v.sidx; o[4] = v.hl;
    }
  }
}
/* mm_kernels.hip: pose_hbits by the owner; relate()'s `head` as it reads the heading, and as relate<true> reads the bits */
#define kPoseHPos 0x200
#define kPoseHNeg 0x400
static int pose_hbits(double h) { return ((h > 0.037) ? kPoseHPos : 0) | ((h < -0.037) ? kPoseHNeg : 0); }
void af_hbits(const double *h, const double *dy, int *out /* bits, head (heading), head (bits) */, long n) {
  for (long i = 0; i < n; i++) {
    const double oh = h[i];
    const int opk = 0x1FF | pose_hbits(oh); /* (every other bit of the code set: the test reads its own bit only) */
    out[3 * i] = pose_hbits(oh);
    out[3 * i + 1] = (dy[i] < 0) ? (oh > 0.037) : (oh < -0.037);
    out[3 * i + 2] = (opk & ((dy[i] < 0) ? kPoseHPos : kPoseHNeg)) != 0;
  }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("act_frame")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                           "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(REPO, "include"), "-shared", "-o", str(so),
                           str(src), "-lm"])
    return C.CDLL(str(so))


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


KB0, AB, BC0, BC1, CD0, JK = 5, 0, 1, 2, 3, 4
SX = {AB: 0.0, BC0: 320.0, BC1: 320.0, CD0: 420.0, JK: 0.0, KB0: 220.0}
LEN = {AB: 320.0, BC0: 100.0, BC1: 100.0, CD0: 1000.0, JK: 220.0, KB0: 100.0}


def _near(x, k=6):
    out = [x]
    up = dn = x
    for _ in range(k):
        up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
        out += [up, dn]
    return out


def test_act_selects_write_what_the_guarded_calls_write(lib):
    """Every action, on every lane, with x at and either side of the lane's hand-over point and of the reach of bc0 / bc1, speeds
    on the rounding points of speed_to_index, for a live and a dead lane, in the first and in a later sub-step."""
    rows, ints = [], []
    speeds = [0.0, 9.99, 12.5, 17.5, float(np.nextafter(17.5, 0.0)), 22.5, 27.5, 30.0, 45.0, -45.0, float("nan")]
    for lane in (AB, BC0, BC1, CD0, JK, KB0):
        xs = _near(SX[lane] + LEN[lane] - 2.5, 2) + [SX[lane] + 10.0, SX[lane] - 1.0] + _near(320.0, 1) + _near(425.0, 1)
        for x in xs:
            for y in (0.0, 2.0, float(np.nextafter(2.0, 3.0)), 4.0, 8.0, float(np.nextafter(8.0, 9.0)), 10.5):
                for k, v in enumerate(speeds):
                    for action in range(5):
                        for live in (0, 1):
                            for first in (0, 1):
                                rows.append((x, y, v, 10.0 + 5.0 * (k % 5), 0.25))
                                ints.append((lane, k % 5, (action + 2) % 5, action, live, first))
    a, ii = np.array(rows, dtype=np.float64), np.array(ints, dtype=np.int32)
    out = np.empty(10 * len(rows))
    lib.af_act(_p(a), _p(ii, C.c_int), _p(out), C.c_long(len(rows)))
    out = out.reshape(-1, 2, 5)
    assert np.array_equal(_bits(out[:, 0]), _bits(out[:, 1]))
    live, first = ii[:, 4] != 0, ii[:, 5] != 0
    dead = ~live  # a dead lane keeps all five fields
    assert np.array_equal(_bits(out[dead, 1, 0]), _bits(a[dead, 3])) and np.array_equal(_bits(out[dead, 1, 1]), _bits(a[dead, 4]))
    assert np.array_equal(out[dead, 1, 2:].astype(np.int32), ii[dead, :3])
    # ... and the live lanes reach every branch: a changed target lane, speed index and hl action, follow_road
    assert (out[live, 1, 2] != ii[live, 0]).any() and (out[live & first, 1, 3] != ii[live & first, 1]).any()
    assert (out[live & first, 1, 4] == ii[live & first, 3]).all() and (out[live & ~first, 1, 4] == ii[live & ~first, 2]).all()
    assert {int(t) for t in out[live, 1, 2]} == {BC0, BC1, CD0, KB0, AB, JK}


def test_heading_bits_on_the_thresholds(lib):
    t = 0.037
    hs = []
    for c in (t, -t):
        hs += _near(c, 3)
    hs += [0.0, -0.0, 0.5, -0.5, 0.036, -0.036, float("nan"), float("inf"), float("-inf")]
    dys = [-1.0, 1.0, 0.0, -0.0, float("nan"), -1e-300, 1e-300]
    h = np.array([w for w in hs for _ in dys])
    dy = np.array([d for _ in hs for d in dys])
    out = np.empty(3 * len(h), dtype=np.int32)
    lib.af_hbits(_p(h), _p(dy), _p(out, C.c_int), C.c_long(len(h)))
    out = out.reshape(-1, 3)
    assert np.array_equal(out[:, 1], out[:, 2])
    with np.errstate(invalid="ignore"):
        want_bits = np.where(h > t, 0x200, 0) | np.where(h < -t, 0x400, 0)
        want_head = np.where(dy < 0, h > t, h < -t).astype(np.int32)  # decentral_layer.py:46-57
    assert np.array_equal(out[:, 0], want_bits) and np.array_equal(out[:, 1], want_head)
    assert set(out[:, 0].tolist()) == {0, 0x200, 0x400}
    assert not out[np.isnan(h)].any()  # a NaN heading: both predicates false
    on = (h == t) | (h == -t)
    assert on.any() and not out[on, 0].any()  # on a threshold: not beyond it
    assert out[(dy < 0) & (h > t), 1].all() and out[~(dy < 0) & (h < -t), 1].all() and out[:, 1].any() and not out[:, 1].all()


# ---- the placed batch ----------------------------------------------------------------------------------------------------------
# (E envs, N CAVs, shield): 8 x 8 one full wave, 16 x 8 two, 9 x 8 a second wave with one env (the ragged copy-out of the float32
# rows), 8 x 7 in 8-lane groups (N < G: the copy-out loop), 4- and 2-lane groups, HSS
CASES = {"E8_N8_mass": (8, 8, "mass"), "E16_N8_mass": (16, 8, "mass"), "E9_N8_mass": (9, 8, "mass"), "E8_N7_mass": (8, 7, "mass"),
         "E8_N4_mass": (8, 4, "mass"), "E8_N2_mass": (8, 2, "mass"), "E8_N8_hss": (8, 8, "hss")}
STEPS, SCRIPT_AT = P.STEPS, P.SCRIPT_AT


def kw(name, **more):
    d = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": H.SHIELDS[CASES[name][2]], "HEADWAY_TIME": 0.5},
             cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=False, auto_reset=True, seed=2718)
    d.update(more)
    return d


def script(env):
    """The caller's edit: the scenes of tests/test_combined_forms_host.py, and in env 7 two vehicles side by side on bc0 / bc1
    whose headings sit exactly on the two thresholds of relate() (+ 0.037 seen from the left, - 0.037 seen from the right)."""
    P.script(env)
    F, B = abi.F, abi.B
    for v, x, y, h, lane in ((0, 352.0, 0.2, 0.037, BC0), (1, 340.0, 3.9, -0.037, BC1)):
        env.f64[F["X"], 7, v] = x
        env.f64[F["Y"], 7, v] = y
        env.f64[F["HEADING"], 7, v] = h
        env.f64[F["SPEED"], 7, v] = 20.0
        env.f64[F["TARGET_SPEED"], 7, v] = 20.0
        env.u8[B["LANE"], 7, v] = lane
        env.u8[B["TARGET_LANE"], 7, v] = lane
        env.u8[B["CRASHED"], 7, v] = 0


def run(env, E, N):
    """Per step: the planes before it, the record after it and whether the step latched an error."""
    env.reset()
    tape = []
    for t, a in enumerate(P.actions(E, N)):
        if t in SCRIPT_AT:
            script(env)
        pre = {"u8": env.u8.detach().cpu().clone(), "f64": env.f64.detach().cpu().clone(), "env_i32": env.env_i32.detach().cpu().clone()}
        rec = H.snap(env, env.step(a.to(env.device)))
        try:
            env.poll_errors()
            latched = False
        except ValueError:
            latched = True
        tape.append({"pre": pre, "rec": rec, "latched": latched, "actions": a})
    return tape


@functools.lru_cache(maxsize=None)
def oracle_tape(name, obs_f64=False):
    """The oracle's run of a case, once (shared by the tests of both files; nothing changes it afterwards)."""
    E, N, _ = CASES[name]
    oracle_env.set_math_mode(1)
    try:
        return run(oracle_env.OracleEnv(E, N, **kw(name, obs_f64=obs_f64)), E, N)
    finally:
        oracle_env.set_math_mode(0)


def count_cases(tape):
    F, B = abi.F, abi.B
    n = dict.fromkeys(("kb0", "kb0_handover", "off_kb0", "dy_neg", "dy_pos", "dy_zero", "h_pos", "h_neg", "h_in_pos", "h_in_neg",
                       "h_on_pos", "h_on_neg", "h_carried", "respawn"), 0)
    for t, st in enumerate(tape):
        u8, f64 = st["pre"]["u8"], st["pre"]["f64"]
        ctrl = u8[B["KIND"]] == 1
        tlane = u8[B["TARGET_LANE"]].long()
        x, y, h = f64[F["X"]], f64[F["Y"]], f64[F["HEADING"]]
        on = ctrl & (tlane == KB0)
        n["kb0"] += int(on.sum())
        n["kb0_handover"] += int((on & ((x - 220.0) > 100.0 - 2.5)).sum())
        n["off_kb0"] += int((ctrl & ~on & on.any(1, keepdim=True)).sum())
        N = x.shape[1]
        pair = ctrl[:, :, None] & ctrl[:, None, :] & ~torch.eye(N, dtype=torch.bool)[None]
        dy = y[:, None, :] - y[:, :, None]
        n["dy_neg"] += int((pair & (dy < 0)).sum())
        n["dy_pos"] += int((pair & (dy > 0)).sum())
        n["dy_zero"] += int((pair & (dy == 0)).sum())
        n["h_pos"] += int((ctrl & (h > 0.037)).sum())
        n["h_neg"] += int((ctrl & (h < -0.037)).sum())
        n["h_on_pos"] += int((ctrl & (h == 0.037)).sum())
        n["h_on_neg"] += int((ctrl & (h == -0.037)).sum())
        n["h_in_pos"] += int((ctrl & (h > 0) & (h <= 0.037)).sum())
        n["h_in_neg"] += int((ctrl & (h < 0) & (h >= -0.037)).sum())
        if t not in SCRIPT_AT:
            n["h_carried"] += int((ctrl & (h.abs() > 0.037)).sum())
        if t in SCRIPT_AT:
            n["respawn"] += int((st["rec"]["env_i32"][abi.EP["EPISODE"]] != st["pre"]["env_i32"][abi.EP["EPISODE"]]).sum())
    return n


def test_the_placed_batch_holds_every_case():
    for name, (E, N, _) in CASES.items():
        tape = oracle_tape(name)
        c = count_cases(tape)
        print(name, c)
        for case, k in c.items():
            assert k >= 1, (name, case, c)
        assert [st["latched"] for st in tape] == [t in SCRIPT_AT for t in range(STEPS)], name  # the bad actions, and only they
        for t in SCRIPT_AT:  # the env with the crashed vehicle is done in the step after the edit and starts its next episode there
            st = tape[t]
            assert bool(st["rec"]["done"][3]) and int(st["rec"]["env_i32"][abi.EP["EPISODE"], 3]) == int(st["pre"]["env_i32"][abi.EP["EPISODE"], 3]) + 1
