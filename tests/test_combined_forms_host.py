"""The combined select forms of the fused step kernels (marl-mass_amd/csrc/mm_device.h: MM_TRIG_SELECTS, MM_ATAN_SELECTS,
MM_CORNER_SELECTS, MM_CLIP_SELECTS) on the host, and the placed batch of tests/test_combined_forms_gpu.py (CPU, oracle only).

Part 1 compiles include/mm_math.h for the host with the oracle's flags and compares, bit for bit and on the corners of each
function, the select forms (mmm_sin_sel, mmm_cos_sel, mmm_atan_ratio_sel / mmm_asin_w_sel) with the forms they replace and with
the oracle's own evaluation (mm_math_eval, orc_get_corner + orc_on_lane in math mode 1).  corner_flags and clip_actions live in
mm_kernels.hip; the shim restates both of their forms, statement for statement, as tests/test_sine_frame_host.py does for the
sine frame, and clip_actions is also compared with the reference's clip written out in Python.

Part 2 is the placed batch: what the caller writes into the state planes before steps 2 and 5 of 7, and what the batch must
then hold, counted from the oracle's own planes so that the GPU test cannot pass on a batch that lost a case:

  kb0        controlled vehicles on the sine lane (corner_flags' sine, lane_local's sine, the carried pose)
  handover   vehicles past the end of their lane minus half a length (follow_road hands them to the next lane)
  mid_lc     vehicles whose target lane is not their lane
  crashed    crashed vehicles that are present (clip_actions' first select; the env is done and re-spawns in the same launch)
  over/under speed above + 40 / below - 40 (second and third select)
  lc_hi/lo   speed_control's acceleration above + 6 / below - 12.5 (the lane-change clip at both ends)
  bad        actions outside 0..4 (latched, act as IDLE)
  respawn    envs whose episode counter moves in the step after an edit (n_merge / episode read in the prologue, written in the
             epilogue of the same launch)
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_env
import test_scan_selects_host as H
from marl_mass_amd import _cabi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <math.h>
#include "mm_math.h"
/* marl-mass_amd/csrc/mm_device.h */
static const double kPi = 3.141592653589793;
#define kSineAmp 3.25
#define kSinePuls (2 * kPi / (2 * 100.0))
#define kSinePhase (kPi / 2)
#define kVehLength 5.0
#define kLaneWidth 4.0
#define kMaxSpeed 40.0
#define kLcMaxAcc 6.0
#define kLcMinAcc -12.5
#define kCornerLen 2.7000824035672517
#define MM_LANE_KB0 5
static double lane_sx(int l) { return l == 0 ? 0.0 : (l <= 2 ? 320.0 : (l == 3 ? 420.0 : (l == 4 ? 0.0 : 220.0))); }
static double lane_sy(int l) { return l == 2 ? 4.0 : (l == 4 ? 10.5 : (l == 5 ? 7.25 : 0.0)); }
static double lane_len(int l) { return l == 0 ? 320.0 : (l == 3 ? 1000.0 : (l == 4 ? 220.0 : 100.0)); }
static double clipd(double x, double a, double b) { return fmin(fmax(x, a), b); }

void cf_trig(const double *x, double *out, long n) { /* out: sin, sin_sel, cos, cos_sel */
  for (long i = 0; i < n; i++) {
    out[4 * i] = mmm_sin(x[i]); out[4 * i + 1] = mmm_sin_sel(x[i]); out[4 * i + 2] = mmm_cos(x[i]); out[4 * i + 3] = mmm_cos_sel(x[i]);
  }
}
void cf_reduce(const double *x, double *r, int *q, long n) { for (long i = 0; i < n; i++) r[i] = mmm_reduce(x[i], &q[i]); }
void cf_atan_ratio(const double *num, const double *den, double *out, long n) { /* out: r, lo, r_sel, lo_sel */
  for (long i = 0; i < n; i++) {
    out[4 * i] = mmm_atan_ratio(num[i], den[i], &out[4 * i + 1]);
    out[4 * i + 2] = mmm_atan_ratio_sel(num[i], den[i], &out[4 * i + 3]);
  }
}
void cf_asin(const double *x, double *out, long n) { /* out: asin, w, asin_sel, w_sel */
  for (long i = 0; i < n; i++) {
    out[4 * i] = mmm_asin_w(x[i], &out[4 * i + 1]);
    out[4 * i + 2] = mmm_asin_w_sel(x[i], &out[4 * i + 3]);
  }
}
/* mm_kernels.hip corner_flags: out = flags of the form it replaces, flags of the select form, s, rL, rR */
void cf_corner(const double *pose /* x, y, h */, const int *lane_of, double *out, long n) {
  for (long i = 0; i < n; i++) {
    const double x = pose[3 * i], y = pose[3 * i + 1];
    const int lane = lane_of[i];
    double sh, ch;
    mmm_sincos(pose[3 * i + 2], &sh, &ch);
    double cx = x + (kCornerLen * mmm_cos_sum(MMM_CORNER_SIN, MMM_CORNER_COS, sh, ch));
    double cyL = y - (kCornerLen * mmm_sin_sum(MMM_CORNER_SIN, MMM_CORNER_COS, sh, ch)) + 0.01;
    double cyR = y - (kCornerLen * mmm_sin_sum(-MMM_CORNER_SIN, MMM_CORNER_COS, sh, ch)) + 0.01;
    double s = cx - lane_sx(lane);
    {
      double off = (lane == MM_LANE_KB0) ? kSineAmp * mmm_sin(kSinePuls * s + kSinePhase) : 0.0;
      int lon = (-kVehLength <= s && s < lane_len(lane) + kVehLength);
      double rL = cyL - lane_sy(lane), rR = cyR - lane_sy(lane);
      if (lane == MM_LANE_KB0) { rL = rL - off; rR = rR - off; }
      out[5 * i] = (!(fabs(rL) <= kLaneWidth / 2 + 0 && lon) ? 1 : 0) | (!(fabs(rR) <= kLaneWidth / 2 + 0 && lon) ? 2 : 0);
      out[5 * i + 2] = s; out[5 * i + 3] = rL; out[5 * i + 4] = rR;
    }
    {
      const int kb = lane == MM_LANE_KB0;
      double sn = 0.0;
      if (kb) sn = mmm_sin_sel(kSinePuls * s + kSinePhase);
      const double off = kb ? kSineAmp * sn : 0.0;
      const int lon = (-kVehLength <= s) & (s < lane_len(lane) + kVehLength);
      const double rL0 = cyL - lane_sy(lane), rR0 = cyR - lane_sy(lane);
      const double rL = kb ? rL0 - off : rL0, rR = kb ? rR0 - off : rR0;
      out[5 * i + 1] = (!((fabs(rL) <= kLaneWidth / 2 + 0) & lon) ? 1 : 0) | (!((fabs(rR) <= kLaneWidth / 2 + 0) & lon) ? 2 : 0);
    }
  }
}
/* mm_kernels.hip clip_actions: in = crashed, speed, act_steer, st_t, act_acc, lc_vehicle; out = act_steer, st_t, act_acc of
 * the form it replaces, then of the select form */
void cf_clip(const double *in, double *out, long n) {
  for (long i = 0; i < n; i++) {
    const int crashed = in[6 * i] != 0, lc = in[6 * i + 5] != 0;
    const double v = in[6 * i + 1];
    {
      double act_steer = in[6 * i + 2], st_t = in[6 * i + 3], act_acc = in[6 * i + 4];
      if (crashed) { act_steer = 0; st_t = 0; act_acc = -1.0 * v; }
      if (v > kMaxSpeed) act_acc = fmin(act_acc, 1.0 * (kMaxSpeed - v));
      else if (v < -kMaxSpeed) act_acc = fmax(act_acc, 1.0 * (kMaxSpeed - v));
      if (lc) act_acc = clipd(act_acc, kLcMinAcc, kLcMaxAcc);
      out[6 * i] = act_steer; out[6 * i + 1] = st_t; out[6 * i + 2] = act_acc;
    }
    {
      double act_steer = in[6 * i + 2], st_t = in[6 * i + 3], act_acc = in[6 * i + 4];
      const int cr = crashed != 0;
      act_steer = cr ? 0.0 : act_steer; st_t = cr ? 0.0 : st_t;
      double acc = cr ? -1.0 * v : act_acc;
      const double room = 1.0 * (kMaxSpeed - v);
      const int over = v > kMaxSpeed, under = !over & (v < -kMaxSpeed);
      const double a_lo = fmin(acc, room), a_hi = fmax(acc, room);
      acc = over ? a_lo : (under ? a_hi : acc);
      const double a_lc = clipd(acc, kLcMinAcc, kLcMaxAcc);
      act_acc = lc ? a_lc : acc;
      out[6 * i + 3] = act_steer; out[6 * i + 4] = st_t; out[6 * i + 5] = act_acc;
    }
  }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("combined_forms")
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


def _around(x, k=3):
    """x, its k neighbours on either side, and the negatives of all of them."""
    out = [x]
    up = dn = x
    for _ in range(k):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        out += [up, dn]
    return out + [-w for w in out]


def _oracle_math(fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    rc = oracle_env.library().lib.mm_math_eval(C.c_int32(fn), C.c_int32(len(x)), x.ctypes.data_as(C.c_void_p), None,
                                               y.ctypes.data_as(C.c_void_p), None)
    assert rc == 0
    return y


# ---- mmm_sin / mmm_cos ---------------------------------------------------------------------------------------------------------
def _trig_points():
    pts = []
    for k in range(-9, 10):  # the reduction boundaries (2k + 1) pi / 4 -- where rint(x 2/pi) steps -- and the quadrant centres k pi / 2
        pts += _around((2 * k + 1) * np.pi / 4, 4) + _around(k * np.pi / 2, 2)
    pts += _around(0.0, 2) + [0.0, -0.0, 1e-300, -1e-300, 0.3, -0.3, 1.2, -1.2, 2.5, -2.5, 4.0, -4.0, 5.5, -5.5]
    s = np.linspace(-500.0, 1500.0, 40001)  # the sine lane's phase over every s the kernels can meet
    pts += list(3.141592653589793 / 100.0 * s + 3.141592653589793 / 2)
    return np.array(pts, dtype=np.float64)


def test_sin_cos_select_forms(lib):
    x = _trig_points()
    out = np.empty(4 * len(x))
    lib.cf_trig(_p(x), _p(out), C.c_long(len(x)))
    out = out.reshape(-1, 4)
    assert np.array_equal(_bits(out[:, 0]), _bits(out[:, 1])) and np.array_equal(_bits(out[:, 2]), _bits(out[:, 3]))
    assert np.array_equal(_bits(out[:, 1]), _bits(_oracle_math(0, x))) and np.array_equal(_bits(out[:, 3]), _bits(_oracle_math(1, x)))
    r, q = np.empty_like(x), np.empty(len(x), dtype=np.int32)
    lib.cf_reduce(_p(x), _p(r), _p(q, C.c_int), C.c_long(len(x)))
    for quad in range(4):  # all four quadrants, each with arguments of either sign
        assert ((q == quad) & (x > 0)).any() and ((q == quad) & (x < 0)).any(), quad
    for k in range(-9, 10):  # either side of each reduction boundary: the quadrant steps between the neighbours
        b = (2 * k + 1) * np.pi / 4
        near = np.abs(x - b) < 1e-14
        assert len(set(q[near].tolist())) == 2, k


# ---- mmm_atan_ratio ------------------------------------------------------------------------------------------------------------
def test_atan_ratio_select_chain(lib):
    num, den = [], []
    for d in (1.0, 0.7, 3.0, 1e-3, 123.456):
        for bp in (0.125, 0.375, 0.625, 0.875):  # every breakpoint of j, exactly on it and either side
            t = bp * d
            for w in _around(t, 3)[:7]:
                num.append(w); den.append(d)
        num += [0.0, -0.0, d, np.nextafter(d, 0.0), 0.5 * d, 0.25 * d, 0.75 * d]
        den += [d] * 7
    num, den = np.array(num), np.array(den)
    out = np.empty(4 * len(num))
    lib.cf_atan_ratio(_p(num), _p(den), _p(out), C.c_long(len(num)))
    out = out.reshape(-1, 4)
    assert np.array_equal(_bits(out[:, 0]), _bits(out[:, 2])) and np.array_equal(_bits(out[:, 1]), _bits(out[:, 3]))
    j = (num >= 0.125 * den).astype(int) + (num >= 0.375 * den) + (num >= 0.625 * den) + (num >= 0.875 * den)
    assert set(j.tolist()) == {0, 1, 2, 3, 4}
    lo_of = {0: 0.0, 1: float.fromhex("0x1.8ab6e3cf7afbdp-57"), 2: float.fromhex("0x1.a2b7f222f65e2p-56"),
             3: float.fromhex("0x1.2419a87f2a458p-56"), 4: float.fromhex("0x1.1a62633145c07p-55")}
    assert np.array_equal(_bits(out[:, 3]), _bits(np.array([lo_of[int(k)] for k in j])))  # the chain picks the entry of j


def test_asin_select_chain_on_the_inversion_boundary_and_zeros(lib):
    x = []
    for c in (np.sqrt(0.5), 0.125, 0.375, 0.625, 0.875, 1.0, 0.5, 0.99):  # sqrt(1/2): y <= w flips (the inversion); the rest: j
        x += _around(c, 4)
    x += [0.0, -0.0, 1e-310, -1e-310, 1.0, -1.0]
    x += list(np.linspace(-1.0, 1.0, 20001))
    x = np.clip(np.array(x), -1.0, 1.0)
    out = np.empty(4 * len(x))
    lib.cf_asin(_p(x), _p(out), C.c_long(len(x)))
    out = out.reshape(-1, 4)
    assert np.array_equal(_bits(out[:, 0]), _bits(out[:, 2])) and np.array_equal(_bits(out[:, 1]), _bits(out[:, 3]))
    assert np.array_equal(_bits(out[:, 2]), _bits(_oracle_math(4, x)))
    w = out[:, 1]
    assert (np.abs(x) <= w).any() and (np.abs(x) > w).any()  # both sides of the inversion
    z = out[np.array([np.signbit(v) and v == 0 for v in x])]
    assert len(z) and np.signbit(z[:, 0]).all() == np.signbit(z[:, 2]).all()


# ---- corner_flags --------------------------------------------------------------------------------------------------------------
KB0, AB = 5, 0


def _corner(lib, pose, lanes):
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    lanes = np.ascontiguousarray(lanes, dtype=np.int32)
    out = np.empty(5 * len(lanes))
    lib.cf_corner(_p(pose), _p(lanes, C.c_int), _p(out), C.c_long(len(lanes)))
    return out.reshape(-1, 5)


def _scan(lib, lane, base, axis, col, target, transform=lambda w: w):
    """Poses around `base` (moved along `axis` in steps of one ulp) whose derived value `col` is below, on and above `target`."""
    poses, v = [], base[axis]
    lo = hi = v
    for _ in range(400):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        for w in (lo, hi):
            p = list(base); p[axis] = w; poses.append(p)
    poses.append(list(base))
    val = transform(_corner(lib, poses, [lane] * len(poses))[:, col])
    assert (val < target).any() and (val > target).any(), (lane, axis, target)
    return poses, val


def test_corner_flags_select_form(lib):
    oracle_env.set_math_mode(1)
    try:
        L = oracle_env.library().lib
        c = 2.7000824035672517 * float.fromhex("0x1.db614bfce6a6ap-1")  # the corner's x offset at heading 0
        cyo = 2.7000824035672517 * float.fromhex("0x1.7c4dd663ebb88p-2")
        cases, exact = [], 0
        for lane, sx, sy, ln in ((AB, 0.0, 0.0, 320.0), (KB0, 220.0, 7.25, 100.0)):
            for target in (-5.0, ln + 5.0):  # s at -L and at len + L, either side of each
                poses, s = _scan(lib, lane, [target + sx - c, sy, 0.0], 0, 2, target)
                exact += int((s == target).any())
                cases += [(p, lane) for p in poses]
            # |r| at the half width, from inside and from outside, for the left and the right corner
            for col, yc in ((3, 2.0 + cyo - 0.01), (3, -2.0 + cyo - 0.01), (4, 2.0 - cyo - 0.01), (4, -2.0 - cyo - 0.01)):
                x0 = sx + 50.0 - c  # kb0 at s = 50: the sine's offset is 3.25 cos(pi / 2) ~ 0
                poses, r = _scan(lib, lane, [x0, sy + yc, 0.0], 1, col, 2.0, np.abs)
                if lane == AB:
                    exact += int((r == 2.0).any())
                cases += [(p, lane) for p in poses]
            rs = np.random.RandomState(5)
            for _ in range(400):  # headings, and corners well inside and well outside
                cases.append(([sx + rs.uniform(-8.0, ln + 8.0), sy + rs.uniform(-3.5, 3.5), rs.uniform(-0.6, 0.6)], lane))
        assert exact >= 4  # on the straight lane the exact values are reached: s == -L, s == len + L, |rL| == |rR| == width / 2
        out = _corner(lib, [p for p, _ in cases], [l for _, l in cases])
        assert np.array_equal(out[:, 0], out[:, 1])
        assert set(out[:, 1].astype(int).tolist()) == {0, 1, 2, 3}
        want = []
        for p, lane in cases:  # the oracle: on_lane of get_corner("L") / ("R")
            bitsum = 0
            for d in (0, 1):
                cx, cy = C.c_double(), C.c_double()
                L.orc_get_corner(p[0], p[1], p[2], d, C.byref(cx), C.byref(cy))
                bitsum |= (0 if L.orc_on_lane(lane, cx.value, cy.value) else 1) << d
            want.append(bitsum)
        assert np.array_equal(out[:, 1].astype(int), np.array(want))
    finally:
        oracle_env.set_math_mode(0)


# ---- clip_actions --------------------------------------------------------------------------------------------------------------
def _ref_clip(crashed, v, steer, acc, lc):
    """kinematics.py:143-152 clip_actions, then MDPLCVehicle's clip (safe_controller.py:100-104)."""
    if crashed:
        steer, acc = 0.0, -1.0 * v
    if v > 40.0:
        acc = min(acc, 1.0 * (40.0 - v))
    elif v < -40.0:
        acc = max(acc, 1.0 * (40.0 - v))
    if lc:
        acc = float(np.clip(acc, -12.5, 6.0))
    return steer, acc


def test_clip_actions_select_form(lib):
    rows = []
    speeds = _around(40.0, 2) + [0.0, 12.0, 39.0, 45.0, -45.0, 60.0, -60.0]
    accs = _around(6.0, 2)[:5] + _around(-12.5, 2)[:5] + [0.0, -0.0, 3.0, -3.0, 33.0, -33.0, 100.0, -100.0]
    for crashed in (0, 1):
        for lc in (0, 1):
            for v in speeds:
                for acc in accs:
                    rows.append([crashed, v, 0.2, 0.11, acc, lc])
    a = np.array(rows, dtype=np.float64)
    out = np.empty(6 * len(a))
    lib.cf_clip(_p(a), _p(out), C.c_long(len(a)))
    out = out.reshape(-1, 6)
    assert np.array_equal(_bits(out[:, :3]), _bits(out[:, 3:]))
    for r, o in zip(rows, out):
        steer, acc = _ref_clip(r[0], r[1], r[2], r[4], r[5])
        assert o[3] == steer and _bits(np.array([o[5]]))[0] == _bits(np.array([acc]))[0], r
        assert o[4] == (0.0 if r[0] else 0.11)
    crashed, v, lc = a[:, 0] != 0, a[:, 1], a[:, 5] != 0
    for name, m in (("crashed", crashed), ("over", v > 40.0), ("under", v < -40.0), ("lc_hi", lc & (out[:, 5] == 6.0)),
                    ("lc_lo", lc & (out[:, 5] == -12.5))):
        assert m.any(), name


# ---- the placed batch ----------------------------------------------------------------------------------------------------------
# (E envs, N CAVs, shield): 8 x 8 is one wave with every lane of it, 16 x 8 two waves; 4- and 2-lane groups; HSS
CASES = {"E8_N8_mass": (8, 8, "mass"), "E16_N8_mass": (16, 8, "mass"), "E8_N4_mass": (8, 4, "mass"), "E8_N2_mass": (8, 2, "mass"),
         "E8_N8_hss": (8, 8, "hss")}
STEPS, SCRIPT_AT, TAPE_SEED = 7, (2, 5), 71
BC0, BC1, CD0 = 1, 2, 3
_kb0_y = lambda x: 7.25 + 3.25 * np.cos(np.pi / 100.0 * (x - 220.0))  # noqa: E731
_kb0_h = lambda x: float(np.arctan(-3.25 * np.pi / 100.0 * np.sin(np.pi / 100.0 * (x - 220.0))))  # noqa: E731


def scenes(N):
    """(env, vehicle, x, y, heading, speed, target speed, lane, target lane, crashed); vehicles 0 and 1 of envs 0 .. 5 (every
    shape holds them), the rest of the env drives on."""
    rows = [
        (0, 0, 270.0, float(_kb0_y(270.0)), _kb0_h(270.0), 20.0, 20.0, KB0, KB0, 0),  # mid sine lane
        (0, 1, 318.0, float(_kb0_y(318.0)), _kb0_h(318.0), 20.0, 20.0, KB0, KB0, 0),  # its end: hand-over kb0 -> bc1
        (1, 0, 318.5, 0.0, 0.0, 22.0, 20.0, AB, AB, 0),                               # hand-over ab -> bc
        (1, 1, 419.0, 0.0, 0.0, 22.0, 20.0, BC0, BC0, 0),                             # hand-over bc0 -> cd
        (2, 0, 350.0, 2.2, -0.08, 20.0, 20.0, BC1, BC0, 0),                           # mid lane change, merging
        (2, 1, 385.0, 1.7, 0.08, 21.0, 20.0, BC0, BC1, 0),                            # ... and the other way
        (3, 0, 150.0, 0.0, 0.0, 12.0, 20.0, AB, AB, 1),                               # crashed (the env is done: re-spawn)
        (3, 1, 100.0, 0.0, 0.0, 45.0, 30.0, AB, AB, 0),                               # speed above + max
        (4, 0, 200.0, 0.0, 0.0, -45.0, 10.0, AB, AB, 0),                              # speed below - max (x decreases: literal sweep)
        (4, 1, 120.0, 0.0, 0.0, 10.0, 30.0, AB, AB, 0),                               # LC clip at + 6
        (5, 0, 240.0, 0.0, 0.0, 30.0, 10.0, AB, AB, 0),                               # LC clip at - 12.5
        (5, 1, 150.0, 10.5, 0.0, 18.0, 20.0, 4, 4, 0),                                # on the ramp jk
    ]
    return [r for r in rows if r[1] < N]


def script(env):
    F, B = abi.F, abi.B
    for e, v, x, y, h, speed, tspeed, lane, tlane, crashed in scenes(env.f64.shape[2]):
        env.f64[F["X"], e, v] = x
        env.f64[F["Y"], e, v] = y
        env.f64[F["HEADING"], e, v] = h
        env.f64[F["SPEED"], e, v] = speed
        env.f64[F["TARGET_SPEED"], e, v] = tspeed
        env.u8[B["LANE"], e, v] = lane
        env.u8[B["TARGET_LANE"], e, v] = tlane
        env.u8[B["CRASHED"], e, v] = crashed


def actions(E, N):
    """Random actions; at the scripted steps env 6 holds two actions outside 0 .. 4 (one above, one below)."""
    tape = H.actions(E, N, steps=STEPS, seed=TAPE_SEED)
    for t in SCRIPT_AT:
        tape[t][6, 0] = 7
        tape[t][6, 1] = -1
    return tape


def kw(name, **more):
    E, N, shield = CASES[name]
    d = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": H.SHIELDS[shield], "HEADWAY_TIME": 0.5},
             cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=True, auto_reset=True, seed=2718)
    d.update(more)
    return d


def run(env, E, N, polled=None):
    """Per step: the planes before it, the record after it and whether the step latched an error."""
    env.reset()
    tape = []
    for t, a in enumerate(actions(E, N)):
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
def oracle_tape(name):
    E, N, _ = CASES[name]
    oracle_env.set_math_mode(1)
    try:
        return run(oracle_env.OracleEnv(E, N, **kw(name)), E, N)
    finally:
        oracle_env.set_math_mode(0)


def count_cases(tape):
    F, B = abi.F, abi.B
    n = dict.fromkeys(("kb0", "handover", "mid_lc", "crashed", "over", "under", "lc_hi", "lc_lo", "bad", "respawn"), 0)
    sx = torch.tensor([0.0, 320.0, 320.0, 420.0, 0.0, 220.0], dtype=torch.float64)
    ln = torch.tensor([320.0, 100.0, 100.0, 1000.0, 220.0, 100.0], dtype=torch.float64)
    for st in tape:
        u8, f64 = st["pre"]["u8"], st["pre"]["f64"]
        ctrl = u8[B["KIND"]] == 1
        lane, tlane = u8[B["LANE"]].long(), u8[B["TARGET_LANE"]].long()
        x, v, ts = f64[F["X"]], f64[F["SPEED"]], f64[F["TARGET_SPEED"]]
        n["kb0"] += int((ctrl & (lane == KB0)).sum())
        n["handover"] += int((ctrl & ((x - sx[tlane]) > ln[tlane] - 2.5) & (tlane != CD0)).sum())
        n["mid_lc"] += int((ctrl & (lane != tlane)).sum())
        n["crashed"] += int((ctrl & (u8[B["CRASHED"]] != 0)).sum())
        n["over"] += int((ctrl & (v > 40.0)).sum())
        n["under"] += int((ctrl & (v < -40.0)).sum())
        acc = (1 / 0.6) * (ts - v)
        n["lc_hi"] += int((ctrl & (acc > 6.0) & (v <= 40.0)).sum())
        n["lc_lo"] += int((ctrl & (acc < -12.5) & (v >= -40.0)).sum())
        n["bad"] += int((ctrl & ((st["actions"] < 0) | (st["actions"] > 4))).sum())
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
            assert int(st["rec"]["env_i32"][abi.EP["STEPS"], 3]) == 0
            assert not bool(st["rec"]["u8"][abi.B["CRASHED"], 3].any())
