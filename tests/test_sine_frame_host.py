"""The sine lane's frame as the step kernel evaluates it (include/mm_math.h compiled for the host, the oracle's flags):

* mmm_atan_small(x) returns the bits of mmm_atan(x) wherever the sine lane can call it (|x| < 0.125);
* mmm_sincos(ph) returns the bits of (mmm_sin(ph), mmm_cos(ph));
* the lateral offset of a pose on kb0 is one expression, whichever of closest_lane / lane_local spells it (what a later
  change that hands the value from predict to the next sub-step's steering_control would rely on).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <math.h>
#include "mm_math.h"
/* marl-mass_amd/csrc/mm_device.h */
static const double kPi = 3.141592653589793;
#define kSineAmp 3.25
#define kSinePuls (2 * kPi / (2 * 100.0))
#define kSinePhase (kPi / 2)
static double lane_sx_kb0(void) { return 220.0; }
void sf_atan(const double *x, double *gen, double *small, long n) {
  for (long i = 0; i < n; i++) { gen[i] = mmm_atan(x[i]); small[i] = mmm_atan_small(x[i]); }
}
/* the heading of kb0 at longitudinal s as both call sites form it: 0.0 + atan(amp * puls * cos(ph)) */
void sf_heading(const double *s, double *arg, double *gen, double *small, long n) {
  for (long i = 0; i < n; i++) {
    double a = kSineAmp * kSinePuls * mmm_cos(kSinePuls * s[i] + kSinePhase);
    arg[i] = a; gen[i] = 0.0 + mmm_atan(a); small[i] = 0.0 + mmm_atan_small(a);
  }
}
void sf_sincos(const double *s, double *out, long n) { /* out: sin, cos, sincos.s, sincos.c */
  for (long i = 0; i < n; i++) {
    double ph = kSinePuls * s[i] + kSinePhase, ss, cc;
    mmm_sincos(ph, &ss, &cc);
    out[4 * i] = mmm_sin(ph); out[4 * i + 1] = mmm_cos(ph); out[4 * i + 2] = ss; out[4 * i + 3] = cc;
  }
}
void sf_offset(const double *x, double *closest, double *local, long n) {
  for (long i = 0; i < n; i++) {
    { /* closest_lane's kb0 block */
      double s = x[i] - 220.0;
      double ph = kSinePuls * s + kSinePhase;
      closest[i] = kSineAmp * mmm_sin(ph);
    }
    { /* lane_local(MM_LANE_KB0, x, y) */
      double s = x[i] - lane_sx_kb0();
      local[i] = kSineAmp * mmm_sin(kSinePuls * s + kSinePhase);
    }
  }
}
double sf_slope(void) { return kSineAmp * kSinePuls; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("sine_frame")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                           "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(REPO, "include"), "-shared", "-o", str(so),
                           str(src), "-lm"])
    L = C.CDLL(str(so))
    L.sf_slope.restype = C.c_double
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _atan_pair(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    g, s = np.empty_like(x), np.empty_like(x)
    lib.sf_atan(_p(x), _p(g), _p(s), C.c_long(len(x)))
    return g, s


# s from -500 to 1 500 m: the kb0 range 0..100 and whatever a masked lane (a vehicle far from the ramp) feeds the frame
S_RANGE = np.concatenate([np.linspace(-500.0, 1500.0, 700_001), np.linspace(-5.0, 105.0, 300_001)])


def test_slope_is_in_the_small_range(lib):
    assert lib.sf_slope() == 3.25 * (2 * np.pi / 200.0) and lib.sf_slope() * (1 + 2.0 ** -40) < 0.125


def test_atan_small_signed_zeros(lib):
    g, s = _atan_pair(lib, [0.0, -0.0])
    assert np.array_equal(_bits(g), _bits(s))
    assert np.array_equal(_bits(g + 0.0), _bits(0.0 + s))  # ... and under the call sites' `0.0 +`


def test_atan_small_on_the_sine_lane_slopes(lib):
    assert len(S_RANGE) >= 1_000_000
    arg, g, s = np.empty_like(S_RANGE), np.empty_like(S_RANGE), np.empty_like(S_RANGE)
    lib.sf_heading(_p(S_RANGE), _p(arg), _p(g), _p(s), C.c_long(len(S_RANGE)))
    assert np.abs(arg).max() < 0.125 and np.abs(arg).max() > 0.1021 and (arg < 0).any() and (arg > 0).any()
    assert np.array_equal(_bits(g), _bits(s))
    g2, s2 = _atan_pair(lib, np.concatenate([arg, -arg]))
    assert np.array_equal(_bits(g2), _bits(s2))


def test_atan_small_around_the_largest_slope(lib):
    top = lib.sf_slope()
    up, dn = [top], [top]
    for _ in range(2000):
        up.append(np.nextafter(up[-1], 1.0)); dn.append(np.nextafter(dn[-1], 0.0))
    x = np.array(up + dn)
    g, s = _atan_pair(lib, np.concatenate([x, -x]))
    assert np.array_equal(_bits(g), _bits(s))


def test_atan_small_subnormals_and_the_whole_range(lib):
    tiny = np.array([5e-324, 1e-323, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-310, 1e-300, 1e-200, 1e-100, 1e-20])
    rs = np.random.RandomState(11)
    sub = rs.randint(1, 2 ** 52, 20000).astype(np.uint64).view(np.float64)  # random subnormals
    wide = np.concatenate([rs.uniform(0, 0.125, 200000), np.nextafter(0.125, 0.0) * np.ones(1), 2.0 ** -rs.uniform(3, 1000, 20000)])
    assert (wide < 0.125).all()
    x = np.concatenate([tiny, sub, wide])
    g, s = _atan_pair(lib, np.concatenate([x, -x]))
    assert np.array_equal(_bits(g), _bits(s))


def test_atan_small_nan_stays_nan(lib):
    g, s = _atan_pair(lib, [np.nan])
    assert np.isnan(g[0]) and np.isnan(s[0])


def test_sincos_is_sin_and_cos(lib):
    out = np.empty(4 * len(S_RANGE))
    lib.sf_sincos(_p(S_RANGE), _p(out), C.c_long(len(S_RANGE)))
    out = out.reshape(-1, 4)
    assert np.array_equal(_bits(out[:, 0]), _bits(out[:, 2])) and np.array_equal(_bits(out[:, 1]), _bits(out[:, 3]))


def test_the_offset_of_a_pose_is_one_expression(lib):
    x = S_RANGE + 220.0
    a, b = np.empty_like(x), np.empty_like(x)
    lib.sf_offset(_p(x), _p(a), _p(b), C.c_long(len(x)))
    assert np.array_equal(_bits(a), _bits(b))
