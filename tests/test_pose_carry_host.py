"""What handing the sine lane's offset from predict (closest_lane: mmm_sincos of the phase) to the next sub-step's
steering_control (lane_local: mmm_sin of the same phase) would rest on: mmm_sincos(p).sin has the bits of mmm_sin(p) over the
sine lane's argument range -- its boundaries, 0 and a few thousand random points (include/mm_math.h compiled for the host with
the oracle's flags)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <math.h>
#include "mm_math.h"
void pc_sin_pair(const double *p, double *plain, double *paired, long n) {
  for (long i = 0; i < n; i++) {
    double s, c;
    mmm_sincos(p[i], &s, &c);
    plain[i] = mmm_sin(p[i]); paired[i] = s;
  }
}
"""
PULS, PHASE = 2 * np.pi / 200.0, np.pi / 2  # marl-mass_amd/csrc/mm_device.h: kSinePuls, kSinePhase


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_carry")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                           "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(REPO, "include"), "-shared", "-o", str(so),
                           str(src), "-lm"])
    return C.CDLL(str(so))


def _pair(lib, p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    a, b = np.empty_like(p), np.empty_like(p)
    ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    lib.pc_sin_pair(ptr(p), ptr(a), ptr(b), C.c_long(len(p)))
    return a.view(np.uint64), b.view(np.uint64)


def test_sincos_sine_is_sin_on_the_sine_lane(lib):
    rs = np.random.RandomState(5)
    # longitudinal s of kb0 is 0..100 m; a pose anywhere on the 500 m road can meet the frame (s = x - 220)
    s = np.concatenate([[0.0, 100.0, -220.0, 280.0, np.nextafter(0.0, 1.0), np.nextafter(100.0, 0.0), np.nextafter(100.0, 200.0)],
                        rs.uniform(0.0, 100.0, 4000), rs.uniform(-220.0, 280.0, 4000)])
    phase = PULS * s + PHASE
    p = np.concatenate([phase, [0.0, -0.0, PHASE, PULS * 100.0 + PHASE]])
    a, b = _pair(lib, p)
    assert np.array_equal(a, b)
