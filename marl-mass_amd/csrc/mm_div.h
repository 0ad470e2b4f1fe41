// mm_div.h -- correctly rounded x / d for a RUN-TIME divisor used more than once (gfx950, fp64): TESTED, NOT USED by any
// step kernel.  The reciprocal is formed once (rcp_rn) and every quotient by it costs the three instructions of div_c
// (mm_device.h); a guard sends every operand outside Markstein's theorems to the plain `/`, so each form is bit-identical
// to `/` on every operand pair (MM_GEOM_DIV of mm_geom_eval, tests/test_step_divisions_gpu.py).  In the step kernels the
// guard's compares and the masks it keeps in SGPRs cost more than the shorter chain saves; the
// interior-point iteration, which divides by the same few values many times, is the intended user.
#pragma once
#include "mm_device.h"

namespace mm {

// v_rcp_f64 (2^29 ulp) and two Newton steps leave y within 1 ulp of 1/d; for such a y one more step with the exact
// residual, e = fma(-d, y, 1), y' = fma(e, y, y), IS RN(1/d) unless the significand of d is all ones (Markstein 1990,
// the theorem div_c rests on).  Seven dependent instructions, against the ~11 of one IEEE division.
MM_DEV double rcp_rn(double d) {
  double y = __builtin_amdgcn_rcp(d);
  double e = fma(-d, y, 1.0);
  y = fma(e, y, y);
  e = fma(-d, y, 1.0);
  y = fma(e, y, y);
  e = fma(-d, y, 1.0);
  return fma(e, y, y);
}
// Where the theorems hold, with room to spare: d normal with 2^-400 <= |d| <= 2^400 (so is 1/d) and not all ones -- the
// test takes every d whose LOW WORD is all ones, a superset; x zero, or finite with 2^-400 <= |x| <= 2^400, so that x*y
// neither overflows nor leaves the normal range and the residual x - q*d (a multiple of 2^-104 |x|) is exact.  NaN fails
// every comparison: zero, subnormal, infinite and NaN operands are all outside.
MM_DEV bool rcp_ok(double d) {
  const double ad = fabs(d);
  const unsigned lo = (unsigned)__double2loint(d);
  return (ad >= 0x1p-400) & (ad <= 0x1p400) & (lo != 0xffffffffu);
}
MM_DEV bool num_ok(double x) {
  const double ax = fabs(x);
  return (ax <= 0x1p400) & ((ax >= 0x1p-400) | (x == 0.0));
}
// x / d with y = rcp_rn(d), d_ok = rcp_ok(d): bit-identical to `/` for EVERY operand pair.  The guard is tested for the
// whole wave at once, so the usual path pays the comparisons and one scalar branch; a wave with a lane outside the
// theorems (and `need`ing its quotient) also runs the plain division and those lanes keep it.  A zero numerator takes
// x*y, whose sign is the quotient's (the residual form would return +0 for -0 / d).
// Operand ranges of the step kernels' run-time divisions (all far inside the guard unless noted):
//   steering_control  d = not_zero(speed): 0.01 <= |d| <= ~45, never NaN (not_zero maps NaN to -0.01);  x = the lateral
//                     command -5/3 r, |x| < ~20, often +-0 (a vehicle on its lane's centre line), or the constant 2.5
//   slip_sincos       d = sqrt(1 + t^2) >= 1;  x = t = 1/2 tan(steer): |t| <= 0.87 out of steering_control; unbounded,
//                     +-inf or NaN (then d is too) for a steering angle that did not come out of it (HDVs, steer_vel)
//   qp_exact          d = g0 = g.vx dt, |d| <= 1/15; NaN for a CAV before its first step (g.vx starts as NaN) and 0 for
//                     g.vx = 0: both fail the sign tests, no quotient is wanted (need = false);  x = the CBF row h0 / h3:
//                     gaps and speeds, |x| < ~1e3, 0 possible, NaN where g.vx of a neighbour is
//   epilogue means    d = a vehicle count 1..16 (table below);  x = sums of rewards / speeds, |x| < ~1e4, 0 possible;
//                     -inf is not reachable (the headway term's log argument is > 0), the guard covers it anyway
// The +-inf sort keys of the neighbour selection never reach a division.
MM_DEV double div_g(double x, double d, double y, bool d_ok, bool need = true) {
  const double q = x * y;
  double f = fma(fma(-q, d, x), y, q);
  f = x == 0.0 ? q : f;
  const bool ok = (d_ok & num_ok(x)) | !need;
  if (__builtin_expect(__any(!ok), 0)) {
    const double s = x / d;
    f = ok ? f : s;
  }
  return f;
}
MM_DEV double rcp_g(double d, double y, bool d_ok) {  // 1 / d itself, same guard
  if (__builtin_expect(__any(!d_ok), 0)) {
    const double s = 1.0 / d;
    y = d_ok ? y : s;
  }
  return y;
}
// x / n for a small integer n: RN(1/n), n = 1..16, from a table (none of them has an all-ones significand)
MM_DEV double div_n(double x, int n, bool need = true) {
  constexpr double kRcp[17] = {0.0,      1.0 / 1,  1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,  1.0 / 6,  1.0 / 7, 1.0 / 8,
                               1.0 / 9,  1.0 / 10, 1.0 / 11, 1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16};
  const bool n_ok = (unsigned)(n - 1) < 16u;
  return div_g(x, (double)n, kRcp[n_ok ? n : 0], n_ok, need);
}

}  // namespace mm
