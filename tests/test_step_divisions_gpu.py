"""The shared-reciprocal division forms (marl-mass_amd/csrc/mm_div.h: rcp_rn, div_g, rcp_g, div_n) and the step kernels'
branch-free epilogue (mm_kernels.hip: the reward scan and the env-level sums).

Nothing about the results may change, so both tests are bit-for-bit: the division forms against IEEE division (NumPy's
`/` on float64) on the operand ranges the call sites reach plus every class of operand outside Markstein's theorems, and
short free-running rollouts against the oracle on group layouts and vehicle counts that exercise the epilogue's scans,
sums and small-integer divisors."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_env
from golden_util import env_kwargs
from marl_mass_amd import VecMergeEnv, _cabi as abi, vec_env


def _geom_div(rows):
    """mm_geom_eval(MM_GEOM_DIV) on [n][2] rows (x, d) -> [n][4]: guarded quotient, reciprocal, table quotient, un-needed quotient."""
    clib = abi.CLib(vec_env.HIP_LIB)
    x = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64), device="cuda:0")
    out = torch.zeros(len(rows), 4, dtype=torch.float64, device="cuda:0")
    clib.check(clib.lib.mm_geom_eval(abi.GEOM_DIV, len(rows), C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _all_ones(exp, sign=1.0):
    """The double with an all-ones significand and binary exponent `exp`: (2 - 2^-52) 2^exp."""
    return sign * np.ldexp(2.0 - 2.0 ** -52, exp)


def _same_bits(got, want):
    """Element-wise: equal bit patterns, NaN matching any NaN (not by payload)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def _division_rows():
    rs = np.random.RandomState(20240)
    n = 1024  # x 4 call-site families = 4096 random pairs from the ranges documented at div_g
    sgn = lambda k: rs.choice([-1.0, 1.0], k)  # noqa: E731
    fam = []
    # steering_control: lateral command / not_zero(speed), and LENGTH / 2 over it
    d = sgn(n) * np.exp(rs.uniform(np.log(0.01), np.log(45.0), n))
    x = np.where(rs.rand(n) < 0.25, 2.5, rs.uniform(-20, 20, n))
    fam.append((x, d))
    # slip angle: t / sqrt(1 + t^2); steering_control's |t| <= 0.87 and the unbounded t of a general steering angle
    t = np.where(rs.rand(n) < 0.7, rs.uniform(-0.87, 0.87, n), sgn(n) * np.exp(rs.uniform(np.log(1e-8), np.log(1e8), n)))
    fam.append((t, np.sqrt(1.0 + t * t)))
    # qp_exact: CBF row / (g.vx dt), |g.vx| <= 1
    fam.append((rs.uniform(-1e3, 1e3, n), sgn(n) * np.exp(rs.uniform(np.log(1e-9), np.log(1.0 / 15), n))))
    # epilogue means: sums over vehicle counts 1..16
    fam.append((rs.uniform(-1e4, 1e4, n), rs.randint(1, 17, n).astype(np.float64)))
    rows = [np.stack(f, 1) for f in fam]
    assert sum(len(r) for r in rows) == 4096
    # edge rows: every special divisor against every special numerator
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    lo_ones = np.array([0x3FF50000FFFFFFFF], dtype=np.uint64).view(np.float64)[0]  # low word all ones, significand not
    ds = [_all_ones(e) for e in (-1022, -300, -1, 0, 5, 300, 1023)] + [_all_ones(3, -1.0), lo_ones, -lo_ones,
          0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, tiny / 2, tiny, -tiny, huge, -huge,
          2.0 ** -401, 2.0 ** -400, 2.0 ** 400, 2.0 ** 401, 3.0, -7.0, 16.0, 17.0, 1.0, -1.0, 0.01, 1e-2 * (1 + 2.0 ** -52),
          1e300, 1e-300, 1e120, -1e-120]
    xs = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.5, 1e300, -1e300, 1e-300, 1e-200, 5e-324, tiny, huge,
          2.0 ** 400, 2.0 ** 401, 2.0 ** -400, -(2.0 ** -401), 1.0 / 3, -123.456]
    rows.append(np.array([(x, d) for d in ds for x in xs], dtype=np.float64))
    return np.concatenate(rows)


@pytest.mark.gpu
def test_division_forms_match_ieee_division():
    """rcp_rn + div_c through the guarded wrapper, the reciprocal itself and the small-integer table against `/`:
    4096 random pairs from the call sites' operand ranges plus the edge rows (all-ones significands, +-0, +-inf, NaN,
    subnormals, the extreme normals, overflowing / underflowing / subnormal quotients, negative operands).  Every row
    must match bit for bit; NaN results compare as NaN."""
    rows = _division_rows()
    x, d = rows[:, 0], rows[:, 1]
    with np.errstate(all="ignore"):
        want_q, want_r = x / d, 1.0 / d
    got = _geom_div(rows)
    for k, (name, want) in enumerate((("x / d", want_q), ("1 / d", want_r))):
        ok = _same_bits(got[:, k], want)
        bad = np.flatnonzero(~ok)
        print("%s: %d rows, %d differ" % (name, len(rows), len(bad)))
        assert len(bad) == 0, (name, [(float(x[i]).hex(), float(d[i]).hex(), float(got[i, k]).hex(), float(want[i]).hex()) for i in bad[:8]])
    # a lane that does not need its quotient takes no fall-back: the residual form alone, right inside the guard
    ad, ax = np.abs(d), np.abs(x)
    inside = (ad >= 2.0 ** -400) & (ad <= 2.0 ** 400) & ((rows[:, 1].view(np.uint64) & 0xFFFFFFFF) != 0xFFFFFFFF) & \
        (ax <= 2.0 ** 400) & ((ax >= 2.0 ** -400) | (x == 0))
    assert inside.sum() >= 4096 and (~inside).sum() >= 300
    ok = _same_bits(got[inside, 3], want_q[inside])
    print("un-needed x / d inside the guard: %d rows, %d differ" % (int(inside.sum()), int((~ok).sum())))
    assert ok.all()
    integral = np.isfinite(d) & (np.abs(d) <= 1e9) & (d == np.trunc(d))
    assert np.isnan(got[~integral, 2]).all()
    assert (integral & (d >= 1) & (d <= 16)).sum() >= 1024 and (integral & ((d < 1) | (d > 16))).sum() >= 40  # table and fallback
    with np.errstate(all="ignore"):  # the table form divides by the INTEGER n = (int)d: a -0.0 in the row arrives as 0
        want_n = x[integral] / d[integral].astype(np.int64).astype(np.float64)
    ok = _same_bits(got[integral, 2], want_n)
    print("x / n: %d rows, %d differ" % (int(integral.sum()), int((~ok).sum())))
    assert ok.all(), [(float(a).hex(), float(b)) for a, b in rows[integral][~ok][:8]]


# E x N of the issue's shapes; the last one draws its vehicle counts per episode in mixed traffic (n_ctrl, n_veh and the
# regional mean's count take values from 1 upward and differ from each other)
CASES = [
    ("E16_N8", 16, 8, {}),
    ("E10_N5", 10, 5, {}),
    ("E5_N12", 5, 12, {}),
    ("E32_N2", 32, 2, {}),
    ("E16_N8_drawn_mixed", 16, 8, {"traffic_density": 1, "traffic_type": "mixed", "mixed_traffic": True}),
]
OUTPUTS = ("agents_rewards", "regional_rewards", "reward", "average_speed", "traffic_speed", "min_headway", "merge_percent", "done")
STEPS = 20


@pytest.mark.gpu
@pytest.mark.parametrize("name,E,N,extra", CASES, ids=[c[0] for c in CASES])
def test_epilogue_forms_against_oracle(name, E, N, extra):
    """20 free-running steps, device library vs oracle, every epilogue output equal bit for bit.  duration = 1 s makes an
    episode 5 policy steps, so every env ends and re-spawns several times inside the test."""
    meta = {"shield": "cbf-cav", "headway_time": 0.5, "env_id": "merge-multi-agent-v1", "eta": 0.03125}
    kw = env_kwargs(meta)  # (tests/golden_util.py: the exact QP, f64 observations, trace planes)
    kw["config"].update({"duration": 1}, **extra)
    kw.update(seed=4242, auto_reset=True, draw_counts=bool(extra))
    oracle_env.set_math_mode(1)
    try:
        gpu, cpu = VecMergeEnv(E, N, device="cuda:0", **kw), oracle_env.OracleEnv(E, N, **kw)
        og, _ = gpu.reset()
        oc, _ = cpu.reset()
        assert torch.equal(og.cpu(), oc)
        g = torch.Generator().manual_seed(7)
        p = torch.tensor([0.2, 0.3, 0.2, 0.15, 0.15])
        episodes, counts = 0, set()
        for t in range(STEPS):
            a = torch.multinomial(p, E * N, True, generator=g).view(E, N).int()
            kind = cpu.u8[abi.B["KIND"]]
            counts.update(zip((kind == 1).sum(1).tolist(), (kind != 0).sum(1).tolist()))
            og, _, _, ig = gpu.step(a.cuda())
            oc, _, _, ic = cpu.step(a)
            assert torch.equal(og.cpu().nan_to_num(nan=-7.0), oc.nan_to_num(nan=-7.0)), (name, t, "obs")
            for k in OUTPUTS:
                x, y = ig[k].cpu(), ic[k]
                if x.is_floating_point():
                    x, y = x.nan_to_num(nan=-7.0), y.nan_to_num(nan=-7.0)
                assert torch.equal(x, y), (name, t, k)
            episodes += int(ic["done"].sum())
        assert episodes >= 2 * E, (name, "episodes ended", episodes)
        if extra:  # (n_ctrl, n_veh) pairs met: several, from one controlled vehicle upward, n_ctrl != n_veh
            assert len(counts) >= 4 and all(c != v for c, v in counts) and min(c for c, _ in counts) == 1, counts
        gpu.poll_errors()
        gpu.close(); cpu.close()
    finally:
        oracle_env.set_math_mode(0)
