"""The placed coverage tapes (cv_* / ipm_cv_*, tests/golden/cv_index.json) on the MI355X: the branches of the step that no
other tape reaches, teacher-forced against the reference in every kernel form that applies, then free-running against the
oracle bit for bit.  One env with the tape's 2-4 vehicles: the smallest shape at which these branches exist."""
import os

import numpy as np
import pytest

import oracle_env
from golden_util import GOLDEN, is_ipm, load_episode, replay
from marl_mass_amd import VecMergeEnv, _cabi as abi
from tape_census_util import cv_files, free_run_pair, tape_name

pytestmark = pytest.mark.gpu

CV = cv_files()
# debug_flags (include/mm_abi.h): 1 the literal front-to-back sweep, 2 power-of-two lane groups, and for the interior-point
# step 4 the fused kernel, 8 the split step (phase kernels + sweep kernel)
FORMS = {"default": 0, "literal": 1, "pow2": 2, "fused": 4, "split": 8}


def _gpu_env(E, N, **kw):
    return VecMergeEnv(E, N, device="cuda:0", **kw)


def _cases():
    for path in CV:
        ipm = is_ipm(load_episode(path)[1])
        for form in FORMS:
            if form in ("fused", "split") and not ipm:
                continue  # the two forms of the interior-point step
            yield pytest.param(path, form, id="%s-%s" % (tape_name(path), form))


@pytest.mark.parametrize("path,form", list(_cases()))
def test_cv_tape_teacher_forced(path, form):
    """Within 1e-9 of the reference with every discrete quantity exact and no knife-edge (tests/test_tape_census_host.py checks
    on the CPU that these placements have none under include/mm_math.h)."""
    flags = FORMS[form]
    err = replay(lambda E, N, **kw: _gpu_env(E, N, debug_flags=flags, **kw), path, tol=1e-9, max_knife_edges=0)
    assert err["knife_edges"] == 0


@pytest.mark.parametrize("path", CV, ids=tape_name)
def test_cv_tape_free_run_bits_vs_oracle(path):
    """From the placed initial state on the tape's own action script, for the tape's length: HIP and the oracle under
    include/mm_math.h agree on every bit of every state plane, observation and output; poll_errors() stays silent."""
    oracle_env.set_math_mode(1)
    try:
        free_run_pair(_gpu_env, oracle_env.OracleEnv, path)
    finally:
        oracle_env.set_math_mode(0)


def test_first_kkt_factorisation_failure_on_the_device():
    """Rows 0-1 of cvqp.npz (a non-finite a: the reference-side coneqp cannot factor its first KKT matrix): the device's QP
    answers as include/mm_qp.h documents and the oracle does -- no iterate (NaN), status "unknown", 0 iterations.  The other
    rows need |a| >= 1e200, far outside the range of the kernels' reciprocal arithmetic (|a| <= 1/15 in the env); they pin
    the oracle only (tests/test_tape_census_host.py)."""
    z = np.load(os.path.join(GOLDEN, "cvqp.npz"))
    env = _gpu_env(1, 2, config={"safety_guarantee": "none"})
    u, st, it = env.shield_qp(z["G"][:2], z["h"][:2], z["rows"][:2], solver="ipm", with_iters=True)
    u = u.cpu().numpy()
    assert np.isnan(u[:, 0]).all() and np.isnan(z["x"][:2, 0]).all()
    assert np.array_equal(st.cpu().numpy(), z["status"][:2]) and np.array_equal(it.cpu().numpy(), z["iters"][:2])
    assert int(st[0]) == abi.QPS_UNKNOWN
    env.poll_errors()
