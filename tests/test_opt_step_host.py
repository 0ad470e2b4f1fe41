"""mm_opt_step (include/mm_opt_step.h) without a GPU: the binding's structure against the C header, the state-dict
converters of the learners against torch.optim's own state dicts, and the header's formulas against the optimiser steps
recorded from the reference."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import optimizer_state_from_torch, optimizer_state_to_torch
from opt_step_util import pre_step_prefix_of, recorded_runs, restated_step, run_lr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mm_opt_step.h")
FIELDS = [name for name, _ in abi.MMOptGroup._fields_]


def test_ctypes_structure_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mm_opt_step.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(MMOptGroup));\n'
                   + "".join('  printf("%s %%zu\\n", offsetof(MMOptGroup, %s));\n' % (f, f) for f in FIELDS)
                   + '  printf("consts %d %d %d %d %d\\n", MM_OPT_RMSPROP, MM_OPT_ADAM, MM_OPT_BLEND, MM_OPT_MAX_TENSORS, '
                   "MM_OPT_MAX_GROUPS);\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"),
                           "-o", exe, str(src)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(abi.MMOptGroup)
    for f in FIELDS:
        assert int(got[f]) == getattr(abi.MMOptGroup, f).offset, f
    assert [int(x) for x in got["consts"].split()] == [abi.OPT_RMSPROP, abi.OPT_ADAM, abi.OPT_BLEND, abi.OPT_MAX_TENSORS,
                                                       abi.OPT_MAX_GROUPS]


def test_constants_match_the_header():
    text = open(HEADER).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (MM_OPT_\w+)\s+(\d+)", text)}
    assert defs == {"MM_OPT_RMSPROP": abi.OPT_RMSPROP, "MM_OPT_ADAM": abi.OPT_ADAM, "MM_OPT_BLEND": abi.OPT_BLEND,
                    "MM_OPT_MAX_TENSORS": abi.OPT_MAX_TENSORS, "MM_OPT_MAX_GROUPS": abi.OPT_MAX_GROUPS}


def test_symbol_is_the_hip_librarys_alone():
    from marl_mass_amd import hip_library
    assert "mm_opt_step" not in abi.CLib.SYMBOLS
    assert hip_library().has_opt_step
    ora = abi.CLib(os.path.join(REPO, "oracle", "libmm_oracle.so"))
    assert not ora.has_opt_step
    with pytest.raises(NotImplementedError, match="mm_opt_step"):
        ora.require_opt_step()


def _same_state_dict(x, y):
    assert x["param_groups"] == y["param_groups"]
    assert list(x["state"].keys()) == list(y["state"].keys())
    for i in x["state"]:
        assert list(x["state"][i].keys()) == list(y["state"][i].keys()), i
        for k in x["state"][i]:
            a, b = x["state"][i][k], y["state"][i][k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(a, b), (i, k)


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
@pytest.mark.parametrize("steps", [0, 2])
def test_state_dict_converters_round_trip(optimizer_type, steps):
    """torch.optim's state dict -> (step, state tensors) -> torch.optim's state dict: keys, order, dtypes and values are the
    same (also for a fresh optimiser, whose state is empty), and what comes back loads into a torch optimiser."""
    torch.manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(*s)) for s in ((4, 3), (4,), (1, 4), (1,))]
    cls = torch.optim.Adam if optimizer_type == "adam" else torch.optim.RMSprop
    opt = cls(params, lr=3e-4)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
    sd = opt.state_dict()
    step, s1, s2 = optimizer_state_from_torch(sd, optimizer_type, len(params))
    assert step == steps and (s2 is None) == (optimizer_type == "rmsprop")
    if steps == 0:  # no state yet: zeros on the fused side
        assert all(t is None for t in s1)
        s1 = [torch.zeros_like(p) for p in params]
        s2 = None if s2 is None else [torch.zeros_like(p) for p in params]
    back = optimizer_state_to_torch(optimizer_type, sd["param_groups"], step, s1, s2)
    _same_state_dict(back, sd)
    if steps:
        assert back["state"][0]["step"].dtype == torch.float32 and back["state"][0]["step"].dim() == 0
        assert back["state"][0][("exp_avg" if optimizer_type == "adam" else "square_avg")].data_ptr() != s1[0].data_ptr()  # cloned
    cls(params, lr=1.0).load_state_dict(back)


def test_state_dict_converters_refuse_what_the_fused_step_lacks():
    params = [torch.nn.Parameter(torch.randn(3))]
    params[0].grad = torch.randn(3)
    opt = torch.optim.RMSprop(params, momentum=0.9)
    opt.step()
    with pytest.raises(ValueError, match="momentum_buffer"):
        optimizer_state_from_torch(opt.state_dict(), "rmsprop", 1)
    with pytest.raises(ValueError, match="2 parameters"):
        optimizer_state_from_torch(torch.optim.RMSprop(params).state_dict(), "rmsprop", 2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_formulas_reproduce_the_recorded_steps(dtype):
    """The formulas of include/mm_opt_step.h (clip, RMSprop) from the recorded pre-step parameters and the recorded gradient,
    RMSprop's square_avg carried from zeros through all six agent steps of a run: the recorded post-step parameters of every
    tensor within 2^-22 max|q| -- each side rounds the stored parameter once (half an ulp each; the float64 form does not
    round its own), the update is about 1e-3 of the parameter so its arithmetic differences are below 0.01 ulp, and the
    bound is twice their sum.  This pins the semantics before any kernel is trusted."""
    worst = 0.0
    for name, meta0, nets, steps in recorded_runs():
        assert meta0["optimizer_type"] == "rmsprop"
        for net, keys in nets.items():
            v = [np.zeros_like(steps[0][0]["p_" + k], dtype=dtype) for k in keys]
            for z, meta, a in steps:
                pre = [z[pre_step_prefix_of(a) + k] for k in keys]
                g = [z["a%d_g_%s" % (a, k)] for k in keys]
                p, v, _, _ = restated_step("rmsprop", dtype, pre, g, v, None, 0, run_lr(meta, net), 0.99, None, 1e-8,
                                           meta["max_grad_norm"])
                for k, x in zip(keys, p):
                    q = z["a%d_q_%s" % (a, k)]
                    diff, bound = float(np.abs(x.astype(np.float64) - q).max()), 2.0 ** -22 * float(np.abs(q).max())
                    worst = max(worst, diff / bound)
                    assert diff <= bound, (name, meta["train_index"], a, k, diff, bound)
    print("worst difference / bound: %.3f" % worst)


def test_kernel_resources(tmp_path):
    """The launch is one kernel of one workgroup per network: no spills, no scratch memory, a kilobyte of LDS for the group's
    table, and what profiles/opt_step/kernel_resources.json records is what the build gives."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_opt_step.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(csrc, "mm_opt_step.o")], stdout=subprocess.DEVNULL)
    rows = json.load(open(path))
    assert [r["kernel"] for r in rows] == ["mm::opt::opt_step_kernel"]
    assert rows[0]["vgpr_spill"] == 0 and rows[0]["scratch_B"] == 0 and rows[0]["vgpr"] <= 128 and rows[0]["lds_B"] <= 1024
    rec = json.load(open(os.path.join(REPO, "profiles", "opt_step", "kernel_resources.json")))
    for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
        assert rows[0][k] == rec[0][k], k
