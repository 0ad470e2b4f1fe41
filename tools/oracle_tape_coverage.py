#!/usr/bin/env python3
"""Which lines and branch outcomes of the oracle's step does no reference tape execute?  (Discovery tool; takes minutes.)

Builds a `-O0 --coverage` copy of oracle/mm_oracle.c in a temporary directory (gcc + gcov, host code only), replays every
reference tape of the step teacher-forced against it (tests/golden_util.replay, 1e-9, as tests/test_oracle_golden.py does),
runs `gcov -b -c` and writes what never ran between py_mod and min_time_headway -- the step's own code -- to
profiles/tape_coverage/coverage.json: never-run lines and never-taken branch outcomes, each with its function, its source
line and the census names (orc_step_census) that stand on that line or the next one.

    python tools/oracle_tape_coverage.py                               # every tape -> coverage.json
    python tools/oracle_tape_coverage.py --without cv_ ipm_cv_ --out profiles/tape_coverage/coverage_before.json

The tapes are replayed under libm (math mode 0, the mode the tapes pin) and once more under include/mm_math.h (mode 1):
the device-arithmetic forms of steering_control, get_corner and vehicle_step are lines of the step as well and run in mode 1
only.  The unit tables of tests/golden/units.npz run too, as tests/test_oracle_golden.py runs them, and one scenario without
the per-sub-step trace.  The census counts during the whole replay; an outcome counts as explained when the census names next
to it that this replay never counted are all in tests/golden/cv_unreached.json.  Two tapes then run once more with the census
off, so that neither outcome of its on/off tests shows up.  The line-to-name match (names on the line or the next one, or
written after "census:" in a comment) is a heuristic of a discovery tool; the test below is what holds.
The IDM env's tapes (idm_*) are not part of this: the oracle has no merge-multi-agent-hdv-v1.

tests/test_tape_census_host.py is the durable form of this measurement: it needs no compiler and names, not line numbers."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(REPO, "oracle", "mm_oracle.c")
FIRST_FN, LAST_FN = "py_mod", "min_time_headway"
CFLAGS = ["-O0", "-g", "--coverage", "-std=gnu11", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC"]


def replay_all(lib, without, modes):
    """Child process: load the instrumented library in place of oracle/libmm_oracle.so and replay the tapes."""
    sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]
    import oracle_env
    oracle_env.build = lambda force=False: lib
    import numpy as np
    import test_oracle_golden as units_tests
    from golden_util import GOLDEN, episode_files, free_run, replay
    tapes = [p for p in episode_files() if not os.path.basename(p).startswith(tuple(without))]
    oracle_env.step_census_reset(True)
    for mode in modes:
        oracle_env.set_math_mode(mode)
        for path in tapes:
            replay(oracle_env.OracleEnv, path, tol=1e-9, max_knife_edges=0 if mode == 0 else 6)
            print("mode %d  %s" % (mode, os.path.basename(path)), flush=True)
    oracle_env.set_math_mode(0)
    with open("census.json", "w") as fh:  # (in the temporary directory: which names the same replay counted)
        json.dump(oracle_env.step_census(), fh)
    oracle_env.step_census_reset(False)  # two tapes once more with the census off, for the other outcome of its on/off tests
    for name in ("am_v0_none_N4_s0", "sc_merge_mass"):
        replay(oracle_env.OracleEnv, os.path.join(GOLDEN, name + ".npz"), tol=1e-9)
    # the reference's unit tables (lane frames, steering control, wrap_to_pi, rectangles) as tests/test_oracle_golden.py runs them
    units, lib = np.load(os.path.join(GOLDEN, "units.npz")), oracle_env.library().lib
    units_tests.test_lane_frames_and_argmin(units, lib)
    units_tests.test_steering_control_and_corners(units, lib)
    units_tests.test_scalar_helpers(units, lib)
    units_tests.test_rotated_rectangles(units, lib)
    free_run(oracle_env.OracleEnv, os.path.join(GOLDEN, "sc_lon_mass.npz"))  # (a run without the per-sub-step trace)
    print("replayed %d tapes" % len(tapes))


def census_names(src_lines):
    """Names on a piece of source: CEN(ID) / CEN_ID uses, and names written out after "census:" in a comment."""
    ids = dict(re.findall(r'X\((\w+), "(\w+)"\)', "".join(src_lines)))
    names = set(ids.values())

    def on(text):
        tagged = [w for tag in re.findall(r"census:([\w ]+)", text) for w in tag.split() if w in names]
        return [ids[i] for i in re.findall(r"CEN[(_](\w+)", text) if i in ids] + tagged
    return on


def parse_gcov(path):
    """-> (never-run lines, never-taken outcomes, totals) of the functions FIRST_FN .. LAST_FN."""
    with open(SRC) as fh:
        src = fh.readlines()
    names_on = census_names(src)
    fn, inside, done = None, False, False
    lines, outcomes = [], []
    n_lines = n_out = 0
    lineno, text = 0, ""
    with open(path) as fh:
        for row in fh:
            m = re.match(r"function (\w+) called", row)
            if m:
                if fn == LAST_FN:
                    done = True
                fn = m.group(1)
                inside = not done and (inside or fn == FIRST_FN)
                continue
            m = re.match(r"\s*([^:]+):\s*(\d+):(.*)$", row)
            if m and not row.startswith(("branch", "call")):
                count, lineno, text = m.group(1).strip(), int(m.group(2)), m.group(3).rstrip()
                if inside and lineno > 0 and count != "-":
                    n_lines += 1
                    if count.startswith(("#####", "=====")):
                        lines.append({"line": lineno, "function": fn, "text": text.strip()})
                continue
            m = re.match(r"branch\s+(\d+) (never executed|taken (\d+))", row)
            if m and inside:
                n_out += 1
                if m.group(2) == "never executed" or int(m.group(3)) == 0:
                    near = text + " " + (src[lineno] if lineno < len(src) else "")
                    outcomes.append({"line": lineno, "function": fn, "branch": int(m.group(1)), "text": text.strip(),
                                     "census": names_on(near)})
    return lines, outcomes, {"executable_lines": n_lines, "branch_outcomes": n_out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tape_coverage", "coverage.json"))
    ap.add_argument("--without", nargs="*", default=[], help="tape-name prefixes to leave out (e.g. cv_ ipm_cv_)")
    ap.add_argument("--math-modes", default="0,1")
    ap.add_argument("--replay", help=argparse.SUPPRESS)
    a = ap.parse_args()
    modes = [int(m) for m in a.math_modes.split(",")]
    if a.replay:
        return replay_all(a.replay, a.without, modes)
    with tempfile.TemporaryDirectory() as tmp:
        obj, lib = os.path.join(tmp, "mm_oracle.o"), os.path.join(tmp, "libmm_oracle_cov.so")
        subprocess.check_call(["gcc"] + CFLAGS + ["-c", SRC, "-o", obj], cwd=tmp)
        subprocess.check_call(["gcc", "--coverage", "-fopenmp", "-shared", "-o", lib, obj, "-lm"], cwd=tmp)
        cmd = [sys.executable, os.path.abspath(__file__), "--replay", lib, "--math-modes", a.math_modes, "--without"] + a.without
        subprocess.check_call(cmd, cwd=tmp)  # (the counters reach mm_oracle.gcda when the child exits)
        subprocess.check_call(["gcov", "-b", "-c", "-o", tmp, SRC], cwd=tmp, stdout=subprocess.DEVNULL)
        lines, outcomes, totals = parse_gcov(os.path.join(tmp, "mm_oracle.c.gcov"))
        with open(os.path.join(tmp, "census.json")) as fh:
            census = json.load(fh)
    with open(os.path.join(REPO, "tests", "golden", "cv_unreached.json")) as fh:
        allowed = set(json.load(fh))
    # explained: of the census names next to the outcome, those the replay never counted are all in the allow-list (and there
    # is one) -- a reachable outcome that merely stands next to an allow-listed name keeps its own uncounted name and shows up
    for o in outcomes:
        o["census_never_counted"] = [n for n in o["census"] if census[n] == 0]
    unexplained = [o for o in outcomes if not o["census_never_counted"] or not set(o["census_never_counted"]) <= allowed]
    out = {"source": "oracle/mm_oracle.c", "functions": [FIRST_FN, LAST_FN], "math_modes": modes, "tapes_left_out": a.without,
           "totals": dict(totals, never_run_lines=len(lines), never_taken_outcomes=len(outcomes),
                          never_taken_not_in_cv_unreached=len(unexplained)),
           "never_run_lines": lines, "never_taken_outcomes": outcomes}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["totals"]))
    for o in unexplained:
        print("not explained: line %d (%s) branch %d: %s" % (o["line"], o["function"], o["branch"], o["text"]))


if __name__ == "__main__":
    main()
