#!/usr/bin/env python3
"""Census of the inputs of tests/test_supervisor_twin_gpu.py, counted by the CPU twin alone (no GPU, no reference): which
branches of the "priority" supervisor the free runs and the placed-state grid go through, and how often.

    python tools/supervisor_census.py        # -> profiles/supervisor_twin/census.json

The GPU test asserts the same conditions on the same inputs every time it runs; this file is their record.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import supervisor_twin_util as U  # noqa: E402
import test_supervisor_twin_gpu as T  # noqa: E402


def main():
    T._CENSUS.clear()
    for name in sorted(T.FREE_RUNS):
        T._free_run(name)
    U.oracle().set_math_mode(1)
    for N in (11, 12):
        st, act = T._placed(N)
        for k, (n_step, sub) in enumerate(T.HORIZONS):
            tw = T._make("oracle", act.shape[0], N, (0.5, 1.2)[k % 2], n_step, sub, n_hdv=1, seed=5)
            T._CENSUS["placed:N%d:%d:%d" % (N, n_step, sub)] = T._supervise_pair(tw, None, st, act, n_step * sub)[3]
    U.oracle().set_math_mode(0)
    union, free, placed = {}, {}, {}
    for key, c in T._CENSUS.items():
        U.add_census(union, c)
        U.add_census(free if key.startswith("free:") else placed, c)
    out = dict(tool="tools/supervisor_census.py", math_mode=1, required_min=U.CENSUS_MIN, free_run_min_replaced=U.FREE_RUN_MIN_REPLACED,
               below_min=[k for k in U.CENSUS_REQUIRED if union[k] < U.CENSUS_MIN], union=union, free_run=free, placed=placed,
               inputs={k: dict(states=c["states"], lookaheads=c["lookaheads"], replaced_actions=c["replaced_actions"]) for k, c in sorted(T._CENSUS.items())},
               unreachable={"replaced_by_2": "LANE_RIGHT is never available: the only higher-numbered side lane, (b, c, 1), is forbidden, "
                                             "so is_reachable_from is False everywhere (see tests/supervisor_twin_util.py)"})
    path = os.path.join(REPO, "profiles", "supervisor_twin", "census.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(below_min=out["below_min"], free_replaced=free["replaced_actions"])))
    return 1 if out["below_min"] or free["replaced_actions"] < U.FREE_RUN_MIN_REPLACED else 0


if __name__ == "__main__":
    sys.exit(main())
