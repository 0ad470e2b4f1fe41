#!/usr/bin/env python3
"""List-scheduling replay of one launch of the headline step kernel (CPU only; DESIGN.md section 6.2, "slot residency").

8 192 waves on 2 048 wave slots.  Wave lengths: mean 1, the standard deviation measured on the GPU (8.8 % of the mean,
profiles/combined_forms/wave_slots.json), as a normal body plus the spikes of the stamp averages (veto passes, re-spawns, lazy
candidates: + 6 .. 12 % in 8 % of the waves each).  Three dispatchers:

  greedy   the next free slot takes the next wave in launch order -- what a ticket counter in persistent waves would do
  static   slot s runs waves s, s + 2048, ... whatever they cost
  lpt      greedy with the waves sorted costliest first, the cost known up to a prediction of correlation rho

Prints the launch length over the mean slot sum (the measured launch: 1.19) and the share of slots that ran exactly four waves
(measured: 99.95 %).

    python tools/launch_tail_model.py [--seeds 20]
"""
import argparse
import heapq

import numpy as np

WAVES, SLOTS, SIGMA = 8192, 2048, 0.088


def lengths(rs):
    x = np.ones(WAVES)
    for _ in range(3):
        x += np.where(rs.random(WAVES) < 0.08, rs.uniform(0.06, 0.12, WAVES), 0.0)
    body = max(SIGMA ** 2 - x.var(), 0.0) ** 0.5
    x = x + rs.normal(0.0, body, WAVES)
    return np.maximum(x / x.mean(), 0.5)


def greedy(x):
    free = [(0.0, s) for s in range(SLOTS)]
    heapq.heapify(free)
    count = np.zeros(SLOTS, dtype=int)
    end = 0.0
    for w in x:
        t, s = heapq.heappop(free)
        count[s] += 1
        end = max(end, t + w)
        heapq.heappush(free, (t + w, s))
    return end, float((count == WAVES // SLOTS).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    args = ap.parse_args()
    rows = {"greedy": [], "static": []}
    four = []
    rhos = (1.0, 0.75, 0.5, 0.25)
    for rho in rhos:
        rows["lpt rho=%.2f" % rho] = []
    for seed in range(args.seeds):
        rs = np.random.RandomState(seed)
        x = lengths(rs)
        mean_sum = x.sum() / SLOTS
        end, f4 = greedy(x)
        rows["greedy"].append(end / mean_sum)
        four.append(f4)
        rows["static"].append(x.reshape(WAVES // SLOTS, SLOTS).sum(0).max() / mean_sum)
        for rho in rhos:
            z = (x - x.mean()) / x.std()
            pred = rho * z + (1.0 - rho ** 2) ** 0.5 * rs.normal(0.0, 1.0, WAVES)
            rows["lpt rho=%.2f" % rho].append(greedy(x[np.argsort(-pred)])[0] / mean_sum)
    for k, v in rows.items():
        print("%-14s launch / mean slot sum  %.3f  (%.3f .. %.3f)" % (k, np.mean(v), min(v), max(v)))
    print("greedy: %.2f %% of the slots ran exactly four waves" % (100.0 * np.mean(four)))


if __name__ == "__main__":
    main()
