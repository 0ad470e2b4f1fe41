"""Diagnostic: the wave-slot timeline of step_kernel launches (stamps build: `make tuning EXTRA="-DMM_STAMPS -DMM_ONLY_G=8
-DMM_ONLY_MIXED=false"`, copied to libmm_hip_stamps.so, or MM_HIP_LIB).

Every wave of the stamps build leaves one record per launch (mm_kernels.hip, g_wave_rec): when it began and ended (s_memtime and
s_memrealtime), where it ran (HW_ID, XCC_ID) and the launch's own counts -- veto passes, MASS rounds, lazy candidates, literal
fallback, re-spawned envs.  This tool steps the benchmark's stationary batch, reads the records of K launches one by one and
writes wave_slots.json into the output directory (MM_OUT_DIR, default profiles/wave_slots/):

  1. slot residency: the waves' lifetimes over (SIMDs x waves per SIMD x launch length);
  2. the idle slot-time split into ramp (before a slot's first wave), gaps (no wave resident between two waves of a slot), tail
     inside an SE (the slot is done, its SE is not), spread between the SEs of an XCD and between XCDs;
  3. the histogram of wave lifetimes;
  4. the share of the lifetime variance each cause accounts for, and what the slowest 1 % of slot sums are made of.

The stamps cost about a tenth of a wave themselves: read the shares, not the lengths.  Clocks: s_memtime is a shader clock
whose origin differs from place to place on the chip, so it gives a wave's LIFETIME only; the waves are placed on one axis by
the 100 MHz s_memrealtime, which all of them share (10 ns = about 24 cycles of resolution), scaled to cycles: a slot -- a
SIMD and one of the two HW_ID wave ids it hands out at two waves per SIMD -- by its first wave's begin, the waves inside it by
the shader clock.
    python tools/wave_slots.py [launches]              (MM_STAMPS_E: envs, default 65536; also writes the raw records to
                                                        wave_records.npy beside the JSON)
    python tools/wave_slots.py --records FILE.npy      (the analysis alone, from such a file: no GPU)
"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("MM_HIP_LIB", os.path.join(REPO, "marl-mass_amd", "csrc", "libmm_hip_stamps.so"))

REC_WORDS, REC_SLOTS, REC_WAVES = 40, 8, 1 << 14
CAUSES = ["veto_passes", "rounds", "lazy_candidates", "respawned_envs", "literal_fallback"]
WAVES_PER_SIMD = 2  # 256 VGPRs
OUT = os.environ.get("MM_OUT_DIR") or os.path.join(REPO, "profiles", "wave_slots")


def decode(rec):
    """Per-wave arrays of one launch from the raw records [W][40]."""
    hw = rec[:, 4] & 0xFFFFFFFF
    d = {"begin": rec[:, 0].astype(np.int64), "end": rec[:, 1].astype(np.int64),
         "rt_begin": rec[:, 2].astype(np.int64), "rt_end": rec[:, 3].astype(np.int64),
         # HW_REG_HW_ID (gfx9): wave_id [3:0], simd_id [5:4], pipe_id [7:6], cu_id [11:8], sh_id [12], se_id [15:13]
         "wave_id": (hw & 0xF).astype(np.int64), "simd": ((hw >> 4) & 3).astype(np.int64), "cu": ((hw >> 8) & 0xF).astype(np.int64),
         "sh": ((hw >> 12) & 1).astype(np.int64), "se": ((hw >> 13) & 7).astype(np.int64),
         "xcc": ((rec[:, 4] >> 32) & 0xF).astype(np.int64)}
    slot = rec[:, REC_SLOTS:REC_SLOTS + 32]
    hi = lambda k: (slot[:, k] >> 32).astype(np.float64)  # noqa: E731  (CAND_COUNT slots: lanes in the low word, wave-level events high)
    d["veto_passes"] = (slot[:, 13] & 0xFFFFFFFF).astype(np.float64)
    d["rounds"] = hi(28)
    d["lazy_candidates"] = hi(18) + hi(22)
    d["literal_fallback"] = hi(19)
    d["respawned_envs"] = rec[:, 5].astype(np.float64)
    return d


def timeline(d):
    """Common time axis, the slots of every SIMD, the idle split and the slot sums of one launch.  A slot is a (SIMD, HW_ID
    wave_id) pair: at two waves per SIMD the hardware reuses the same two wave ids, so the waves of a slot follow each other.
    A slot is placed on the axis by its first wave's real-time begin; inside the slot the shader clock gives begins and ends."""
    life = (d["end"] - d["begin"]).astype(np.float64)
    rt_life = (d["rt_end"] - d["rt_begin"]).astype(np.float64)
    cyc_per_tick = life.sum() / max(rt_life.sum(), 1.0)
    rt_b = (d["rt_begin"] - d["rt_begin"].min()).astype(np.float64) * cyc_per_tick
    simd_key = ((d["xcc"] * 8 + d["se"]) * 2 + d["sh"]) * 64 + d["cu"] * 4 + d["simd"]
    slot_key = simd_key * 16 + d["wave_id"]
    b, e = np.zeros(len(life)), np.zeros(len(life))
    tracks, overlap = [], 0
    order = np.argsort(slot_key * (1 << 20) + np.argsort(np.argsort(d["rt_begin"], kind="stable")), kind="stable")
    keys_sorted = slot_key[order]
    cuts = np.flatnonzero(np.diff(keys_sorted)) + 1
    for idx in np.split(order, cuts):
        idx = idx[np.argsort(d["begin"][idx], kind="stable")]  # (one slot = one place on the chip: one shader-clock origin)
        first = idx[0]
        b[idx] = rt_b[first] + (d["begin"][idx] - d["begin"][first])
        e[idx] = rt_b[first] + (d["end"][idx] - d["begin"][first])
        overlap += int((b[idx][1:] < e[idx][:-1]).sum())
        tracks.append([int(i) for i in idx])
    T = e.max()
    skew = {int(x): float(b[d["xcc"] == x].min()) for x in np.unique(d["xcc"])}  # an XCD's first begin after the launch's first
    se_key, xcc_key = d["xcc"] * 8 + d["se"], d["xcc"]
    se_end = {int(k): e[se_key == k].max() for k in np.unique(se_key)}
    xcc_end = {int(k): e[xcc_key == k].max() for k in np.unique(xcc_key)}
    idle = dict.fromkeys(("ramp", "gaps_no_wave_resident", "tail_inside_se", "spread_between_ses_of_an_xcd", "spread_between_xcds"), 0.0)
    for t in tracks:
        idle["ramp"] += b[t[0]]
        idle["gaps_no_wave_resident"] += sum(b[t[j + 1]] - e[t[j]] for j in range(len(t) - 1))
        sk, xk = int(se_key[t[0]]), int(xcc_key[t[0]])
        idle["tail_inside_se"] += se_end[sk] - e[t[-1]]
        idle["spread_between_ses_of_an_xcd"] += xcc_end[xk] - se_end[sk]
        idle["spread_between_xcds"] += T - xcc_end[xk]
    n_simd = len(np.unique(simd_key))
    per_simd = np.unique(simd_key[[t[0] for t in tracks]], return_counts=True)[1]
    return {"life": life, "b": b, "e": e, "T": T, "tracks": tracks, "n_simd": n_simd, "n_tracks": len(tracks), "max_tracks_per_simd": int(per_simd.max()),
            "waves_begun_before_the_slots_previous_end": overlap, "capacity": len(tracks) * T, "busy": float(life.sum()), "idle": idle,
            "xcd_start_skew_cycles": skew, "cycles_per_realtime_tick": cyc_per_tick}


def ols(X, y):
    A = np.column_stack([np.ones(len(y))] + [X[:, k] for k in range(X.shape[1])])
    coef, *_ = np.linalg.lstsq(A, y, rcond=None)
    res = y - A @ coef
    return coef, 1.0 - res.var() / max(y.var(), 1e-300)


def collect(K, E):
    """The raw records [K][W][40] of K launches on the benchmark's stationary batch."""
    import torch
    from marl_mass_amd import VecMergeEnv, hip_library
    from marl_mass_amd import _cabi as abi
    N = 8
    W = E * 8 // 64
    assert W <= REC_WAVES
    env = VecMergeEnv(E, N, config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5,
                      seed=1000, auto_reset=True)
    env.enable_metrics()
    env.reset()
    env.env_i32[abi.EP["STEPS"]] = ((torch.arange(E, device="cuda:0") * 37) % 100).to(torch.int32)  # stationary batch, as bench.py
    g = torch.Generator(device="cuda:0").manual_seed(123)
    p = torch.tensor([0.1, 0.6, 0.1, 0.1, 0.1], device="cuda:0")
    ring = [torch.multinomial(p, E * N, True, generator=g).view(E, N).int() for _ in range(8)]
    lib = hip_library().lib
    for t in range(100):
        env.step(ring[t % 8])
    torch.cuda.synchronize()
    raw = np.zeros((K, W, REC_WORDS), dtype=np.uint64)
    for t in range(K):
        env.step(ring[t % 8])
        torch.cuda.synchronize()
        rc = lib.mm_debug_read_wave_records(raw[t].ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), ctypes.c_int32(W))
        assert rc == 0, rc
    return raw


def main():
    os.makedirs(OUT, exist_ok=True)
    if len(sys.argv) > 2 and sys.argv[1] == "--records":
        raw = np.load(sys.argv[2])
    else:
        raw = collect(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(os.environ.get("MM_STAMPS_E", "65536")))
        np.save(os.path.join(OUT, "wave_records.npy"), raw)
    K, W = raw.shape[0], raw.shape[1]
    E = W * 64 // 8
    launches = []
    for t in range(K):
        d = decode(raw[t])
        launches.append((d, timeline(d)))
    d0 = launches[0][0]
    seen = {k: sorted(int(x) for x in np.unique(d0[k])) for k in ("xcc", "se", "sh", "cu", "simd", "wave_id")}

    # 1 + 2: residency and the idle split, per launch, then the mean over the launches
    per = []
    for d, tl in launches:
        idle_total = tl["capacity"] - tl["busy"]
        sums = np.array([tl["life"][t].sum() if t else 0.0 for t in tl["tracks"]])
        jobs = np.array([len(t) for t in tl["tracks"]])
        last = int(np.argmax(tl["e"]))
        last_track = next(k for k, t in enumerate(tl["tracks"]) if last in t)
        per.append({"launch_cycles": tl["T"], "simds": tl["n_simd"], "slots": tl["n_tracks"], "slots_per_simd_max": tl["max_tracks_per_simd"], "waves_begun_before_the_slots_previous_end": tl["waves_begun_before_the_slots_previous_end"],
                    "clock_ghz": tl["cycles_per_realtime_tick"] / 10.0,
                    "residency": tl["busy"] / tl["capacity"],
                    "idle_share_of_slot_time": {k: v / tl["capacity"] for k, v in tl["idle"].items()},
                    "idle_split_accounts_for": sum(tl["idle"].values()) / max(idle_total, 1e-9),
                    "waves_per_slot": {str(int(k)): int((jobs == k).sum()) for k in np.unique(jobs)},
                    "launch_over_mean_slot_sum": tl["T"] / sums.mean(),
                    "launch_over_max_slot_sum": tl["T"] / sums.max(),
                    "slot_of_the_last_wave_has_the_largest_sum": bool(sums[last_track] == sums.max()),
                    "rank_of_the_last_waves_slot_sum": int((sums > sums[last_track]).sum()),
                    "max_slot_sum_over_mean": sums.max() / sums.mean(),
                    "xcd_start_skew_cycles_max": max(tl["xcd_start_skew_cycles"].values())})

    def mean_of(f):
        return float(np.mean([f(q) for q in per]))

    # 3: lifetimes, pooled
    life = np.concatenate([tl["life"] for _, tl in launches])
    med = float(np.median(life))
    edges = med * np.array([0.0, 0.80, 0.85, 0.90, 0.95, 1.00, 1.05, 1.10, 1.15, 1.20, 1.30, 1.50, 2.00, 1e9])
    hist, _ = np.histogram(life, bins=edges)
    # 4: causes, pooled over the launches
    X = np.column_stack([np.concatenate([d[c] for d, _ in launches]) for c in CAUSES])
    coef, r2 = ols(X, life)
    cause = {}
    for k, c in enumerate(CAUSES):
        _, r2_without = ols(np.delete(X, k, axis=1), life)
        _, r2_alone = ols(X[:, k:k + 1], life)
        cause[c] = {"mean_per_wave": float(X[:, k].mean()), "share_of_waves_with_any": float((X[:, k] > 0).mean()),
                    "cycles_per_event": float(coef[1 + k]), "cycles_per_event_over_median_lifetime": float(coef[1 + k] / med),
                    "variance_share_alone": float(r2_alone), "variance_share_unique": float(r2 - r2_without)}
    # the placement: how much of the variance the position of the wave (XCD, SE) and its begin time explain on top
    pos = np.column_stack([np.concatenate([(d["xcc"] == x).astype(float) for d, _ in launches]) for x in range(1, 8)] +
                          [np.concatenate([(d["se"] == s).astype(float) for d, _ in launches]) for s in range(1, 8)] +
                          [np.concatenate([tl["b"] / tl["T"] for _, tl in launches])])
    _, r2_pos = ols(np.column_stack([X, pos]), life)
    # the slowest 1 % of slot sums: their excess over the mean slot sum, attributed by the pooled coefficients
    exc = dict.fromkeys(CAUSES + ["unexplained"], 0.0)
    exc_total = 0.0
    for d, tl in launches:
        sums = np.array([tl["life"][t].sum() if t else 0.0 for t in tl["tracks"]])
        csum = np.array([[d[c][t].sum() if t else 0.0 for c in CAUSES] for t in tl["tracks"]])
        top = np.argsort(sums)[-max(1, len(sums) // 100):]
        ex = sums[top] - sums.mean()
        part = (csum[top] - csum.mean(axis=0)) * coef[1:]
        exc_total += ex.sum()
        for k, c in enumerate(CAUSES):
            exc[c] += part[:, k].sum()
        exc["unexplained"] += ex.sum() - part.sum()
    out = {"workload": "%d envs x 8 CAVs, MASS, exact QP, stationary batch (staggered phases + 100-step pre-roll), %d launches read one by one" % (E, K),
           "build": "-DMM_STAMPS -DMM_ONLY_G=8 -DMM_ONLY_MIXED=false (the stamps cost about 10 % of a wave themselves: shares, not lengths)",
           "waves_per_launch": W, "slots_assumed_per_simd": WAVES_PER_SIMD, "hw_id_values_seen_first_launch": seen,
           "1_slot_residency": {"mean": mean_of(lambda q: q["residency"]), "min": min(q["residency"] for q in per), "max": max(q["residency"] for q in per),
                                "simds": per[0]["simds"], "slots": per[0]["slots"], "slots_per_simd_max": max(q["slots_per_simd_max"] for q in per),
                                "waves_begun_before_the_slots_previous_end": sum(q["waves_begun_before_the_slots_previous_end"] for q in per),
                                "shader_clock_ghz_mean": mean_of(lambda q: q["clock_ghz"]),
                                "launch_cycles_mean": mean_of(lambda q: q["launch_cycles"]), "waves_per_slot_first_launch": per[0]["waves_per_slot"]},
           "2_idle_share_of_slot_time": {k: mean_of(lambda q: q["idle_share_of_slot_time"][k]) for k in per[0]["idle_share_of_slot_time"]},
           "2_idle_split_accounts_for_share_of_idle": mean_of(lambda q: q["idle_split_accounts_for"]),
           "2_last_xcd_first_wave_after_launch_start_cycles_mean": mean_of(lambda q: q["xcd_start_skew_cycles_max"]),
           "3_lifetime": {"median_cycles": med, "mean_cycles": float(life.mean()), "std_over_mean": float(life.std() / life.mean()),
                          "percentiles_over_median": {str(q): float(np.percentile(life, q) / med) for q in (1, 5, 25, 50, 75, 90, 95, 99, 99.9, 100)},
                          "histogram_edges_over_median": [float(x) for x in edges[:-1] / med] + ["inf"], "histogram_share": [float(h) / len(life) for h in hist]},
           "4_lifetime_variance": {"explained_by_the_counts_r2": float(r2), "explained_by_counts_and_placement_r2": float(r2_pos), "by_cause": cause},
           "4_slowest_1pct_slot_sums": {"excess_over_mean_slot_sum_share": {k: v / max(exc_total, 1e-9) for k, v in exc.items()}},
           "simulation_check": {"launch_over_mean_slot_sum": mean_of(lambda q: q["launch_over_mean_slot_sum"]),
                                "launch_over_max_slot_sum": mean_of(lambda q: q["launch_over_max_slot_sum"]),
                                "max_slot_sum_over_mean": mean_of(lambda q: q["max_slot_sum_over_mean"]),
                                "launches_whose_last_wave_sits_in_the_slot_with_the_largest_sum": sum(q["slot_of_the_last_wave_has_the_largest_sum"] for q in per),
                                "launches": K, "slots_with_exactly_4_waves_share": mean_of(lambda q: q["waves_per_slot"].get("4", 0) / q["slots"])},
           "per_launch": per}
    path = os.path.join(OUT, "wave_slots.json" if E == 65536 else "wave_slots_E%d.json" % E)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "per_launch"}, indent=1))


if __name__ == "__main__":
    main()
