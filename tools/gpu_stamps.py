"""Diagnostic: per-phase cycle shares of step_kernel (build with `make tuning EXTRA="-DMM_STAMPS -DMM_ONLY_G=8 -DMM_ONLY_MIXED=false"`, copy to libmm_hip_stamps.so),
and its second-candidate evaluations by cause (up front from the veto prior, lazily after a veto fired / was lifted, literal fallback), and how often the collision pre-check's 5 m test lets a pair through.
Exact-mode MASS: the round loop alone (its cycles are part of "select+rounds"), rounds per veto pass, and the share of passes in which no
QP is active when evaluated from the MM_ROUNDS_PRIOR seed (round 0 would reproduce the seed in every lane).
MM_HIP_LIB: another stamps library (e.g. one built with -DMM_ROUNDS_PRIOR=0)."""
import ctypes, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("MM_HIP_LIB", os.path.join(REPO, "marl-mass_amd", "csrc", "libmm_hip_stamps.so"))
import torch
from marl_mass_amd import VecMergeEnv, hip_library
shield = sys.argv[1] if len(sys.argv) > 1 else "cbf-cav"
n_hdv = int(sys.argv[2]) if len(sys.argv) > 2 else 0   # mixed traffic: build the stamps library with -DMM_ONLY_MIXED=true
E, N = int(os.environ.get("MM_STAMPS_E", "65536")), 8   # (MM_STAMPS_E=8192: one wave per SIMD, the latency-bound case)
metrics_on = not os.environ.get("MM_BENCH_NO_METRICS")
env = VecMergeEnv(E, N, config={"safety_guarantee": shield, "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5, seed=1000, auto_reset=True, n_hdv=n_hdv)
if metrics_on: env.enable_metrics()
env.reset()
from marl_mass_amd import _cabi as abi
env.env_i32[abi.EP["STEPS"]] = ((torch.arange(E, device="cuda:0") * 37) % 100).to(torch.int32)  # stationary batch, as bench.py
g = torch.Generator(device="cuda:0").manual_seed(123)
p = torch.tensor([0.1, 0.6, 0.1, 0.1, 0.1], device="cuda:0")
ring = [torch.multinomial(p, E * N, True, generator=g).view(E, N).int() for _ in range(8)]
lib = hip_library().lib
buf = (ctypes.c_ulonglong * 16)()
cand = (ctypes.c_ulonglong * 32)()  # second-candidate evaluations by cause (mm_kernels.hip, MM_CS_*): lanes [k], waves [16 + k]
for t in range(100): env.step(ring[t % 8])
torch.cuda.synchronize(); lib.mm_debug_read_stamps(buf, 1); lib.mm_debug_read_cand_stamps(cand, 1)
K = 50
for t in range(K): env.step(ring[t % 8])
torch.cuda.synchronize(); lib.mm_debug_read_stamps(buf, 1); lib.mm_debug_read_cand_stamps(cand, 1)
names = ["load+setup", "act", "predict A", "S1 classify", "select+rounds", "lazy B", "sweep exit/serial", "commit", "collisions", "trace+terminal", "rewards+outputs", "respawn+store", "observation", "(count)", "barrier before obs", "metrics"]
names[5] = "lazy candidate"
round_cycles = cand[11]  # the exact-mode MASS round loop (slot MM_CS_ROUND_CYCLES): billed to "select+rounds" as before
buf[4] += round_cycles
upfront_cycles = cand[0]  # between "predict A" and the veto passes: candidate B up front, from the prior (billed to "S1 classify" before)
tot = sum(buf[k] for k in range(16) if k != 13) + upfront_cycles
waves = E * 8 / 64
for k, nme in enumerate(names):
    if k == 13: continue
    print("%-20s %6.2f %%   %8.0f cycles/wave/step" % (nme, 100.0 * buf[k] / tot, buf[k] / waves / K))
print("%-20s %6.2f %%   %8.0f cycles/wave/step" % ("B up front (prior)", 100.0 * upfront_cycles / tot, upfront_cycles / waves / K))
print("total %.0f cycles/wave/step" % (tot / waves / K))
rounds, passes, seed_active_passes = int(cand[16 + 12]), int(cand[16 + 13]), int(cand[16 + 14])
rounds_out = {"round_loop_cycles_per_wave_step": round_cycles / waves / K, "round_loop_share": round_cycles / tot,
              "selection_gather_static_cycles_per_wave_step": (buf[4] - round_cycles) / waves / K,
              "rounds_per_wave_step": rounds / waves / K, "passes_per_wave_step": passes / waves / K,
              "rounds_per_pass": rounds / max(passes, 1), "cycles_per_round": round_cycles / max(rounds, 1),
              "shielded_lanes_per_pass": cand[13] / max(passes, 1),
              "active_qp_lanes_from_the_seed_per_pass": cand[14] / max(passes, 1),
              "share_of_passes_without_an_active_qp_from_the_seed": 1.0 - seed_active_passes / max(passes, 1),
              "diagnostic_cycles_per_wave_step_not_in_total": cand[15] / waves / K}
for k_, v_ in rounds_out.items(): print("%-60s %12.5f" % (k_, v_))
cand_names = ["", "(a) B up front, from the prior", "(b) B lazily, a veto fired in a pass", "(c) literal fallback", "prior 'vetoed', veto held",
              "prior 'vetoed', veto lifted", "A lazily, the veto of a first-B lane was lifted", "B is the main pass's candidate"]
cand_out = {}
for k in range(1, 8):
    cand_out[cand_names[k]] = {"lanes_per_wave_step": cand[k] / waves / K, "waves_per_wave_step": cand[16 + k] / waves / K}
    print("%-50s %8.4f lanes   %8.4f wave evaluations   per wave and step" % (cand_names[k], cand[k] / waves / K, cand[16 + k] / waves / K))
# collision pre-check: how often `near` (within 5 m) is set -- per (partner, sub-step) evaluation of a wave and per sub-step
pre_checks = int(cand[26])  # wave-sub-steps whose pre-check had a live lane (slot MM_CS_PRECHECK: counted where the pre-check runs, shield or not)
pair_evals = pre_checks * (N - 1)
near_out = {"near_lanes_per_wave_step": cand[8] / waves / K, "wave_partner_substeps_with_a_near_lane_per_wave_step": cand[24] / waves / K,
            "share_of_wave_partner_substeps_with_a_near_lane": cand[24] / max(pair_evals, 1),
            "wave_substeps_with_a_near_lane_per_wave_step": cand[25] / waves / K,
            "share_of_wave_substeps_with_a_near_lane": cand[25] / max(pre_checks, 1),
            "wave_substeps_with_a_live_lane_per_wave_step": pre_checks / waves / K}
for k_, v_ in near_out.items(): print("%-60s %10.5f" % (k_, v_))
import json
out = {"workload": "%d envs x 8 CAVs, %s, stationary batch (staggered phases + 100-step pre-roll), %d steps" % (E, shield, K),
       "build": "-DMM_STAMPS -DMM_ONLY_G=8 -DMM_ONLY_MIXED=false (s_memtime stamps cost ~10 %% themselves)",
       "cycles_per_wave_step": dict({n: buf[k] / waves / K for k, n in enumerate(names) if k != 13}, **{"B up front (prior)": upfront_cycles / waves / K}),
       "total_cycles_per_wave_step": tot / waves / K,
       "share": dict({n: buf[k] / tot for k, n in enumerate(names) if k != 13}, **{"B up front (prior)": upfront_cycles / tot}),
       "second_candidate_evaluations": cand_out,
       "collision_pre_check_near": near_out,
       "mass_rounds": rounds_out,
       "shielded_wave_substeps": int(buf[13]) >> 32, "veto_passes": int(buf[13]) & 0xFFFFFFFF,
       "veto_passes_per_wave_substep": (int(buf[13]) & 0xFFFFFFFF) / max(int(buf[13]) >> 32, 1)}
os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
json.dump(out, open(os.path.join(REPO, "gpurun_out", "phase_cycles_%s%s%s.json" % (shield, "_hdv%d" % n_hdv if n_hdv else "", "" if E == 65536 else "_E%d" % E)), "w"), indent=1)
print("shielded wave-sub-steps %d, veto passes per wave-sub-step %.3f" % (int(buf[13]) >> 32, (int(buf[13]) & 0xFFFFFFFF) / max(int(buf[13]) >> 32, 1)))
