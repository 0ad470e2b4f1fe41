"""ctypes binding of the C ABI in include/mm_abi.h (the drop-in boundary).

Pure plumbing: structures, prototypes and error mapping.  The same binding serves the HIP
library (device pointers) and -- from tests only -- the CPU oracle (host pointers); which
shared object is loaded is decided by the caller, never silently.
"""
import ctypes as C
import os

MM_ABI_VERSION = 6
MM_MAX_AGENTS = 16
ENV_V0, ENV_V1, ENV_HDV_V1 = 0, 1, 2
ENV_IDS = {"merge-multi-agent-v0": ENV_V0, "merge-multi-agent-v1": ENV_V1, "merge-multi-agent-hdv-v1": ENV_HDV_V1}
MIXED_CAV, MIXED_MIXED, MIXED_AV, MIXED_HDV = 0, 1, 2, 3  # MMConfig.mixed_traffic count codes (include/mm_counts.h)
SHIELD_NONE, SHIELD_HSS, SHIELD_MASS = 0, 1, 2

# plane indices (keep in sync with include/mm_abi.h; checked by tests/test_abi.py)
F_PLANES = ["X", "Y", "HEADING", "SPEED", "TARGET_SPEED", "SAFE_STEER", "SAFE_ACC", "G_VX",
            "H1_X", "H1_VX", "H2_X", "H2_VX", "STEER_ANGLE"]
B_PLANES = ["LANE", "TARGET_LANE", "SPEED_INDEX", "CRASHED", "HL_ACTION", "FLAGS", "HIST_LEN", "KIND"]
E_PLANES = ["STEPS", "TIME", "N_MERGE", "EPISODE"]
T_PLANES = ["X", "Y", "HEADING", "SPEED", "ACT_STEER", "ACT_ACC", "SAFE_STEER", "SAFE_ACC", "LANE",
            "TARGET_LANE", "CRASHED", "FLAGS", "QP_ROWS", "QP_A", "QP_H0", "QP_H1", "QP_H2", "QP_H3",
            "QP_D", "LC_MARGIN", "STATUS", "HEADWAY"]
F = {n: i for i, n in enumerate(F_PLANES)}
B = {n: i for i, n in enumerate(B_PLANES)}
EP = {n: i for i, n in enumerate(E_PLANES)}
T = {n: i for i, n in enumerate(T_PLANES)}

FLAG_COLLABORATE_ADJ, FLAG_IS_LC_SAFE, FLAG_IS_COLLABORATING = 1, 2, 4
HL_NONE = 255

ST_RAN, ST_IS_OPTIMAL, ST_IS_SAFE, ST_IS_INVARIANT, ST_IS_LC_SAFE, ST_IS_COLLABORATING, ST_COLLABORATE_ADJ = 1, 2, 4, 8, 16, 32, 64
ST_QP_BOUNDS = 128
QP_EXACT, QP_IPM = 0, 1
QPS_UNKNOWN, QPS_OPTIMAL, QPS_BAD_STRUCTURE = 0, 1, 255
MM_OK, MM_ERR_INVALID_ARG, MM_ERR_NOT_READY, MM_ERR_DEVICE, MM_ERR_QP_BOUNDS = 0, -1, -2, -3, -4

# (from, to, id) lane tuples of the reference <-> lane ids (merge_env_v1.py:231-245)
LANE_INDEX = [("a", "b", 0), ("b", "c", 0), ("b", "c", 1), ("c", "d", 0), ("j", "k", 0), ("k", "b", 0)]
LANE_ID = {l: i for i, l in enumerate(LANE_INDEX)}


class MMStateLayout(C.Structure):
    _fields_ = [("f64_offset", C.c_uint64), ("u8_offset", C.c_uint64), ("env_offset", C.c_uint64),
                ("seed_offset", C.c_uint64), ("total_bytes", C.c_uint64)]


class MMConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("env_kind", C.c_int32), ("shield", C.c_int32),
                ("simulation_frequency", C.c_int32), ("policy_frequency", C.c_int32),
                ("duration", C.c_int32), ("action_masking", C.c_int32), ("auto_reset", C.c_int32),
                ("obs_f64", C.c_int32), ("debug_flags", C.c_int32),
                ("collision_reward", C.c_double), ("high_speed_reward", C.c_double),
                ("headway_cost", C.c_double), ("headway_time", C.c_double),
                ("merging_lane_cost", C.c_double), ("reward_speed_lo", C.c_double),
                ("reward_speed_hi", C.c_double), ("cbf_eta", C.c_double), ("cbf_tau", C.c_double),
                ("seed", C.c_uint64), ("n_hdv", C.c_int32), ("agent_reward", C.c_int32),
                ("lateral_control", C.c_int32), ("qp_solver", C.c_int32),
                ("traffic_density", C.c_int32), ("mixed_traffic", C.c_int32), ("num_cav", C.c_int32), ("reserved1", C.c_int32)]


GEOM_POSE, GEOM_STEER, GEOM_RECT, GEOM_SPEED_INDEX, GEOM_DIV = 0, 1, 2, 3, 4  # mm_geom_eval functions (include/mm_abi.h; GEOM_DIV: device library only)


class MMStepOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "obs", "reward", "done", "agents_rewards", "regional_rewards", "agents_dones", "agents_info",
        "crashed", "average_speed", "traffic_speed", "min_headway", "merge_percent", "action_mask",
        "trace")]


GI_PARAMS = ("W11", "b11", "W12", "b12", "W13", "b13", "W2", "b2", "Wa", "ba", "Wc", "bc")
GI_CRITIC_LOSS = {"mse": 0, "huber": 1}  # MM_GI_CRITIC_* (include/mm_policy_gi_train.h)


class MMGiParams(C.Structure):
    """The twelve parameter (or gradient) pointers of the shared actor-critic (include/mm_policy_gi_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in GI_PARAMS]


MLP_PARAMS = ("W1", "b1", "W2", "b2", "W3", "b3")
PT_CRITIC_LOSS = {"mse": 0, "huber": 1}  # MM_PT_CRITIC_* (include/mm_policy_train.h)


class MMMlpParams(C.Structure):
    """The six parameter (or gradient) pointers of MAPPO's actor or critic (include/mm_policy_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in MLP_PARAMS]


BANK_MAX_GROUPS = 64  # MM_BANK_MAX_GROUPS (include/mm_policy_bank.h): members of one mm_policy_bank_act launch
PT_FORM = {"reference": 0, "per_sample": 1}  # MM_PT_FORM_* (include/mm_policy_bank_train.h)
# the scratch figures of mm_policy_bank_train_scratch_bytes (MM_PBT_*_BYTES): header, per member, per padded sample, per tile,
# per partial block
PBT_HEADER_BYTES, PBT_MEMBER_BYTES, PBT_SAMPLE_BYTES, PBT_TILE_BYTES, PBT_PARTIAL_BYTES = 1024, 131072, 2240, 32, 107584
# the same figures of mm_policy_gi_bank_train_scratch_bytes (MM_GBT_*_BYTES, include/mm_policy_gi_bank_train.h)
GBT_HEADER_BYTES, GBT_MEMBER_BYTES, GBT_SAMPLE_BYTES, GBT_TILE_BYTES, GBT_PARTIAL_BYTES = 1024, 81920, 2496, 40, 111808


OPT_RMSPROP, OPT_ADAM, OPT_BLEND = 0, 1, 2  # MM_OPT_* (include/mm_opt_step.h)
OPT_MAX_TENSORS, OPT_MAX_GROUPS = 16, 4


class MMOptGroup(C.Structure):
    """One network = one clipping group = one optimiser of mm_opt_step (include/mm_opt_step.h)."""
    _fields_ = [("algo", C.c_int32), ("n_tensors", C.c_int32), ("count", C.c_int64 * OPT_MAX_TENSORS),
                ("param", C.c_void_p * OPT_MAX_TENSORS), ("grad", C.c_void_p * OPT_MAX_TENSORS),
                ("state1", C.c_void_p * OPT_MAX_TENSORS), ("state2", C.c_void_p * OPT_MAX_TENSORS),
                ("target", C.c_void_p * OPT_MAX_TENSORS), ("step", C.c_void_p),
                ("lr", C.c_double), ("alpha_or_beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("max_grad_norm", C.c_double), ("tau", C.c_double), ("soft_update", C.c_int32), ("grad_norm", C.c_void_p)]


SUPERVISED = ("priority", "dmc")


def check_supervisor(value):
    """"priority" (the reference's DEFAULT, merge_env_v1.py:47) and "dmc" make AbstractEnv.step rewrite the joint
    action through safety_supervisor / safety_layer_dmc (abstract.py:460-464) -- competing baselines outside
    this path.  Stepping them as if unsupervised would silently change behaviour and safety,
    so step() raises: set "none" or "cbf-*" explicitly, as run_mappo.py does from the .ini.  (reset() is
    unaffected, as in the reference: the supervisor only acts inside step.)"""
    if value in SUPERVISED:
        raise NotImplementedError(
            "safety_guarantee=%r (the reference's action-replacement supervisors, abstract.py:460-464) is not part of "
            "this path: set env.config['safety_guarantee'] to 'none' or 'cbf-*' before stepping" % (value,))


SUP_NONE, SUP_PRIORITY, SUP_DMC = 0, 1, 2  # include/mm_supervisor.h
DMC_LITERAL = 1  # MM_DMC_LITERAL
DMC_TRACE_DOUBLES = 20  # MM_DMC_TRACE_DOUBLES


def supervisor_id(value, env_kind, dmc=False):
    """config["safety_guarantee"] -> the supervisor AbstractEnv.step runs (abstract.py:460-464): SUP_PRIORITY for "priority"
    on merge-multi-agent-v0 (mm_supervise, include/mm_supervisor.h), SUP_NONE for everything without one.  "dmc" and
    "priority" on v1 still raise NotImplementedError through check_supervisor.  merge-multi-agent-hdv-v1 runs none whatever
    the setting: MergeEnvLCHDV.step never calls a supervisor (merge_env_v1.py:604-666).
    dmc=True (the caller opted in, VecMergeEnv(enable_dmc=True)): "dmc" on merge-multi-agent-v0 is SUP_DMC (mm_supervise_dmc);
    on v1 it still raises."""
    if env_kind == ENV_HDV_V1:
        return SUP_NONE
    if value == "priority" and env_kind == ENV_V0:
        return SUP_PRIORITY
    if dmc and value == "dmc" and env_kind == ENV_V0:
        return SUP_DMC
    check_supervisor(value)
    return SUP_NONE


def shield_from_safety_guarantee(value, env_kind=None):
    """config["safety_guarantee"] -> VEHICLE-level shield id, as safe_controller.py:229-241 +
    decentral_layer.py:767-817 dispatch it ("priority" / "dmc" have none: their supervisor sits in
    AbstractEnv.step, see check_supervisor).  Unknown "cbf-*" types raise ValueError like safety_layer does.
    env_kind ENV_HDV_V1: none whatever the setting (no controlled vehicle carries a shield)."""
    if env_kind == ENV_HDV_V1:
        return SHIELD_NONE
    if value in (None, "none") or value in SUPERVISED or "cbf-" not in value:
        return SHIELD_NONE
    kind = value.split("-")[1]
    if kind in ("hss", "av", "avs", "avs_cint"):
        return SHIELD_HSS
    if kind in ("mass", "cav"):
        return SHIELD_MASS
    raise ValueError("Undefined safety_type:{0}".format(kind))


def default_env_config(env_id):
    """Default config of the registered envs (merge_env_v1.py:33-57, :389-437, abstract.py:106-133)."""
    cfg = {
        "simulation_frequency": 15, "policy_frequency": 5, "duration": 20,
        "reward_speed_range": [10, 30], "COLLISION_REWARD": 200, "HIGH_SPEED_REWARD": 1,
        "HEADWAY_COST": 4, "HEADWAY_TIME": 1.2, "MERGING_LANE_COST": 4, "traffic_density": 1,
        "safety_guarantee": "priority", "seed": 0, "action_masking": True, "mixed_traffic": True,
        "controlled_vehicles": 4,
    }
    if env_id == "merge-multi-agent-v1":
        cfg.update({"action_masking": False, "lateral_control": "steer", "traffic_type": "cav",
                    "agent_reward": "default"})
    elif env_id == "merge-multi-agent-hdv-v1":  # MergeEnvLCHDV.default_config (merge_env_v1.py:556-580)
        cfg.update({"action_masking": False, "lateral_control": "steer", "traffic_type": "hdv", "agent_reward": "default",
                    "other_vehicles_type": "highway_env.vehicle.behavior.IDMVehicleHist"})
    elif env_id != "merge-multi-agent-v0":
        raise ValueError("unsupported env id %r (hot path covers merge-multi-agent-v0 / -v1 / -hdv-v1)" % env_id)
    return cfg


def env_kind(env_id):
    """Registered env id -> MMConfig.env_kind (merge_env_v1.py:681-694)."""
    try:
        return ENV_IDS[env_id]
    except KeyError:
        raise ValueError("unsupported env id %r (hot path covers merge-multi-agent-v0 / -v1 / -hdv-v1)" % (env_id,))


def obs_features(env_id):
    """Features per observation row: Kinematics (v0) 5, KinematicLC (v1, hdv-v1) 6 (observation.py:132,228-273)."""
    return 5 if env_kind(env_id) == ENV_V0 else 6


def qp_solver_id(name):
    """'ipm' (the iterate cvxopt's coneqp stops at -- the reference's own behaviour, the default of every entry point) |
    'exact' (the closed-form KKT point: explicit opt-in, outside north_star's 1e-5 of the interior-point iterate)."""
    try:
        return {"exact": QP_EXACT, "ipm": QP_IPM, QP_EXACT: QP_EXACT, QP_IPM: QP_IPM}[name]
    except KeyError:
        raise ValueError("qp_solver must be 'exact' or 'ipm', got %r" % (name,))


def make_config(env_id, config, cbf_eta=0.0, cbf_tau=None, auto_reset=False, obs_f64=False, seed=0, debug_flags=0,
                n_hdv=0, qp_solver="ipm", draw_counts=False, num_cav=0):
    """env.config dict (+ CBFType.GAMMA_B / CBFType.TAU, run_mappo.py:138-139) -> MMConfig."""
    c = MMConfig()
    c.abi_version = MM_ABI_VERSION
    c.env_kind = ENV_IDS.get(env_id, ENV_V0)
    c.shield = shield_from_safety_guarantee(config.get("safety_guarantee")) if c.env_kind == ENV_V1 else SHIELD_NONE
    lat = config.get("lateral_control", "steer") if c.env_kind == ENV_V1 else "steer"
    if lat not in ("steer", "steer_vel"):  # safe_controller.py:181-184
        raise AttributeError("Lateral control: {0} is not supported".format(lat))
    c.lateral_control = 1 if lat == "steer_vel" else 0
    c.simulation_frequency = int(config["simulation_frequency"])
    c.policy_frequency = int(config["policy_frequency"])
    c.duration = int(config["duration"])
    c.action_masking = int(bool(config.get("action_masking", False)))
    c.auto_reset = int(bool(auto_reset))
    c.obs_f64 = int(bool(obs_f64))
    c.debug_flags = int(debug_flags)
    c.collision_reward = float(config["COLLISION_REWARD"])
    c.high_speed_reward = float(config["HIGH_SPEED_REWARD"])
    c.headway_cost = float(config["HEADWAY_COST"])
    c.headway_time = float(config["HEADWAY_TIME"])
    c.merging_lane_cost = float(config["MERGING_LANE_COST"])
    c.reward_speed_lo = float(config["reward_speed_range"][0])
    c.reward_speed_hi = float(config["reward_speed_range"][1])
    c.cbf_eta = float(cbf_eta)
    c.cbf_tau = float(config["HEADWAY_TIME"] if cbf_tau is None else cbf_tau)
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c.n_hdv = int(n_hdv)
    ar = config.get("agent_reward", "default") if c.env_kind == ENV_V1 else "default"
    c.agent_reward = {"srew": 1, "mrew": 2}.get(ar, 0)  # anything else falls back to the default reward (:446)
    c.qp_solver = qp_solver_id(qp_solver)
    # draw_counts: the device reset draws the vehicle counts per episode like MergeEnv._num_vehicles does
    # (config["traffic_density"] 1..3, config["mixed_traffic"]); otherwise every episode has N - n_hdv CAVs + n_hdv HDVs
    c.traffic_density = int(config.get("traffic_density", 1)) if draw_counts else 0
    if draw_counts and c.traffic_density not in (1, 2, 3):
        raise ValueError("traffic_density must be 1, 2 or 3 when the vehicle counts are drawn")
    # MergeEnv._num_vehicles folds the HDVs into the CAVs only when mixed_traffic `is not None and not ...`
    # (merge_env_v1.py:206-209): None -- run_mappo.py's fallback -- means mixed
    mixed = config.get("mixed_traffic", True)
    mixed = 1 if mixed is None else int(bool(mixed))
    if c.env_kind == ENV_V1:  # MergeEnvLCMARL._num_vehicles: traffic_type decides (merge_env_v1.py:476-495)
        tt = config.get("traffic_type", "cav")
        if tt in ("mixed", "cav"):
            mixed = int(tt == "mixed")
        elif tt == "av":  # one CAV, every other drawn vehicle an HDV (:485-489); the total does not depend on mixed_traffic
            mixed = 2
        elif tt == "hdv" and draw_counts:  # no controlled vehicle at all: nothing to step or observe on this path
            raise NotImplementedError("traffic_type='hdv' (zero controlled vehicles) is not supported by the device-side count draw")
    elif c.env_kind == ENV_HDV_V1:  # MergeEnvLCHDV: num_HDV = num_CAV + num_HDV, num_CAV = 0 (merge_env_v1.py:490-494)
        if config.get("traffic_type", "hdv") != "hdv":
            raise NotImplementedError("merge-multi-agent-hdv-v1 is supported with traffic_type='hdv' only")
        mixed = MIXED_HDV
        c.n_hdv = 0  # (every vehicle is an HDV: the library takes no separate HDV count for this env)
    c.mixed_traffic = mixed
    c.num_cav = int(num_cav)
    return c


class CLib(object):
    """One loaded implementation of include/mm_abi.h."""

    SYMBOLS = ["mm_abi_version", "mm_state_layout", "mm_create", "mm_destroy", "mm_set_config",
               "mm_reset", "mm_init_from_kinematics", "mm_observe", "mm_step", "mm_shield_qp",
               "mm_set_metrics_buffer", "mm_last_error", "mm_math_eval", "mm_shield_actions", "mm_sample_actions",
               "mm_policy_act", "mm_poll_errors", "mm_geom_eval", "mm_defer_metrics", "mm_flush_metrics", "mm_discount_returns"]

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError(
                "%s is missing: build it first (python -c 'import __graft_entry__ as g; g.build()')" % path)
        self.path = path
        self.lib = lib = C.CDLL(path)
        vp, i32, u64, i64 = C.c_void_p, C.c_int32, C.c_uint64, C.c_int64
        lib.mm_abi_version.restype = i32
        lib.mm_state_layout.argtypes = [i32, i32, C.POINTER(MMStateLayout)]
        lib.mm_create.argtypes = [C.POINTER(MMConfig), i32, i32, i32, vp, u64, i64, C.POINTER(vp)]
        lib.mm_destroy.argtypes = [vp]
        lib.mm_set_config.argtypes = [vp, C.POINTER(MMConfig)]
        lib.mm_reset.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.mm_init_from_kinematics.argtypes = [vp, vp, vp]
        lib.mm_observe.argtypes = [vp, vp, vp, vp]
        lib.mm_step.argtypes = [vp, vp, C.POINTER(MMStepOut), vp]
        lib.mm_shield_qp.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
        lib.mm_poll_errors.argtypes = [vp, vp]
        lib.mm_set_metrics_buffer.argtypes = [vp, vp]
        lib.mm_defer_metrics.argtypes = [vp, i32, vp]
        lib.mm_flush_metrics.argtypes = [vp, vp]
        lib.mm_discount_returns.argtypes = [vp, vp, vp, i32, i64, i32, C.c_double, C.c_double, vp, vp]
        lib.mm_last_error.argtypes = [vp]
        lib.mm_math_eval.argtypes = [i32, i32, vp, vp, vp, vp]
        lib.mm_geom_eval.argtypes = [i32, i32, vp, vp, vp]
        lib.mm_shield_actions.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.mm_sample_actions.argtypes = [vp, i64, i32, u64, vp, vp, vp]
        lib.mm_policy_act.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp, i32, i32, u64, vp, vp, vp, vp]
        lib.mm_last_error.restype = C.c_char_p
        for s in self.SYMBOLS:
            if s not in ("mm_abi_version", "mm_last_error"):
                getattr(lib, s).restype = i32
        # entry points only libmm_hip.so exports (the oracle has no twin): bound when present, absent -> None
        self.has_supervisor = hasattr(lib, "mm_supervise")
        if self.has_supervisor:
            lib.mm_supervise_scratch_bytes.argtypes = [i32, i32, i32, i32, C.POINTER(u64)]
            lib.mm_supervise_scratch_bytes.restype = i32
            lib.mm_supervise.argtypes = [vp, i32, i32, vp, vp, i32, vp, u64, vp, vp, vp]
            lib.mm_supervise.restype = i32
        # the "dmc" supervisor (include/mm_supervisor.h, mm_supervise_dmc): an optional export like the other late entries
        self.has_supervisor_dmc = hasattr(lib, "mm_supervise_dmc") and hasattr(lib, "mm_supervise_dmc_scratch_bytes")
        if self.has_supervisor_dmc:
            lib.mm_supervise_dmc_scratch_bytes.argtypes = [i32, i32, i32, i32, C.POINTER(u64)]
            lib.mm_supervise_dmc_scratch_bytes.restype = i32
            lib.mm_supervise_dmc.argtypes = [vp, i32, C.c_uint32, vp, vp, i32, vp, u64, vp, vp, vp, vp]
            lib.mm_supervise_dmc.restype = i32
        # MAPPO_GI's shared actor-critic + sample in one launch (include/mm_policy_gi.h), also libmm_hip.so only
        self.has_policy_gi = hasattr(lib, "mm_policy_gi_act")
        if self.has_policy_gi:
            lib.mm_policy_gi_act.argtypes = [vp, i64, i32] + [vp] * 12 + [i32, i32, u64, vp, vp, vp, vp, vp]
            lib.mm_policy_gi_act.restype = i32
        # the hidden-512 actor + sample in one launch (include/mm_policy_wide.h: mm_policy_act's arguments), also
        # libmm_hip.so only; mm_policy_act(hidden = 512) forwards to it
        self.has_policy_wide = hasattr(lib, "mm_policy_wide_act")
        if self.has_policy_wide:
            lib.mm_policy_wide_act.argtypes = list(lib.mm_policy_act.argtypes)
            lib.mm_policy_wide_act.restype = i32
        # K hidden-128 actors on the K contiguous groups of one batch + sample in one launch (include/mm_policy_bank.h), also
        # libmm_hip.so only; mm_policy_bank_grid is its host-side grid split
        self.has_policy_bank = hasattr(lib, "mm_policy_bank_act") and hasattr(lib, "mm_policy_bank_grid")
        if self.has_policy_bank:
            lib.mm_policy_bank_act.argtypes = [vp, i64, i32, C.POINTER(MMMlpParams), i32, C.POINTER(i64), i32, i32, u64, vp, vp, vp, vp]
            lib.mm_policy_bank_act.restype = i32
            lib.mm_policy_bank_grid.argtypes = [i32, C.POINTER(i64), C.POINTER(i32)]
            lib.mm_policy_bank_grid.restype = i32
        # K hidden-128 shared actor-critics on the K contiguous groups of one batch + sample + value in one launch
        # (include/mm_policy_gi_bank.h), also libmm_hip.so only; its grid split is mm_policy_bank_grid
        self.has_policy_gi_bank = hasattr(lib, "mm_policy_gi_bank_act")
        if self.has_policy_gi_bank:
            lib.mm_policy_gi_bank_act.argtypes = [vp, i64, i32, C.POINTER(MMGiParams), i32, C.POINTER(i64), i32, i32, u64, vp, vp, vp, vp, vp]
            lib.mm_policy_gi_bank_act.restype = i32
        # the shared actor-critic's loss + parameter gradient (include/mm_policy_gi_train.h), also libmm_hip.so only
        self.has_policy_gi_train = hasattr(lib, "mm_policy_gi_train")
        if self.has_policy_gi_train:
            f32 = C.c_float
            lib.mm_policy_gi_train_scratch_bytes.argtypes = [i64, C.POINTER(u64)]
            lib.mm_policy_gi_train_scratch_bytes.restype = i32
            lib.mm_policy_gi_train.argtypes = [vp, i64, i64, i32, vp, i64, vp, i64, vp, vp, C.POINTER(MMGiParams), i32, i32, f32,
                                               i32, vp, C.POINTER(MMGiParams), vp, vp, vp, vp, vp, u64, vp]
            lib.mm_policy_gi_train.restype = i32
        # MAPPO's separate actor + critic: loss + gradients and the forward-only evaluation (include/mm_policy_train.h),
        # also libmm_hip.so only
        self.has_policy_train = hasattr(lib, "mm_policy_train")
        if self.has_policy_train:
            f32, pp = C.c_float, C.POINTER(MMMlpParams)
            lib.mm_policy_eval.argtypes = [vp, i64, i64, i32, vp, i64, vp, pp, pp, i32, i32, vp, vp, vp]
            lib.mm_policy_eval.restype = i32
            lib.mm_policy_train_scratch_bytes.argtypes = [i64, C.POINTER(u64)]
            lib.mm_policy_train_scratch_bytes.restype = i32
            lib.mm_policy_train.argtypes = [vp, i64, i64, i32, vp, i64, vp, i64, vp, vp, pp, pp, i32, i32, f32, i32, vp, vp, pp, pp,
                                            vp, vp, vp, vp, vp, u64, vp]
            lib.mm_policy_train.restype = i32
        # both gradient entries in passes of `chunk` samples under a fixed scratch budget (the same two headers): the
        # unchunked entry's arguments and the chunk
        self.has_policy_gi_train_chunked = self.has_policy_gi_train and hasattr(lib, "mm_policy_gi_train_chunked")
        if self.has_policy_gi_train_chunked:
            lib.mm_policy_gi_train_chunked_scratch_bytes.argtypes = [i64, i64, C.POINTER(u64)]
            lib.mm_policy_gi_train_chunked_scratch_bytes.restype = i32
            lib.mm_policy_gi_train_chunked.argtypes = list(lib.mm_policy_gi_train.argtypes) + [i64]
            lib.mm_policy_gi_train_chunked.restype = i32
        self.has_policy_train_chunked = self.has_policy_train and hasattr(lib, "mm_policy_train_chunked")
        if self.has_policy_train_chunked:
            lib.mm_policy_train_chunked_scratch_bytes.argtypes = [i64, i64, C.POINTER(u64)]
            lib.mm_policy_train_chunked_scratch_bytes.restype = i32
            lib.mm_policy_train_chunked.argtypes = list(lib.mm_policy_train.argtypes) + [i64]
            lib.mm_policy_train_chunked.restype = i32
        # the same two gradients over a batch sharded over ranks (mm_policy_sharded.hip, the same two headers): `partial` is the
        # chunked entry without gradients and loss, with the whole batch's count and the shard block; `finish` folds R blocks
        sharded = lambda fam: all(hasattr(lib, "mm_policy_%s_%s" % (fam, s)) for s in ("shard_bytes", "partial", "finish"))  # noqa: E731
        self.has_policy_gi_train_sharded = self.has_policy_gi_train_chunked and sharded("gi_train")
        if self.has_policy_gi_train_sharded:
            a = list(lib.mm_policy_gi_train_chunked.argtypes)  # [16] grads, [17] loss -> count, shard
            lib.mm_policy_gi_train_shard_bytes.argtypes = [C.POINTER(u64)]
            lib.mm_policy_gi_train_shard_bytes.restype = i32
            lib.mm_policy_gi_train_partial.argtypes = a[:16] + [vp, vp] + a[18:]
            lib.mm_policy_gi_train_partial.restype = i32
            lib.mm_policy_gi_train_finish.argtypes = [vp, i32, i64, i32, i32, C.POINTER(MMGiParams), vp, vp]
            lib.mm_policy_gi_train_finish.restype = i32
        self.has_policy_train_sharded = self.has_policy_train_chunked and sharded("train")
        if self.has_policy_train_sharded:
            a = list(lib.mm_policy_train_chunked.argtypes)  # [18], [19] the gradients, [20] loss -> count, shard
            lib.mm_policy_train_shard_bytes.argtypes = [C.POINTER(u64)]
            lib.mm_policy_train_shard_bytes.restype = i32
            lib.mm_policy_train_partial.argtypes = a[:18] + [vp, vp] + a[21:]
            lib.mm_policy_train_partial.restype = i32
            lib.mm_policy_train_finish.argtypes = [vp, i32, i64, i32, i32, C.POINTER(MMMlpParams), C.POINTER(MMMlpParams), vp, vp]
            lib.mm_policy_train_finish.restype = i32
        # the same two entries and the scratch query at hidden 512 (include/mm_policy_wide_train.h: mm_policy_eval's and
        # mm_policy_train's arguments), also libmm_hip.so only
        self.has_policy_wide_train = self.has_policy_train and all(
            hasattr(lib, s) for s in ("mm_policy_wide_train", "mm_policy_wide_eval", "mm_policy_wide_train_scratch_bytes"))
        if self.has_policy_wide_train:
            lib.mm_policy_wide_eval.argtypes = list(lib.mm_policy_eval.argtypes)
            lib.mm_policy_wide_eval.restype = i32
            lib.mm_policy_wide_train_scratch_bytes.argtypes = [i64, C.POINTER(u64)]
            lib.mm_policy_wide_train_scratch_bytes.restype = i32
            lib.mm_policy_wide_train.argtypes = list(lib.mm_policy_train.argtypes)
            lib.mm_policy_wide_train.restype = i32
        # and its form in passes of `chunk` samples under a fixed scratch budget: the unchunked entry's arguments and the chunk
        self.has_policy_wide_train_chunked = self.has_policy_wide_train and all(
            hasattr(lib, s) for s in ("mm_policy_wide_train_chunked", "mm_policy_wide_train_chunked_scratch_bytes"))
        if self.has_policy_wide_train_chunked:
            lib.mm_policy_wide_train_chunked_scratch_bytes.argtypes = [i64, i64, C.POINTER(u64)]
            lib.mm_policy_wide_train_chunked_scratch_bytes.restype = i32
            lib.mm_policy_wide_train_chunked.argtypes = list(lib.mm_policy_wide_train.argtypes) + [i64]
            lib.mm_policy_wide_train_chunked.restype = i32
        # and over a batch sharded over ranks (mm_policy_sharded.hip): the argument lists of mm_policy_train_partial /
        # mm_policy_train_finish, hidden 512
        self.has_policy_wide_train_sharded = self.has_policy_wide_train_chunked and sharded("wide_train")
        if self.has_policy_wide_train_sharded:
            a = list(lib.mm_policy_wide_train_chunked.argtypes)  # [18], [19] the gradients, [20] loss -> count, shard
            lib.mm_policy_wide_train_shard_bytes.argtypes = [C.POINTER(u64)]
            lib.mm_policy_wide_train_shard_bytes.restype = i32
            lib.mm_policy_wide_train_partial.argtypes = a[:18] + [vp, vp] + a[21:]
            lib.mm_policy_wide_train_partial.restype = i32
            lib.mm_policy_wide_train_finish.argtypes = [vp, i32, i64, i32, i32, C.POINTER(MMMlpParams), C.POINTER(MMMlpParams), vp, vp]
            lib.mm_policy_wide_train_finish.restype = i32
        # clip_grad_norm_ + RMSprop / Adam + soft target update in one launch (include/mm_opt_step.h), also libmm_hip.so only
        self.has_opt_step = hasattr(lib, "mm_opt_step")
        if self.has_opt_step:
            lib.mm_opt_step.argtypes = [C.POINTER(MMOptGroup), i32, vp]
            lib.mm_opt_step.restype = i32
        # the policy bank's training half: K actor / critic pairs on the K column groups of one batch (include/
        # mm_policy_bank_train.h) and the K optimiser tails (mm_opt_step_bank, include/mm_opt_step.h), also libmm_hip.so only
        self.has_policy_bank_train = self.has_policy_train and self.has_opt_step and all(
            hasattr(lib, s) for s in ("mm_policy_bank_eval", "mm_policy_bank_train", "mm_policy_bank_train_scratch_bytes",
                                      "mm_opt_step_bank"))
        if self.has_policy_bank_train:
            f32, pp, pi64 = C.c_float, C.POINTER(MMMlpParams), C.POINTER(i64)
            lib.mm_policy_bank_eval.argtypes = [vp, i64, i64, i64, i32, vp, i64, vp, pp, pp, i32, pi64, i32, i32, vp, vp, vp]
            lib.mm_policy_bank_eval.restype = i32
            lib.mm_policy_bank_train_scratch_bytes.argtypes = [i64, i64, i32, pi64, C.POINTER(u64)]
            lib.mm_policy_bank_train_scratch_bytes.restype = i32
            lib.mm_policy_bank_train.argtypes = [vp, i64, i64, i64, i32, vp, i64, vp, i64, vp, vp, pp, pp, i32, pi64, i32, i32, f32,
                                                 i32, i32, vp, vp, pp, pp, vp, vp, vp, vp, vp, vp, u64, vp]
            lib.mm_policy_bank_train.restype = i32
            lib.mm_opt_step_bank.argtypes = [C.POINTER(MMOptGroup), i32, i32, u64, vp]
            lib.mm_opt_step_bank.restype = i32
        # the training half of the bank of shared actor-critics: K shared networks on the K column groups of one batch
        # (include/mm_policy_gi_bank_train.h); its optimiser tail is mm_opt_step_bank.  Also libmm_hip.so only
        self.has_policy_gi_bank_train = self.has_policy_gi_train and self.has_policy_gi_bank and all(
            hasattr(lib, s) for s in ("mm_policy_gi_bank_eval", "mm_policy_gi_bank_train", "mm_policy_gi_bank_train_scratch_bytes",
                                      "mm_opt_step_bank"))
        if self.has_policy_gi_bank_train:
            f32, pg, pi64 = C.c_float, C.POINTER(MMGiParams), C.POINTER(i64)
            lib.mm_policy_gi_bank_eval.argtypes = [vp, i64, i64, i64, i32, vp, i64, vp, pg, i32, pi64, i32, i32, vp, vp, vp]
            lib.mm_policy_gi_bank_eval.restype = i32
            lib.mm_policy_gi_bank_train_scratch_bytes.argtypes = [i64, i64, i32, pi64, C.POINTER(u64)]
            lib.mm_policy_gi_bank_train_scratch_bytes.restype = i32
            lib.mm_policy_gi_bank_train.argtypes = [vp, i64, i64, i64, i32, vp, i64, vp, i64, vp, vp, pg, i32, pi64, i32, i32, f32, i32,
                                                    i32, vp, pg, vp, vp, vp, vp, vp, vp, u64, vp]
            lib.mm_policy_gi_bank_train.restype = i32
            lib.mm_opt_step_bank.argtypes = [C.POINTER(MMOptGroup), i32, i32, u64, vp]
            lib.mm_opt_step_bank.restype = i32
        # per-env cbf_eta / cbf_tau / HEADWAY_TIME planes (include/mm_env_params.h), also libmm_hip.so only
        self.has_env_params = hasattr(lib, "mm_set_env_params")
        if self.has_env_params:
            lib.mm_set_env_params.argtypes = [vp, vp]
            lib.mm_set_env_params.restype = i32
        if lib.mm_abi_version() != MM_ABI_VERSION:
            raise RuntimeError("ABI version mismatch in %s" % path)

    def check(self, rc, handle=None):
        """Map C status codes to the exception types the reference raises (SURVEY 8b 'errors')."""
        if rc == MM_OK:
            return
        msg = self.lib.mm_last_error(handle if handle else None).decode()  # (no handle: why the last mm_create refused)
        if rc in (MM_ERR_INVALID_ARG, MM_ERR_QP_BOUNDS):
            raise ValueError(msg or "invalid argument")
        if rc == MM_ERR_NOT_READY:
            raise NotImplementedError(msg or "The road and vehicle must be initialized in the environment implementation")
        raise RuntimeError("mm error %d: %s" % (rc, msg))

    def supervise_scratch_bytes(self, E, N, n_step, sub_steps=3):
        """Bytes of the lookahead scratch mm_supervise needs (include/mm_supervisor.h); sub_steps =
        simulation_frequency // policy_frequency."""
        self.require_supervisor()
        b = C.c_uint64()
        self.check(self.lib.mm_supervise_scratch_bytes(E, N, n_step, sub_steps, C.byref(b)))
        return b.value

    def supervise_dmc_scratch_bytes(self, E, N, n_step, sub_steps=3):
        """Bytes of the scratch mm_supervise_dmc needs (include/mm_supervisor.h)."""
        if not self.has_supervisor_dmc:
            raise NotImplementedError("%s does not export mm_supervise_dmc: safety_guarantee='dmc' needs the HIP library"
                                      % os.path.basename(self.path))
        b = C.c_uint64()
        self.check(self.lib.mm_supervise_dmc_scratch_bytes(E, N, n_step, sub_steps, C.byref(b)))
        return b.value

    def require_env_params(self):
        if not self.has_env_params:
            raise NotImplementedError("%s does not export mm_set_env_params: per-env cbf_eta / cbf_tau / HEADWAY_TIME need the "
                                      "HIP library" % os.path.basename(self.path))

    def require_supervisor(self):
        if not self.has_supervisor:
            raise NotImplementedError("%s does not export mm_supervise: safety_guarantee='priority' needs the HIP library"
                                      % os.path.basename(self.path))

    def require_policy_gi(self):
        if not self.has_policy_gi:
            raise NotImplementedError("%s does not export mm_policy_gi_act: the fused shared actor-critic needs the HIP library"
                                      % os.path.basename(self.path))

    def require_policy_wide(self):
        if not self.has_policy_wide:
            raise NotImplementedError("%s does not export mm_policy_wide_act: the fused hidden-512 actor needs the HIP library"
                                      % os.path.basename(self.path))

    def require_policy_bank(self):
        if not self.has_policy_bank:
            raise NotImplementedError("%s does not export mm_policy_bank_act: the one-launch policy bank needs the HIP library"
                                      % os.path.basename(self.path))

    def require_policy_gi_bank(self):
        if not self.has_policy_gi_bank:
            raise NotImplementedError("%s does not export mm_policy_gi_bank_act: the one-launch bank of shared actor-critics "
                                      "needs the HIP library" % os.path.basename(self.path))

    def require_policy_gi_train(self):
        if not self.has_policy_gi_train:
            raise NotImplementedError("%s does not export mm_policy_gi_train: the shared actor-critic's gradient needs the HIP "
                                      "library" % os.path.basename(self.path))

    def policy_gi_train_scratch_bytes(self, n):
        """Bytes of scratch mm_policy_gi_train needs for n samples (include/mm_policy_gi_train.h)."""
        self.require_policy_gi_train()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_gi_train_scratch_bytes(n, C.byref(b)))
        return b.value

    def require_policy_gi_train_chunked(self):
        if not self.has_policy_gi_train_chunked:
            raise NotImplementedError("%s does not export mm_policy_gi_train_chunked: the shared actor-critic's gradient under a "
                                      "scratch budget needs the HIP library" % os.path.basename(self.path))

    def policy_gi_train_chunked_scratch_bytes(self, n, chunk):
        """Bytes of scratch mm_policy_gi_train_chunked needs for n samples in passes of chunk (include/mm_policy_gi_train.h)."""
        self.require_policy_gi_train_chunked()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_gi_train_chunked_scratch_bytes(n, chunk, C.byref(b)))
        return b.value

    def require_policy_train(self):
        if not self.has_policy_train:
            raise NotImplementedError("%s does not export mm_policy_train: the separate actor's and critic's gradients need the "
                                      "HIP library" % os.path.basename(self.path))

    def policy_train_scratch_bytes(self, n):
        """Bytes of scratch mm_policy_train needs for n samples (include/mm_policy_train.h)."""
        self.require_policy_train()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_train_scratch_bytes(n, C.byref(b)))
        return b.value

    def require_policy_train_chunked(self):
        if not self.has_policy_train_chunked:
            raise NotImplementedError("%s does not export mm_policy_train_chunked: the separate actor's and critic's gradients "
                                      "under a scratch budget need the HIP library" % os.path.basename(self.path))

    def policy_train_chunked_scratch_bytes(self, n, chunk):
        """Bytes of scratch mm_policy_train_chunked needs for n samples in passes of chunk (include/mm_policy_train.h)."""
        self.require_policy_train_chunked()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_train_chunked_scratch_bytes(n, chunk, C.byref(b)))
        return b.value

    def require_policy_gi_train_sharded(self):
        if not self.has_policy_gi_train_sharded:
            raise NotImplementedError("%s does not export mm_policy_gi_train_partial / _finish: the shared actor-critic's gradient "
                                      "over rank-sharded batches needs the HIP library" % os.path.basename(self.path))

    def require_policy_train_sharded(self):
        if not self.has_policy_train_sharded:
            raise NotImplementedError("%s does not export mm_policy_train_partial / _finish: the separate actor's and critic's "
                                      "gradients over rank-sharded batches need the HIP library" % os.path.basename(self.path))

    def policy_gi_train_shard_doubles(self):
        """Doubles of the shared network's shard block (include/mm_policy_gi_train.h: MM_GI_SHARD_DOUBLES)."""
        self.require_policy_gi_train_sharded()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_gi_train_shard_bytes(C.byref(b)))
        return b.value // 8

    def policy_train_shard_doubles(self):
        """Doubles of the separate networks' shard block (include/mm_policy_train.h: MM_PT_SHARD_DOUBLES)."""
        self.require_policy_train_sharded()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_train_shard_bytes(C.byref(b)))
        return b.value // 8

    def require_policy_wide_train(self):
        if not self.has_policy_wide_train:
            raise NotImplementedError("%s does not export mm_policy_wide_train: the hidden-512 actor's and critic's gradients "
                                      "need the HIP library" % os.path.basename(self.path))

    def policy_wide_train_scratch_bytes(self, n):
        """Bytes of scratch mm_policy_wide_train needs for n samples (include/mm_policy_wide_train.h)."""
        self.require_policy_wide_train()
        if n < 0:
            raise ValueError("n must be >= 0, got %d" % n)
        b = C.c_uint64()
        self.check(self.lib.mm_policy_wide_train_scratch_bytes(n, C.byref(b)))
        return b.value

    def require_policy_wide_train_chunked(self):
        if not self.has_policy_wide_train_chunked:
            raise NotImplementedError("%s does not export mm_policy_wide_train_chunked: the hidden-512 actor's and critic's "
                                      "gradients under a scratch budget need the HIP library" % os.path.basename(self.path))

    def policy_wide_train_chunked_scratch_bytes(self, n, chunk):
        """Bytes of scratch mm_policy_wide_train_chunked needs for n samples in passes of chunk (include/mm_policy_wide_train.h)."""
        self.require_policy_wide_train_chunked()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_wide_train_chunked_scratch_bytes(n, chunk, C.byref(b)))
        return b.value

    def require_policy_wide_train_sharded(self):
        if not self.has_policy_wide_train_sharded:
            raise NotImplementedError("%s does not export mm_policy_wide_train_partial / _finish: the hidden-512 actor's and "
                                      "critic's gradients over rank-sharded batches need the HIP library"
                                      % os.path.basename(self.path))

    def policy_wide_train_shard_doubles(self):
        """Doubles of the hidden-512 networks' shard block (include/mm_policy_wide_train.h: MM_PW_SHARD_DOUBLES)."""
        self.require_policy_wide_train_sharded()
        b = C.c_uint64()
        self.check(self.lib.mm_policy_wide_train_shard_bytes(C.byref(b)))
        return b.value // 8

    def require_policy_bank_train(self):
        if not self.has_policy_bank_train:
            raise NotImplementedError("%s does not export mm_policy_bank_train: training the policy bank's members in one "
                                      "launch set needs the HIP library" % os.path.basename(self.path))

    def policy_bank_train_scratch_bytes(self, rows, row_len, col_start):
        """Bytes of scratch mm_policy_bank_train needs (include/mm_policy_bank_train.h); col_start: the K + 1 column prefix."""
        self.require_policy_bank_train()
        b = C.c_uint64()
        cs = (C.c_int64 * len(col_start))(*col_start)
        self.check(self.lib.mm_policy_bank_train_scratch_bytes(rows, row_len, len(col_start) - 1, cs, C.byref(b)))
        return b.value

    def require_policy_gi_bank_train(self):
        if not self.has_policy_gi_bank_train:
            raise NotImplementedError("%s does not export mm_policy_gi_bank_train: training the bank's shared actor-critic members "
                                      "in one launch set needs the HIP library" % os.path.basename(self.path))

    def policy_gi_bank_train_scratch_bytes(self, rows, row_len, col_start):
        """Bytes of scratch mm_policy_gi_bank_train needs (include/mm_policy_gi_bank_train.h); col_start: the K + 1 column prefix."""
        self.require_policy_gi_bank_train()
        b = C.c_uint64()
        cs = (C.c_int64 * len(col_start))(*col_start)
        self.check(self.lib.mm_policy_gi_bank_train_scratch_bytes(rows, row_len, len(col_start) - 1, cs, C.byref(b)))
        return b.value

    def opt_step_bank(self, groups, K, soft_mask, stream):
        """mm_opt_step_bank on a sequence of prototype MMOptGroup (include/mm_opt_step.h)."""
        if not self.has_policy_gi_bank_train:
            self.require_policy_bank_train()
        arr = (MMOptGroup * len(groups))(*groups)
        self.check(self.lib.mm_opt_step_bank(arr, len(groups), K, soft_mask, stream))

    def require_opt_step(self):
        if not self.has_opt_step:
            raise NotImplementedError("%s does not export mm_opt_step: the fused optimiser step needs the HIP library"
                                      % os.path.basename(self.path))

    def opt_step(self, groups, stream):
        """mm_opt_step on a sequence of MMOptGroup (include/mm_opt_step.h); stream: the hipStream_t as c_void_p."""
        self.require_opt_step()
        arr = (MMOptGroup * len(groups))(*groups)
        self.check(self.lib.mm_opt_step(arr, len(groups), stream))

    def state_layout(self, E, N):
        lay = MMStateLayout()
        self.check(self.lib.mm_state_layout(E, N, C.byref(lay)))
        return lay
