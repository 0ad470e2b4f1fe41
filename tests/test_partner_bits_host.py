"""What a lane sees of a partner in the classification pass, from rank words and from the rank scan's bits (CPU only), and
the placed batch of tests/test_partner_bits_gpu.py.

Part 1 restates both forms of marl-mass_amd/csrc/mm_kernels.hip (step_kernel, the `kMailbox` branch of the pass's partner
loop and its `kPBits` branch) and compares, for every reader a and partner p of a group, the image the reader selects, `o_first`
and "present":

  rank words   every lane posts `rank | 99 if not live`, bit 8 = "the candidate I commit is B"; the reader takes the partner's
               word, then its candidate image A or B if the partner steps before it, else the pre-step image;
  scan bits    the reader keeps `before_p = live_p & (x_p > x_a | (x_p == x_a & p < a))` and `plive_p = live_p` from the rank scan
               and reads the partner's fixed post image -- kept equal to the candidate the partner commits -- or its pre-step
               image; a reader that is not live takes `plive_p` for `before_p`.

exhaustively for G = 2, 4 (every subset of live lanes, every x in {0, 1, 2}^G -- ties in both index orders --, every use_B
assignment) and for G = 8 over every live subset and x pattern with the use_B assignments USE_B_8 (none, all, the two
alternating patterns, two nibbles and two irregular ones).  The post image's upkeep (written with the main pass's candidate,
re-published by the lanes whose use_B flipped) is replayed over sequences of flips, and the pairwise predicate is checked to
order live lanes exactly as `rank` does, with rank the population count of the `before` bits.

Part 2 is the placed batch: the scenes of tests/test_act_frame_host.py, a pair at bit-equal x, IS_LC_SAFE cleared before the
second edit so that the prior starts lane changes from B, and a lane-change-heavy action tape.  What the batch must hold is
counted from the oracle's planes and per-sub-step trace, per case of the GPU test:

  tie_lo / tie_hi   (reader, partner) pairs of live vehicles at bit-equal x at the start of a sub-step, partner index below / above
  early_end         envs whose episode ends in sub-step 0 or 1 of a step (their lanes are not live for the rest of the launch)
  crashed           crashed vehicles whose shield runs
  veto_from_A       sub-steps in which a veto fires on a vehicle that started from candidate A
  lift_with_follower   sub-steps in which the veto of a vehicle that started from B is lifted while a shielded vehicle behind it
                    steps after it (a second pass reads the re-published post image)
  respawn           envs whose episode counter moves inside the stepped window
"""
import functools
import itertools

import numpy as np
import torch

import oracle_env
import test_act_frame_host as A
import test_candidate_prior_host as CP
import test_scan_selects_host as H
from marl_mass_amd import _cabi as abi

# ---- part 1: the two forms ------------------------------------------------------------------------------------------------------
USE_B_8 = (0x00, 0xFF, 0x55, 0xAA, 0x0F, 0xF0, 0x2D, 0xC6)  # the stated sample at G = 8 (bit i: lane i commits B)


def _ranks(live, x):
    """rank_i = live j with x_j > x_i, or x_j == x_i and j < i (Road.act order: x descending, stable).  [..., G] arrays."""
    G = x.shape[-1]
    idx = np.arange(G)
    ahead = (x[..., None, :] > x[..., :, None]) | ((x[..., None, :] == x[..., :, None]) & (idx[None, :] < idx[:, None]))
    return (ahead & live[..., None, :]).sum(-1)


def parent_form(live, x, use_b):
    """[..., a, p]: image id, o_first, present, from rank words.  Image ids: 0 pre-step, 1 candidate A, 2 candidate B."""
    rank = _ranks(live, x)
    word = np.where(live, rank, 99) | np.where(use_b, 256, 0)
    p_rank = (word & 255)[..., None, :]
    i_first = live[..., :, None] & (rank[..., :, None] < p_rank)
    committed = ~i_first & (p_rank < 99)
    image = np.where(committed, np.where((word & 256)[..., None, :] != 0, 2, 1), 0)
    return image, committed, np.broadcast_to(p_rank < 99, image.shape)


def scan_bits(live, x):
    """before[..., a, p], plive[..., a, p] as the rank scan of lane a forms them, and the word a lane carries into the passes."""
    G = x.shape[-1]
    idx = np.arange(G)
    plive = np.broadcast_to(live[..., None, :], live.shape + (G,))
    before = plive & ((x[..., None, :] > x[..., :, None]) | ((x[..., None, :] == x[..., :, None]) & (idx[None, :] < idx[:, None])))
    return before, plive


def new_form(live, x, post_image):
    """[..., a, p]: image id, o_first, present, from the scan's bits; post_image[..., p]: what lane p's post image holds."""
    before, plive = scan_bits(live, x)
    sees = np.where(live[..., :, None], before, plive)  # a lane that is not live: every live partner's committed image
    image = np.where(sees, post_image[..., None, :], 0)
    return image, sees, plive


def _off_diagonal(G):
    return ~np.eye(G, dtype=bool)


def _compare(live, x, use_b):
    post = np.where(use_b, 2, 1)  # the post image holds the candidate the lane commits
    G = x.shape[-1]
    m = _off_diagonal(G)
    for got, want in zip(new_form(live, x, post), parent_form(live, x, use_b)):
        assert ((got == want) | ~m).all()  # (every reader and partner; a lane is no partner of itself)


def _patterns(G):
    return np.array(list(itertools.product((0.0, 1.0, 2.0), repeat=G)))  # every x in {0, 1, 2}^G: ties in both index orders


def _bits(n, G):
    return np.array([[(k >> i) & 1 for i in range(G)] for k in n], dtype=bool)


def test_both_forms_select_the_same_image_small_groups():
    for G in (2, 4):
        xs = _patterns(G)
        sets = _bits(range(1 << G), G)
        for live in sets:
            for use_b in sets:
                _compare(np.broadcast_to(live, xs.shape), xs, np.broadcast_to(use_b, xs.shape))


def test_both_forms_select_the_same_image_eight_lanes():
    xs = _patterns(8)[None]
    ub = _bits(USE_B_8, 8)[:, None, :]  # (the assignments ride in a leading axis: ranks and bits are formed once per live subset)
    for live in _bits(range(256), 8):
        _compare(np.broadcast_to(live, xs.shape), xs, ub)


def test_every_selection_occurs():
    """The comparison above is not vacuous: each image, a reader that is not live, an absent partner and ties occur."""
    xs = _patterns(4)
    seen = set()
    for live in _bits(range(16), 4):
        for use_b in _bits(range(16), 4):
            lv, ubb = np.broadcast_to(live, xs.shape), np.broadcast_to(use_b, xs.shape)
            image, o_first, present = parent_form(lv, xs, ubb)
            m = _off_diagonal(4)
            code = image[..., m] * 4 + o_first[..., m] * 2 + np.broadcast_to(present, image.shape)[..., m]
            seen |= {(int(c) >> 2, bool(c & 2), bool(c & 1)) for c in np.unique(code)}
    assert seen == {(0, False, False), (0, False, True), (1, True, True), (2, True, True)}, seen


def test_the_pairwise_predicate_orders_live_lanes_as_rank_does():
    for G in (2, 4, 8):
        xs = _patterns(G)
        m = _off_diagonal(G)
        for live in _bits(range(1 << G), G):
            lv = np.broadcast_to(live, xs.shape)
            rank = _ranks(lv, xs)
            before, plive = scan_bits(lv, xs)
            before = before & m  # (a lane is no partner of itself)
            assert np.array_equal(before.sum(-1), rank)  # rank = population count of the `before` bits
            both = lv[..., :, None] & lv[..., None, :] & m
            assert np.array_equal((rank[..., None, :] < rank[..., :, None])[both], before[both])
            assert not (before & np.swapaxes(before, -1, -2))[both].any()  # strict: never both ways
            assert (before | np.swapaxes(before, -1, -2))[both].all()      # total: always one way
            lr = np.where(lv, rank, -1)
            for r in range(int(live.sum())):  # the live lanes hold the ranks 0 .. n_live - 1 once each
                assert ((lr == r).sum(-1) == 1).all()


def test_the_post_image_follows_the_flips():
    """pass 0: the main pass parks its candidate (B iff first_B) in the post image; after a pass the lanes whose use_B flipped copy
    their other candidate image.  Before every pass the post image is the candidate the lane commits."""
    g = np.random.default_rng(5)
    for G in (2, 4, 8):
        for _ in range(200):
            first_b = g.integers(0, 2, G).astype(bool)
            use_b = first_b.copy()
            post = np.where(first_b, 2, 1)
            for _pass in range(G + 1):
                assert np.array_equal(post, np.where(use_b, 2, 1))
                want_b = np.where(g.random(G) < 0.3, ~use_b, use_b)
                flip = want_b != use_b
                use_b = want_b
                if not flip.any():
                    break
                post = np.where(flip, np.where(use_b, 2, 1), post)


# ---- part 2: the placed batch ---------------------------------------------------------------------------------------------------
CASES = A.CASES
STEPS, SCRIPT_AT, TAPE_SEED = 8, (2, 5), 29
kw = A.kw


def script(env, t):
    """The caller's edit before step t: the scenes of tests/test_act_frame_host.py; the second vehicle of env 7 level with the
    first (bit-equal x, one lane apart); before the second edit every IS_LC_SAFE cleared (the prior starts lane changes from B)."""
    A.script(env)
    env.f64[abi.F["X"], 7, 1] = 352.0
    if t == SCRIPT_AT[1]:
        CP.mark_unsafe(env)


def actions(E, N):
    """Lane-change-heavy random actions (the mix of tests/test_candidate_prior_host.py); at the scripted steps env 6 holds two
    actions outside 0 .. 4."""
    g = torch.Generator().manual_seed(TAPE_SEED)
    tape = [torch.multinomial(CP.P_ACT, E * N, True, generator=g).view(E, N).int() for _ in range(STEPS)]
    for t in SCRIPT_AT:
        tape[t][6, 0] = 7
        tape[t][6, 1] = -1
    return tape


def run(env, E, N):
    """Per step: the planes before it, the record after it, whether the step latched an error, the trace where the env has one."""
    env.reset()
    tape = []
    for t, a in enumerate(actions(E, N)):
        if t in SCRIPT_AT:
            script(env, t)
        pre = {"u8": env.u8.detach().cpu().clone(), "f64": env.f64.detach().cpu().clone(), "env_i32": env.env_i32.detach().cpu().clone()}
        pre["time"] = pre["env_i32"][abi.EP["TIME"]]
        rec = H.snap(env, env.step(a.to(env.device)))
        try:
            env.poll_errors()
            latched = False
        except ValueError:
            latched = True
        trace = getattr(env, "trace", None)
        tape.append({"pre": pre, "rec": rec, "latched": latched, "act": a, "trace": None if trace is None else trace.detach().cpu().clone()})
    return tape


@functools.lru_cache(maxsize=None)
def oracle_tape(name, obs_f64=False):
    """The oracle's run of a case with its per-sub-step trace, once (shared by the tests of both files; nothing changes it)."""
    E, N, _ = CASES[name]
    oracle_env.set_math_mode(1)
    try:
        return run(oracle_env.OracleEnv(E, N, trace=True, **kw(name, obs_f64=obs_f64)), E, N)
    finally:
        oracle_env.set_math_mode(0)


def count_cases(tape, N):
    fns = CP._lane_fns()
    T, B, F, SAFE = abi.T, abi.B, abi.F, abi.FLAG_IS_LC_SAFE
    n = dict.fromkeys(("tie_lo", "tie_hi", "early_end", "crashed", "veto_from_A", "lift_with_follower", "respawn"), 0)
    for st in tape:
        tr, pre, act = st["trace"], st["pre"], st["act"]
        nsub, E = tr.shape[0], tr.shape[2]
        n["respawn"] += int((st["rec"]["env_i32"][abi.EP["EPISODE"]] != pre["env_i32"][abi.EP["EPISODE"]]).sum())
        for e in range(E):
            veh = [v for v in range(N) if int(pre["u8"][B["KIND"], e, v]) != 0]
            if not veh:
                continue
            s = {v: {"lane": int(pre["u8"][B["LANE"], e, v]), "tl": int(pre["u8"][B["TARGET_LANE"], e, v]),
                     "crashed": int(pre["u8"][B["CRASHED"], e, v]), "flags": int(pre["u8"][B["FLAGS"], e, v]),
                     "x": float(pre["f64"][F["X"], e, v]), "y": float(pre["f64"][F["Y"], e, v])} for v in veh}
            for k in range(nsub):
                if bool(torch.isnan(tr[k, T["X"], e, veh[0]])):
                    n["early_end"] += 1  # the episode ended in sub-step k - 1 < nsub - 1
                    break
                for a in veh:  # live vehicles at bit-equal x, as the rank scan of sub-step k compares them
                    for p in veh:
                        if p != a and s[p]["x"] == s[a]["x"]:
                            n["tie_lo" if p < a else "tie_hi"] += 1
                ev = {}
                for v in veh:
                    t = tr[k, :, e, v]
                    hl = (int(pre["time"][e]) + k) % nsub == 0
                    tl_act = CP._target_after_act(fns, s[v]["tl"], s[v]["x"], s[v]["y"], int(act[e, v]), hl)
                    ran = float(t[T["QP_ROWS"]]) > 0
                    flags_post = int(t[T["FLAGS"]])
                    veto = ran and not (flags_post & SAFE)
                    if not veto:
                        assert tl_act == int(t[T["TARGET_LANE"]]), ("target-lane replay", e, v, k)
                    need_b = ran and (tl_act != s[v]["lane"] or s[v]["crashed"] != 0)
                    first_b = need_b and not (s[v]["flags"] & SAFE)
                    ev[v] = (ran, need_b, first_b, veto, flags_post)
                    n["crashed"] += int(ran and s[v]["crashed"] != 0)
                    n["veto_from_A"] += int(need_b and not first_b and veto)
                for v in veh:
                    ran, need_b, first_b, veto, _ = ev[v]
                    if first_b and not veto and any(ev[w][0] and s[w]["x"] < s[v]["x"] for w in veh if w != v):
                        n["lift_with_follower"] += 1
                for v in veh:
                    t = tr[k, :, e, v]
                    s[v] = {"lane": int(t[T["LANE"]]), "tl": int(t[T["TARGET_LANE"]]), "crashed": int(t[T["CRASHED"]]),
                            "flags": ev[v][4], "x": float(t[T["X"]]), "y": float(t[T["Y"]])}
    return n


def test_the_placed_batch_holds_every_case():
    for name, (E, N, _) in CASES.items():
        tape = oracle_tape(name)
        c = count_cases(tape, N)
        print(name, c)
        for case, k in c.items():
            assert k >= 1, (name, case, c)
        assert [st["latched"] for st in tape] == [t in SCRIPT_AT for t in range(STEPS)], name  # the bad actions, and only they
        for t in SCRIPT_AT:  # the env with the crashed vehicle is done in the step after the edit and starts its next episode there
            st = tape[t]
            assert bool(st["rec"]["done"][3]) and int(st["rec"]["env_i32"][abi.EP["EPISODE"], 3]) == int(st["pre"]["env_i32"][abi.EP["EPISODE"], 3]) + 1


def test_the_trace_does_not_change_the_oracle():
    """The counts come from a run with the trace on; the GPU is compared with the same records, so the trace must not move them."""
    name = "E8_N4_mass"
    E, N, _ = CASES[name]
    oracle_env.set_math_mode(1)
    try:
        plain = run(oracle_env.OracleEnv(E, N, **kw(name)), E, N)
    finally:
        oracle_env.set_math_mode(0)
    for t, (a, b) in enumerate(zip(plain, oracle_tape(name))):
        H.assert_same(a["rec"], b["rec"], (name, t))
