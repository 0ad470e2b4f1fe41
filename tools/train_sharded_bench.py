#!/usr/bin/env python3
"""What the two-phase (rank-sharded) gradient costs on one MI355X, device time by events (include/mm_policy_gi_train.h,
include/mm_policy_train.h: mm_policy_*_train_partial / _finish):

  * one partial + finish with R = 1 against mm_policy_gi_train_chunked / mm_policy_train_chunked on the same n samples with the
    same chunk, the two alternating in one process (the chunked entries are the baseline: same kernels A and B, same passes);
  * the finish launch alone over R = 1, 2, 4, 8 blocks;
  * the bytes a rank gathers per agent step (R blocks and R triples of doubles).

    python tools/train_sharded_bench.py [n] [--chunk C] [--reps K] [--json profiles/train_sharded/bench.json]

Every figure is the median of `reps` (>= 10) timed repetitions after a warm-up, with the lowest and the highest beside it.  A
call is timed alone (partial + finish: ~ms); the finish launch, which is microseconds, in windows of 50 back-to-back launches.
No GPU, no figure: the tool fails rather than time anything else.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import _cabi as abi, hip_library  # noqa: E402
from marl_mass_amd.learner import PPOLearner, SharedPPOLearner, _mlp_struct, _params  # noqa: E402
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork  # noqa: E402

N_S, N_A = 30, 5


def timed(fn, reps, window=1):
    """Milliseconds per call of fn: `reps` windows of `window` back-to-back calls, each between two events."""
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(window):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / window)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


class Family(object):
    """One gradient family on n synthetic samples: the chunked call, the partial call and the finish call as closures."""

    def __init__(self, kind, n, chunk, clib):
        g = torch.Generator().manual_seed(3)
        self.kind, self.clib = kind, clib
        obs = (torch.randn(n, N_S, generator=g) * 1.5).cuda()
        act = torch.randint(0, N_A, (n,), generator=g, dtype=torch.int32).cuda()
        ret = (torch.randn(n, generator=g) * 1.5 + 0.3).cuda()
        if kind == "gi":
            torch.manual_seed(5)
            self.learner = L = SharedPPOLearner(ActorCriticNetwork(N_S, N_A, 128, 1, state_split=True).cuda(), clib)
            old = L.old_log_probs(obs, act) + 0.05 * torch.randn(n, generator=g).cuda()
            sums, adv = L.advantage_sums(obs, ret), None
            query, self.K = clib.policy_gi_train_chunked_scratch_bytes, clib.policy_gi_train_shard_doubles()
            W, G = L._structs(True)
            nets = (C.byref(W),)
            grads = (C.byref(G),)
            crit = abi.GI_CRITIC_LOSS["mse"]
            extra = (sums.data_ptr(),)
            self.chunked_fn, self.partial_fn, self.finish_fn = (clib.lib.mm_policy_gi_train_chunked, clib.lib.mm_policy_gi_train_partial,
                                                                clib.lib.mm_policy_gi_train_finish)
        else:
            torch.manual_seed(5)
            self.learner = L = PPOLearner(ActorNetwork(N_S, 128, N_A).cuda(), CriticNetwork(N_S, N_A, 128, 1).cuda(), clib)
            old, value = L.evaluate(obs, act, actor=L.actor_target, critic=L.critic_target)
            old = old + 0.05 * torch.randn(n, generator=g).cuda()
            adv = ret - value
            sums = torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])
            query, self.K = clib.policy_train_chunked_scratch_bytes, clib.policy_train_shard_doubles()
            W = [_mlp_struct(L.actor), _mlp_struct(L.critic)]
            G = [_mlp_struct(L.actor, True), _mlp_struct(L.critic, True)]
            nets = (C.byref(W[0]), C.byref(W[1]))
            grads = (C.byref(G[0]), C.byref(G[1]))
            crit = abi.PT_CRITIC_LOSS["mse"]
            extra = (sums.data_ptr(), None)
            self.chunked_fn, self.partial_fn, self.finish_fn = (clib.lib.mm_policy_train_chunked, clib.lib.mm_policy_train_partial,
                                                                clib.lib.mm_policy_train_finish)
        self.keep = (obs, act, ret, old, sums, adv, W, G)
        self.scratch = torch.empty(query(n, chunk), dtype=torch.uint8, device="cuda")
        self.loss = torch.empty(3, dtype=torch.float32, device="cuda")
        self.count = torch.tensor([n], dtype=torch.int32, device="cuda")
        self.blocks = torch.zeros(8, self.K, dtype=torch.float64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (obs.data_ptr(), N_S, n, N_S, act.data_ptr(), 1, ret.data_ptr(), 1, old.data_ptr(), None) + nets + (128, N_A, 0.2, crit) + extra
        tail = (None, None, None, self.scratch.data_ptr(), self.scratch.numel(), stream, chunk)
        self._chunked = head + grads + (self.loss.data_ptr(),) + tail
        self._partial = head + (self.count.data_ptr(), self.blocks.data_ptr()) + tail
        self._finish = lambda R: (self.blocks.data_ptr(), R, self.K, N_S, N_A) + grads + (self.loss.data_ptr(), stream)  # noqa: E731

    def chunked(self):
        self.clib.check(self.chunked_fn(*self._chunked))

    def partial(self):
        self.clib.check(self.partial_fn(*self._partial))

    def finish(self, R=1):
        self.clib.check(self.finish_fn(*self._finish(R)))

    def two_phase(self):
        self.partial()
        self.finish(1)

    def grads(self):
        nets = [self.learner.policy] if self.kind == "gi" else [self.learner.actor, self.learner.critic]
        params = sum((_params(m) if self.kind == "gi" else list(m.parameters()) for m in nets), [])
        return [p.grad.detach().clone() for p in params] + [self.loss.clone()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=524288)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("train_sharded_bench.py needs the GPU: nothing is measured without it")
    clib = hip_library()
    out = {"device": torch.cuda.get_device_name(0), "n": a.n, "chunk": a.chunk, "n_s": N_S, "n_a": N_A,
           "clock": "device events; median [min, max] over reps after a warm-up"}
    for kind in ("gi", "pt"):
        f = Family(kind, a.n, a.chunk, clib)
        for _ in range(3):  # warm-up of every launch that is timed
            f.chunked()
            f.two_phase()
        torch.cuda.synchronize()
        f.chunked()
        want = f.grads()
        f.two_phase()
        got = f.grads()
        same = all(torch.equal(x, y) for x, y in zip(want, got))  # (R = 1: the chunked entry's bits)
        base, two, part = [], [], []
        for _ in range(a.reps):  # alternating, so that a drift of the machine hits both alike
            base += timed(f.chunked, 1)
            two += timed(f.two_phase, 1)
            part += timed(f.partial, 1)
        rec = {"chunked": summary(base), "partial_plus_finish_R1": summary(two), "partial": summary(part), "bit_equal_R1": bool(same)}
        rec["overhead_ms_median"] = rec["partial_plus_finish_R1"]["median_ms"] - rec["chunked"]["median_ms"]
        rec["chunked_spread_ms"] = rec["chunked"]["max_ms"] - rec["chunked"]["min_ms"]
        f.partial()
        for r in range(1, 8):
            f.blocks[r].copy_(f.blocks[0])
        f.blocks[1:, 1] = 0.0  # (consistent headers: the local counts add up to B; only the timing is read)
        rec["finish_alone"] = {}
        for R in (1, 2, 4, 8):
            f.finish(R)
            torch.cuda.synchronize()
            rec["finish_alone"]["R%d" % R] = summary(timed(lambda: f.finish(R), a.reps, window=50))
        rec["shard_block_bytes"] = f.K * 8
        rec["gathered_bytes_per_agent_step"] = {"R%d" % R: R * (f.K * 8 + 24) for R in (2, 4, 8)}
        out[kind] = rec
        print(kind, json.dumps(rec))
        del f
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
