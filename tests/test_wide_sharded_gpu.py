"""One hidden-512 gradient over rank-sharded batches on the MI355X: mm_policy_wide_train_partial / mm_policy_wide_train_finish
(include/mm_policy_wide_train.h), PPOLearner's shard_block / finish_shards at hidden 512 and train() with shard_group.

tests/test_train_sharded_gpu.py's plan at the other hidden size, asserted as the design states it.  One shard whose B is its own
count IS the chunked entry, bit for bit.  The finish is the documented fold: float32 of the blocks' fp64 sum in index order,
through the documented layout.  R shards of a batch give the gradient of ONE loss over all of it: within the project's rule
against float64 autograd (4 e32 + 1e-6 max|g64|, e32 the float32 torch error on the same tensor -- another slicing of the sample
sum is one more summation order), with the per-sample diagnostics the unchunked entry's bits.  Blocks that do not belong together
give NaN, never a plausible gradient.  Every double of a shard block is a function of the inputs.  The batches, the networks, the
knife-edge filter, the float64 references and the comparison are tests/test_wide_chunked_gpu.py's; no new batch is drawn."""
import ctypes as C
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_policy_wide_train_gpu as wt_t
import test_wide_chunked_gpu as wc
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import _mlp_struct
from policy_train_util import GRAD_NAMES, sums_of
from test_train_chunked_gpu import shared_refusals

pytestmark = pytest.mark.gpu

NAN = float("nan")
FORMS = wc.FORMS
HEADER, LOSS = 4, 2  # doubles: (B, local count, configuration word, 0), then the two loss sums
ACC = HEADER + LOSS  # where the two accumulator blocks start
PART = 304144        # doubles of one accumulator block: MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES / 4
K = ACC + 2 * PART   # MM_PW_SHARD_DOUBLES
WIDE_BIT = 1 << 26
# the documented offsets of an accumulator block
O_W2, O_HD, O_W1, O_B2, O_BH, O_B1 = 0, 278528, 286720, 303104, 303616, 303632


def _opt(t):
    return None if t is None else t.data_ptr()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cut(case, lo, hi):
    """Samples [lo, hi) of a case as a rank's shard (the strides stay; hi == lo is an empty shard)."""
    cut = lambda t: None if t is None else t[lo:hi]  # noqa: E731
    return wc.Case(case.learner, case.obs[lo:hi], case.act[lo:hi], case.ret[lo:hi], case.old[lo:hi].contiguous(), cut(case.adv),
                   None if case.valid is None else case.valid[lo:hi].contiguous(), case.critic_loss, case.clip)


def _bounds(sizes):
    out, lo = [], 0
    for s in sizes:
        out.append((lo, lo + s))
        lo += s
    return out


def _local(case):
    return case.n if case.valid is None else int(case.valid.sum())


def _count(case):
    """B of a case: an int32 [1] device tensor."""
    return torch.tensor([_local(case)], dtype=torch.int32, device="cuda")


def partial_rc(case, form, chunk, count, sums=None, block=None, scratch=None, scratch_ptr=None, scratch_bytes=None, networks="both",
               count_ptr=None, shard_ptr=None, hidden=512, clip=None, critic_loss=None, both_adv=False, stray=None):
    """(status, block, diagnostics) of the partial entry on a case's samples, straight through the binding.
    hidden .. stray: the arguments of shared_refusals (critic_loss: the raw code)."""
    clip = case.clip if clip is None else clip
    L, clib, n, S = case.learner, case.learner.clib, case.n, case.obs.shape[1]
    if block is None:
        block = torch.full((K,), NAN, dtype=torch.float64, device="cuda")
    with_a, with_c = networks != "critic", networks != "actor"
    diag = [torch.full((n,), NAN, device="cuda") if on or stray == i else None for i, on in enumerate((with_a, with_c, with_a))]
    if scratch is None and scratch_ptr is None:
        scratch = torch.empty(max(case.chunked_bytes(chunk), 16), dtype=torch.uint8, device="cuda")
    ptr = scratch.data_ptr() if scratch_ptr is None else (scratch_ptr or None)
    nbytes = scratch.numel() if scratch_bytes is None else scratch_bytes
    obs, act, ret = case.obs, case.act, case.ret
    head = (obs.data_ptr(), obs.stride(0) if n else S, n, S, act.data_ptr(), act.stride(0) if n else 1, ret.data_ptr(),
            ret.stride(0) if n else 1, case.old.data_ptr(), _opt(case.valid))
    cp = count.data_ptr() if count_ptr is None else (count_ptr or None)
    sp = block.data_ptr() if shard_ptr is None else (shard_ptr or None)
    W = [_mlp_struct(L.actor) if with_a else None, _mlp_struct(L.critic) if with_c else None]
    ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
    adv = case.adv if (sums is None or both_adv) else None
    code = abi.PT_CRITIC_LOSS[case.critic_loss] if critic_loss is None else critic_loss
    rc = clib.lib.mm_policy_wide_train_partial(*head, ref(W[0]), ref(W[1]), hidden, L.n_a, clip, code, _opt(sums) if with_a else None,
                                               _opt(adv) if with_a else None, cp, sp, _opt(diag[0]), _opt(diag[1]), _opt(diag[2]),
                                               ptr, nbytes, _stream(), chunk)
    return rc, block, diag


def finish_rc(case, blocks, networks="both", n_blocks=None, stride=None, blocks_ptr=None, n_s=None, loss=None):
    """(status, [loss] + the twelve gradients) of the finish entry; the gradients are read whatever the status."""
    L, clib = case.learner, case.learner.clib
    loss = torch.full((2,), NAN, device="cuda") if loss is None else loss
    R = blocks.shape[0] if n_blocks is None else n_blocks
    stride = blocks.stride(0) if stride is None else stride
    bp = blocks.data_ptr() if blocks_ptr is None else (blocks_ptr or None)
    n_s = case.obs.shape[1] if n_s is None else n_s
    G = [_mlp_struct(L.actor, True) if networks != "critic" else None, _mlp_struct(L.critic, True) if networks != "actor" else None]
    ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
    rc = clib.lib.mm_policy_wide_train_finish(bp, R, stride, n_s, L.n_a, ref(G[0]), ref(G[1]), loss.data_ptr(), _stream())
    return rc, [loss] + case.grads()


def sharded(case, form, sizes, chunk, count=None, sums=None, scratch=None, networks="both"):
    """partial on every shard of `sizes` with the whole case's B and (S+, S-), then finish: ([loss] + gradients + the
    concatenated diagnostics, the [R, K] blocks)."""
    count = _count(case) if count is None else count
    sums = case.sums(form) if sums is None else sums
    blocks = torch.full((len(sizes), K), NAN, dtype=torch.float64, device="cuda")
    diags = []
    for r, (lo, hi) in enumerate(_bounds(sizes)):
        rc, _, d = partial_rc(_cut(case, lo, hi), form, chunk, count, sums=sums, block=blocks[r], scratch=scratch, networks=networks)
        assert rc == abi.MM_OK
        diags.append(d)
    case.fill_grads(NAN)
    rc, out = finish_rc(case, blocks, networks=networks)
    assert rc == abi.MM_OK
    cat = [None if diags[0][i] is None else torch.cat([d[i] for d in diags]) for i in range(3)]
    return out + cat, blocks


def _word(case, form, nets=3):
    L = case.learner
    return (case.obs.shape[1] + 256 * L.n_a + 65536 * ((1 if form == "reference" else 0) + 2 * (case.critic_loss == "huber"))
            + (nets << 24) + WIDE_BIT)


# ---- 1. one shard is the chunked entry
@pytest.mark.parametrize("n,chunk", [(31, 64), (1000, 1024), (1000, 64)])
def test_one_shard_is_the_chunked_entry(n, chunk):
    case = wc._base(n)
    for form in FORMS:
        want = case.chunked(form, chunk)
        got, _ = sharded(case, form, [n], chunk)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        wc._bit_equal(got, want, (form, "losses, gradients and diagnostics against the chunked entry"))
        if chunk < n:
            continue
        # the learner's two phases without a budget are that one pass
        kw = dict(valid=case.valid, adv_sums=case.sums(form), diagnostics=True)
        if form != "reference":
            kw["advantages"] = case.adv
        assert case.learner.shard_doubles() == K
        block, diag = case.learner.shard_block(case.obs, case.act, case.ret, case.old, _count(case), **kw)
        case.fill_grads(NAN)
        loss = case.learner.finish_shards(block.unsqueeze(0))
        wc._bit_equal([loss] + case.grads() + list(diag), want, (form, "shard_block + finish_shards"))


# ---- 2. the finish is the documented fold of the documented layout
def _fold_numpy(blocks, n_s, n_a):
    """[R, K] float64 -> the twelve gradients: the blocks added in index order in float64, rounded once to float32, read through
    the layout of the public header."""
    acc = blocks[0].copy()
    for r in range(1, blocks.shape[0]):
        acc = acc + blocks[r]
    f = acc.astype(np.float32)
    out = []
    for i, (k2, n_out) in enumerate(((512, n_a), (512 + n_a, 1))):
        a = f[ACC + i * PART:ACC + (i + 1) * PART]
        w2 = a[O_W2:O_W2 + 512 * 544].reshape(512, 544)[:, :k2]
        hd = a[O_HD:O_HD + 16 * 512].reshape(16, 512)
        w1 = a[O_W1:O_W1 + 512 * 32].reshape(512, 32)
        out += [w1[:, :n_s], a[O_B1:O_B1 + 512], w2, a[O_B2:O_B2 + 512], hd[0:n_out], a[O_BH:O_BH + n_out]]
    return out


@pytest.mark.parametrize("form", FORMS)
def test_finish_is_the_stated_fold(form):
    case = wc._base(1000)
    sizes = [333, 333, 334]
    got, blocks = sharded(case, form, sizes, 192)
    b = blocks.cpu().numpy()
    B = int(_count(case))
    # the header: B, the local counts, the configuration word with the hidden-512 bit, 0
    assert (b[:, 0] == B).all() and (b[:, 2] == _word(case, form)).all() and (b[:, 3] == 0).all()
    assert list(b[:, 1]) == [_local(_cut(case, lo, hi)) for lo, hi in _bounds(sizes)]
    want = _fold_numpy(b, case.obs.shape[1], case.learner.n_a)
    for i, (g, w) in enumerate(zip(got[1:13], want)):
        assert g.numel() == w.size, i
        assert np.array_equal(g.cpu().numpy().reshape(w.shape), w), (form, i)
    s0, s1 = float(b[0, 4]), float(b[0, 5])
    for r in (1, 2):
        s0, s1 = s0 + float(b[r, 4]), s1 + float(b[r, 5])
    inv = 1.0 / B
    a = np.float32(-s0 * inv * inv) if form == "reference" else np.float32(-s0 * inv)
    assert np.array_equal(got[0].cpu().numpy(), np.array([a, np.float32(s1 * inv)], dtype=np.float32)), (got[0], a, s1 * inv)


# ---- 3. R shards sum to the whole batch: the configurations of wc.MULTI, the 6208 rows cut in eight at chunk 320
EIGHT = [777] * 7 + [769]
CUTS = {1000: [333, 333, 334], 129: [64, 64, 1], 6208: EIGHT}
SHARDED = [(n, CUTS[n], 320 if n == 6208 else chunk, cfg) for n, chunk, cfg in wc.MULTI]


@pytest.mark.parametrize("n,sizes,chunk,cfg", SHARDED,
                         ids=["%d_%d_%s_a%d_s%d" % (n, c, k["form"], k.get("n_a", 5), k.get("n_s", 30)) for n, _, c, k in SHARDED])
def test_shards_sum_to_the_whole_batch(n, sizes, chunk, cfg):
    cfg = dict(cfg)
    form = cfg.pop("form")
    case = wc._base(1000, **cfg).prefix(n) if n == 129 else wc._base(n, **cfg)
    assert sum(sizes) == n
    if n == 6208:  # no boundary on a 32-sample tile, and every shard takes three passes
        assert all(lo % 32 for lo, _ in _bounds(sizes)[1:]) and all((s + chunk - 1) // chunk == 3 for s in sizes)
    elif n == 1000:
        assert all(lo % 32 for lo, _ in _bounds(sizes)[1:])
    want = case.unchunked(form)
    got, _ = sharded(case, form, sizes, chunk)
    wc._bit_equal(got[13:], want[13:], "diagnostics against the unchunked entry")
    f32, f64 = case.torch_sides(form, case.sums(form))
    case.compare("sharded_n%d_c%d_%s_a%d" % (n, chunk, form, case.learner.n_a), got, f32, f64)


# ---- 4. empty and all-masked shards
def test_empty_and_all_masked_shards():
    base = wc._base(1000)
    valid = base.valid.clone()
    valid[600:] = 0
    case = base.masked(valid)
    for form in FORMS:
        got, blocks = sharded(case, form, [600, 0, 400], 192)  # a full shard, an empty one, one without a valid sample
        assert float(blocks[1, 1]) == 0.0 and float(blocks[2, 1]) == 0.0
        assert float(blocks[1, 4:].abs().max()) == 0.0 and float(blocks[2, 4:].abs().max()) == 0.0
        explicit = blocks.clone()
        explicit[1:, 4:] = 0.0  # the remaining shard's block plus explicit zero blocks (same header)
        case.fill_grads(NAN)
        rc, want = finish_rc(case, explicit)
        assert rc == abi.MM_OK
        wc._bit_equal(got[:13], want, (form, "against the finish of explicit zero blocks"))
        f32, f64 = case.torch_sides(form, case.sums(form))
        case.compare("sharded_empty_shards_%s" % form, got, f32, f64)
    none = base.masked(torch.zeros(1000, dtype=torch.uint8, device="cuda"))
    for form in FORMS:
        got, blocks = sharded(none, form, [600, 0, 400], 192)
        assert float(blocks[0, 0]) == 0.0
        for t in got:
            assert float(t.abs().max()) == 0.0


# ---- 5. blocks that do not belong together
def test_inconsistent_blocks_give_nan():
    case = wc._base(1000)
    form, sizes = "reference", [500, 500]
    good, blocks = sharded(case, form, sizes, 192)
    assert all(bool(torch.isfinite(t).all()) for t in good[:13])
    B = int(_count(case))
    sums = case.sums(form)

    def all_nan(out, which=slice(0, 13)):
        return all(bool(torch.isnan(t).all()) for t in out[which])

    # one block built with another B
    other = blocks.clone()
    rc, _, _ = partial_rc(_cut(case, 500, 1000), form, 192, torch.tensor([B + 1], dtype=torch.int32, device="cuda"), sums=sums,
                          block=other[1])
    assert rc == abi.MM_OK
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, other)
    assert rc == abi.MM_OK and all_nan(out)
    # the same B everywhere, but the local counts do not add up to it
    case.fill_grads(-7.0)
    out, _ = sharded(case, form, sizes, 192, count=torch.tensor([B + 5], dtype=torch.int32, device="cuda"))
    assert all_nan(out)
    # another form in one block
    other = blocks.clone()
    rc, _, _ = partial_rc(_cut(case, 500, 1000), "flat", 192, _count(case), sums=None, block=other[1])
    assert rc == abi.MM_OK
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, other)
    assert rc == abi.MM_OK and all_nan(out)
    # finish called for other state columns than the blocks were built with
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, blocks, n_s=case.obs.shape[1] - 1)
    assert rc == abi.MM_OK and bool(torch.isnan(out[0]).all())
    for g in out[1:13]:  # (with fewer columns the call addresses fewer elements of fc1.weight: what it writes is NaN)
        assert bool(torch.isnan(g).any()) and bool((torch.isnan(g) | (g == -7.0)).all())
    # blocks whose word lacks the hidden-512 bit (a hidden-128 block's word)
    narrow = blocks.clone()
    narrow[:, 2] -= float(WIDE_BIT)
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, narrow)
    assert rc == abi.MM_OK and all_nan(out)
    # blocks without the critic: NaN when the critic's gradients are requested ...
    actor_only = blocks.clone()
    for r, (lo, hi) in enumerate(_bounds(sizes)):
        rc, _, _ = partial_rc(_cut(case, lo, hi), form, 192, _count(case), sums=sums, block=actor_only[r], networks="actor")
        assert rc == abi.MM_OK
    assert float(actor_only[:, 2][0]) == _word(case, form, nets=1)
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, actor_only)
    assert rc == abi.MM_OK and all_nan(out)
    # ... and all that is needed when only the actor's are: the actor's gradients of the full run, the critic's untouched
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, actor_only, networks="actor")
    assert rc == abi.MM_OK
    wc._bit_equal(out[1:7], good[1:7], "the actor's gradients")
    assert float(out[0][0]) == float(good[0][0]) and float(out[0][1]) == 0.0
    assert all(bool((g == -7.0).all()) for g in out[7:13])
    # a network that was not requested keeps its canary when the blocks are inconsistent, too
    bad = blocks.clone()
    bad[1, 0] += 1.0
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, bad, networks="critic")
    assert rc == abi.MM_OK and all_nan(out, slice(7, 13)) and bool(torch.isnan(out[0]).all())
    assert all(bool((g == -7.0).all()) for g in out[1:7])


# ---- 6. refusals enqueue nothing
CANARY = 7.25


def test_refusals_leave_everything_alone():
    case = wc._base(1000)
    form, chunk = "reference", 64
    need = case.chunked_bytes(chunk)
    pad = 64
    arena = torch.full((pad + need + pad,), 0x5A, dtype=torch.uint8, device="cuda")  # canaries | scratch | canaries
    base = arena.data_ptr() + pad
    base += (-base) % 16
    assert base + need <= arena.data_ptr() + arena.numel()
    sums, count = case.sums(form), _count(case)
    guarded = torch.full((pad + 2 + pad,), CANARY, device="cuda")  # canaries | loss [2] | canaries
    loss = guarded[pad:pad + 2]
    block = torch.full((K,), CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def untouched():
        torch.cuda.synchronize()
        return (bool((block == CANARY).all()) and bool((arena == 0x5A).all()) and bool((guarded == CANARY).all())
                and all(bool((g == CANARY).all()) for g in case.grads()))

    case.fill_grads(CANARY)
    refused = [dict(chunk=0), dict(chunk=32), dict(chunk=100), dict(chunk=-64), dict(chunk=64, scratch_bytes=need - 1),
               dict(chunk=64, scratch_ptr=base + 4), dict(chunk=64, scratch_ptr=base + 8), dict(chunk=64, scratch_ptr=0), dict(chunk=128),  # (chunk 128: the scratch is chunk 64's)
               dict(chunk=64, count_ptr=0), dict(chunk=64, count_ptr=count.data_ptr() + 2), dict(chunk=64, shard_ptr=0),
               dict(chunk=64, shard_ptr=block.data_ptr() + 8), dict(chunk=64, hidden=128)]
    refused += [dict(chunk=64, **kw) for kw in shared_refusals(True, (64, 128))]  # the check shared with the chunked entry
    for kw in refused:
        kw = dict(kw)
        rc, _, diag = partial_rc(case, form, kw.pop("chunk"), count, sums=sums, block=block, scratch_ptr=kw.pop("scratch_ptr", base),
                                 scratch_bytes=kw.pop("scratch_bytes", need), **kw)
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert untouched(), kw
        assert all(bool(torch.isnan(d).all()) for d in diag if d is not None), kw
    blocks = torch.full((2, K + 2), CANARY, dtype=torch.float64, device="cuda")
    for kw in (dict(n_blocks=0), dict(n_blocks=65), dict(n_blocks=2, stride=K - 1), dict(blocks_ptr=0), dict(n_blocks=-1),
               dict(n_s=24), dict(n_s=33)):
        rc, out = finish_rc(case, blocks, loss=loss, **kw)
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert untouched() and bool((blocks == CANARY).all()), kw
    # the well-formed calls go through, stay inside the scratch and give the bits of the calls on a scratch of their own
    rc, block, diag = partial_rc(case, form, chunk, count, sums=sums, block=block, scratch_ptr=base, scratch_bytes=need)
    assert rc == abi.MM_OK
    rc, out = finish_rc(case, block.unsqueeze(0), loss=loss)
    torch.cuda.synchronize()
    assert rc == abi.MM_OK
    lo = base - arena.data_ptr()
    assert bool((arena[:lo] == 0x5A).all()) and bool((arena[lo + need:] == 0x5A).all())
    assert bool((guarded[:pad] == CANARY).all()) and bool((guarded[pad + 2:] == CANARY).all())
    mine = [loss.clone()] + out[1:] + diag
    wc._bit_equal(mine, sharded(case, form, [1000], chunk)[0], "inside the arena against a scratch of its own")


# ---- 7. every double of the block is a function of the inputs
def _unread(n_s, n_a):
    """bool [K]: the accumulator slots the finish index map does not read (the header and the loss sums are read)."""
    mask = np.zeros(K, dtype=bool)
    for i, (k2, n_out) in enumerate(((512, n_a), (512 + n_a, 1))):
        m = np.zeros(PART, dtype=bool)
        m[O_W2:O_HD].reshape(512, 544)[:, k2:] = True
        m[O_HD:O_W1].reshape(16, 512)[n_out:] = True
        m[O_W1:O_B2].reshape(512, 32)[:, n_s:] = True
        m[O_BH + n_out:O_B1] = True
        mask[ACC + i * PART:ACC + (i + 1) * PART] = m
    return mask


@pytest.mark.parametrize("networks", ["both", "actor"])
def test_the_block_is_a_function_of_the_inputs(networks):
    case = wc._base(1000)
    chunk = 192
    scratch = torch.empty(case.chunked_bytes(chunk), dtype=torch.uint8, device="cuda")
    unread = torch.from_numpy(_unread(case.obs.shape[1], case.learner.n_a)).cuda()
    for form in FORMS:
        runs = []
        for fill in (0xFF, 0x00, None):
            if fill is not None:
                scratch.fill_(fill)
            rc, block, _ = partial_rc(case, form, chunk, _count(case), sums=case.sums(form), scratch=scratch, networks=networks)
            assert rc == abi.MM_OK
            runs.append(block)
        assert bool(torch.isfinite(runs[0]).all())
        bits = [r.view(torch.int64) for r in runs]
        assert torch.equal(bits[0], bits[1]) and torch.equal(bits[1], bits[2]), (form, networks)
        assert bool((bits[0][unread] == 0).all()), (form, networks)  # exactly 0.0
        if networks == "actor":
            assert bool((bits[0][ACC + PART:] == 0).all()) and float(runs[0][5]) == 0.0
        assert float(runs[0][ACC:ACC + PART].abs().max()) > 0.0


# ---- 8. graph capture
def test_graph_capturable():
    case = wc._base(1000)
    form, chunk = "reference", 192
    sums, count = case.sums(form), _count(case)
    scratch = torch.empty(case.chunked_bytes(chunk), dtype=torch.uint8, device="cuda")
    blocks = torch.full((1, K), NAN, dtype=torch.float64, device="cuda")
    eager = [t.clone() for t in sharded(case, form, [1000], chunk, scratch=scratch)[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        partial_rc(case, form, chunk, count, sums=sums, block=blocks[0], scratch=scratch)
        finish_rc(case, blocks)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one chain: partial, then finish
        rc_p, _, diag = partial_rc(case, form, chunk, count, sums=sums, block=blocks[0], scratch=scratch)
        rc_f, captured = finish_rc(case, blocks)
    assert rc_p == abi.MM_OK and rc_f == abi.MM_OK
    for _ in range(2):
        case.fill_grads(NAN)
        scratch.fill_(0xFF)
        blocks.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        wc._bit_equal([captured[0]] + case.grads() + diag, eager, "replay against the eager calls")


# ---- 9. the learner's two phases composed by hand, on one device
B_ALL, N_AGENTS, S_COLS, N_ACT, HALF = 600, 4, 30, 5, 300


def _budget(clib):
    """Room for passes of 128 samples of the largest call (the flat step's 2 400 samples): below every call's unchunked scratch."""
    return clib.policy_wide_train_chunked_scratch_bytes(B_ALL * N_AGENTS, 128)


def _make_learner(fused, **kw):
    """Identically seeded networks on every call (and in every process), under the budget."""
    clib = wc._lib()
    return wt_t._learner(*wt_t._nets(S_COLS, n_a=N_ACT), fused_step=fused, scratch_budget_bytes=_budget(clib), **kw)


def _agent_step_inputs(L, obs, act, ret, form):
    """(old_logp, the local float32 (S+, S-) or None, the advantages) as train() takes them."""
    old, value = L.evaluate(obs, act, actor=L.actor_target, critic=L.critic_target)
    adv = ret - value
    return old, (sums_of(adv) if form == "reference" else None), adv


def _composed_step(replicas, shards, form):
    """One agent step of a sharded train(): shards[r] = rank r's (obs, act, ret)."""
    ins = [_agent_step_inputs(L, *sh, form) for L, sh in zip(replicas, shards)]
    count = torch.tensor([sum(sh[0].shape[0] for sh in shards)], dtype=torch.int32, device="cuda")
    sums = None
    if form == "reference":
        sums = ins[0][1]
        for i in ins[1:]:
            sums = sums + i[1]  # float32, in rank order
    blocks = []
    for L, sh, (old, _, adv) in zip(replicas, shards, ins):
        kw = dict(adv_sums=sums)
        if form != "reference":
            kw["advantages"] = adv
        blocks.append(L.shard_block(sh[0], sh[1], sh[2], old, count, **kw))
    blocks = torch.stack(blocks)
    for L in replicas:
        L.finish_shards(blocks)
        L._step(False)


def _schedule(states, actions, returns):
    """The two train() calls of tests 9 and 10 as agent steps: form "reference" on agents 0 and 1, then "flat" on all four."""
    steps = [("reference", (states[:, a, :], actions[:, a], returns[:, a])) for a in range(2)]
    steps.append(("flat", (states.reshape(-1, S_COLS), actions.reshape(-1), returns.reshape(-1))))
    return steps


_COMPOSED = {}


def _hand_composed(fused):
    """Two replicas on this device, each with its half of the 600 x 4 batch; returns (the replicas, a checker's twin trail)."""
    if fused not in _COMPOSED:
        states, actions, returns = wc._rollout_like(B_ALL, N_AGENTS, S_COLS, N_ACT, seed=21)
        replicas = [_make_learner(fused) for _ in range(2)]
        twin = _make_learner(fused)
        e32 = dict.fromkeys(GRAD_NAMES, 0.0)
        halves = [(states[r * HALF:(r + 1) * HALF], actions[r * HALF:(r + 1) * HALF], returns[r * HALF:(r + 1) * HALF]) for r in range(2)]
        trail = []
        for i, (form, whole) in enumerate(_schedule(states, actions, returns)):
            # e32 of the step the twin is about to take (test_learner_under_a_budget's measure)
            old, sums, adv = _agent_step_inputs(twin, *whole, form)
            f32, f64 = wc.Case(twin, whole[0], whole[1], whole[2], old, adv, None, "mse").torch_sides(form, sums)
            for k, x, y in zip(GRAD_NAMES, f32[1], f64[1]):
                e32[k] = max(e32[k], float((x.double() - y).abs().max()))
            if form == "reference":
                twin.train(states[:, i:i + 1], actions[:, i:i + 1], returns[:, i:i + 1], form="reference")
            else:
                twin.train(states, actions, returns, form="flat")
            _composed_step(replicas, [_schedule(*h)[i][1] for h in halves], form)
            trail.append((form + str(i), {k: v.detach().clone() for k, v in wc._named(twin).items()},
                          {k: v.detach().clone() for k, v in wc._named(replicas[0]).items()}, dict(e32)))
        # the budget forced several passes everywhere: the twin's calls and the replicas' shards
        for L, sizes in ((twin, (B_ALL, B_ALL * N_AGENTS)), (replicas[0], (HALF, HALF * N_AGENTS))):
            for n in sizes:
                chunk = L._chunks[n][0]
                assert chunk is not None and chunk < n, (n, chunk)
            assert L._scratch.numel() <= L.scratch_budget_bytes
        _COMPOSED[fused] = (replicas, trail)
    return _COMPOSED[fused]


@pytest.mark.parametrize("fused", [False, True], ids=["torch_tail", "fused_tail"])
def test_learner_phases_on_one_device(fused):
    """Two agent steps of train(form="reference") and one train(form="flat") at hidden 512 composed from shard_block /
    finish_shards over a 2-way split of 600 samples, against the unsharded learner under a budget that forces several passes:
    per tensor (lr / eps) 4 e32 + 1e-7, the rule (and its reason) of test_learner_under_a_budget.  The two replicas stay
    bit-equal."""
    replicas, trail = _hand_composed(fused)
    start = wc._named(_make_learner(fused))
    for step, twin, mine, e32 in trail:
        for k in GRAD_NAMES:
            diff = float((mine[k] - twin[k]).abs().max())
            bound = (wc.LR / wc.RMS_EPS) * 4.0 * e32[k] + 1e-7
            print("wide %s %-11s %-22s diff %.3e bound %.3e" % ("fused" if fused else "torch", step, k, diff, bound))
            assert diff <= bound, (step, k, diff, bound)
    a, b = wc._named(replicas[0]), wc._named(replicas[1])
    assert all(torch.equal(a[k].detach(), b[k].detach()) for k in a)
    assert all(not torch.equal(a[k].detach(), start[k].detach()) for k in a)
    assert all(L.replicas_in_sync() for L in replicas)  # (no shard group: one replica each)


# ---- 10. two processes on one GPU
def _worker(rank, world, port, out_dir):
    """One rank: its own process and library handle on cuda:0 (on a node every rank has its own GPU and the gathers are
    RCCL's), its half of the batch, train() twice with shard_group="world", the gathers over gloo through host copies."""
    import datetime
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        states, actions, returns = wc._rollout_like(B_ALL, N_AGENTS, S_COLS, N_ACT, seed=21)
        sl = slice(rank * HALF, (rank + 1) * HALF)
        states, actions, returns = states[sl], actions[sl], returns[sl]
        learner = _make_learner(False, shard_group="world")
        assert learner.hidden == 512 and learner.sharded
        in_sync = [learner.replicas_in_sync()]
        learner.train(states[:, :2], actions[:, :2], returns[:, :2], form="reference")
        learner.train(states, actions, returns, form="flat")
        in_sync.append(learner.replicas_in_sync())
        params = {k: v.detach().cpu() for k, v in wc._named(learner).items()}
        if rank == 1:  # one element of one replica moves: both ranks must see it
            with torch.no_grad():
                next(iter(wc._named(learner).values())).view(-1)[3] += 1e-3
        in_sync.append(learner.replicas_in_sync())
        torch.save({"params": params, "in_sync": in_sync}, os.path.join(out_dir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_processes_train_one_model(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)  # started first; they work while this process does
    replicas, _ = _hand_composed(False)
    hand = {k: v.detach().cpu() for k, v in wc._named(replicas[0]).items()}
    deadline = time.monotonic() + 60.0
    done = False
    while not done and time.monotonic() < deadline:
        done = ctx.join(timeout=max(0.0, deadline - time.monotonic()))
    if not done:
        for p in ctx.processes:
            p.kill()
    assert done, "the two ranks did not finish within 60 s"
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    assert parts[0]["in_sync"] == [True, True, False] and parts[1]["in_sync"] == [True, True, False]
    for k in hand:
        assert torch.equal(parts[0]["params"][k], parts[1]["params"][k]), ("rank 0 against rank 1", k)
        assert torch.equal(parts[0]["params"][k], hand[k]), ("against the hand-composed run", k)
