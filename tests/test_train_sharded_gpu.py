"""One gradient over rank-sharded batches on the MI355X: mm_policy_gi_train_partial / _finish and mm_policy_train_partial /
_finish (include/mm_policy_gi_train.h, include/mm_policy_train.h), the learners' shard_block / finish_shards and train() with
shard_group.

What the design promises is asserted as stated.  One shard whose B is its own count IS the chunked entry, bit for bit.  The
finish is the documented fold: float32 of the blocks' fp64 sum in index order, through the documented layout.  R shards of a
batch give the gradient of ONE loss over all of it: within the project's rule against float64 autograd (4 e32 + 1e-6 max|g64|,
e32 the float32 torch error on the same tensor -- another slicing of the sample sum is one more summation order), with the
per-sample diagnostics the unchunked entry's bits.  Blocks that do not belong together give NaN, never a plausible gradient.
The batches, the networks, the float64 references and the comparison are those of the unchunked and chunked test modules."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import policy_train_util
import test_policy_gi_train_gpu as gi_t
import test_policy_train_gpu as pt_t
import test_train_chunked_gpu as ch
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import SharedPPOLearner, _mlp_struct, _params

pytestmark = pytest.mark.gpu

ENTRIES = ch.ENTRIES
NAN = float("nan")
HEADER, LOSS = 4, 2  # doubles: (B, local count, configuration word, 0), then the two loss sums
ACC = HEADER + LOSS  # where the accumulator block(s) start
PART_GI, PART_PT = 27952, 26896
K = {"gi": ACC + PART_GI, "pt": ACC + 2 * PART_PT}


def _opt(t):
    return None if t is None else t.data_ptr()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cut(case, lo, hi):
    """Samples [lo, hi) of a case as a rank's shard (the strides stay; hi == lo is an empty shard)."""
    cut = lambda t: None if t is None else t[lo:hi]  # noqa: E731
    return ch.Case(case.kind, case.learner, case.obs[lo:hi], case.act[lo:hi], case.ret[lo:hi], case.old[lo:hi].contiguous(),
                   cut(case.adv), None if case.valid is None else case.valid[lo:hi].contiguous(), case.critic_loss, case.clip)


def _bounds(sizes):
    out, lo = [], 0
    for s in sizes:
        out.append((lo, lo + s))
        lo += s
    return out


def _count(case):
    """B of a case: an int32 [1] device tensor."""
    b = case.n if case.valid is None else int(case.valid.sum())
    return torch.tensor([b], dtype=torch.int32, device="cuda")


def _local(case):
    return case.n if case.valid is None else int(case.valid.sum())


def partial_rc(case, form, chunk, count, sums=None, block=None, scratch=None, scratch_bytes=None, networks="both", count_ptr=None,
               shard_ptr=None, hidden=128, clip=None, critic_loss=None, both_adv=False, stray=None):
    """(status, block, diagnostics) of the partial entry on a case's samples, straight through the binding.
    hidden .. stray: the arguments of ch.shared_refusals (critic_loss: the raw code)."""
    clip = case.clip if clip is None else clip
    L, clib, n, S = case.learner, case.learner.clib, case.n, case.obs.shape[1]
    if block is None:
        block = torch.full((K[case.kind],), NAN, dtype=torch.float64, device="cuda")
    with_a, with_c = networks != "critic", networks != "actor"
    diag = [torch.full((n,), NAN, device="cuda") if on or stray == i else None for i, on in enumerate((with_a, with_c, with_a))]
    if scratch is None:
        scratch = torch.empty(max(case.chunked_bytes(chunk), 16), dtype=torch.uint8, device="cuda")
    nbytes = scratch.numel() if scratch_bytes is None else scratch_bytes
    obs, act, ret = case.obs, case.act, case.ret
    head = (obs.data_ptr(), obs.stride(0) if n else S, n, S, act.data_ptr(), act.stride(0) if n else 1, ret.data_ptr(),
            ret.stride(0) if n else 1, case.old.data_ptr(), _opt(case.valid))
    cp = count.data_ptr() if count_ptr is None else count_ptr
    sp = block.data_ptr() if shard_ptr is None else shard_ptr
    tail = (cp, sp, _opt(diag[0]), _opt(diag[1]), _opt(diag[2]), scratch.data_ptr(), nbytes, _stream(), chunk)
    if case.kind == "gi":
        W = abi.MMGiParams()
        for name, p in zip(abi.GI_PARAMS, _params(L.policy)):
            setattr(W, name, p.detach().data_ptr())
        code = abi.GI_CRITIC_LOSS[case.critic_loss] if critic_loss is None else critic_loss
        rc = clib.lib.mm_policy_gi_train_partial(*head, C.byref(W), hidden, case.n_a, clip, code, _opt(sums), *tail)
    else:
        W = [_mlp_struct(L.actor) if with_a else None, _mlp_struct(L.critic) if with_c else None]
        ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
        adv = case.adv if (sums is None or both_adv) else None
        code = abi.PT_CRITIC_LOSS[case.critic_loss] if critic_loss is None else critic_loss
        rc = clib.lib.mm_policy_train_partial(*head, ref(W[0]), ref(W[1]), hidden, case.n_a, clip, code,
                                              _opt(sums) if with_a else None, _opt(adv) if with_a else None, *tail)
    return rc, block, diag


def finish_rc(case, blocks, networks="both", n_blocks=None, stride=None, blocks_ptr=None, n_s=None):
    """(status, [loss] + the twelve gradients) of the finish entry; the gradients are read whatever the status."""
    L, clib = case.learner, case.learner.clib
    loss = torch.full((3 if case.kind == "gi" else 2,), NAN, device="cuda")
    R = blocks.shape[0] if n_blocks is None else n_blocks
    stride = blocks.stride(0) if stride is None else stride
    bp = blocks.data_ptr() if blocks_ptr is None else blocks_ptr
    n_s = case.obs.shape[1] if n_s is None else n_s
    if case.kind == "gi":
        G = abi.MMGiParams()
        for name, p in zip(abi.GI_PARAMS, _params(L.policy)):
            setattr(G, name, p.grad.data_ptr())
        rc = clib.lib.mm_policy_gi_train_finish(bp, R, stride, n_s, case.n_a, C.byref(G), loss.data_ptr(), _stream())
    else:
        G = [_mlp_struct(L.actor, True) if networks != "critic" else None, _mlp_struct(L.critic, True) if networks != "actor" else None]
        ref = lambda st: None if st is None else C.byref(st)  # noqa: E731
        rc = clib.lib.mm_policy_train_finish(bp, R, stride, n_s, case.n_a, ref(G[0]), ref(G[1]), loss.data_ptr(), _stream())
    return rc, [loss] + case.grads()


def sharded(case, form, sizes, chunk, count=None, sums=None, scratch=None):
    """partial on every shard of `sizes` with the whole case's B and (S+, S-), then finish: ([loss] + gradients + the
    concatenated diagnostics, the [R, K] blocks)."""
    count = _count(case) if count is None else count
    sums = case.sums(form) if sums is None else sums
    blocks = torch.full((len(sizes), K[case.kind]), NAN, dtype=torch.float64, device="cuda")
    diags = []
    for r, (lo, hi) in enumerate(_bounds(sizes)):
        rc, _, d = partial_rc(_cut(case, lo, hi), form, chunk, count, sums=sums, block=blocks[r], scratch=scratch)
        assert rc == abi.MM_OK
        diags.append(d)
    case.fill_grads(NAN)
    rc, out = finish_rc(case, blocks)
    assert rc == abi.MM_OK
    return out + [torch.cat([d[i] for d in diags]) for i in range(3)], blocks


# ---- 1. one shard is the chunked entry
@pytest.mark.parametrize("n,chunk", [(31, 64), (1000, 1024), (1000, 64)])
@pytest.mark.parametrize("kind", ENTRIES)
def test_one_shard_is_the_chunked_entry(kind, n, chunk):
    case = ch._base(kind, n)
    for form in ("reference", "flat"):
        want = case.chunked(form, chunk)
        got, _ = sharded(case, form, [n], chunk)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        ch._bit_equal(got, want, (form, "losses, gradients and diagnostics against the chunked entry"))
        if chunk < n:
            continue
        ch._bit_equal(got, case.unchunked(form), (form, "against the unchunked entry"))
        # the learner's two phases without a budget are that one pass
        kw = dict(valid=case.valid, adv_sums=case.sums(form), diagnostics=True)
        if kind == "pt" and form != "reference":
            kw["advantages"] = case.adv
        block, diag = case.learner.shard_block(case.obs, case.act, case.ret, case.old, _count(case), **kw)
        case.fill_grads(NAN)
        loss = case.learner.finish_shards(block.unsqueeze(0))
        ch._bit_equal([loss] + case.grads() + list(diag), want, (form, "shard_block + finish_shards"))


# ---- 2. the finish is the documented fold of the documented layout
def _fold_numpy(kind, blocks, n_s, n_a):
    """[R, K] float64 -> the twelve gradients: the blocks added in index order in float64, rounded once to float32, read through
    the layout of the two public headers."""
    acc = blocks[0].copy()
    for r in range(1, blocks.shape[0]):
        acc = acc + blocks[r]
    f = acc.astype(np.float32)

    def net(a, l1_rows, k2, n_out):
        w2 = a[0:128 * 160].reshape(128, 160)[:, :k2]
        hd = a[20480:20480 + 16 * 128].reshape(16, 128)
        w1 = a[22528:22528 + l1_rows * 32].reshape(l1_rows, 32)
        o = 22528 + l1_rows * 32
        return w2, hd, w1, a[o:o + 128], a[o + 128:o + 144], a[o + 144:o + 144 + l1_rows]  # ... b2, head biases, b1

    if kind == "gi":
        w2, hd, w1, b2, bh, b1 = net(f[ACC:], 160, 160, 0)
        c11 = [5 * k for k in range(5)]
        c12 = [5 * (k >> 1) + 1 + (k & 1) for k in range(10)]
        c13 = [5 * (k >> 1) + 3 + (k & 1) for k in range(10)]
        return [w1[0:32][:, c11], b1[0:32], w1[32:96][:, c12], b1[32:96], w1[96:160][:, c13], b1[96:160], w2, b2,
                hd[0:n_a], bh[0:n_a], hd[8:9], bh[8:9]]
    out = []
    for i, (k2, n_out) in enumerate(((128, n_a), (128 + n_a, 1))):
        w2, hd, w1, b2, bh, b1 = net(f[ACC + i * PART_PT:], 128, k2, n_out)
        out += [w1[:, :n_s], b1, w2, b2, hd[0:n_out], bh[0:n_out]]
    return out


@pytest.mark.parametrize("form", ["reference", "flat"])
@pytest.mark.parametrize("kind", ENTRIES)
def test_finish_is_the_stated_fold(kind, form):
    case = ch._base(kind, 1000)
    sizes = [333, 333, 334]
    got, blocks = sharded(case, form, sizes, 192)
    b = blocks.cpu().numpy()
    B = int(_count(case))
    # the header: B, the local counts, the configuration word, 0
    nets = 3
    word = case.obs.shape[1] + 256 * case.n_a + 65536 * ((1 if form == "reference" else 0) + 2 * (case.critic_loss == "huber")) + (nets << 24)
    assert (b[:, 0] == B).all() and (b[:, 2] == word).all() and (b[:, 3] == 0).all()
    assert list(b[:, 1]) == [_local(_cut(case, lo, hi)) for lo, hi in _bounds(sizes)]
    want = _fold_numpy(kind, b, case.obs.shape[1], case.n_a)
    for i, (g, w) in enumerate(zip(got[1:13], want)):
        assert g.shape == w.shape or g.numel() == w.size, i
        assert np.array_equal(g.cpu().numpy().reshape(w.shape), w), (kind, form, i)
    s0, s1 = float(b[0, 4]), float(b[0, 5])
    for r in (1, 2):
        s0, s1 = s0 + float(b[r, 4]), s1 + float(b[r, 5])
    inv = 1.0 / B
    a = np.float32(-s0 * inv * inv) if form == "reference" else np.float32(-s0 * inv)
    c = np.float32(s1 * inv)
    want_loss = [a, c, np.float32(a + c)] if kind == "gi" else [a, c]
    assert np.array_equal(got[0].cpu().numpy(), np.array(want_loss, dtype=np.float32)), (got[0], want_loss)


# ---- 3. R shards sum to the whole batch
EIGHT = [8750] * 7 + [8751]
SHARDED = [
    (1000, [333, 333, 334], 64, dict(form="reference", critic_loss="mse", strided=True, with_valid=True)),
    (1000, [333, 333, 334], 192, dict(form="flat", critic_loss="huber", strided=True, with_valid=True, n_a=8)),
    (1000, [333, 333, 334], 960, dict(form="reference", critic_loss="huber", strided=True, with_valid=True, n_a=1)),
    (129, [64, 64, 1], 64, dict(form="flat", critic_loss="mse", strided=True, with_valid=True)),
    (70001, EIGHT, 4096, dict(form="reference", critic_loss="huber", strided=True, with_valid=True)),
    (70001, EIGHT, 4096, dict(form="flat", critic_loss="mse", strided=False, with_valid=False)),
]


@pytest.mark.parametrize("n,sizes,chunk,cfg", SHARDED, ids=["%d_%d_%s" % (n, c, k["form"]) for n, _, c, k in SHARDED])
@pytest.mark.parametrize("kind", ENTRIES)
def test_shards_sum_to_the_whole_batch(kind, n, sizes, chunk, cfg):
    cfg = dict(cfg)
    form = cfg.pop("form")
    case = ch._base(kind, 1000, **cfg).prefix(n) if n == 129 else ch._base(kind, n, seed=77 if n == 70001 else None, **cfg)
    assert sum(sizes) == n and all(lo % 32 for lo, _ in _bounds(sizes)[1:] if n != 129)  # no boundary on a tile
    want = case.unchunked(form)
    got, _ = sharded(case, form, sizes, chunk)
    ch._bit_equal(got[13:], want[13:], "diagnostics against the unchunked entry")
    sums = case.sums(form)
    f32, f64 = case.torch_sides(form, sums)
    case.compare("sharded_n%d_c%d_%s" % (n, chunk, form), got, f32, f64)


# ---- 4. empty and all-masked shards
@pytest.mark.parametrize("kind", ENTRIES)
def test_empty_and_all_masked_shards(kind):
    base = ch._base(kind, 1000)
    valid = base.valid.clone()
    valid[600:] = 0
    case = base.masked(valid)
    for form in ("reference", "flat"):
        got, blocks = sharded(case, form, [600, 0, 400], 192)  # a full shard, an empty one, one without a valid sample
        b = blocks.cpu()
        assert float(b[1, 1]) == 0.0 and float(b[2, 1]) == 0.0 and float(b[1, 4:].abs().max()) == 0.0
        explicit = blocks.clone()
        explicit[1:, 4:] = 0.0  # the remaining shard's block plus explicit zero blocks (same header)
        case.fill_grads(NAN)
        rc, want = finish_rc(case, explicit)
        assert rc == abi.MM_OK
        ch._bit_equal(got[:13], want, (form, "against the finish of explicit zero blocks"))
        f32, f64 = case.torch_sides(form, case.sums(form))
        case.compare("empty_shards_%s" % form, got, f32, f64)
    none = base.masked(torch.zeros(1000, dtype=torch.uint8, device="cuda"))
    for form in ("reference", "flat"):
        got, blocks = sharded(none, form, [600, 0, 400], 192)
        assert float(blocks[0, 0]) == 0.0
        for t in got:
            assert float(t.abs().max()) == 0.0


# ---- 5. blocks that do not belong together
@pytest.mark.parametrize("kind", ENTRIES)
def test_inconsistent_blocks_give_nan(kind):
    case = ch._base(kind, 1000)
    form, sizes = "reference", [500, 500]
    good, blocks = sharded(case, form, sizes, 192)
    assert all(bool(torch.isfinite(t).all()) for t in good[:13])
    B = int(_count(case))
    sums = case.sums(form)

    def all_nan(out, which=slice(0, 13)):
        return all(bool(torch.isnan(t).all()) for t in out[which])

    # one block built with another count
    other = blocks.clone()
    rc, _, _ = partial_rc(_cut(case, 500, 1000), form, 192, torch.tensor([B + 1], dtype=torch.int32, device="cuda"), sums=sums, block=other[1])
    assert rc == abi.MM_OK
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, other)
    assert rc == abi.MM_OK and all_nan(out)
    # the same B everywhere, but the local counts do not add up to it
    wrong = torch.tensor([B + 5], dtype=torch.int32, device="cuda")
    case.fill_grads(-7.0)
    out, _ = sharded(case, form, sizes, 192, count=wrong)
    assert all_nan(out)
    # another configuration (the per-sample form in one block)
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
    if kind == "gi":
        return
    # blocks without the critic: NaN when the critic's gradients are requested ...
    actor_only = blocks.clone()
    for r, (lo, hi) in enumerate(_bounds(sizes)):
        rc, _, _ = partial_rc(_cut(case, lo, hi), form, 192, _count(case), sums=sums, block=actor_only[r], networks="actor")
        assert rc == abi.MM_OK
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, actor_only)
    assert rc == abi.MM_OK and all_nan(out)
    # ... and all that is needed when only the actor's are: the actor's gradients of the good blocks, the critic's untouched
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, actor_only, networks="actor")
    assert rc == abi.MM_OK
    ch._bit_equal(out[1:7], good[1:7], "the actor's gradients")
    assert float(out[0][0]) == float(good[0][0]) and float(out[0][1]) == 0.0
    assert all(bool((g == -7.0).all()) for g in out[7:13])
    # a network that was not requested keeps its canary when the blocks are inconsistent, too
    bad = blocks.clone()
    bad[1, 0] += 1.0
    case.fill_grads(-7.0)
    rc, out = finish_rc(case, bad, networks="critic")
    assert rc == abi.MM_OK and all_nan(out, slice(7, 13)) and bool(torch.isnan(out[0]).all())
    assert all(bool((g == -7.0).all()) for g in out[1:7])


# ---- 6. refusals enqueue nothing; the scratch is written before it is read; two calls give the same bits
@pytest.mark.parametrize("kind", ENTRIES)
def test_refusals_leave_everything_alone(kind):
    case = ch._base(kind, 1000)
    form, chunk = "reference", 64
    need = case.chunked_bytes(chunk)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    sums, count = case.sums(form), _count(case)
    good, blocks = sharded(case, form, [1000], chunk, scratch=scratch)
    block = torch.full((K[kind],), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    refused = [dict(chunk=0), dict(chunk=32), dict(chunk=100), dict(chunk=64, scratch_bytes=need - 1), dict(chunk=64, count_ptr=0),
               dict(chunk=64, count_ptr=count.data_ptr() + 2), dict(chunk=64, shard_ptr=0), dict(chunk=64, shard_ptr=block.data_ptr() + 8)]
    refused += [dict(chunk=64, **kw) for kw in ch.shared_refusals(kind == "pt", (64, 512))]  # the checks shared with the chunked entry
    for kw in refused:
        kw = dict(kw)
        rc, _, diag = partial_rc(case, form, kw.pop("chunk"), count, sums=sums, block=block, scratch=scratch, **kw)
        torch.cuda.synchronize()
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert bool((block == -7.0).all()), kw
        assert all(bool(torch.isnan(d).all()) for d in diag if d is not None), kw
    pad = torch.zeros(2, K[kind] + 2, dtype=torch.float64, device="cuda")
    for kw in (dict(n_blocks=0), dict(n_blocks=65), dict(n_blocks=2, stride=K[kind] - 1), dict(blocks_ptr=0), dict(n_blocks=-1)):
        case.fill_grads(-7.0)
        rc, out = finish_rc(case, pad, **kw)
        torch.cuda.synchronize()
        assert rc == abi.MM_ERR_INVALID_ARG, kw
        assert all(bool((g == -7.0).all()) for g in out[1:13]), kw
        assert bool(torch.isnan(out[0]).all()), kw  # the losses were not written either
    # the well-formed calls go through, over a NaN-filled scratch as over zeros, twice the same
    runs = []
    for fill in (0xFF, 0x00, 0x00):
        scratch.fill_(fill)
        runs.append(sharded(case, form, [1000], chunk, scratch=scratch)[0])
    ch._bit_equal(runs[0], good, "0xFF-filled scratch")
    ch._bit_equal(runs[1], good, "zero-filled scratch")
    ch._bit_equal(runs[2], runs[1], "two calls")


# ---- 6b. every double of the separate networks' block is a function of the inputs (tests/test_wide_sharded_gpu.py's, at 128)
# the offsets of a PartialBlock<4> accumulator block: dW2 [128][160], head rows [16][128], dW1 [128][32], db2, head bias [16], db1
O_W2, O_HD, O_W1, O_B2, O_BH, O_B1 = 0, 20480, 22528, 26624, 26752, 26768


def _unread(n_s, n_a):
    """bool [K["pt"]]: the accumulator slots the finish index map does not read (the header and the loss sums are read)."""
    assert O_B1 + 128 == PART_PT
    mask = np.zeros(K["pt"], dtype=bool)
    for i, (k2, n_out) in enumerate(((128, n_a), (128 + n_a, 1))):
        m = np.zeros(PART_PT, dtype=bool)
        m[O_W2:O_HD].reshape(128, 160)[:, k2:] = True
        m[O_HD:O_W1].reshape(16, 128)[n_out:] = True
        m[O_W1:O_B2].reshape(128, 32)[:, n_s:] = True
        m[O_BH + n_out:O_B1] = True
        mask[ACC + i * PART_PT:ACC + (i + 1) * PART_PT] = m
    return mask


@pytest.mark.parametrize("networks", ["both", "actor"])
def test_the_block_is_a_function_of_the_inputs(networks):
    case = ch._base("pt", 1000)
    chunk = 64
    scratch = torch.empty(case.chunked_bytes(chunk), dtype=torch.uint8, device="cuda")
    unread = torch.from_numpy(_unread(case.obs.shape[1], case.n_a)).cuda()
    assert bool(unread.any())
    for form in ("reference", "flat"):
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
            assert bool((bits[0][ACC + PART_PT:] == 0).all()) and float(runs[0][5]) == 0.0
        assert float(runs[0][ACC:ACC + PART_PT].abs().max()) > 0.0


# ---- 7. the learner's two phases composed by hand, on one device
B_ALL, N_AGENTS, S_COLS, N_ACT, HALF = 600, 4, 30, 5, 300


def _make_learner(kind, fused, **kw):
    """Identically seeded networks on every call (and in every process)."""
    if kind == "gi":
        return SharedPPOLearner(gi_t._net(S_COLS), ch._lib(), fused_step=fused, **kw)
    return pt_t._learner(*pt_t._nets(S_COLS), fused_step=fused, **kw)


def _agent_step_inputs(kind, L, obs, act, ret, form):
    """(old_logp, the local float32 (S+, S-) or None, the separate networks' advantages or None) as train() takes them."""
    if kind == "gi":
        dense = obs.contiguous()
        return L.old_log_probs(dense, act), (L.advantage_sums(dense, ret) if form == "reference" else None), None
    old, value = L.evaluate(obs, act, actor=L.actor_target, critic=L.critic_target)
    adv = ret - value
    return old, (policy_train_util.sums_of(adv) if form == "reference" else None), adv


def _composed_step(kind, replicas, shards, form):
    """One agent step of a sharded train(): shards[r] = rank r's (obs, act, ret)."""
    ins = [_agent_step_inputs(kind, L, *sh, form) for L, sh in zip(replicas, shards)]
    count = torch.tensor([sum(sh[0].shape[0] for sh in shards)], dtype=torch.int32, device="cuda")
    sums = None
    if form == "reference":
        sums = ins[0][1]
        for i in ins[1:]:
            sums = sums + i[1]  # float32, in rank order
    blocks = []
    for L, sh, (old, _, adv) in zip(replicas, shards, ins):
        kw = dict(adv_sums=sums)
        if kind == "pt" and form != "reference":
            kw["advantages"] = adv
        blocks.append(L.shard_block(sh[0], sh[1], sh[2], old, count, **kw))
    blocks = torch.stack(blocks)
    for L in replicas:
        L.finish_shards(blocks)
        L._step(0) if kind == "gi" else L._step(False)


def _schedule(states, actions, returns):
    """The two train() calls of tests 7 and 8 as agent steps: form "reference" on agents 0 and 1, then "flat" on all four."""
    steps = [("reference", (states[:, a, :], actions[:, a], returns[:, a])) for a in range(2)]
    steps.append(("flat", (states.reshape(-1, S_COLS), actions.reshape(-1), returns.reshape(-1))))
    return steps


_COMPOSED = {}


def _hand_composed(kind, fused):
    """Two replicas on this device, each with its half of the 600 x 4 batch; returns (the replicas, a checker's twin trail)."""
    key = (kind, fused)
    if key not in _COMPOSED:
        states, actions, returns = ch._rollout_like(B_ALL, N_AGENTS, S_COLS, N_ACT, seed=21)
        replicas = [_make_learner(kind, fused) for _ in range(2)]
        twin = _make_learner(kind, fused)
        names = gi_t.GRAD_NAMES if kind == "gi" else policy_train_util.GRAD_NAMES
        e32 = dict.fromkeys(names, 0.0)
        halves = [(states[r * HALF:(r + 1) * HALF], actions[r * HALF:(r + 1) * HALF], returns[r * HALF:(r + 1) * HALF]) for r in range(2)]
        trail = []
        for i, (form, whole) in enumerate(_schedule(states, actions, returns)):
            # e32 of the step the twin is about to take (test_learner_under_a_budget's measure)
            old, sums, adv = _agent_step_inputs(kind, twin, *whole, form)
            case = ch.Case(kind, twin, whole[0], whole[1], whole[2], old, adv, None, "mse")
            f32, f64 = case.torch_sides(form, sums)
            for k, x, y in zip(names, f32[1], f64[1]):
                e32[k] = max(e32[k], float((x.double() - y).abs().max()))
            if form == "reference":
                a = i
                twin.train(states[:, a:a + 1], actions[:, a:a + 1], returns[:, a:a + 1], form="reference")
            else:
                twin.train(states, actions, returns, form="flat")
            _composed_step(kind, replicas, [_schedule(*h)[i][1] for h in halves], form)
            trail.append((form + str(i), {k: v.detach().clone() for k, v in ch._named(twin, kind).items()},
                          {k: v.detach().clone() for k, v in ch._named(replicas[0], kind).items()}, dict(e32)))
        _COMPOSED[key] = (replicas, trail)
    return _COMPOSED[key]


@pytest.mark.parametrize("fused", [False, True], ids=["torch_tail", "fused_tail"])
@pytest.mark.parametrize("kind", ENTRIES)
def test_learner_phases_on_one_device(kind, fused):
    """Two agent steps of train(form="reference") and one train(form="flat") composed from shard_block / finish_shards over a
    2-way split of 600 samples, against the unsharded learner: per tensor (lr / eps) 4 e32 + 1e-7, the rule (and its reason)
    of test_learner_under_a_budget.  The two replicas stay bit-equal."""
    replicas, trail = _hand_composed(kind, fused)
    names = gi_t.GRAD_NAMES if kind == "gi" else policy_train_util.GRAD_NAMES
    start = ch._named(_make_learner(kind, fused), kind)
    for step, twin, mine, e32 in trail:
        for k in names:
            diff = float((mine[k] - twin[k]).abs().max())
            bound = (ch.LR / ch.RMS_EPS) * 4.0 * e32[k] + 1e-7
            print("%s %s %-11s %-22s diff %.3e bound %.3e" % (kind, "fused" if fused else "torch", step, k, diff, bound))
            assert diff <= bound, (step, k, diff, bound)
    a, b = ch._named(replicas[0], kind), ch._named(replicas[1], kind)
    assert all(torch.equal(a[k].detach(), b[k].detach()) for k in a)
    assert all(not torch.equal(a[k].detach(), start[k].detach()) for k in a)
    assert all(L.replicas_in_sync() for L in replicas)  # (no shard group: one replica each)


# ---- 8. two processes on one GPU
def _worker(rank, world, port, out_dir, kind):
    """One rank: its own process and library handle on cuda:0 (on a node every rank has its own GPU and the gathers are
    RCCL's), its half of the batch, train() twice with shard_group="world", the gathers over gloo through host copies."""
    import datetime
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        states, actions, returns = ch._rollout_like(B_ALL, N_AGENTS, S_COLS, N_ACT, seed=21)
        sl = slice(rank * HALF, (rank + 1) * HALF)
        states, actions, returns = states[sl], actions[sl], returns[sl]
        learner = _make_learner(kind, False, shard_group="world")
        in_sync = [learner.replicas_in_sync()]
        learner.train(states[:, :2], actions[:, :2], returns[:, :2], form="reference")
        learner.train(states, actions, returns, form="flat")
        in_sync.append(learner.replicas_in_sync())
        params = {k: v.detach().cpu() for k, v in ch._named(learner, kind).items()}
        if rank == 1:  # one element of one replica moves: both ranks must see it
            with torch.no_grad():
                next(iter(ch._named(learner, kind).values())).view(-1)[3] += 1e-3
        in_sync.append(learner.replicas_in_sync())
        torch.save({"params": params, "in_sync": in_sync}, os.path.join(out_dir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ENTRIES)
def test_two_processes_train_one_model(kind, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path), kind), nprocs=2, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    assert parts[0]["in_sync"] == [True, True, False] and parts[1]["in_sync"] == [True, True, False]
    replicas, _ = _hand_composed(kind, False)
    hand = {k: v.detach().cpu() for k, v in ch._named(replicas[0], kind).items()}
    for k in hand:
        assert torch.equal(parts[0]["params"][k], parts[1]["params"][k]), ("rank 0 against rank 1", k)
        assert torch.equal(parts[0]["params"][k], hand[k]), ("against the hand-composed run", k)
