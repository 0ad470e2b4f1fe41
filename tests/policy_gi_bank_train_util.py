"""What the tests of the shared actor-critic bank's training half share (test_policy_gi_bank_train_host.py without a GPU,
test_policy_gi_bank_train_gpu.py on the MI355X): the layouts, batches and member-local gather of policy_bank_train_util, stacked
members of MAPPO_GI's shared network, and the raw calls of mm_policy_gi_bank_eval / mm_policy_gi_bank_train
(include/mm_policy_gi_bank_train.h) and of mm_policy_gi_act / mm_policy_gi_train, the reference a member is compared with.  A plain
module: nothing here touches the GPU unless it is called."""
import ctypes as C
import functools

import torch

from marl_mass_amd import _cabi as abi
from policy_bank_train_util import LAYOUTS, MASKED, Batch, gather_index, c_cols, tiles, N_A  # noqa: F401  (re-exported)

SHAPES = [(32, 5), (32,), (64, 10), (64,), (64, 10), (64,), (128, 160), (128,), (N_A, 128), (N_A,), (1, 128), (1,)]
FORM = {"reference": abi.PT_FORM["reference"], "per_sample": abi.PT_FORM["per_sample"]}


def group_need(n_k):
    """Bytes of one group of n_k samples in mm_policy_gi_bank_train's scratch (the header's formula)."""
    t = tiles(n_k)
    return 32 * t * abi.GBT_SAMPLE_BYTES + t * abi.GBT_TILE_BYTES + min((t + 1) // 2, 512) * abi.GBT_PARTIAL_BYTES


def scratch_need(rows, cols):
    K = len(cols) - 1
    return abi.GBT_HEADER_BYTES + K * abi.GBT_MEMBER_BYTES + sum(group_need(rows * (cols[k + 1] - cols[k])) for k in range(K))


def stacks(K, seed, device):
    """Twelve stacked [K, ...] float32 tensors (MMGiParams' order) with the scales of a trained network: every member different."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, shp in enumerate(SHAPES):
        fan = shp[1] if len(shp) == 2 else 4
        t = (torch.rand((K,) + shp, generator=g) * 2 - 1) * (1.5 / fan ** 0.5 if len(shp) == 2 else 0.5)
        if i == 8:
            t = t * 3.0  # the actor head: distinct log-probabilities
        if i == 10:
            t = t * 2.0
        out.append(t.contiguous().to(device))
    return out


def struct(tensors):
    p = abi.MMGiParams(*[t.data_ptr() for t in tensors])
    p.tensors = tensors
    return p


def member(tensors, k):
    """The twelve tensors of member k as views of the stacks."""
    return [t[k] for t in tensors]


def _p(t):
    return None if t is None else t.data_ptr()


def _ref(s):
    return None if s is None else C.byref(s)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bank_eval(clib, b, bank, logp, value, valid=True):
    """The raw mm_policy_gi_bank_eval on a Batch: status code out."""
    return clib.lib.mm_policy_gi_bank_eval(b.obs.data_ptr(), b.obs.stride(0), b.rows, b.row_len, b.n_s, b.act.data_ptr(),
                                           b.act.stride(0), _p(b.valid) if valid else None, _ref(bank), b.K, c_cols(b.cols), 128, N_A,
                                           _p(logp), _p(value), _stream())


def bank_train(clib, b, bank, grads, form, critic_loss, scratch, clip=0.2, cols=None):
    """The raw mm_policy_gi_bank_train on a Batch (value_now = b.target_value in the reference form).  Returns (status, loss
    [K, 3], adv_sums [K, 2], (logp, value, ratio)), the outputs NaN-filled before the call."""
    dev = b.device
    loss = torch.full((b.K, 3), float("nan"), device=dev)
    sums = torch.full((b.K, 2), float("nan"), device=dev)
    diag = tuple(torch.full((b.n,), float("nan"), device=dev) for _ in range(3))
    rc = clib.lib.mm_policy_gi_bank_train(
        b.obs.data_ptr(), b.obs.stride(0), b.rows, b.row_len, b.n_s, b.act.data_ptr(), b.act.stride(0), b.ret.data_ptr(),
        b.ret.stride(0), b.old_logp.data_ptr(), _p(b.valid), _ref(bank), b.K, c_cols(b.cols if cols is None else cols), 128, N_A, clip,
        abi.GI_CRITIC_LOSS[critic_loss], FORM[form], _p(b.target_value) if form == "reference" else None, _ref(grads),
        loss.data_ptr(), sums.data_ptr(), _p(diag[0]), _p(diag[1]), _p(diag[2]), scratch.data_ptr(), scratch.numel(), _stream())
    return rc, loss, sums, diag


def gi_act(clib, obs, weights, n_s):
    """mm_policy_gi_act (nothing sampled) on dense obs [n, n_s] with one member's twelve tensors: (logp [n, N_A], value [n])."""
    n = obs.shape[0]
    logp = torch.empty(n, N_A, device=obs.device)
    value = torch.empty(n, device=obs.device)
    clib.check(clib.lib.mm_policy_gi_act(obs.data_ptr(), n, n_s, *[w.data_ptr() for w in weights], 128, N_A, 0, None, None,
                                         logp.data_ptr(), value.data_ptr(), _stream()))
    return logp, value


@functools.lru_cache(maxsize=None)
def _gi_scratch(clib, n):
    return torch.empty(clib.policy_gi_train_scratch_bytes(n), dtype=torch.uint8, device="cuda")


def gi_train(clib, obs, act, ret, old, valid, weights, n_s, critic_loss, adv_sums, clip=0.2):
    """mm_policy_gi_train on gathered dense samples with one member's parameters: (loss [3], the twelve gradients, (logp, value,
    ratio)); the gradients are fresh NaN-filled tensors the call must overwrite."""
    n, dev = obs.shape[0], obs.device
    grads = [torch.full_like(t, float("nan")) for t in weights]
    W, G = struct([w.contiguous() for w in weights]), struct(grads)
    loss = torch.full((3,), float("nan"), device=dev)
    diag = tuple(torch.full((n,), float("nan"), device=dev) for _ in range(3))
    scratch = _gi_scratch(clib, n)
    clib.check(clib.lib.mm_policy_gi_train(
        obs.data_ptr(), obs.stride(0) if n else n_s, n, n_s, act.data_ptr(), 1, ret.data_ptr(), 1, old.data_ptr(), _p(valid), _ref(W),
        128, N_A, clip, abi.GI_CRITIC_LOSS[critic_loss], _p(adv_sums), _ref(G), loss.data_ptr(), _p(diag[0]), _p(diag[1]),
        _p(diag[2]), scratch.data_ptr(), scratch.numel(), _stream()))
    return loss, grads, diag
