"""What the bank-training tests share (test_policy_bank_train_host.py without a GPU, test_policy_bank_train_gpu.py on the MI355X):
the layouts of the issue, synthetic members and batches, the member-local gather, and the raw calls of mm_policy_bank_eval /
mm_policy_bank_train (include/mm_policy_bank_train.h) and of mm_policy_eval / mm_policy_train, the reference a member is compared
with.  A plain module: nothing here touches the GPU unless it is called."""
import ctypes as C
import functools

import torch

from marl_mass_amd import _cabi as abi

N_A = 5
# name -> (rows, row_len, col_start, n_s, obs_stride, act_stride, ret_stride): the smallest layouts at which lookup, tiling,
# slicing or the fold can go wrong; strided rows on two of them
LAYOUTS = {
    "mixed": (7, 23, (0, 0, 5, 6, 23), 30, 37, 3, 2),     # an empty group, a tile that crosses rows, a one-column group, 4 tiles -> 2 slices
    "slices": (3, 96, (0, 64, 96), 25, 25, 1, 1),         # 6 tiles -> 3 slices, 3 tiles -> 2 uneven slices
    "big": (41, 801, (0, 800, 801), 30, 30, 1, 1),        # 1 025 tiles -> 3 tiles per slice
    "k64": (2, 64, tuple(range(65)), 25, 32, 2, 1),       # 64 members of 2 samples
    "k1": (5, 13, (0, 13), 30, 30, 1, 1),                 # a single member
}
# valid masks: name -> (the group that is fully masked or None, the groups that are partly masked)
MASKED = {"mixed": (1, (3,)), "slices": (1, (0,)), "big": (1, (0,)), "k64": (5, (0, 17, 63)), "k1": (None, (0,))}


def tiles(n):
    return (n + 31) // 32


def group_need(n_k):
    """Bytes of one group of n_k samples in mm_policy_bank_train's scratch (the header's formula)."""
    t = tiles(n_k)
    return 32 * t * abi.PBT_SAMPLE_BYTES + t * abi.PBT_TILE_BYTES + min((t + 1) // 2, 512) * abi.PBT_PARTIAL_BYTES


def scratch_need(rows, cols):
    K = len(cols) - 1
    return abi.PBT_HEADER_BYTES + K * abi.PBT_MEMBER_BYTES + sum(group_need(rows * (cols[k + 1] - cols[k])) for k in range(K))


def c_cols(cols):
    return (C.c_int64 * len(cols))(*cols)


def gather_index(rows, row_len, cols, k, device="cpu"):
    """The batch's sample indices of member k, in member-local order."""
    r = torch.arange(rows, device=device).unsqueeze(1) * row_len
    c = torch.arange(cols[k], cols[k + 1], device=device).unsqueeze(0)
    return (r + c).reshape(-1)


def shapes(n_s, critic):
    k2 = 128 + N_A if critic else 128
    n_out = 1 if critic else N_A
    return [(128, n_s), (128,), (128, k2), (128,), (n_out, 128), (n_out,)]


def stacks(K, n_s, critic, seed, device):
    """Six stacked [K, ...] float32 tensors with the scales of a trained network: every member different."""
    g = torch.Generator().manual_seed(seed + (1000 if critic else 0))
    out = []
    for i, shp in enumerate(shapes(n_s, critic)):
        fan = shp[1] if len(shp) == 2 else 4
        t = (torch.rand((K,) + shp, generator=g) * 2 - 1) * (1.5 / fan ** 0.5 if len(shp) == 2 else 0.5)
        if i == 4:
            t = t * (2.0 if critic else 3.0)
        out.append(t.contiguous().to(device))
    return out


def struct(tensors):
    p = abi.MMMlpParams(*[t.data_ptr() for t in tensors])
    p.tensors = tensors
    return p


def member(tensors, k):
    """The six tensors of member k as views of the stacks."""
    return [t[k] for t in tensors]


class Batch(object):
    """A synthetic batch in the layout's strides, on `device`: obs [n, obs_stride], actions [n * act_stride], returns
    [n * ret_stride] (strided views .obs / .act / .ret), old_logp, target_value, advantages [n], valid uint8 [n] or None."""

    def __init__(self, name, with_valid, seed=1, device="cuda"):
        self.rows, self.row_len, self.cols, self.n_s, os_, as_, rs_ = LAYOUTS[name]
        self.K, self.n = len(self.cols) - 1, self.rows * self.row_len
        n, g = self.n, torch.Generator().manual_seed(seed)
        obs = torch.randn(n, os_, generator=g) * 1.5
        act = torch.randint(0, N_A, (n * as_,), generator=g, dtype=torch.int32)
        ret = torch.randn(n * rs_, generator=g) * 2.0
        self.obs_store, self.act_store, self.ret_store = obs.to(device), act.to(device), ret.to(device)
        self.obs, self.act, self.ret = self.obs_store[:, :self.n_s], self.act_store[::as_], self.ret_store[::rs_]
        self.old_logp = (-1.6 + 0.3 * torch.randn(n, generator=g)).to(device)
        self.target_value = (0.5 * torch.randn(n, generator=g)).to(device)
        self.valid = None
        if with_valid:
            full, partly = MASKED[name]
            v = torch.ones(n, dtype=torch.uint8)
            if full is not None:
                v[gather_index(self.rows, self.row_len, self.cols, full)] = 0
            for k in partly:
                idx = gather_index(self.rows, self.row_len, self.cols, k)
                v[idx[torch.rand(idx.numel(), generator=g) < 0.4]] = 0
            self.valid = v.to(device)
        self.advantages = self.ret - self.target_value  # torch's float32 returns - value
        self.device = device

    def index(self, k):
        return gather_index(self.rows, self.row_len, self.cols, k, self.device)

    def n_k(self, k):
        return self.rows * (self.cols[k + 1] - self.cols[k])


def _p(t):
    return None if t is None else t.data_ptr()


def _ref(s):
    return None if s is None else C.byref(s)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bank_eval(clib, b, actors, critics, logp, value, valid=True):
    """The raw mm_policy_bank_eval on a Batch: status code out.  actors / critics: MMMlpParams or None."""
    return clib.lib.mm_policy_bank_eval(b.obs.data_ptr(), b.obs.stride(0), b.rows, b.row_len, b.n_s, b.act.data_ptr(), b.act.stride(0),
                                        _p(b.valid) if valid else None, _ref(actors), _ref(critics), b.K, c_cols(b.cols), 128, N_A,
                                        _p(logp), _p(value), _stream())


def bank_train(clib, b, actors, critics, ga, gc, form, critic_loss, mode, scratch, clip=0.2):
    """The raw mm_policy_bank_train on a Batch; mode "target_value" | "advantages".  Returns (status, loss [K, 2], adv_sums
    [K, 2], (logp, value, ratio))."""
    dev = b.device
    loss = torch.full((b.K, 2), float("nan"), device=dev)
    sums = torch.full((b.K, 2), float("nan"), device=dev)
    new = lambda on: torch.full((b.n,), float("nan"), device=dev) if on else None  # noqa: E731
    diag = (new(actors is not None), new(critics is not None), new(actors is not None))
    adv = b.advantages.contiguous() if (actors is not None and mode == "advantages") else None
    tv = b.target_value if (actors is not None and mode == "target_value") else None
    rc = clib.lib.mm_policy_bank_train(
        b.obs.data_ptr(), b.obs.stride(0), b.rows, b.row_len, b.n_s, b.act.data_ptr(), b.act.stride(0), b.ret.data_ptr(),
        b.ret.stride(0), b.old_logp.data_ptr(), _p(b.valid), _ref(actors), _ref(critics), b.K, c_cols(b.cols), 128, N_A, clip,
        abi.PT_CRITIC_LOSS[critic_loss], abi.PT_FORM[form], _p(adv), _p(tv), _ref(ga), _ref(gc), loss.data_ptr(), sums.data_ptr(),
        _p(diag[0]), _p(diag[1]), _p(diag[2]), scratch.data_ptr(), scratch.numel(), _stream())
    return rc, loss, sums, diag


@functools.lru_cache(maxsize=None)
def _pt_scratch(clib, n):
    return torch.empty(clib.policy_train_scratch_bytes(n), dtype=torch.uint8, device="cuda")


def pt_eval(clib, obs, act, valid, actor, critic, n_s):
    """mm_policy_eval on gathered dense samples: (logp, value)."""
    n = obs.shape[0]
    logp = torch.empty(n, device=obs.device) if actor is not None else None
    value = torch.empty(n, device=obs.device) if critic is not None else None
    clib.check(clib.lib.mm_policy_eval(obs.data_ptr(), obs.stride(0), n, n_s, act.data_ptr(), 1, _p(valid), _ref(actor), _ref(critic),
                                       128, N_A, _p(logp), _p(value), _stream()))
    return logp, value


def pt_train(clib, obs, act, ret, old, valid, actor, critic, n_s, critic_loss, adv_sums, advantages, clip=0.2):
    """mm_policy_train on gathered dense samples with one member's parameters: (loss [2], actor grads, critic grads, (logp,
    value, ratio)); the gradients are fresh NaN-filled tensors the call must overwrite."""
    n, dev = obs.shape[0], obs.device
    grads = [[torch.full_like(t, float("nan")) for t in net.tensors] if net is not None else None for net in (actor, critic)]
    G = [struct(g) if g is not None else None for g in grads]
    loss = torch.full((2,), float("nan"), device=dev)
    new = lambda on: torch.full((n,), float("nan"), device=dev) if on else None  # noqa: E731
    diag = (new(actor is not None), new(critic is not None), new(actor is not None))
    scratch = _pt_scratch(clib, n)
    clib.check(clib.lib.mm_policy_train(
        obs.data_ptr(), obs.stride(0), n, n_s, act.data_ptr(), 1, ret.data_ptr(), 1, old.data_ptr(), _p(valid), _ref(actor), _ref(critic),
        128, N_A, clip, abi.PT_CRITIC_LOSS[critic_loss], _p(adv_sums) if actor is not None else None,
        _p(advantages) if actor is not None else None, _ref(G[0]), _ref(G[1]), loss.data_ptr(), _p(diag[0]), _p(diag[1]), _p(diag[2]),
        scratch.data_ptr(), scratch.numel(), _stream()))
    return loss, grads[0], grads[1], diag
