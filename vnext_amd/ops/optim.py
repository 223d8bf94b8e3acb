"""The tail of a training step as one op: full-model gradient-norm clipping and the AdamW update of every parameter in three
launches (vnext_amd/csrc/optim.hip; include/vnext_hip.h).

`torch.nn.utils.clip_grad_norm_` followed by `torch.optim.AdamW.step` is a chain of multi-tensor kernels: per-tensor norms, a
stack, a norm, scalar ops, the clip's in-place multiply over every gradient, then the update -- more than 44 launches on
SeqFormer-R50, and every gradient written back and read again.  `ClippedAdamW.step()` does the same arithmetic in a norm pass,
a fold and an update pass that reads the clip coefficient from device memory.

`chunk_plan(counts) -> int64 [n_chunks, 2]`: the tensors cut into pieces {tensor index, element offset} of at most
`_lib.OPT_CHUNK` elements; it depends on the element counts alone.
`arena_layout(counts) -> (offsets, total)`: where each tensor's slice of the `exp_avg` / `exp_avg_sq` arenas starts, in
elements: multiples of 4 (16 bytes), with at least one unused element before and after every slice.
`ClippedAdamW(params, lr, betas, eps, weight_decay, max_norm)`: a `torch.optim.Optimizer`.

* Parameter groups, `state_dict()` and `load_state_dict()` have `torch.optim.AdamW`'s format in both directions; `lr` and
  `weight_decay` are read from `param_groups` at every step, so LR schedulers work.
* `state[p]["exp_avg"]` / `["exp_avg_sq"]` are views, with p's shape and strides, into two flat fp32 arenas; `state[p]["step"]`
  is a 0-dim CPU fp32 tensor as torch keeps it (a view into one CPU array).  Loading a state dict copies INTO them.
* `step()` returns the total norm as a 0-dim device tensor (also `last_total_norm`) and never synchronises.
* ONE difference from the eager chain: the clipped gradients are not written back.  After `step()` the `.grad`s still hold the
  unclipped values; nothing in `train_step` reads them before `zero_grad`.
* fp32 dense parameters on one CUDA device; `amsgrad`, `maximize`, `capturable`, sparse gradients and other dtypes raise.
  On CPU parameters construction and the state dicts work and `step()` raises.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib

ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("group", "<i4"), ("flags", "<i4"),
                ("bias_correction1", "<f4"), ("bias_correction2_sqrt", "<f4"), ("reserved", "<i4", (2,))])
GROUP = np.dtype([(k, "<f8") for k in ("lr", "weight_decay", "beta1", "beta2", "eps", "decay", "one_minus_beta1",
                                        "one_minus_beta2")])
assert ROW.itemsize == ctypes.sizeof(_lib.AdamWTensor) == 64 and GROUP.itemsize == ctypes.sizeof(_lib.AdamWGroup) == 64

CALLS = {"step": 0, "upload": 0}      # steps through the C ABI / table uploads (tests: an unchanged table is not sent again)


def chunk_plan(counts) -> np.ndarray:
    """int64 [n_chunks, 2] = {tensor index, element offset}: tensor t in pieces of `_lib.OPT_CHUNK` elements (its last one may
    be shorter), the tensors in order; a tensor without elements has no piece"""
    counts = np.asarray(list(counts), dtype=np.int64).reshape(-1)
    assert (counts >= 0).all()
    pieces = (counts + _lib.OPT_CHUNK - 1) // _lib.OPT_CHUNK
    tensor = np.repeat(np.arange(counts.size, dtype=np.int64), pieces)
    first = np.cumsum(pieces) - pieces
    offset = (np.arange(int(pieces.sum()), dtype=np.int64) - first[tensor]) * _lib.OPT_CHUNK
    return np.ascontiguousarray(np.stack([tensor, offset], axis=1))


def arena_layout(counts):
    """-> (int64 [n] element offsets, total elements): slice t is [offsets[t], offsets[t] + counts[t]); every offset is a
    multiple of 4 and an unused element lies before and after every slice"""
    offsets, at = [], 4
    for n in counts:
        offsets.append(at)
        at = (at + int(n) + 1 + 3) & ~3
    return np.asarray(offsets, dtype=np.int64), at


def _core_strides(t):
    """(size, stride) of the dimensions that have more than one element"""
    return [(sz, st) for sz, st in zip(t.shape, t.stride()) if sz != 1]


def _is_dense(t) -> bool:
    """the tensor's elements are one run of memory, in some order of its dimensions"""
    if t.numel() == 0:
        return True
    expect = 1
    for st, sz in sorted((st, sz) for sz, st in _core_strides(t)):
        if st != expect:
            return False
        expect *= sz
    return True


class ClippedAdamW(torch.optim.Optimizer):
    """see the module docstring"""

    clips_gradients = True      # `train.train_step` leaves the clipping to step()

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.01, *, amsgrad=False,
                 maximize=False, capturable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("ClippedAdamW: a tensor lr is not supported (it would be read on the host at every step)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not 0.0 <= max_norm:
            raise ValueError(f"ClippedAdamW: lr {lr}, eps {eps}, weight_decay {weight_decay}, max_norm {max_norm} must be >= 0")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"ClippedAdamW: betas {betas} must lie in [0, 1)")
        # every key a torch.optim.AdamW group has, so that a state dict crosses in both directions
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=capturable, differentiable=False, fused=None, decoupled_weight_decay=True)
        self.max_norm = float(max_norm)
        self.last_total_norm = None
        self._built = False
        super().__init__(params, defaults)
        self._check_groups()
        self._build()

    # ---- construction ----------------------------------------------------------------------------------------------------------
    def _check_groups(self):
        for g in self.param_groups:
            for key in ("amsgrad", "maximize", "capturable", "differentiable"):
                if g.get(key, False):
                    raise ValueError(f"ClippedAdamW: {key}=True is not supported")
            if not g.get("decoupled_weight_decay", True):
                raise ValueError("ClippedAdamW: decoupled_weight_decay=False (Adam's L2 penalty) is not supported")
            if isinstance(g["lr"], torch.Tensor):
                raise ValueError("ClippedAdamW: a tensor lr is not supported")

    def add_param_group(self, param_group):
        if self._built:
            raise NotImplementedError("ClippedAdamW: add_param_group after construction is not supported (the state arenas "
                                      "are laid out once)")
        super().add_param_group(param_group)

    def _build(self):
        self._params = [p for g in self.param_groups for p in g["params"]]
        self._group_of = np.asarray([gi for gi, g in enumerate(self.param_groups) for _ in g["params"]], dtype=np.int32)
        devices = {p.device for p in self._params}
        if len(devices) != 1:
            raise ValueError(f"ClippedAdamW: the parameters must live on one device, not {sorted(map(str, devices))}")
        self._device = devices.pop()
        for p in self._params:
            if p.dtype != torch.float32:
                raise ValueError(f"ClippedAdamW: a {p.dtype} parameter of shape {tuple(p.shape)}: only torch.float32 "
                                 "parameters are supported")
            if p.layout != torch.strided or not _is_dense(p):
                raise ValueError(f"ClippedAdamW: a parameter of shape {tuple(p.shape)} and strides {p.stride()} is not a dense "
                                 "strided tensor")
        counts = [p.numel() for p in self._params]
        self._counts = np.asarray(counts, dtype=np.int64)
        self.arena_offsets, total = arena_layout(counts)
        self.exp_avg_arena = torch.zeros(total, dtype=torch.float32, device=self._device)
        self.exp_avg_sq_arena = torch.zeros(total, dtype=torch.float32, device=self._device)
        self._steps = torch.zeros(len(counts), dtype=torch.float32)      # CPU: state[p]["step"] are its elements
        self._install_views()
        self._chunks_host = chunk_plan(counts)
        self._chunks = self._partials = self._tables = self._last_tables = None
        self._built = True

    def _install_views(self):
        for i, p in enumerate(self._params):
            off = int(self.arena_offsets[i])
            self.state[p] = {"step": self._steps[i],
                             "exp_avg": torch.as_strided(self.exp_avg_arena, p.shape, p.stride(), off),
                             "exp_avg_sq": torch.as_strided(self.exp_avg_sq_arena, p.shape, p.stride(), off)}

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """a `torch.optim.AdamW` state dict or this class's own: the values are copied INTO the arenas; the views stay.  A
        parameter the dict has no state for starts from zero."""
        super().load_state_dict(state_dict)      # torch's checks, casts and group update; it leaves foreign tensors in self.state
        loaded = dict(self.state)
        self.state.clear()
        self._install_views()
        self._check_groups()
        for p in self._params:
            mine, theirs = self.state[p], loaded.get(p)
            if not theirs:
                for t in mine.values():
                    t.zero_()
                continue
            if "max_exp_avg_sq" in theirs:
                raise ValueError("ClippedAdamW.load_state_dict: the state holds max_exp_avg_sq: amsgrad is not supported")
            mine["exp_avg"].copy_(theirs["exp_avg"])
            mine["exp_avg_sq"].copy_(theirs["exp_avg_sq"])
            step = theirs["step"]
            mine["step"].fill_(float(step))      # (a device `step` of a fused optimizer's checkpoint: one read per tensor, at load)
        self._last_tables = None

    # ---- the step --------------------------------------------------------------------------------------------------------------
    def _device_plan(self):
        if self._chunks is None:
            n = self._chunks_host.shape[0]
            self._chunks = torch.from_numpy(self._chunks_host).to(self._device)
            self._partials = torch.empty(max(n, 1), dtype=torch.float32, device=self._device)
        return self._chunks, self._partials

    def _host_tables(self):
        """-> (uint8 array: the group rows, then the tensor rows; gradients kept alive until the launches are queued)"""
        n, keep, f32, dev = len(self._params), [], torch.float32, self._device
        pp, gp = [0] * n, [0] * n
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.layout is not torch.strided:
                raise ValueError("ClippedAdamW: sparse gradients are not supported")
            if g.dtype is not f32 or g.device != dev:
                raise ValueError(f"ClippedAdamW: a {g.dtype} gradient on {g.device} for a torch.float32 parameter on {dev}")
            # channels-last weights with a contiguous gradient, and the like (dimensions of one element may differ freely)
            if g.stride() != p.stride() and _core_strides(g) != _core_strides(p):
                g = torch.empty_like(p).copy_(g)
                if _core_strides(g) != _core_strides(p):
                    g = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device).copy_(p.grad)
            keep.append(g)
            gp[i], pp[i] = g.data_ptr(), p.data_ptr()
        rows = np.zeros(n, dtype=ROW)
        rows["p"], rows["g"] = np.asarray(pp, dtype=np.uint64), np.asarray(gp, dtype=np.uint64)
        gp = rows["g"]
        active = gp != 0
        steps = self._steps.numpy()
        steps[active] += 1.0
        item = self.exp_avg_arena.element_size()
        rows["m"] = self.exp_avg_arena.data_ptr() + item * self.arena_offsets.astype(np.uint64)
        rows["v"] = self.exp_avg_sq_arena.data_ptr() + item * self.arena_offsets.astype(np.uint64)
        rows["numel"] = self._counts
        rows["group"] = self._group_of
        rows["flags"] = np.where(((rows["p"] | gp | rows["m"] | rows["v"]) & np.uint64(15)) != 0, _lib.ADAMW_UNALIGNED, 0)
        groups = np.zeros(len(self.param_groups), dtype=GROUP)
        b1, b2 = np.zeros(len(self.param_groups)), np.zeros(len(self.param_groups))
        for gi, g in enumerate(self.param_groups):
            lr, wd, (b1[gi], b2[gi]) = float(g["lr"]), float(g["weight_decay"]), g["betas"]
            groups[gi] = (lr, wd, b1[gi], b2[gi], float(g["eps"]), 1.0 - lr * wd, 1.0 - b1[gi], 1.0 - b2[gi])
        t = steps.astype(np.float64)
        t[~active] = 1.0      # (not read by the kernels; any step >= 1 keeps the corrections finite)
        rows["bias_correction1"] = 1.0 - b1[self._group_of] ** t
        rows["bias_correction2_sqrt"] = np.sqrt(1.0 - b2[self._group_of] ** t)
        head = (groups.nbytes + 63) & ~63
        out = np.zeros(head + rows.nbytes, dtype=np.uint8)
        out[:groups.nbytes] = groups.view(np.uint8)
        out[head:] = rows.view(np.uint8)
        return out, head, keep

    @torch.no_grad()
    def step(self, closure=None):
        """-> total_norm, a 0-dim fp32 tensor on the parameters' device (the norm BEFORE clipping, as clip_grad_norm_ returns
        it).  With a closure its loss is kept as `last_loss`."""
        if closure is not None:
            with torch.enable_grad():
                self.last_loss = closure()
        if self._device.type != "cuda":
            raise RuntimeError("ClippedAdamW.step: Not implemented on the CPU")
        self._check_groups()
        chunks, partials = self._device_plan()
        host, head, keep = self._host_tables()
        if self._last_tables is None or not np.array_equal(host, self._last_tables):
            buf = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
            buf.numpy()[:] = host
            self._tables = buf.to(self._device, non_blocking=True)
            self._last_tables = host
            CALLS["upload"] += 1
        tables = self._tables
        norm = torch.empty(4, dtype=torch.float32, device=self._device)      # {total_norm, coef, coef as a double}
        n, n_chunks = len(self._params), chunks.shape[0]
        lib, stream = _lib.lib(), _lib.current_stream(norm)
        with torch.cuda.device(self._device):
            _lib.check(lib.vnx_adamw_grad_norm(tables.data_ptr() + head, n, chunks.data_ptr(), n_chunks, self.max_norm,
                                               partials.data_ptr(), norm.data_ptr(), stream))
            _lib.check(lib.vnx_adamw_clipped_step(tables.data_ptr() + head, n, tables.data_ptr(), len(self.param_groups),
                                                  chunks.data_ptr(), n_chunks, norm.data_ptr(), stream))
        CALLS["step"] += 1
        del keep
        self.last_total_norm = norm[0]
        return self.last_total_norm
