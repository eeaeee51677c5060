"""Fused multi-tensor optimizers on libdram_hip (``dram_adam_multi`` / ``dram_sgd_multi``).

Drop-in for ``torch.optim.Adam(self.parameters(), lr=args.lr)`` at reference
models.py:385-387 / :689-691 (and the SGD(momentum, weight_decay) variant whose
arguments the reference keeps, train.py:25,27): ``torch.optim.Optimizer`` subclasses, so
``ExponentialLR`` (models.py:392-394), ``param_groups[0]['lr']``, ``state_dict()`` /
``load_state_dict()`` (keys ``step``, ``exp_avg``, ``exp_avg_sq``) and Lightning's
``step(closure)`` protocol keep working.  One kernel launch updates every parameter.

Gradient clipping (Lightning's ``--gradient_clip_val`` / ``--gradient_clip_algorithm``) rides the update's own
multiplication by ``grad_scale``: ``max_grad_norm`` costs one read-only pass over the gradients
(``dram_grad_norm_multi``), ``clip_grad_value`` nothing, and neither rewrites a gradient.  ``clip_grad_norm_`` /
``clip_grad_value_`` below are the in-place forms of ``torch.nn.utils`` for callers who look at the gradients afterwards.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from . import _lib, ops

_TABLE_DT = np.dtype(_lib.DramTensorRef)
_CHUNK_DT = np.dtype(_lib.DramChunkRef)


def build_chunks(sizes, chunk: int = _lib.OPT_CHUNK):
    """One DramChunkRef per `chunk` elements of every tensor (depends on the tensor SIZES only)."""
    parts = []
    for i, n in enumerate(sizes):
        c = np.zeros((n + chunk - 1) // chunk, dtype=_CHUNK_DT)
        c["tensor"] = i
        c["offset"] = np.arange(0, n, chunk, dtype=np.int64)
        parts.append(c)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=_CHUNK_DT)


def build_tables(ptrs: List[tuple], chunk: int = _lib.OPT_CHUNK):
    """Host-side layout of the kernel's work list: one DramTensorRef per tensor and one
    DramChunkRef per `chunk` elements.  ptrs: [(p, g, m, v, n), ...] as integers."""
    table = np.array(ptrs, dtype=_TABLE_DT) if ptrs else np.zeros(0, dtype=_TABLE_DT)
    return table, build_chunks([t[4] for t in ptrs], chunk)


def _check_clip(max_grad_norm, clip_grad_value):
    if max_grad_norm is not None and clip_grad_value is not None:
        raise ValueError("set max_grad_norm or clip_grad_value, not both")
    for name, v in (("max_grad_norm", max_grad_norm), ("clip_grad_value", clip_grad_value)):
        if v is not None and not float(v) >= 0.0:
            raise ValueError(f"{name} must be >= 0, got {v!r}")


def _clip_inputs(max_grad_norm, clip_grad_value):
    """clip[0:2] as the kernels read them: a negative clip[1] selects the norm mode."""
    return [float(max_grad_norm), -1.0] if max_grad_norm is not None else [0.0, float(clip_grad_value)]


class _FusedBase(torch.optim.Optimizer):
    """max_grad_norm / clip_grad_value: plain attributes (NOT param_groups entries: state_dict() keeps its keys), may
    be changed between steps; at most one is set.  With max_grad_norm, step() takes the 2-norm of ALL gradients of the
    optimizer (times |grad_scale|) in one launch and every update launch of the step multiplies by the same
    coefficient; `last_grad_norm` is that norm, a 0-dim device tensor (no host synchronisation)."""

    def __init__(self, params, defaults, max_grad_norm=None, clip_grad_value=None):
        _check_clip(max_grad_norm, clip_grad_value)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.clip_grad_value = clip_grad_value
        self._clip = None             # device float32[4]: max_norm, clip_value (< 0: norm mode) | total_norm, coef
        self._clip_host = None
        self._partials = None         # device float64: one sum of squares per chunk
        self._norm_tables = None      # (key, (table, chunks, count)) of the all-parameter list when it is not the update's
        self._cache_key = None
        self._cache = None
        self._chunk_cache = None      # (sizes, device) -> (device chunk list, count): independent of the pointers
        self._pinned_spare = None     # pinned staging pair for the next graph capture (capturable mode)
        self._pinned_owned = []       # pairs captured graphs read on every replay: never written again
        self.grad_scale = 1.0   # DDP folds the 1/world_size of the gradient mean in here

    def _tables(self, key, ptrs, device):
        if key != self._cache_key:
            table, chunks = build_tables(ptrs)
            ht, hc = torch.from_numpy(table.view(np.uint8).copy()), torch.from_numpy(chunks.view(np.uint8).copy())
            capturing = torch.cuda.is_current_stream_capturing()
            if capturing:
                # inside a hipGraph capture neither a pageable host->device copy nor a pinned allocation is
                # allowed: the tables go through a pinned pair that an EAGER step allocated beforehand (sizes depend
                # only on the parameter sizes).  The pair now belongs to this graph -- its copy node re-reads it on
                # every replay -- so it is never written again; the next eager step allocates a new spare.
                sp = self._pinned_spare
                if sp is None or sp[0].numel() != ht.numel() or sp[1].numel() != hc.numel():
                    raise RuntimeError("run one eager step with the same parameters before capturing")
                self._pinned_spare = None
                sp[0].copy_(ht)
                sp[1].copy_(hc)
                t = torch.empty(ht.shape, dtype=ht.dtype, device=device)
                c = torch.empty(hc.shape, dtype=hc.dtype, device=device)
                t.copy_(sp[0], non_blocking=True)
                c.copy_(sp[1], non_blocking=True)
                self._pinned_owned.append(sp)
                ops._keep_for_capture((t, c))         # the captured update reads them on every replay
            else:
                # Gradients are fresh tensors every step (zero_grad(set_to_none=True)), so the POINTER table changes
                # every step.  A pageable host->device copy blocks the host until the stream has drained -- the host then
                # starts issuing the next step on an idle GPU, every step -- so the table goes through pinned memory,
                # asynchronously; the chunk list depends on the sizes only and is uploaded once.
                ck = (tuple(int(n) for n in table["n"]), str(device))
                if self._chunk_cache is None or self._chunk_cache[0] != ck:
                    self._chunk_cache = (ck, hc.to(device), len(chunks))
                c = self._chunk_cache[1]
                # (a fresh pinned block per step from torch's caching host allocator, which hands a block out again
                # only after the copy that read it has executed: the host runs several steps ahead of the GPU, a ring
                # of two staging buffers with an event wait measured 13 ms of host stall per step)
                t = torch.empty(ht.shape, dtype=ht.dtype, device=device)
                t.copy_(ht.pin_memory(), non_blocking=True)
                if getattr(self, "capturable", False) and self._pinned_spare is None:
                    self._pinned_spare = (torch.empty_like(ht).pin_memory(), torch.empty_like(hc).pin_memory())
            self._cache_key, self._cache = key, (t, c, len(chunks))
        return self._cache

    # ---- clipping ------------------------------------------------------------------------------------------
    @property
    def last_grad_norm(self):
        """|grad_scale| * ||g||_2 of the last step taken with max_grad_norm (a view of clip[2]); None before that."""
        return None if self._clip is None else self._clip[2]

    @property
    def last_clip_coef(self):
        """min(1, max_grad_norm / (last_grad_norm + 1e-6)), what that step multiplied its gradients by (clip[3])."""
        return None if self._clip is None else self._clip[3]

    def _clip_on(self) -> bool:
        _check_clip(self.max_grad_norm, self.clip_grad_value)
        return self.max_grad_norm is not None or self.clip_grad_value is not None

    def sync_clip(self):
        """Push a changed max_grad_norm / clip_grad_value to the device copy; never inside a capture."""
        if self._clip is None or not self._clip_on():
            return
        want = _clip_inputs(self.max_grad_norm, self.clip_grad_value)
        if want != self._clip_host:
            self._clip[:2].copy_(torch.tensor(want, dtype=torch.float32))
            self._clip_host = want

    def _clip_array(self, device, nchunks, capturing):
        """The device clip array (inputs current) with room for `nchunks` partial sums behind it; allocated by an eager
        step, so a capture finds both in place."""
        if self._clip is None or self._partials is None or self._partials.numel() < nchunks:
            if capturing:
                raise RuntimeError("run one eager step with the same clipping before capturing")
            if self._clip is None:
                self._clip = torch.zeros(4, dtype=torch.float32, device=device)
                self._clip_host = None
            if self._partials is None or self._partials.numel() < nchunks:
                self._partials = torch.empty(nchunks, dtype=torch.float64, device=device)
        if capturing:
            ops._keep_for_capture((self._clip, self._partials))   # the captured launches read and write them on every replay
        else:
            self.sync_clip()
        return self._clip

    def _norm(self, launches, device, hyper=None):
        """One norm launch over the gradients of every update launch of this step.  launches: [(ptrs, (t, c, n))]."""
        if len(launches) == 1:
            t, c, n = launches[0][1]
        else:
            # several parameter groups / step-count buckets: the norm still spans them all, through a work list of its
            # own (gradient pointers only)
            ptrs = [(0, q[1], 0, 0, q[4]) for ptrs_, _ in launches for q in ptrs_]
            key = tuple(ptrs)
            if self._norm_tables is None or self._norm_tables[0] != key:
                table, chunks = build_tables(ptrs)
                ht = torch.from_numpy(table.view(np.uint8).copy()).pin_memory()
                hc = torch.from_numpy(chunks.view(np.uint8).copy()).pin_memory()
                self._norm_tables = (key, (ht.to(device, non_blocking=True), hc.to(device, non_blocking=True),
                                           len(chunks)))
            t, c, n = self._norm_tables[1]
        clip = self._clip_array(device, n, torch.cuda.is_current_stream_capturing())
        ops.grad_norm_multi(t, c, n, self._partials, clip, float(self.grad_scale), hyper)
        return clip

    def _clipped(self, launches, update):
        """launches: [(key, ptrs, device, args)] of one step; update: ops.adam_multi_clip / ops.sgd_multi_clip."""
        device = launches[0][2]
        if len(launches) == 1:
            key, ptrs, _, args = launches[0]
            tabs = self._tables(key, ptrs, device)
            clip = (self._norm([(ptrs, tabs)], device) if self.max_grad_norm is not None
                    else self._clip_array(device, 0, False))
            update(*tabs, *args, clip)
            return
        # (_tables keeps ONE work list: with several launches per step each is rebuilt in its turn, as without clipping)
        clip = (self._norm([(ptrs, None) for _, ptrs, _, _ in launches], device) if self.max_grad_norm is not None
                else self._clip_array(device, 0, False))
        for key, ptrs, dev, args in launches:
            update(*self._tables(key, ptrs, dev), *args, clip)

    @staticmethod
    def _check(p):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("fused optimizer: parameters must be contiguous fp32 device tensors")
        g = p.grad
        if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
            raise RuntimeError("fused optimizer: gradients must be dense contiguous fp32")


class FusedAdam(_FusedBase):
    """capturable=True keeps lr / betas / eps / weight decay / grad scale AND the step count in a device tensor
    (`dram_adam_multi_dev`): the update can then be captured in a hipGraph together with forward and backward
    (graph.GraphedTrainStep) and replayed across steps and lr changes; requires one parameter group whose
    parameters share their step count."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 max_grad_norm=None, clip_grad_value=None):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm,
                         clip_grad_value)
        self.capturable = bool(capturable)
        self._hyper = None            # device float32[7]: lr, b1, b2, eps, wd, grad_scale, step (int32 bits)
        self._hyper_host = None
        self._replayed = 0            # graph replays whose step the host-side state has not absorbed yet

    # ---- capturable mode -----------------------------------------------------------------------------------
    def _host_hyper(self, group):
        b1, b2 = group["betas"]
        return [float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                float(self.grad_scale)]

    def sync_hyper(self):
        """Push lr (ExponentialLR mutates param_groups[0]['lr']) and friends -- max_grad_norm / clip_grad_value among
        them -- to the device copy when they changed.  Called by step() and by GraphedTrainStep before every replay;
        never inside a capture."""
        self.sync_clip()
        if self._hyper is None:
            return
        want = self._host_hyper(self.param_groups[0])
        if want != self._hyper_host:
            self._hyper[:6].copy_(torch.tensor(want, dtype=torch.float32))
            self._hyper_host = want

    def note_replayed_step(self):
        """A captured step was replayed: the device-side step counter advanced without this object's step(), and
        the replayed update rewrote every parameter through raw pointers -- no torch version counter moved -- so
        the packed / Winograd-transformed weights cached for no_grad forwards are stale from here on."""
        self._replayed += 1
        ops.weights_changed()

    def _absorb_replays(self):
        if self._replayed:
            for st in self.state.values():
                if "step" in st:
                    st["step"] += self._replayed
            self._replayed = 0

    def state_dict(self):
        self._absorb_replays()
        return super().state_dict()

    def _step_capturable(self):
        if len(self.param_groups) != 1:
            raise RuntimeError("FusedAdam(capturable=True) supports one parameter group")
        group = self.param_groups[0]
        plist = [p for p in group["params"] if p.grad is not None]
        if not plist:
            return
        capturing = torch.cuda.is_current_stream_capturing()
        self._absorb_replays()
        steps = set()
        for p in plist:
            self._check(p)
            st = self.state[p]
            if len(st) == 0:
                if capturing:
                    raise RuntimeError("run at least one eager step before capturing (optimizer state is created lazily)")
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            steps.add(int(st["step"].item()))
        if len(steps) != 1:
            raise RuntimeError("FusedAdam(capturable=True): parameters must share their step count")
        if self._hyper is None:
            if capturing:
                raise RuntimeError("run at least one eager step before capturing")
            self._hyper_host = self._host_hyper(group)
            self._hyper = torch.tensor(self._hyper_host + [0.0], dtype=torch.float32, device=plist[0].device)
            self._hyper[6:].view(torch.int32).fill_(int(steps.pop()))      # the kernel keeps the step count as int32 bits
        elif not capturing:
            self.sync_hyper()
        ptrs = [(p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                 self.state[p]["exp_avg_sq"].data_ptr(), p.numel()) for p in plist]
        t, c, n = self._tables((0, "dev", tuple(ptrs)), ptrs, plist[0].device)
        if self._clip_on():
            if self.max_grad_norm is not None:
                clip = self._norm([(ptrs, (t, c, n))], plist[0].device, self._hyper)
            else:
                clip = self._clip_array(plist[0].device, 0, capturing)
            ops.adam_multi_dev_clip(t, c, n, self._hyper, clip)
        else:
            ops.adam_multi_dev(t, c, n, self._hyper)
        if not capturing:             # a capture pass records the update without executing it; replays are counted
            for p in plist:           # through note_replayed_step()
                self.state[p]["step"] += 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_capturable()
            ops.weights_changed()
            return loss
        clip_on = self._clip_on()
        launches = []                # clipping: the update launches wait for the norm over all of them
        for gi, group in enumerate(self.param_groups):
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check(p)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append(p)
            b1, b2 = group["betas"]
            for step, plist in by_step.items():
                ptrs = [(p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                         self.state[p]["exp_avg_sq"].data_ptr(), p.numel()) for p in plist]
                key = (gi, tuple(ptrs))
                args = (float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], 1.0 - b1 ** step,
                        1.0 - b2 ** step, float(self.grad_scale))
                if clip_on:
                    launches.append((key, ptrs, plist[0].device, args))
                    continue
                t, c, n = self._tables(key, ptrs, plist[0].device)
                ops.adam_multi(t, c, n, *args)
        if launches:
            self._clipped(launches, ops.adam_multi_clip)
        ops.weights_changed()        # the kernel wrote the parameters through raw pointers
        return loss


class FusedSGD(_FusedBase):
    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, max_grad_norm=None, clip_grad_value=None):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameter")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay), max_grad_norm,
                         clip_grad_value)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip_on = self._clip_on()
        launches = []
        for gi, group in enumerate(self.param_groups):
            first, rest = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check(p)
                st = self.state[p]
                if group["momentum"] != 0 and "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(p)
                    first.append(p)
                else:
                    rest.append(p)
            for is_first, plist in ((True, first), (False, rest)):
                if not plist:
                    continue
                ptrs = [(p.data_ptr(), p.grad.data_ptr(),
                         self.state[p]["momentum_buffer"].data_ptr() if group["momentum"] != 0 else 0, 0, p.numel())
                        for p in plist]
                args = (float(group["lr"]), group["momentum"], group["weight_decay"], is_first, float(self.grad_scale))
                if clip_on:
                    launches.append(((gi, is_first, tuple(ptrs)), ptrs, plist[0].device, args))
                    continue
                t, c, n = self._tables((gi, is_first, tuple(ptrs)), ptrs, plist[0].device)
                ops.sgd_multi(t, c, n, *args)
        if launches:
            self._clipped(launches, ops.sgd_multi_clip)
        ops.weights_changed()
        return loss


# ---- drop-in torch.nn.utils.clip_grad_norm_ / clip_grad_value_ (in place) -------------------------------------------
def _grad_tables(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
            raise RuntimeError("gradients must be dense contiguous fp32 device tensors")
        if g.device != grads[0].device:
            raise RuntimeError("gradients must live on one device")
    if not grads:
        return None
    table, chunks = build_tables([(0, g.data_ptr(), 0, 0, g.numel()) for g in grads])
    dev = grads[0].device
    return (torch.from_numpy(table.view(np.uint8).copy()).to(dev), torch.from_numpy(chunks.view(np.uint8).copy()).to(dev),
            len(chunks), dev)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ on the HIP kernels: scales the gradients IN PLACE by min(1, max_norm / (norm +
    1e-6)) and returns the total 2-norm as a 0-dim device tensor.  The fused optimizers' max_grad_norm does the same
    without rewriting a gradient; this form is for callers who look at the gradients afterwards."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_: only norm_type=2 is implemented")
    _check_clip(max_norm, None)
    tabs = _grad_tables(parameters)
    if tabs is None:
        return torch.tensor(0.0)
    t, c, n, dev = tabs
    with ops.launch_scope(dev):
        clip = torch.tensor(_clip_inputs(max_norm, None) + [0.0, 0.0], dtype=torch.float32).to(dev)
        ops.grad_norm_multi(t, c, n, torch.empty(n, dtype=torch.float64, device=dev), clip, 1.0)
        ops.grad_scale_multi(t, c, n, clip)
    return clip[2]


@torch.no_grad()
def clip_grad_value_(parameters, clip_value):
    """torch.nn.utils.clip_grad_value_ on the HIP kernels: clamps every gradient element to [-clip_value, clip_value]
    IN PLACE (a NaN stays a NaN)."""
    _check_clip(None, clip_value)
    tabs = _grad_tables(parameters)
    if tabs is None:
        return
    t, c, n, dev = tabs
    with ops.launch_scope(dev):
        ops.grad_scale_multi(t, c, n, torch.tensor(_clip_inputs(None, clip_value) + [0.0, 0.0],
                                                   dtype=torch.float32).to(dev))
