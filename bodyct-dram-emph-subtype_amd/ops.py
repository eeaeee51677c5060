"""Tensor-level wrappers over the C ABI (include/dram_hip.h).

PyTorch is used here for device memory (``torch.empty``) and the current HIP stream
only; every computation is a hand-written kernel in libdram_hip.so.  Each wrapper
validates on the host that operand shapes/dtypes match what the kernel and its grid
assume *before* launching (a faulting kernel can reset the whole GPU host).

Activations are NDHWC float32: ``[B, D, H, W, C]``.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import math
import os
import threading
import weakref
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import DramConvDesc

Tensor = torch.Tensor


def _L():
    return _lib.load()


_TLS = threading.local()        # forward runs on the caller's thread, backward on autograd's device thread


@contextlib.contextmanager
def launch_scope(device):
    """Pin the launch device for a run of kernels: makes `device` torch's current device (so the
    stream handed to the library belongs to the GPU the operand pointers live on), caches the stream
    handle, and lets `_req` reject operands that live on any other GPU *before* a kernel is launched
    with foreign pointers (a page fault / GPU reset instead of a Python error)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("libdram_hip has no CPU path")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    prev = getattr(_TLS, "scope", None)
    with torch.cuda.device(idx):
        _TLS.scope = (idx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        try:
            yield
        finally:
            _TLS.scope = prev


def tuning_env(name: str, default: str) -> str:
    """A/B and test switches (DRAM_WGRAD_STREAM, DRAM_BF16_S2, DRAM_STEM_BF16, DRAM_SIDE_PRIORITY and the kernel-variant
    switches read inside the library) count ONLY under DRAM_TUNING=1 (tests/conftest.py, tools/, bench.py set it): a
    stray DRAM_* variable cannot change which kernels the product path runs.  User-facing settings --
    DRAM_STORAGE, DRAM_RECOMPUTE, DRAM_DIST_FORCE -- are read directly (README)."""
    return os.environ.get(name, default) if os.environ.get("DRAM_TUNING", "0") == "1" else default


_SIDE: Dict[tuple, "torch.cuda.Stream"] = {}


def side_stream(device_index: int, which: int = 0) -> "torch.cuda.Stream":
    """The per-device side HIP streams of the engine (weight-gradient kernels run there, concurrently with the
    data-gradient chain on the caller's stream; `which` = 0, 1: consecutive layers alternate, so one layer's HBM-bound
    transforms run under the previous layer's matrix-bound GEMM)."""
    s = _SIDE.get((device_index, which))
    if s is None:
        prio = int(tuning_env("DRAM_SIDE_PRIORITY", "0"))     # A/B switch (tools): HIP stream priority of the side stream
        s = _SIDE[(device_index, which)] = torch.cuda.Stream(device=device_index, priority=prio)
    return s


@contextlib.contextmanager
def on_stream(stream: "torch.cuda.Stream"):
    """Launch the enclosed kernels (and make the enclosed allocations) on `stream`; inside a launch_scope the
    cached stream handle follows."""
    prev = getattr(_TLS, "scope", None)
    with torch.cuda.stream(stream):
        if prev is not None:
            _TLS.scope = (prev[0], ctypes.c_void_p(stream.cuda_stream))
        try:
            yield
        finally:
            _TLS.scope = prev


def _launch_device() -> int:
    sc = getattr(_TLS, "scope", None)
    return sc[0] if sc is not None else torch.cuda.current_device()


def _stream():
    sc = getattr(_TLS, "scope", None)
    if sc is not None:
        return sc[1]
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


def _req(t: Tensor, name: str, dtype=torch.float32, shape=None):
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (libdram_hip has no CPU path)")
    if t.device.index != _launch_device():
        raise RuntimeError(f"{name}: lives on cuda:{t.device.index} but kernels launch on cuda:{_launch_device()} "
                           "(all operands of a call must be on the current device)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _n_regions(fn: str, n_regions, hi: int = 15) -> int:
    """n_regions as an int in 1..hi: 15 rows are what the region kernels hold, 7 what ``lung_zones`` can still double,
    5 what ``lobe_zones`` can still triple."""
    n = int(n_regions)
    if not 1 <= n <= hi:
        note = {7: " (2 n <= 15 rows downstream)", 5: " (3 n <= 15 rows downstream)"}.get(hi, "")
        raise ValueError(f"{fn}: n_regions must be 1..{hi}{note}, got {n_regions}")
    return n


def _label_view(fn: str, t, name: str, like_shape=None):
    """The label-volume operand of ``fn``, as the kernels read it in place: a non-empty [D,H,W] tensor of uint8 / int16
    / bool (seen as uint8), of ``like_shape`` where given, below 2^31 voxels; a view whose x stride is not 1 is made
    contiguous first.  -> (tensor, dtype code 1 | 2, z stride, y stride).  The host-only refusals come first; the one
    device check (a CPU tensor ends there) is the last step."""
    if not isinstance(t, Tensor) or t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{fn}: {name} must be a non-empty [D,H,W] tensor")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype not in (torch.uint8, torch.int16):
        raise TypeError(f"{fn}: expected uint8, int16 or bool {name}, got {t.dtype}")
    if like_shape is not None and tuple(t.shape) != tuple(like_shape):
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} must have the image's shape {tuple(like_shape)}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: volumes of 2^31 voxels or more are not supported")
    if (t.shape[2] > 1 and t.stride(2) != 1) or min(t.stride()) < 0:
        t = t.contiguous()
    with launch_scope(t.device):
        _req(t[0, 0], f"{fn}: {name}", t.dtype)                    # device; a row is contiguous
    return t, (2 if t.dtype == torch.int16 else 1), int(t.stride(0)), int(t.stride(1))


def _volume(fn: str, t, name: str, dtypes=None, nonempty: bool = True) -> Tuple[int, int, int]:
    """The host-only refusals of the [D,H,W] operand ``name`` that a scan-side wrapper reads through a plain pointer: a
    non-empty 3-D tensor, one of ``dtypes`` (None: left to ``_req`` behind the device check, as ``lobe_histogram`` has
    it), below 2^31 voxels.  ``nonempty=False`` is ``laa_components``: there an empty image falls to the labels' check.
    -> (D, H, W) as ints."""
    if not isinstance(t, Tensor) or t.dim() != 3 or (nonempty and min(t.shape) < 1):
        raise ValueError(f"{fn}: {name} must be a {'non-empty ' if nonempty else ''}[D,H,W] tensor")
    if dtypes is not None and t.dtype not in dtypes:
        kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise TypeError(f"{fn}: expected {'' if name.endswith('s') else 'an '}{kinds} {name}, got {t.dtype}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: volumes of 2^31 voxels or more are not supported")
    return tuple(int(v) for v in t.shape)


def _out(fn: str, name: str, t, shape, dtype, device, apart, a: Optional[str] = None,
         of: Optional[str] = "the image's shape", rest: str = "image"):
    """The refusals of a caller's output tensor ``name``: its type (``a``: how the message names it), ``shape`` and
    contiguity in one (``of`` names the shape; None: the shape alone, for ``local_fraction3d``, whose ``out_u8`` is a
    view), the image's ``device``, and no storage shared with a tensor in ``apart`` (``rest`` names them)."""
    if not isinstance(t, Tensor) or t.dtype != dtype:
        raise TypeError(f"{fn}: {name} must be {a or f'a {dtype}'} tensor")
    if of is None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{fn}: {name} must have the image's shape {tuple(shape)}, got {tuple(t.shape)}")
    if of is not None and (tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
        raise ValueError(f"{fn}: {name} must be contiguous and of {of} {tuple(shape)}")
    if t.device != device:
        raise ValueError(f"{fn}: {name} must live on the image's device")
    if any(t.untyped_storage().data_ptr() == o.untyped_storage().data_ptr() for o in apart):
        raise ValueError(f"{fn}: {name} must not share storage with {rest}")


def _radius(fn: str, sigma, truncate) -> int:
    """``int(truncate * sigma + 0.5)``; ValueError in the name of ``fn`` for a negative or non-finite sigma and for
    ``truncate`` <= 0"""
    sigma, truncate = float(sigma), float(truncate)
    if not math.isfinite(sigma) or sigma < 0:
        raise ValueError(f"{fn}: sigma must be finite and >= 0, got {sigma!r}")
    if not math.isfinite(truncate) or truncate <= 0:
        raise ValueError(f"{fn}: truncate must be finite and > 0, got {truncate!r}")
    return int(truncate * sigma + 0.5)


def _sigma3(fn: str, sigma) -> Tuple[float, float, float]:
    try:
        sig = [float(v) for v in sigma] if hasattr(sigma, "__len__") or hasattr(sigma, "__iter__") else [float(sigma)] * 3
    except (TypeError, ValueError):
        sig = []
    if len(sig) != 3:
        raise ValueError(f"{fn}: sigma must be a number or three of them (z, y, x), got {sigma!r}")
    return tuple(sig)


def _spacing3(fn: str, spacing) -> List[float]:
    """A voxel spacing in mm as three floats (z, y, x); ValueError unless it is three finite numbers > 0"""
    try:
        sp = [float(v) for v in spacing]
    except (TypeError, ValueError):
        sp = []
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"{fn}: spacing must be three finite numbers > 0 (z, y, x), got {spacing!r}")
    return sp


def _hu_threshold(fn: str, threshold, noun: str = "an integer", bools: bool = False) -> int:
    """An LAA threshold as an int: a whole number in -32768..32768 -- one past int16, so that ``image < threshold`` can
    hold everywhere -- or ValueError; a bool is none, except to ``laa_components`` (``bools``), which always took it"""
    try:
        ok = (bools or not isinstance(threshold, bool)) and int(threshold) == threshold and -32768 <= int(threshold) <= 32768
    except (TypeError, ValueError, OverflowError):                     # None, a string, NaN, inf
        ok = False
    if not ok:
        raise ValueError(f"{fn}: threshold must be {noun} in -32768..32768, got {threshold!r}")
    return int(threshold)


BF16 = torch.bfloat16


def _act(t: Tensor, name: str, shape=None, like: Optional[Tensor] = None) -> str:
    """Validate an ACTIVATION tensor (float32, or bfloat16 on the bf16-storage path) and return the entry-point
    suffix of its storage type ("" | "_bf16").  `like`: another activation of the same call, whose type it must share."""
    if not isinstance(t, Tensor) or t.dtype not in (torch.float32, BF16):
        raise TypeError(f"{name}: expected a float32 or bfloat16 device tensor, got {getattr(t, 'dtype', type(t))}")
    _req(t, name, t.dtype, shape)
    if like is not None and like.dtype != t.dtype:
        raise TypeError(f"{name}: {t.dtype} but the call's other activations are {like.dtype}")
    return "_bf16" if t.dtype == BF16 else ""


def _fn(name: str, sfx: str):
    return getattr(_L(), name + sfx)


def cast(t: Tensor, dtype) -> Tensor:
    """float32 <-> bfloat16 copy of an activation tensor (round to nearest even) with the library's cast kernels."""
    if t.dtype == dtype:
        return t
    _act(t, "t")
    out = torch.empty(t.shape, device=t.device, dtype=dtype)
    if dtype == BF16:
        _chk(_L().dram_cast_f32_to_bf16(_p(t), _p(out), t.numel(), _stream()), "dram_cast_f32_to_bf16")
    elif dtype == torch.float32:
        _chk(_L().dram_cast_bf16_to_f32(_p(t), _p(out), t.numel(), _stream()), "dram_cast_bf16_to_f32")
    else:
        raise TypeError(f"cast: unsupported target {dtype}")
    return out


class KernelTimeline:
    """The library's own kernel timeline (dram_profile_*): every kernel launch bracketed by two
    hipEvents on its launch stream, tagged with family / executed MFMA FLOPs / direct-convolution FLOPs
    / algorithmic HBM bytes.  bench.py's roofline table is built from it."""

    def __init__(self, max_records: int = 1 << 16):
        self.max_records = int(max_records)

    def start(self):
        _chk(_L().dram_profile_start(self.max_records), "dram_profile_start")

    def stop(self):
        _chk(_L().dram_profile_stop(), "dram_profile_stop")

    def families(self):
        """{family name: dict(bound, launches, ms, mfma_flops, alg_flops, hbm_bytes, variants{variant: [launches, ms]})}
        (synchronises the device)"""
        L = _L()
        buf = (_lib.DramProfRecord * self.max_records)()
        n = L.dram_profile_read(buf, self.max_records)
        if n < 0:
            raise RuntimeError(f"dram_profile_read failed with code {n}")
        out = {}
        for i in range(n):
            r = buf[i]
            name = L.dram_profile_family_name(r.family).decode()
            d = out.setdefault(name, dict(bound="mfma" if L.dram_profile_family_is_mfma(r.family) else "hbm",
                                          launches=0, ms=0.0, mfma_flops=0.0, alg_flops=0.0, hbm_bytes=0.0,
                                          variants={}))
            d["launches"] += 1
            d["ms"] += r.ms
            d["mfma_flops"] += r.mfma_flops
            d["alg_flops"] += r.alg_flops
            d["hbm_bytes"] += r.hbm_bytes
            v = d["variants"].setdefault(int(r.variant), [0, 0.0])
            v[0] += 1
            v[1] += r.ms
        self.dropped = int(L.dram_profile_dropped())
        return out


class KernelProfiler:
    """HIP-event timing of whole convolution calls on torch's current stream (bench.py --detail: the
    per-layer table).  Records (family, algorithmic flops, start, end) per call; summary() after a sync."""

    def __init__(self):
        self.records = []

    def span(self, family: str, flops: float, detail: str = ""):
        return _Span(self, family, flops, detail)

    def by_launch(self):
        """{(family, detail): dict(launches, ms, flops)} -- per-geometry breakdown."""
        torch.cuda.synchronize()
        out = {}
        for fam, flops, a, b, detail in self.records:
            d = out.setdefault((fam, detail), dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += a.elapsed_time(b)
            d["flops"] += flops
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for fam, flops, a, b, _ in self.records:
            d = out.setdefault(fam, dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += a.elapsed_time(b)
            d["flops"] += flops
        return out


class _Span:
    def __init__(self, prof, family, flops, detail=""):
        self.prof, self.family, self.flops, self.detail = prof, family, flops, detail

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        self.prof.records.append((self.family, self.flops, self.a, self.b, self.detail))


class _NoSpan:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


_PROFILER: Optional[KernelProfiler] = None
_NOSPAN = _NoSpan()


def set_profiler(p: Optional[KernelProfiler]):
    global _PROFILER
    _PROFILER = p


def _span(family: str, flops: float, detail: str = ""):
    return _NOSPAN if _PROFILER is None else _PROFILER.span(family, flops, detail)


@dataclass(frozen=True)
class ConvGeom:
    """Forward-sense geometry of one convolution call."""
    B: int
    D: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int
    stride: int
    pad: int
    dil: int
    tol: int = 0        # 0 or _lib.DRAM_CONV_ROUNDING_TOLERANT: plan hint set by the engine for BasicBlock networks

    def out(self, n: int) -> int:
        return (n + 2 * self.pad - (self.dil * (self.k - 1) + 1)) // self.stride + 1

    @property
    def Do(self):
        return self.out(self.D)

    @property
    def Ho(self):
        return self.out(self.H)

    @property
    def Wo(self):
        return self.out(self.W)

    @property
    def taps(self):
        return self.k ** 3

    @property
    def flops(self) -> float:
        """algorithmic FLOPs of one pass (fwd, dgrad and wgrad each): 2*M*N*K"""
        return 2.0 * self.B * self.Do * self.Ho * self.Wo * self.Cout * self.Cin * self.taps

    @property
    def in_shape(self):
        return (self.B, self.D, self.H, self.W, self.Cin)

    @property
    def out_shape(self):
        return (self.B, self.Do, self.Ho, self.Wo, self.Cout)

    def desc(self) -> DramConvDesc:
        return DramConvDesc(self.B, self.D, self.H, self.W, self.Cin, self.Do, self.Ho, self.Wo, self.Cout,
                            self.k, self.stride, self.pad, self.dil, self.tol)


# --------------------------------------------------------------------------- conv
# Memory a CAPTURED launch bakes a pointer of (scratch buffers, device work lists) must outlive the graph, and must not
# be handed to anybody else meanwhile.  Whoever owns a capture passes a list to capture_keepalive() and keeps it as long
# as the graph (graph.GraphedTrainStep does); captures made without one pin such memory for the life of the process.
_CAPTURE_KEEP: List[object] = []
_CAPTURE_OWNER: Optional[List[object]] = None       # process-wide: backward runs on autograd's thread, not the caller's


@contextlib.contextmanager
def capture_keepalive(owner: List[object]):
    global _CAPTURE_OWNER
    prev, _CAPTURE_OWNER = _CAPTURE_OWNER, owner
    try:
        yield owner
    finally:
        _CAPTURE_OWNER = prev


def capture_id() -> int:
    """0 when the launch stream is not being captured into a hipGraph, else a number unique to that capture."""
    return int(_L().dram_stream_capture_id(_stream()))


def _keep_for_capture(obj):
    keep = _CAPTURE_OWNER if _CAPTURE_OWNER is not None else _CAPTURE_KEEP
    if not any(o is obj for o in keep[-16:]):
        keep.append(obj)


_WORKSPACE: Dict[tuple, Tensor] = {}
_CAPTURE_WS: Dict[tuple, "weakref.ref"] = {}        # (device, stream, capture id) -> the capture's own scratch (weak)


def _workspace(nbytes: int, device) -> Tensor:
    """Grow-only scratch shared by the conv passes that run back to back on ONE stream (one buffer per
    (device, launch stream): the weight-gradient stream has its own)."""
    device = torch.device(device)
    n = (nbytes + 3) // 4
    cid = capture_id()
    if cid:
        # capturing: a buffer of THIS capture's own (from the graph's private pool), owned by the capture's keep-alive
        # list -- never shared with an eager call or another capture on the same stream, never evicted: the graph
        # writes to it on every replay.  A buffer it outgrows stays alive too (earlier captured launches use it).
        key = (device, _stream().value, cid)
        ref = _CAPTURE_WS.get(key)
        ws = ref() if ref is not None else None
        if ws is None or ws.numel() < n:
            ws = torch.empty((n,), device=device, dtype=torch.float32)
            _keep_for_capture(ws)
            for k in [k for k, r in _CAPTURE_WS.items() if r() is None]:
                del _CAPTURE_WS[k]
            _CAPTURE_WS[key] = weakref.ref(ws)
        return ws
    key = (device, _stream().value)
    ws = _WORKSPACE.pop(key, None)                  # re-inserted below: the dict stays in least-recently-used order
    if ws is None or ws.numel() < n:
        ws = None
        ws = torch.empty((n,), device=device, dtype=torch.float32)
        while len(_WORKSPACE) >= 6:                 # caller stream + side stream + a few more; streams that went away
            _WORKSPACE.pop(next(iter(_WORKSPACE)))  # must not pin up to 0.7 GB each
    _WORKSPACE[key] = ws
    return ws


# environment switches the library's plan functions read (tests flip them between cases): part of the plan-cache key
_PLAN_ENV = ("DRAM_CONV_ALGO", "DRAM_WINO_TILING", "DRAM_MATH", "DRAM_W2D_V", "DRAM_IGEMM_V", "DRAM_IGEMM_V3_FORCE",
             "DRAM_WGRAD_V", "DRAM_BF16_NW", "DRAM_BF16_WGRAD", "DRAM_NN_STREAM")


class _ConvAlgo(NamedTuple):
    """One forward / data-gradient algorithm: what a caller has to know to pack for it and to launch it."""
    family: str                 # profiler family of its launches
    rows: str                   # query: rows of the forward's statistics
    points: object              # leading dimension of the packed wf and wb: None the kernel's taps, or the (wf, wb) queries
    pack: str                   # (w, wf, wb, ...
    pack_ints: int              # ... the first so many of Cout, Cin, taps -- none of them: the desc -- and the stream)
    fwd: str                    # (x, wf, bias, y, stats, ...
    bwd: str                    # (dy, wb, dx, add, gate, ...
    ws: bool = False            # ... v, desc, ws, nbytes, stream) with the plan's ws_fwd / ws_bwd, else ... desc, stream)
    rows_bwd: Optional[str] = None      # query: rows of the statistics its data gradient can take along


class _WgradAlgo(NamedTuple):
    """One weight-gradient algorithm: (x, [v_cache,] dy, dw, desc, ws, nbytes, stream)."""
    family: str
    fn: str
    workspace: tuple            # query of its workspace bytes, and what it takes behind the desc
    v_cache: bool = False       # takes the forward's transformed input, and can run from it alone
    min_ws: int = 0             # scratch to hold even where the plan asks for none

    def ws_bytes(self, L, d) -> int:
        return int(getattr(L, self.workspace[0])(d, *self.workspace[1:]))


# dram_conv_algo's answers, and the bf16-storage kernels (ConvPlan.bf16: 3x3x3 stride 1 and 1x1x1)
_CONV_ALGOS = {
    0: _ConvAlgo("conv_igemm_kernel", "dram_conv_num_mtiles", None, "dram_pack_conv_weight", 3,
                 "dram_conv3d_fwd", "dram_conv3d_bwd_data"),
    1: _ConvAlgo("conv_wino_kernels", "dram_wino_num_stat_rows", ("dram_wino_num_points", "dram_wino_num_points_bwd"),
                 "dram_wino_pack_weight", 0, "dram_wino_conv3d_fwd", "dram_wino_conv3d_bwd_data", ws=True,
                 rows_bwd="dram_wino_num_stat_rows_bwd"),
    2: _ConvAlgo("conv_wino2d_kernel", "dram_wino2d_num_stat_rows", 48, "dram_wino2d_pack_weight", 2,
                 "dram_wino2d_conv3d_fwd", "dram_wino2d_conv3d_bwd_data"),
    3: _ConvAlgo("conv1x1_gemm", "dram_conv1x1_num_stat_rows", None, "dram_pack_conv_weight", 3,      # wf IS the weight
                 "dram_conv1x1_fwd", "dram_conv1x1_bwd_data"),
    BF16: _ConvAlgo("conv3_bf16_kernel", "dram_conv_bf16_num_stat_rows", None, "dram_pack_conv_weight_bf16", 3,
                    "dram_conv3d_fwd_bf16", "dram_conv3d_bwd_data_bf16"),
}
# dram_conv_wgrad_algo's answers, and the bf16-storage kernel
_WGRAD_ALGOS = {
    0: _WgradAlgo("conv_wgrad_kernel+reduce", "dram_conv3d_bwd_weight", ("dram_conv3d_bwd_weight_workspace",)),
    1: _WgradAlgo("conv_wino_kernels", "dram_wino_conv3d_bwd_weight", ("dram_wino_workspace", 2), v_cache=True),
    2: _WgradAlgo("conv_wgrad_w2d_kernel+reduce", "dram_wgrad_w2d", ("dram_wgrad_w2d_workspace",)),
    3: _WgradAlgo("conv1x1_gemm", "dram_conv1x1_bwd_weight", ("dram_conv1x1_bwd_weight_workspace",), min_ws=4),
    BF16: _WgradAlgo("wgrad3_bf16_kernel+reduce", "dram_conv3d_bwd_weight_bf16", ("dram_conv3d_bwd_weight_bf16_workspace",)),
}


class ConvPlan:
    """Everything the host needs to know about one convolution geometry, asked from the library ONCE per
    (geometry, plan-relevant environment): forward / weight-gradient algorithm (the rows of _CONV_ALGOS / _WGRAD_ALGOS
    its launches go through), packed-weight leading dimensions, statistic rows, workspace sizes, cached-transform
    size -- ~12 host calls into the library (each of which re-derives tilings and reads the environment) instead of
    that many per launch."""
    __slots__ = ("desc", "dref", "desc_ovl", "dref_ovl", "algo", "walgo", "conv", "wgrad", "taps_f", "taps_b", "stat_rows",
                 "stat_rows_bwd", "ws_fwd", "ws_bwd", "ws_wgrad", "wgrad_from_v", "v_elems", "bf16", "bf16_stat_rows",
                 "bf16_ws_wgrad", "prologue")

    def __init__(self, g: "ConvGeom"):
        L = _L()
        self.desc = g.desc()
        self.dref = d = ctypes.byref(self.desc)
        # the same geometry with DRAM_CONV_BWD_OVERLAPPED (include/dram_hip.h): a data gradient launched while another
        # stream runs weight-gradient kernels (conv3d_bwd_data(..., overlapped=True))
        self.desc_ovl = g.desc()
        self.desc_ovl.flags |= _lib.DRAM_CONV_BWD_OVERLAPPED
        self.dref_ovl = ctypes.byref(self.desc_ovl)
        self.algo = int(L.dram_conv_algo(d))
        self.walgo = int(L.dram_conv_wgrad_algo(d))
        conv = self.conv = _CONV_ALGOS[self.algo]
        pts = conv.points
        self.taps_f, self.taps_b = [int(getattr(L, q)(d)) for q in pts] if isinstance(pts, tuple) else [pts or g.taps] * 2
        self.stat_rows = int(getattr(L, conv.rows)(d))
        self.stat_rows_bwd = int(getattr(L, conv.rows_bwd)(d)) if conv.rows_bwd else 0
        self.ws_fwd, self.ws_bwd = (int(L.dram_wino_workspace(d, 0)), int(L.dram_wino_workspace(d, 1))) if conv.ws else (0, 0)
        # the weight gradient that RUNS: a pipeline geometry whose TN plan fails reports no workspace and stays on the
        # direct kernel (which needs the input tensor itself)
        self.wgrad = _WGRAD_ALGOS[self.walgo]
        self.v_elems = int(L.dram_wino_v_elems(d)) if (conv.ws or self.wgrad.v_cache) else 0
        self.ws_wgrad = self.wgrad.ws_bytes(L, d)
        if self.wgrad.v_cache and not self.ws_wgrad:
            self.wgrad = _WGRAD_ALGOS[0]
            self.ws_wgrad = self.wgrad.ws_bytes(L, d)
        # can conv3d_bwd_weight run from the forward's cached Winograd-domain input alone (x=None, v_cache=...)?
        self.wgrad_from_v = self.wgrad.v_cache
        # bf16-storage path: the direct bf16-MFMA kernels take the 3x3x3 stride-1 and the 1x1x1 convolutions; the one
        # stride-2 convolution per network runs on them through its space-to-depth form (s2_geom), whatever is left
        # (odd extents) on the fp32 kernels above around cast passes (bf16_route)
        self.prologue = bool(conv.ws and L.dram_wino_prologue_supported(d))
        self.bf16 = bool(L.dram_conv_bf16_supported(d))
        self.bf16_stat_rows = int(getattr(L, _CONV_ALGOS[BF16].rows)(d)) if self.bf16 else 0
        self.bf16_ws_wgrad = _WGRAD_ALGOS[BF16].ws_bytes(L, d) if self.bf16 else 0


_PLANS: Dict[tuple, ConvPlan] = {}


def conv_plan(g: "ConvGeom") -> ConvPlan:
    env = os.environ
    # the library reads the A/B switches under DRAM_TUNING=1 only (csrc/common.h tune_env): without it the plan depends
    # on the geometry alone (13 environment look-ups per call were 1.2 ms of a ResNet-50 step's host time)
    key = (g,) + tuple(env.get(k) for k in _PLAN_ENV) if env.get("DRAM_TUNING") == "1" else g
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = ConvPlan(g)
    return p


def conv_algo(g: "ConvGeom") -> int:
    """Library plan for this geometry (dram_conv_algo): 0 direct implicit GEMM, 1 Winograd
    F(2x2x2,3x3x3) pipeline, 2 fused in-plane Winograd F(2x2,3x3) x direct-z, 3 1x1x1 GEMM."""
    return conv_plan(g).algo


def conv_use_wino(g: "ConvGeom") -> bool:
    return conv_algo(g) == 1


def s2_geom(g: "ConvGeom") -> Optional["ConvGeom"]:
    """bf16 storage: the stride-1 geometry that runs a stride-2 3x3x3 convolution on the bf16 kernels (space to depth:
    eight parity sub-lattices as 8 Cin channels at half the extents, embedded weights -- include/dram_hip.h,
    dram_s2d_bf16), or None (odd extents, another kernel size, or DRAM_BF16_S2=0: fp32 kernels around casts)."""
    if (g.k != 3 or g.stride != 2 or g.pad != 1 or g.dil != 1 or ((g.D | g.H | g.W) & 1) or g.Cin % 8
            or tuning_env("DRAM_BF16_S2", "1") == "0"):
        return None
    g8 = ConvGeom(g.B, g.D // 2, g.H // 2, g.W // 2, 8 * g.Cin, g.Cout, 3, 1, 1, 1, g.tol)
    return g8 if (conv_plan(g8).bf16 and tuple(g8.out_shape) == tuple(g.out_shape)) else None


def s2d(x: Tensor) -> Tensor:
    B, D, H, W, C = x.shape
    x8 = torch.empty((B, D // 2, H // 2, W // 2, 8 * C), device=x.device, dtype=BF16)
    _chk(_L().dram_s2d_bf16(_p(x), _p(x8), B, D, H, W, C, _stream()), "dram_s2d_bf16")
    return x8


def bf16_route(g: "ConvGeom", plan: ConvPlan, w: Optional[Tensor] = None, cin_axis: int = 2
               ) -> Tuple[str, Optional["ConvGeom"]]:
    """How a convolution (g, its plan) runs on bf16 activations -> (route, the geometry its kernels are launched for):
    "native" the bf16 kernels on g; "s2d" stride 2 as stride 1 over the space-to-depth tensor (s2_geom(g)); "casts" the
    fp32 kernels around cast passes.  A pass with a weight operand runs what `w` was packed for (its type, and the
    8 * Cin channels of the embedded weights on `cin_axis`); pack_conv_weight and the weight gradient, which have none,
    ask the plan and then s2_geom."""
    if w is not None:
        if w.dtype != BF16:
            return "casts", g
        return ("s2d", s2_geom(g)) if w.shape[cin_axis] == 8 * g.Cin else ("native", g)
    if plan.bf16:
        return "native", g
    g8 = s2_geom(g)
    return ("casts", g) if g8 is None else ("s2d", g8)


def pack_conv_weight(w: Tensor, want_fwd=True, want_bwd=True, g: Optional["ConvGeom"] = None, dtype=torch.float32
                     ) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """[Cout,Cin,k,k,k] -> wf [taps,Cout,Cin], wb [taps,Cin,Cout]; for a geometry the library plans
    on the Winograd path the packed copies are the transformed weights (64 'taps', wb tap-flipped).
    dtype=bfloat16 (bf16-storage path): bf16 copies for the geometries the bf16 kernels take, the fp32 packing
    otherwise (the convolution then runs on the fp32 kernels around casts; the consumer looks at wf.dtype)."""
    _req(w, "w")
    Cout, Cin = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    plan = conv_plan(g) if g is not None else None
    route = bf16_route(g, plan)[0] if (dtype == BF16 and g is not None) else "casts"
    if route == "casts":
        algo, out_dtype = plan.conv if plan else _CONV_ALGOS[0], torch.float32
        pt, ptb = (plan.taps_f, plan.taps_b) if plan else (taps, taps)
    else:
        algo, out_dtype, pt, ptb = _CONV_ALGOS[BF16], BF16, taps, taps
        if route == "s2d":                              # stride 2: embedded weights of the stride-1 form
            w3 = torch.empty((Cout, 8 * Cin, 3, 3, 3), device=w.device, dtype=torch.float32)
            _chk(_L().dram_s2_embed_weight(_p(w), _p(w3), Cout, Cin, _stream()), "dram_s2_embed_weight")
            w, Cin = w3, 8 * Cin
    wf = torch.empty((pt, Cout, Cin), device=w.device, dtype=out_dtype) if want_fwd else None
    wb = torch.empty((ptb, Cin, Cout), device=w.device, dtype=out_dtype) if want_bwd else None
    ints = (Cout, Cin, taps)[:algo.pack_ints] or (plan.dref,)
    _chk(getattr(_L(), algo.pack)(_p(w), _p(wf), _p(wb), *ints, _stream()), algo.pack)
    return wf, wb


# All bf16 weight packings of a training step in ONE launch (dram_pack_conv_weight_bf16_multi): the device work list is
# built once per set of weights (their addresses and shapes: parameters are updated in place) by an EAGER step and
# reused, also inside hipGraph captures, where a host->device copy is not allowed.
_PACK_TABLES: Dict[tuple, tuple] = {}


def pack_conv_weights_bf16_multi(weights: List[Tensor]):
    """[Cout,Cin,k,k,k] fp32 weights -> [(wf [taps,Cout,Cin], wb [taps,Cin,Cout])] bf16, views of one flat buffer
    written by one kernel; None when no work list exists yet and the stream is capturing (the caller packs one by one)."""
    import numpy as np
    if not weights:
        return []
    key = tuple((w.data_ptr(), tuple(w.shape)) for w in weights)
    ent = _PACK_TABLES.pop(key, None)               # (re-inserted below: least recently USED is evicted first)
    if ent is not None:
        _PACK_TABLES[key] = ent
    if ent is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        tab = np.zeros(len(weights), dtype=np.dtype(_lib.DramPackRef))
        chunks, layout, off = [], [], 0
        for i, w in enumerate(weights):
            _req(w, "w")
            Cout, Cin = w.shape[0], w.shape[1]
            taps = w.shape[2] * w.shape[3] * w.shape[4]
            n = Cout * Cin * taps
            npad = (n + 63) // 64 * 64
            tab[i] = (w.data_ptr(), off, off + npad, Cout, Cin, taps, 0)
            layout.append((off, off + npad, n, taps, Cout, Cin))
            off += 2 * npad
            ntiles = _L().dram_pack_conv_weight_bf16_tiles(Cout, Cin, taps)
            _chk(min(ntiles, 0), "dram_pack_conv_weight_bf16_tiles")
            chunks.extend((i, 0, t) for t in range(ntiles))
        ch = np.array(chunks, dtype=np.dtype(_lib.DramChunkRef))
        dev = weights[0].device
        ent = (torch.from_numpy(tab.view(np.uint8).copy()).to(dev), torch.from_numpy(ch.view(np.uint8).copy()).to(dev),
               len(chunks), off, layout)
        while len(_PACK_TABLES) >= 8:
            _PACK_TABLES.pop(next(iter(_PACK_TABLES)))
        _PACK_TABLES[key] = ent
    if torch.cuda.is_current_stream_capturing():
        _keep_for_capture(ent)                      # the captured launch reads this work list on every replay
    table, chunks, nchunks, total, layout = ent
    flat = torch.empty((total,), device=weights[0].device, dtype=BF16)
    _chk(_L().dram_pack_conv_weight_bf16_multi(_p(table), _p(chunks), nchunks, _p(flat), float(total // 2), _stream()),
         "dram_pack_conv_weight_bf16_multi")
    return [(flat[of:of + n].view(taps, Cout, Cin), flat[ob:ob + n].view(taps, Cin, Cout))
            for of, ob, n, taps, Cout, Cin in layout]


# Packed forward weights of inference calls (no_grad): repacking / re-transforming every weight on every
# forward is pure overhead when the weights did not change.  Entries hang off the weight TENSOR OBJECT (weakly:
# they die with it) and hold a reference to the storage they were packed from, so that address cannot be
# recycled for another tensor while the entry lives; an entry is valid while the tensor still uses that storage,
# its torch version counter is unchanged and no raw-pointer writer (FusedAdam / FusedSGD bump WEIGHT_EPOCH)
# has run.

WEIGHT_EPOCH = 0
_PACKED: Dict[int, tuple] = {}      # id(weight) -> (weakref to the weight, {plan key: entry}); removed when it dies


def weights_changed():
    """Called by anything that rewrites parameters through raw pointers (FusedAdam / FusedSGD)."""
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1


def packed_forward_weight(w: Tensor, g: "ConvGeom", dtype=torch.float32) -> Tensor:
    slot = _PACKED.get(id(w))
    if slot is None or slot[0]() is not w:          # identity, never tensor ==
        wid = id(w)
        slot = _PACKED[wid] = (weakref.ref(w, lambda _r, wid=wid: _PACKED.pop(wid, None)), {})
    per = slot[1]
    key = (g, dtype) + tuple(os.environ.get(k) for k in _PLAN_ENV)
    ent = per.get(key)
    st = w.untyped_storage()
    if ent is not None and ent[0].data_ptr() == st.data_ptr() and ent[1] == (w.data_ptr(), w._version, WEIGHT_EPOCH):
        return ent[2]
    wf = pack_conv_weight(w, True, False, g, dtype)[0]
    per[key] = (st, (w.data_ptr(), w._version, WEIGHT_EPOCH), wf)
    return wf


def conv3d_fwd(x: Tensor, wf: Tensor, bias: Optional[Tensor], g: ConvGeom, want_stats: bool):
    y, stats, _ = conv3d_fwd_keep(x, wf, bias, g, want_stats, False)
    return y, stats


def conv_prologue_ok(g: ConvGeom, dtype=torch.float32) -> bool:
    """Can the convolution apply the producing unit's BatchNorm + ReLU on the way in (conv3d_fwd_keep(prologue=...))?
    The fp32 Winograd pipeline with F(4,3)^3 tiles; DRAM_BN_PROLOGUE=0 under DRAM_TUNING=1 switches it off (A/B)."""
    return dtype == torch.float32 and tuning_env("DRAM_BN_PROLOGUE", "1") != "0" and conv_plan(g).prologue


def _launch_fwd(algo: _ConvAlgo, fn: str, lead: tuple, like: Tensor, wf: Tensor, bias: Optional[Tensor], g: ConvGeom,
                plan: ConvPlan, rows: int, want_stats: bool, keep: bool):
    """Allocation and launch of every forward form: `fn` is algo.fwd or one of the pipeline's forms with more input
    operands, `lead` the pointers ahead of wf, `like` an input (device and storage type of y).  -> (y, stats, V)"""
    y = torch.empty(g.out_shape, device=like.device, dtype=like.dtype)
    stats = None
    if want_stats:
        if rows <= 0:
            raise RuntimeError(f"dram_conv_num_mtiles rejected {g}")
        stats = torch.empty((rows, 2, g.Cout), device=like.device, dtype=torch.float32)
    v, tail = None, (plan.dref,)
    if algo.ws:
        ws = _workspace(plan.ws_fwd, like.device)
        if keep:
            v = torch.empty((plan.v_elems,), device=like.device, dtype=torch.float32)
        tail = (_p(v), plan.dref, _p(ws), plan.ws_fwd)
    with _span(algo.family, g.flops, f"fwd {g}"):
        _chk(getattr(_L(), fn)(*lead, _p(wf), _p(bias), _p(y), _p(stats), *tail, _stream()), f"{fn}{g}")
    return y, stats, v


def conv3d_fwd_keep(x: Tensor, wf: Tensor, bias: Optional[Tensor], g: ConvGeom, want_stats: bool, keep: bool,
                    prologue: Optional[Tuple[Tensor, Tensor]] = None):
    """Forward conv; with keep=True on the Winograd path also returns the transformed input V
    (reused by conv3d_bwd_weight instead of transforming x again), else None.
    prologue=(scale, shift): x is the PRE-BatchNorm output of the producing unit and max(x*scale + shift, 0) is applied
    inside the input transform (only where conv_prologue_ok(g))."""
    plan = conv_plan(g)
    if prologue is not None and not (x.dtype == torch.float32 and plan.prologue):
        raise RuntimeError(f"conv3d_fwd_keep: no BatchNorm prologue for {g}")
    if _act(x, "x", g.in_shape):                       # bf16 storage
        if bias is not None:
            _req(bias, "bias", shape=(g.Cout,))
        route, gk = bf16_route(g, plan, wf)
        if route == "s2d":                              # stride 2 as stride 1 over the space-to-depth tensor
            return conv3d_fwd_keep(s2d(x), wf, bias, gk, want_stats, False)
        if route == "casts":                            # fp32 kernels around casts (statistics of the fp32 result)
            y32, stats, _ = conv3d_fwd_keep(cast(x, torch.float32), wf, bias, g, want_stats, False)
            return cast(y32, BF16), stats, None
        _req(wf, "wf", BF16, (g.taps, g.Cout, g.Cin))
        return _launch_fwd(_CONV_ALGOS[BF16], _CONV_ALGOS[BF16].fwd, (_p(x),), x, wf, bias, g, plan, plan.bf16_stat_rows,
                           want_stats, False)
    _req(wf, "wf", shape=(plan.taps_f, g.Cout, g.Cin))
    if bias is not None:
        _req(bias, "bias", shape=(g.Cout,))
    if prologue is None:
        return _launch_fwd(plan.conv, plan.conv.fwd, (_p(x),), x, wf, bias, g, plan, plan.stat_rows, want_stats, keep)
    _req(prologue[0], "scale", shape=(g.Cin,))
    _req(prologue[1], "shift", shape=(g.Cin,))
    return _launch_fwd(plan.conv, "dram_wino_conv3d_fwd_bn", (_p(x), _p(prologue[0]), _p(prologue[1])), x, wf, bias, g, plan,
                       plan.stat_rows, want_stats, keep)


def _launch_bwd_data(algo: _ConvAlgo, fn: str, dy: Tensor, wb: Tensor, operands: tuple, g: ConvGeom, plan: ConvPlan,
                     overlapped: bool, detail: str, rows: int = 0):
    """Allocation and launch of every data-gradient form: `fn` is algo.bwd or the pipeline's form that also takes the
    BatchNorm-backward statistics (`rows` of them), `operands` the pointers behind dx.  -> (dx, partial)"""
    dx = torch.empty(g.in_shape, device=dy.device, dtype=dy.dtype)
    partial = torch.empty((rows, 2, g.Cin), device=dy.device, dtype=torch.float32) if rows else None
    if partial is not None:
        operands += (_p(partial),)
    tail = (plan.dref,)
    if algo.ws:                                         # (the overlapped hint is the pipeline's alone)
        ws = _workspace(plan.ws_bwd, dy.device)
        tail = (plan.dref_ovl if overlapped else plan.dref, _p(ws), plan.ws_bwd)
    with _span(algo.family, g.flops, detail):
        _chk(getattr(_L(), fn)(_p(dy), _p(wb), _p(dx), *operands, *tail, _stream()), f"{fn}{g}")
    return dx, partial


def conv3d_bwd_data(dy: Tensor, wb: Tensor, g: ConvGeom, add: Optional[Tensor] = None,
                    gate: Optional[Tensor] = None, overlapped: bool = False) -> Tensor:
    """overlapped: weight-gradient kernels run on another stream meanwhile (DRAM_CONV_BWD_OVERLAPPED: a hint for the
    Winograd pipeline's choice of GEMM form; results do not depend on it)."""
    plan = conv_plan(g)
    if _act(dy, "dy", g.out_shape):                    # bf16 storage
        if add is not None:
            _act(add, "add", g.in_shape, like=dy)
        if gate is not None:
            _act(gate, "gate", g.in_shape, like=dy)
        route, gk = bf16_route(g, plan, wb, 1)
        if route == "s2d":                              # stride 2: gradient of the space-to-depth tensor, then back
            dx8 = conv3d_bwd_data(dy, wb, gk)
            dx = torch.empty(g.in_shape, device=dy.device, dtype=BF16)
            _chk(_L().dram_d2s_bf16(_p(dx8), _p(add), _p(gate), _p(dx), g.B, g.D, g.H, g.W, g.Cin, _stream()),
                 "dram_d2s_bf16")
            return dx
        if route == "casts":
            f32 = torch.float32
            return cast(conv3d_bwd_data(cast(dy, f32), wb, g, None if add is None else cast(add, f32),
                                        None if gate is None else cast(gate, f32)), BF16)
        algo = _CONV_ALGOS[BF16]
        _req(wb, "wb", BF16, (g.taps, g.Cin, g.Cout))
    else:
        algo = plan.conv
        _req(wb, "wb", shape=(plan.taps_b, g.Cin, g.Cout))
        if add is not None:
            _req(add, "add", shape=g.in_shape)
        if gate is not None:
            _req(gate, "gate", shape=g.in_shape)
    return _launch_bwd_data(algo, algo.bwd, dy, wb, (_p(add), _p(gate)), g, plan, overlapped, f"dgrad {g}")[0]


def conv_bwd_bnstats_ok(g: ConvGeom, dtype=torch.float32) -> bool:
    """Can the data gradient of this convolution also take the BatchNorm-backward statistics of the unit in front of it
    (conv3d_bwd_data_bnstats)?  The fp32 Winograd pipeline; DRAM_BWD_BNSTATS=0 under DRAM_TUNING=1 switches it off (A/B)."""
    return (dtype == torch.float32 and tuning_env("DRAM_BWD_BNSTATS", "1") != "0" and conv_plan(g).algo == 1
            and g.Cin % 64 == 0)


def conv3d_bwd_data_bnstats(dy: Tensor, wb: Tensor, g: ConvGeom, bn_y: Tensor, mean: Tensor, invstd: Tensor,
                            scale: Tensor, shift: Tensor, overlapped: bool = False):
    """-> (dx, partial): the data gradient (bit-identical to conv3d_bwd_data) and, from its output transform, the rows
    bn_bwd_reduce(dx, None, bn_y, mean, invstd, True, scale, shift) would produce in a pass of its own -- dx is dz of the
    BatchNorm + ReLU unit in front of this convolution (reference med3d.py:121-124 backward), bn_y that unit's
    pre-BatchNorm output."""
    plan = conv_plan(g)
    if not conv_bwd_bnstats_ok(g, dy.dtype):
        raise RuntimeError(f"conv3d_bwd_data_bnstats: not available for {g}")
    _req(dy, "dy", shape=g.out_shape)
    _req(wb, "wb", shape=(plan.taps_b, g.Cin, g.Cout))
    _req(bn_y, "bn_y", shape=g.in_shape)
    for name, t in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift)):
        _req(t, name, shape=(g.Cin,))
    if plan.stat_rows_bwd <= 0:
        raise RuntimeError(f"conv3d_bwd_data_bnstats: no statistic rows for {g}")
    return _launch_bwd_data(plan.conv, "dram_wino_conv3d_bwd_data_bn", dy, wb,
                            (_p(bn_y), _p(mean), _p(invstd), _p(scale), _p(shift)), g, plan, overlapped, f"dgrad+bnstats {g}",
                            rows=plan.stat_rows_bwd)


def conv3d_bwd_weight(x: Tensor, dy: Tensor, g: ConvGeom, out: Optional[Tensor] = None,
                      v_cache: Optional[Tensor] = None) -> Tensor:
    plan = conv_plan(g)
    shape = (g.Cout, g.Cin, g.k, g.k, g.k)
    dw = out if out is not None else torch.empty(shape, device=dy.device, dtype=torch.float32)
    _req(dw, "dw", shape=shape)
    if x is not None and _act(x, "x", g.in_shape):     # bf16 storage: the gradient itself is fp32
        _act(dy, "dy", g.out_shape, like=x)
        route, gk = bf16_route(g, plan)
        if route == "s2d":                              # stride 2: gradient of the embedded weights, 27 of 216 slots kept
            dw3 = conv3d_bwd_weight(s2d(x), dy, gk)
            _chk(_L().dram_s2_extract_wgrad(_p(dw3), _p(dw), g.Cout, g.Cin, _stream()), "dram_s2_extract_wgrad")
            return dw
        if route == "casts":
            return conv3d_bwd_weight(cast(x, torch.float32), cast(dy, torch.float32), g, out=dw)
        algo, nbytes = _WGRAD_ALGOS[BF16], plan.bf16_ws_wgrad
    else:
        if x is None:                                   # the forward's transformed input stands in for x (pipeline only)
            if not (plan.wgrad_from_v and v_cache is not None):
                raise RuntimeError(f"conv3d_bwd_weight: x missing and no cached Winograd-domain input for {g}")
        else:
            _req(x, "x", shape=g.in_shape)
        _req(dy, "dy", shape=g.out_shape)
        algo, nbytes = plan.wgrad, plan.ws_wgrad
        if nbytes == 0 and algo is _WGRAD_ALGOS[0]:
            raise RuntimeError(f"{algo.fn}: unsupported geometry {g}")
    ws = _workspace(max(nbytes, algo.min_ws), dy.device)
    lead = (_p(x),)
    if algo.v_cache:
        if v_cache is not None:
            _req(v_cache, "v_cache", shape=(plan.v_elems,))
        lead = (_p(x), _p(v_cache))
    with _span(algo.family, g.flops, f"wgrad {g}"):
        _chk(getattr(_L(), algo.fn)(*lead, _p(dy), _p(dw), plan.dref, _p(ws), nbytes, _stream()), f"{algo.fn}{g}")
    return dw


# --------------------------------------------------------------------------- stem
def stem_out(n: int) -> int:
    return (n + 6 - 7) // 2 + 1


def stem_fwd(x: Tensor, w: Tensor, want_stats: bool, out_dtype=torch.float32):
    """x [B,D,H,W] (C=1), w [64,1,7,7,7] -> y [B,Do,Ho,Wo,64] (fp32 arithmetic; y stored as out_dtype)."""
    _req(x, "x")
    if x.dim() != 4:
        raise ValueError("stem_fwd: x must be [B,D,H,W]")
    _req(w, "w", shape=(64, 1, 7, 7, 7))
    B, D, H, W = x.shape
    Do, Ho, Wo = stem_out(D), stem_out(H), stem_out(W)
    if out_dtype not in (torch.float32, BF16):
        raise TypeError(f"stem_fwd: unsupported storage type {out_dtype}")
    y = torch.empty((B, Do, Ho, Wo, 64), device=x.device, dtype=out_dtype)
    stats = None
    if want_stats:
        nt = _L().dram_stem_num_tiles(B, Do, Ho, Wo)
        stats = torch.empty((nt, 2, 64), device=x.device, dtype=torch.float32)
    with _span("stem_fwd_kernel", 2.0 * B * Do * Ho * Wo * 64 * 343):
        sfx = "" if out_dtype != BF16 else ("_bf16mm" if tuning_env("DRAM_STEM_BF16", "1") != "0" else "_bf16")
        _chk(_fn("dram_stem_fwd", sfx)(_p(x), _p(w), _p(y), _p(stats), B, D, H, W, _stream()), "dram_stem_fwd" + sfx)
    return y, stats


def stem_bwd_weight(x: Tensor, dy: Tensor, out: Optional[Tensor] = None) -> Tensor:
    _req(x, "x")
    B, D, H, W = x.shape
    sfx = _act(dy, "dy", (B, stem_out(D), stem_out(H), stem_out(W), 64))
    nbytes = _L().dram_stem_bwd_weight_workspace(B, D, H, W)
    ws = torch.empty(((nbytes + 3) // 4,), device=x.device, dtype=torch.float32)
    dw = out if out is not None else torch.empty((64, 1, 7, 7, 7), device=x.device, dtype=torch.float32)
    _req(dw, "dw", shape=(64, 1, 7, 7, 7))
    with _span("stem_wgrad_kernel+reduce", 2.0 * dy.numel() * 343):
        if sfx and tuning_env("DRAM_STEM_BF16", "1") != "0":
            sfx = "_bf16mm"                          # bf16 matrix cores (the "_bf16" form: fp32 MFMA on the up-cast dy)
        _chk(_fn("dram_stem_bwd_weight", sfx)(_p(x), _p(dy), _p(dw), B, D, H, W, _p(ws), nbytes, _stream()),
             "dram_stem_bwd_weight" + sfx)
    return dw


def stem_bwd_data(dy: Tensor, w: Tensor, in_shape) -> Tensor:
    """Data gradient of the stem convolution: dy [B,Do,Ho,Wo,64] (float32 or bfloat16), w [64,1,7,7,7] -> dx [B,D,H,W]
    float32 for in_shape = (B, D, H, W).  fp32 arithmetic, deterministic (two launches: scatter GEMM + ordered fold)."""
    B, D, H, W = (int(v) for v in in_shape)
    if min(B, D, H, W) < 1:
        raise ValueError(f"stem_bwd_data: bad input shape {tuple(in_shape)}")
    sfx = _act(dy, "dy", (B, stem_out(D), stem_out(H), stem_out(W), 64))
    _req(w, "w", shape=(64, 1, 7, 7, 7))
    nbytes = _L().dram_stem_bwd_data_workspace(B, D, H, W)
    ws = torch.empty(((nbytes + 3) // 4,), device=dy.device, dtype=torch.float32)
    dx = torch.empty((B, D, H, W), device=dy.device, dtype=torch.float32)
    with _span("stem_dgrad_kernel+fold", 2.0 * dy.numel() * 343):
        _chk(_fn("dram_stem_bwd_data", sfx)(_p(dy), _p(w), _p(dx), B, D, H, W, _p(ws), nbytes, _stream()),
             "dram_stem_bwd_data" + sfx)
    return dx


# --------------------------------------------------------------------------- batch norm
FOLD_TICKET_DOUBLES = _lib.DRAM_FOLD_TICKET_DOUBLES     # per-call ticket words behind the stage rows


def reduce_partials(partial: Tensor, tail: Optional[float] = None, want_f32: bool = False):
    """[P,R,C] float32 -> [R,C] float64, ONE launch (dram_fold_partials).  With `tail` (SyncBN: the rank's element
    count) returns (flat [R*C+1] float64 whose last element is tail -- the buffer to all-reduce --, its [R,C] view);
    with want_f32 additionally a list of R float32 [C] tensors (the rows, separately allocated) written by the same
    kernel (appended to the result)."""
    _req(partial, "partial")
    Pn, R, C = partial.shape
    stages = _L().dram_fold_partials_stages(Pn)
    n = R * C + (1 if tail is not None else 0)
    buf = torch.empty((n + stages * R * C + (FOLD_TICKET_DOUBLES if stages > 1 else 0),), device=partial.device,
                      dtype=torch.float64)
    flat = buf[:n]
    # float copy: one tensor PER ROW (whole tensors, which autograd takes over as .grad without a copy; row views of
    # one [R, C] tensor are cloned by AccumulateGrad -- 108 copies per ResNet-50 step)
    f32 = [torch.empty((C,), device=partial.device, dtype=torch.float32) for _ in range(R)] if want_f32 else None
    if want_f32 and R > 2:
        raise ValueError("reduce_partials: the float copy supports at most two rows")
    _chk(_L().dram_fold_partials(_p(partial), _p(flat), _p(buf[n:]), _p(f32[0]) if f32 else None,
                                 _p(f32[1]) if (f32 and R == 2) else None, Pn, R, C,
                                 float(tail) if tail is not None else 0.0, int(tail is not None), _stream()),
         "dram_fold_partials")
    res = (flat, flat[:R * C].view(R, C)) if tail is not None else (flat.view(R, C),)
    if want_f32:
        res = res + (f32,)
    return res if len(res) > 1 else res[0]


def bn_fold_finalize(partial: Tensor, count: float, gamma: Tensor, beta: Tensor, running_mean: Tensor,
                     running_var: Tensor, momentum: float, eps: float):
    """Training-mode statistics of a single-process step in ONE launch: fold of the convolution epilogue's
    [P,2,C] partial sums + bn_finalize (running-statistic update included) -> (mean, invstd, scale, shift)."""
    _req(partial, "partial")
    Pn, R, C = partial.shape
    if R != 2:
        raise ValueError("bn_fold_finalize: expected [P,2,C] partial sums")
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _req(t, nm, shape=(C,))
    stages = _L().dram_fold_partials_stages(Pn)
    buf = torch.empty(((1 + stages) * 2 * C + (FOLD_TICKET_DOUBLES if stages > 1 else 0),), device=partial.device,
                      dtype=torch.float64)
    out = torch.empty((4, C), device=partial.device, dtype=torch.float32)
    _chk(_L().dram_bn_fold_finalize(_p(partial), _p(buf), _p(buf[2 * C:]), Pn, C, float(count), _p(gamma), _p(beta),
                                    _p(running_mean), _p(running_var), float(momentum), float(eps), 1, _p(out[0]),
                                    _p(out[1]), _p(out[2]), _p(out[3]), _stream()), "dram_bn_fold_finalize")
    return out[0], out[1], out[2], out[3]


def bn_finalize(sums: Optional[Tensor], count: float, gamma: Tensor, beta: Tensor, running_mean: Tensor,
                running_var: Tensor, momentum: float, eps: float, update_running: bool,
                count_dev: Optional[Tensor] = None):
    """count_dev: optional 1-element float64 device tensor (the all-reduced global count) read by the
    kernel instead of `count`."""
    C = gamma.numel()
    if count_dev is not None:
        _req(count_dev, "count_dev", dtype=torch.float64, shape=(1,))
    _req(gamma, "gamma", shape=(C,))
    _req(beta, "beta", shape=(C,))
    _req(running_mean, "running_mean", shape=(C,))
    _req(running_var, "running_var", shape=(C,))
    if sums is not None:
        _req(sums, "sums", dtype=torch.float64, shape=(2, C))
    out = torch.empty((4, C), device=gamma.device, dtype=torch.float32)
    mean, invstd, scale, shift = out[0], out[1], out[2], out[3]
    _chk(_L().dram_bn_finalize(_p(sums), float(count), _p(count_dev), _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                               float(momentum), float(eps), int(update_running), _p(mean), _p(invstd), _p(scale),
                               _p(shift), C, _stream()), "dram_bn_finalize")
    return mean, invstd, scale, shift


def bn_apply(y: Tensor, scale: Tensor, shift: Tensor, residual: Optional[Tensor], rs: int, relu: bool) -> Tensor:
    sfx = _act(y, "y")
    B, D, H, W, C = y.shape
    _req(scale, "scale", shape=(C,))
    _req(shift, "shift", shape=(C,))
    Dr = Hr = Wr = Cr = 0
    if residual is not None:
        _act(residual, "residual", like=y)
        if residual.shape[0] != B:
            raise ValueError("bn_apply: residual batch mismatch")
        _, Dr, Hr, Wr, Cr = residual.shape
        if Cr > C or (D - 1) * rs >= Dr or (H - 1) * rs >= Hr or (W - 1) * rs >= Wr:
            raise ValueError(f"bn_apply: residual {tuple(residual.shape)} incompatible with {tuple(y.shape)} rs={rs}")
        # F.avg_pool3d(kernel_size=1, stride=rs) output size must equal ours
        if ((Dr - 1) // rs + 1, (Hr - 1) // rs + 1, (Wr - 1) // rs + 1) != (D, H, W):
            raise ValueError("bn_apply: strided residual does not match the output grid")
    z = torch.empty_like(y)
    _chk(_fn("dram_bn_apply", sfx)(_p(y), _p(scale), _p(shift), _p(residual), Dr, Hr, Wr, Cr, rs, _p(z), B, D, H, W, C,
                                   int(relu), _stream()), "dram_bn_apply")
    return z


def _rows(t: Tensor) -> int:
    return t.numel() // t.shape[-1]


def _mask_args(z, y, scale, shift, relu):
    """ReLU mask source of the BN backward kernels: the saved output z, or (z None) scale / shift to
    re-derive it from y."""
    C = y.shape[-1]
    if relu and z is not None:
        _act(z, "z", y.shape, like=y)
    elif relu:
        if scale is None or shift is None:
            raise ValueError("BN backward with ReLU needs z, or scale and shift")
        _req(scale, "scale", shape=(C,))
        _req(shift, "shift", shape=(C,))


def bn_bwd_reduce(dz: Tensor, z: Optional[Tensor], y: Tensor, mean: Tensor, invstd: Tensor, relu: bool,
                  scale: Optional[Tensor] = None, shift: Optional[Tensor] = None) -> Tensor:
    sfx = _act(y, "y")
    _act(dz, "dz", y.shape, like=y)
    _mask_args(z, y, scale, shift, relu)
    C = y.shape[-1]
    _req(mean, "mean", shape=(C,))
    _req(invstd, "invstd", shape=(C,))
    rows = _rows(y)
    nparts = _L().dram_colsum_nparts(rows, C)
    partial = torch.empty((nparts, 2, C), device=y.device, dtype=torch.float32)
    _chk(_fn("dram_bn_bwd_reduce", sfx)(_p(dz), _p(z), _p(y), _p(mean), _p(invstd), _p(scale), _p(shift), _p(partial), rows, C,
                                        int(relu), _stream()), "dram_bn_bwd_reduce")
    return partial


def bn_bwd_apply(dz: Tensor, z: Optional[Tensor], y: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, sums: Tensor,
                 count: float, relu: bool, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
                 want_colsum: bool = False, count_dev: Optional[Tensor] = None):
    """-> dy, or (dy, partial [P,1,C] column sums of dy) with want_colsum (None when C is unsupported there)."""
    C = y.shape[-1]
    if count_dev is not None:
        _req(count_dev, "count_dev", dtype=torch.float64, shape=(1,))
    sfx = _act(y, "y")
    _act(dz, "dz", y.shape, like=y)
    _mask_args(z, y, scale, shift, relu)
    colpart = None
    if want_colsum:
        npart = _L().dram_bn_bwd_apply_nparts(_rows(y), C)
        if npart >= 1:
            colpart = torch.empty((npart, 1, C), device=y.device, dtype=torch.float32)
    _req(sums, "sums", dtype=torch.float64, shape=(2, C))
    _req(gamma, "gamma", shape=(C,))
    dy = torch.empty_like(y)
    _chk(_fn("dram_bn_bwd_apply", sfx)(_p(dz), _p(z), _p(y), _p(mean), _p(invstd), _p(gamma), _p(scale), _p(shift), _p(sums),
                                       float(count), _p(count_dev), _p(dy), _p(colpart), _rows(y), C, int(relu), _stream()),
         "dram_bn_bwd_apply")
    return (dy, colpart) if want_colsum else dy


def bn_bwd_apply_eval(dz: Tensor, z: Optional[Tensor], y: Optional[Tensor], scale: Tensor, shift: Optional[Tensor],
                      relu: bool, want_colsum: bool = False):
    """Backward of a BatchNorm that ran on its running statistics: dy = scale * dz * mask, the mask from z (y is not
    read and may be None) or, z None, re-derived from y with the forward's scale / shift.
    -> dy, or (dy, partial [P,1,C] column sums of dy) with want_colsum (None when C is unsupported there)."""
    sfx = _act(dz, "dz")
    C = dz.shape[-1]
    _req(scale, "scale", shape=(C,))
    if relu and z is not None:
        _act(z, "z", dz.shape, like=dz)
        y = None
    elif relu:
        if y is None or shift is None:
            raise ValueError("BN backward with ReLU needs z, or y with scale and shift")
        _act(y, "y", dz.shape, like=dz)
        _req(shift, "shift", shape=(C,))
    colpart = None
    if want_colsum:
        npart = _L().dram_bn_bwd_apply_nparts(_rows(dz), C)
        if npart >= 1:
            colpart = torch.empty((npart, 1, C), device=dz.device, dtype=torch.float32)
    dy = torch.empty_like(dz)
    _chk(_fn("dram_bn_bwd_apply_eval", sfx)(_p(dz), _p(z) if relu else None, _p(y) if relu else None, _p(scale),
                                            _p(shift) if relu else None, _p(dy), _p(colpart), _rows(dz), C, int(relu),
                                            _stream()), "dram_bn_bwd_apply_eval")
    return (dy, colpart) if want_colsum else dy


def colsum(a: Tensor) -> Tensor:
    """[..., C] -> partial [P,1,C]."""
    sfx = _act(a, "a")
    C = a.shape[-1]
    rows = _rows(a)
    nparts = _L().dram_colsum_nparts(rows, C)
    partial = torch.empty((nparts, 1, C), device=a.device, dtype=torch.float32)
    _chk(_fn("dram_colsum", sfx)(_p(a), _p(partial), rows, C, _stream()), "dram_colsum")
    return partial


def add(a: Tensor, b: Tensor) -> Tensor:
    _req(a, "a")
    _req(b, "b", shape=a.shape)
    out = torch.empty_like(a)
    _chk(_L().dram_add(_p(a), _p(b), _p(out), a.numel(), _stream()), "dram_add")
    return out


# --------------------------------------------------------------------------- pool / up-projection
def pool_out(n: int) -> int:
    return (n + 2 - 3) // 2 + 1


def maxpool_fwd(x: Tensor):
    sfx = _act(x, "x")
    B, D, H, W, C = x.shape
    shape = (B, pool_out(D), pool_out(H), pool_out(W), C)
    y = torch.empty(shape, device=x.device, dtype=x.dtype)
    am = torch.empty(shape, device=x.device, dtype=torch.uint8)
    _chk(_fn("dram_maxpool_fwd", sfx)(_p(x), _p(y), _p(am), B, D, H, W, C, _stream()), "dram_maxpool_fwd")
    return y, am


def bn_maxpool_fwd(y: Tensor, scale: Tensor, shift: Tensor):
    """Stem (med3d.py:272-275): z = relu(y*scale + shift), max-pool 3/2/1 of z and its taps in ONE pass over y --
    bit-identical to bn_apply(...) + maxpool_fwd(...).  -> (z, pooled, argmax)."""
    sfx = _act(y, "y")
    B, D, H, W, C = y.shape
    _req(scale, "scale", shape=(C,))
    _req(shift, "shift", shape=(C,))
    shape = (B, pool_out(D), pool_out(H), pool_out(W), C)
    z = torch.empty_like(y)
    pooled = torch.empty(shape, device=y.device, dtype=y.dtype)
    am = torch.empty(shape, device=y.device, dtype=torch.uint8)
    _chk(_fn("dram_bn_maxpool_fwd", sfx)(_p(y), _p(scale), _p(shift), _p(z), _p(pooled), _p(am), B, D, H, W, C, _stream()),
         "dram_bn_maxpool_fwd")
    return z, pooled, am


def maxpool_bwd(dy: Tensor, argmax: Tensor, in_shape, add_: Optional[Tensor] = None) -> Tensor:
    B, D, H, W, C = in_shape
    oshape = (B, pool_out(D), pool_out(H), pool_out(W), C)
    sfx = _act(dy, "dy", oshape)
    _req(argmax, "argmax", dtype=torch.uint8, shape=oshape)
    add_stride = C
    if add_ is not None:
        # a dense tensor shaped like dx, or a channel slice [..., c0:c0+C] of a dense wider tensor (read in place)
        if (not add_.is_cuda or add_.dtype != dy.dtype or tuple(add_.shape) != tuple(in_shape)
                or add_.stride(-1) != 1):
            raise ValueError("maxpool_bwd: add must be a device tensor of dy's type shaped like the pooled input")
        add_stride = add_.stride(3)
        want = (D * H * W * add_stride, H * W * add_stride, W * add_stride, add_stride, 1)
        if tuple(add_.stride()) != want or add_stride % 4 or add_.data_ptr() % (4 * add_.element_size()):
            raise ValueError("maxpool_bwd: add must be dense or an aligned channel slice of a dense tensor")
    dx = torch.empty(in_shape, device=dy.device, dtype=dy.dtype)
    _chk(_fn("dram_maxpool_bwd", sfx)(_p(dy), _p(argmax), _p(add_), add_stride, _p(dx),
                                      B, D, H, W, C, _stream()), "dram_maxpool_bwd")
    return dx


def upcat_fwd(src: Tensor, skip: Tensor) -> Tensor:
    sfx = _act(src, "src")
    _act(skip, "skip", like=src)
    B, Ds, Hs, Ws, Cu = src.shape
    Bk, Dk, Hk, Wk, Ck = skip.shape
    if Bk != B or Dk < 2 * Ds or Hk < 2 * Hs or Wk < 2 * Ws:
        raise ValueError(f"upcat_fwd: skip {tuple(skip.shape)} smaller than upsampled {tuple(src.shape)}")
    cat = torch.empty((B, 2 * Ds, 2 * Hs, 2 * Ws, Cu + Ck), device=src.device, dtype=src.dtype)
    _chk(_fn("dram_upcat_fwd", sfx)(_p(src), _p(skip), _p(cat), B, Ds, Hs, Ws, Cu, Dk, Hk, Wk, Ck, _stream()),
         "dram_upcat_fwd")
    return cat


def up_fwd(src: Tensor) -> Tensor:
    """x2 trilinear up-sampling (align_corners) alone: the first Cu channels of upcat_fwd(src, skip), bit for bit,
    without the concatenation (the convolution behind it reads the skip tensor as its second source: conv3d_fwd_cat)."""
    sfx = _act(src, "src")
    B, Ds, Hs, Ws, Cu = src.shape
    up = torch.empty((B, 2 * Ds, 2 * Hs, 2 * Ws, Cu), device=src.device, dtype=src.dtype)
    _chk(_fn("dram_upcat_fwd", sfx)(_p(src), None, _p(up), B, Ds, Hs, Ws, Cu, 2 * Ds, 2 * Hs, 2 * Ws, 0, _stream()),
         "dram_upcat_fwd (up only)")
    return up


def conv_cat_ok(g: "ConvGeom", C0: int, dtype=torch.float32) -> bool:
    """Can the convolution take its input as two channel blocks [C0 | g.Cin - C0] (conv3d_fwd_cat)?  The fp32 Winograd
    pipeline with F(4,3)^3 tiles, both blocks multiples of 64; DRAM_CONV_CAT=0 under DRAM_TUNING=1 switches it off (A/B)."""
    return (dtype == torch.float32 and tuning_env("DRAM_CONV_CAT", "1") != "0" and conv_plan(g).prologue
            and C0 >= 64 and C0 % 64 == 0 and (g.Cin - C0) >= 64 and (g.Cin - C0) % 64 == 0)


def conv3d_fwd_cat(x0: Tensor, x1: Tensor, wf: Tensor, bias: Optional[Tensor], g: "ConvGeom", want_stats: bool, keep: bool):
    """Forward convolution of concat([x0, x1], channels) WITHOUT the concatenated tensor (reference med3d.py:87 feeding
    :67): each source's input transform fills its channel range of the Winograd-domain image.  Returns (y, stats, V) like
    conv3d_fwd_keep; bit-identical to it on the concatenation."""
    plan = conv_plan(g)
    C0, C1 = x0.shape[-1], x1.shape[-1]
    if not conv_cat_ok(g, C0, x0.dtype) or C0 + C1 != g.Cin:
        raise RuntimeError(f"conv3d_fwd_cat: not available for {g} with blocks {C0} | {C1}")
    _req(x0, "x0", shape=g.in_shape[:4] + (C0,))
    _req(x1, "x1", shape=g.in_shape[:4] + (C1,))
    _req(wf, "wf", shape=(plan.taps_f, g.Cout, g.Cin))
    if bias is not None:
        _req(bias, "bias", shape=(g.Cout,))
    return _launch_fwd(plan.conv, "dram_wino_conv3d_fwd_cat", (_p(x0), C0, _p(x1), C1), x0, wf, bias, g, plan, plan.stat_rows,
                       want_stats, keep)


def upcat_bwd(dcat: Tensor, src_shape, skip_shape, need_src=True, need_skip=True):
    B, Ds, Hs, Ws, Cu = src_shape
    _, Dk, Hk, Wk, Ck = skip_shape
    sfx = _act(dcat, "dcat", (B, 2 * Ds, 2 * Hs, 2 * Ws, Cu + Ck))
    dsrc = torch.empty(src_shape, device=dcat.device, dtype=dcat.dtype) if need_src else None
    dskip = torch.empty(skip_shape, device=dcat.device, dtype=dcat.dtype) if need_skip else None
    _chk(_fn("dram_upcat_bwd", sfx)(_p(dcat), _p(dsrc), _p(dskip), B, Ds, Hs, Ws, Cu, Dk, Hk, Wk, Ck, _stream()),
         "dram_upcat_bwd")
    return dsrc, dskip


# --------------------------------------------------------------------------- us1.0 without the up-sampled tensor
def upmix_mode() -> int:
    """0 = never, 1 = where it pays (default), 2 = wherever the geometry allows (tests): DRAM_UPMIX under DRAM_TUNING=1."""
    return int(tuning_env("DRAM_UPMIX", "1"))


def upmix_split_weight(w: Tensor, Cu: int) -> Tuple[Tensor, Tensor]:
    """w [Co, Cu+Cs, 3,3,3] -> (wlo [27*Co, Cu, 1,1,1]: the low-resolution mixing GEMM's weight, row t*Co + co;
    ws [Co, Cs, 3,3,3]: the skip channels' convolution weight).  csrc/upmix.hip."""
    _req(w, "w")
    Co, Ct = w.shape[0], w.shape[1]
    Cs = Ct - Cu
    if tuple(w.shape[2:]) != (3, 3, 3) or Cu < 1 or Cs < 1:
        raise ValueError(f"upmix_split_weight: weight {tuple(w.shape)}, Cu={Cu}")
    wlo = torch.empty((27 * Co, Cu, 1, 1, 1), device=w.device, dtype=torch.float32)
    ws = torch.empty((Co, Cs, 3, 3, 3), device=w.device, dtype=torch.float32)
    _chk(_L().dram_upmix_split_weight(_p(w), _p(wlo), _p(ws), Co, Cu, Cs, _stream()), "dram_upmix_split_weight")
    return wlo, ws


def upmix_merge_wgrad(dwlo: Tensor, dws: Tensor, out: Optional[Tensor] = None) -> Tensor:
    Co, Cs = dws.shape[0], dws.shape[1]
    Cu = dwlo.shape[1]
    _req(dwlo, "dwlo", shape=(27 * Co, Cu, 1, 1, 1))
    _req(dws, "dws", shape=(Co, Cs, 3, 3, 3))
    dw = out if out is not None else torch.empty((Co, Cu + Cs, 3, 3, 3), device=dws.device, dtype=torch.float32)
    _req(dw, "dw", shape=(Co, Cu + Cs, 3, 3, 3))
    _chk(_L().dram_upmix_merge_wgrad(_p(dwlo), _p(dws), _p(dw), Co, Cu, Cs, _stream()), "dram_upmix_merge_wgrad")
    return dw


def upmix_gather_fwd(b: Tensor, base: Optional[Tensor], Co: int, want_stats: bool, out_dtype=None):
    """b [B,Ds,Hs,Ws,27*Co] (tap-major: column t*Co + co) -> y [B,2Ds,2Hs,2Ws,Co] = sum over the 27 taps of the
    trilinearly up-sampled tap images, shifted by the tap (zero outside the volume), + base (written IN PLACE into
    base when given).  Three separable passes; intermediates fp32.  Returns (y, BatchNorm partial sums or None)."""
    bf = _act(b, "b") != ""
    B, Ds, Hs, Ws, N = b.shape
    if N != 27 * Co:
        raise ValueError(f"upmix_gather_fwd: {N} columns for Co={Co}")
    dev = b.device
    if base is not None:
        _act(base, "base", (B, 2 * Ds, 2 * Hs, 2 * Ws, Co))
        y = base
    else:
        y = torch.empty((B, 2 * Ds, 2 * Hs, 2 * Ws, Co), device=dev, dtype=out_dtype or b.dtype)
    L = _L()
    with _span("upmix_gather", 0.0, f"fwd {tuple(b.shape)}"):
        q1 = torch.empty((B, Ds, Hs, 2 * Ws, 9, Co), device=dev, dtype=torch.float32)
        _chk(L.dram_upmix_axis_fwd(_p(b), int(bf), _p(q1), B * Ds * Hs, Ws, 9, Co, _stream()), "dram_upmix_axis_fwd[x]")
        q2 = torch.empty((B, Ds, 2 * Hs, 2 * Ws, 3, Co), device=dev, dtype=torch.float32)
        _chk(L.dram_upmix_axis_fwd(_p(q1), 0, _p(q2), B * Ds, Hs, 2 * Ws * 3, Co, _stream()), "dram_upmix_axis_fwd[y]")
        del q1
        nvox = B * 8 * Ds * Hs * Ws
        stats = torch.empty((L.dram_upmix_stat_rows(nvox), 2, Co), device=dev, dtype=torch.float32) if want_stats else None
        _chk(L.dram_upmix_axis_fwd_final(_p(q2), _p(base), _p(y), int(y.dtype == BF16), _p(stats), B, Ds, 4 * Hs * Ws, Co,
                                         _stream()), "dram_upmix_axis_fwd_final")
    return y, stats


def upmix_gather_bwd(dy: Tensor, out_dtype=None) -> Tensor:
    """Transpose of upmix_gather_fwd: dy [B,2Ds,2Hs,2Ws,Co] -> h [B,Ds,Hs,Ws,27*Co] (storage type of dy unless given)."""
    gbf = _act(dy, "dy") != ""
    B, Do, Ho, Wo, Co = dy.shape
    if (Do | Ho | Wo) & 1:
        raise ValueError(f"upmix_gather_bwd: odd extents {tuple(dy.shape)}")
    Ds, Hs, Ws = Do // 2, Ho // 2, Wo // 2
    dev = dy.device
    odt = out_dtype or dy.dtype
    L = _L()
    with _span("upmix_gather", 0.0, f"bwd {tuple(dy.shape)}"):
        g2 = torch.empty((B, Ds, Ho, Wo, 3, Co), device=dev, dtype=torch.float32)
        _chk(L.dram_upmix_axis_bwd(_p(dy), int(gbf), _p(g2), 0, B, Ds, Ho * Wo, Co, _stream()), "dram_upmix_axis_bwd[z]")
        g1 = torch.empty((B, Ds, Hs, Wo, 9, Co), device=dev, dtype=torch.float32)
        _chk(L.dram_upmix_axis_bwd(_p(g2), 0, _p(g1), 0, B * Ds, Hs, Wo * 3, Co, _stream()), "dram_upmix_axis_bwd[y]")
        del g2
        h = torch.empty((B, Ds, Hs, Ws, 27 * Co), device=dev, dtype=odt)
        _chk(L.dram_upmix_axis_bwd(_p(g1), 0, _p(h), int(odt == BF16), B * Ds * Hs, Ws, 9, Co, _stream()),
             "dram_upmix_axis_bwd[x]")
    return h


def upproject(dense: Tensor, ess: Tensor, size):
    """dense [B,D,H,W] -> out [B,Do,Ho,Wo] = trilinear(align_corners)(dense)*ess, partial [B,nblk]."""
    _req(dense, "dense")
    B, D, H, W = dense.shape
    Do, Ho, Wo = size
    _req(ess, "ess", shape=(B, Do, Ho, Wo))
    nblk = _L().dram_upproject_nblk(Do * Ho * Wo)
    out = torch.empty((B, Do, Ho, Wo), device=dense.device, dtype=torch.float32)
    partial = torch.empty((B, nblk), device=dense.device, dtype=torch.float32)
    _chk(_L().dram_upproject(_p(dense), _p(ess), _p(out), _p(partial), B, D, H, W, Do, Ho, Wo, _stream()),
         "dram_upproject")
    return out, partial


def upproject_regions(cle: Tensor, pse: Tensor, ess_u8: Tensor, labels_u8: Tensor, size, n_regions: int = 5,
                      want_volumes: bool = True):
    """Both heads' ``upproject`` and the per-region table in one pass (csrc/regions.hip).

    cle, pse [B,D,H,W] float32: each sample contiguous, ONE batch stride for both (two channel views of the engine's one
    dense tensor work without a copy); ess_u8, labels_u8 [B,Do,Ho,Wo] uint8 (bool is viewed as bytes), ess non-zero =
    1.0.  -> (up_cle, up_pse, table): the volumes [B,Do,Ho,Wo], bit for bit ``upproject(head, ess.float(), size)[0]``
    (None, None when ``want_volumes`` is off), and table [B, n_regions + 1, 4] float64, row r = (sum up_cle, sum up_pse,
    #(ess != 0), #voxels) over labels == r; row 0 also takes every label above n_regions.  Deterministic; every check
    runs before any launch."""
    n = _n_regions("upproject_regions", n_regions)
    for t, name in ((cle, "cle"), (pse, "pse")):
        if not isinstance(t, Tensor) or t.dim() != 4 or min(t.shape) < 1:
            raise ValueError(f"upproject_regions: {name} must be a non-empty [B,D,H,W] tensor")
        try:
            _req(t[0], f"upproject_regions: {name}[b]")          # device, dtype, contiguous [D,H,W]
        except ValueError:
            raise ValueError(f"upproject_regions: the innermost three dimensions of {name} must be contiguous") from None
    B, D, H, W = (int(s) for s in cle.shape)
    if tuple(pse.shape) != (B, D, H, W):
        raise ValueError(f"upproject_regions: pse {tuple(pse.shape)} must have cle's shape {(B, D, H, W)}")
    sb = int(cle.stride(0)) if B > 1 else D * H * W
    if B > 1 and (int(pse.stride(0)) != sb or sb < D * H * W):
        raise ValueError("upproject_regions: cle and pse must share one batch stride >= D*H*W "
                         f"(got {cle.stride(0)} and {pse.stride(0)})")
    Do, Ho, Wo = (int(v) for v in size)
    if min(Do, Ho, Wo) < 1 or Do * Ho * Wo >= 2 ** 31 or D * H * W >= 2 ** 31:
        raise ValueError(f"upproject_regions: size {(Do, Ho, Wo)} must be positive and below 2^31 voxels")
    masks = []
    for t, name in ((ess_u8, "ess_u8"), (labels_u8, "labels_u8")):
        if isinstance(t, Tensor) and t.dtype == torch.bool:
            t = t.contiguous().view(torch.uint8)
        masks.append(_req(t, f"upproject_regions: {name}", torch.uint8, shape=(B, Do, Ho, Wo)))
    ess_u8, labels_u8 = masks
    dev = cle.device
    nblk = _L().dram_region_nblk(Do * Ho * Wo)
    up_c = torch.empty((B, Do, Ho, Wo), device=dev, dtype=torch.float32) if want_volumes else None
    up_p = torch.empty((B, Do, Ho, Wo), device=dev, dtype=torch.float32) if want_volumes else None
    partial = torch.empty((B, nblk, n + 1, 4), device=dev, dtype=torch.float32)
    table = torch.empty((B, n + 1, 4), device=dev, dtype=torch.float64)
    _chk(_L().dram_upproject_regions(_p(cle), _p(pse), sb, _p(ess_u8), _p(labels_u8), _p(up_c), _p(up_p), _p(partial),
                                     _p(table), B, D, H, W, Do, Ho, Wo, n, _stream()), "dram_upproject_regions")
    return up_c, up_p, table


def lobe_histogram(image: Tensor, labels: Tensor, n_regions: int = 5, hu_lo: int = -1024, nbins: int = 1024):
    """Per-region 1-HU histogram of a scan in one pass (csrc/densito.hip).

    image [D,H,W] int16 HU, contiguous (``prepare_case``'s 'image'); labels [D,H,W] uint8 / int16 / bool, read in place
    through their z / y strides when the x stride is 1 (``prepare_case``'s 'lobe_labels' view; any other view is made
    contiguous first).  -> (hist, sums): hist [n_regions + 1, nbins] int64, voxels per row and bin
    ``clamp(hu, hu_lo, hu_lo + nbins - 1) - hu_lo`` (the end bins collect the tails); sums [n_regions + 1, 2] int64 =
    (voxel count, sum of the raw HU values).  Label r in 1..n_regions -> row r, a label above n_regions -> row 0, a
    label <= 0 is counted nowhere, so the rows add up to ``labels > 0``.  Supported: nbins a multiple of 64 in 64..2048,
    (n_regions + 1) * nbins <= 32768, hu_lo .. hu_lo + nbins - 1 inside int16, fewer than 2^31 voxels.  Integer counts:
    bit-identical from call to call; never synchronises; every check runs before any launch."""
    n, lo, nb = _n_regions("lobe_histogram", n_regions), int(hu_lo), int(nbins)
    D, H, W = _volume("lobe_histogram", image, "image")
    labels, code, sz, sy = _label_view("lobe_histogram", labels, "labels", image.shape)
    dev = labels.device
    with launch_scope(dev):
        _req(image, "lobe_histogram: image", torch.int16)
        nblk = _L().dram_lobe_hist_nblk(D * H * W)
        part_hist = torch.empty((nblk, n + 1, nb), device=dev, dtype=torch.int32)
        part_sums = torch.empty((nblk, n + 1, 2), device=dev, dtype=torch.int64)
        hist = torch.empty((n + 1, nb), device=dev, dtype=torch.int64)
        sums = torch.empty((n + 1, 2), device=dev, dtype=torch.int64)
        _chk(_L().dram_lobe_hist(_p(image), _p(labels), code, sz, sy, _p(part_hist), _p(part_sums), _p(hist), _p(sums),
                                 D, H, W, n, lo, nb, _stream()), "dram_lobe_hist")
    return hist, sums


LOCAL_MAX_RADIUS = _lib.DRAM_BOXFRAC_MAX_RADIUS      # (2 * 16 + 1)^3 < 2^16: both counts of a box share one 32-bit word


def local_window(spacing, local_mm) -> Tuple[int, int, int]:
    """The radii (rz, ry, rx) in voxels of the box of ``local_fraction3d`` whose sides are ``local_mm`` millimetres, in
    whole micrometres like ``lung_zones_units``: ``r_a = round(local_mm * 1000) // (2 * round(spacing_a * 1000))``.  The
    box has 2 r + 1 voxels per axis: at most ``local_mm`` plus one voxel, and an axis whose voxels are larger than
    ``local_mm / 2`` is one voxel thick.  ValueError for a spacing or ``local_mm`` that is not positive and finite (or
    rounds to 0 um), for an axis whose radius exceeds 16 (the message names the axis and its spacing) and when all
    three radii are 0: the window would hold one voxel.  Pure host code."""
    sp = _spacing3("local_window", spacing)
    if isinstance(local_mm, bool) or not isinstance(local_mm, (int, float)) or not math.isfinite(local_mm) or not local_mm > 0:
        raise ValueError(f"local_window: local_mm must be one finite number > 0, got {local_mm!r}")
    s_um, l_um = [int(round(v * 1000.0)) for v in sp], int(round(float(local_mm) * 1000.0))
    if min(s_um) < 1 or l_um < 1:
        raise ValueError(f"local_window: spacing {tuple(sp)} mm and local_mm {local_mm} must round to at least 1 um")
    radius = tuple(l_um // (2 * s) for s in s_um)
    for axis, r, v in zip("zyx", radius, sp):
        if r > LOCAL_MAX_RADIUS:
            raise ValueError(f"local_window: local_mm {local_mm} on axis {axis} with spacing {v} mm is radius {r}; the "
                             f"box count holds radius <= {LOCAL_MAX_RADIUS}")
    if max(radius) == 0:
        raise ValueError(f"local_window: local_mm {local_mm} is below two voxels on every axis of spacing {tuple(sp)} "
                         "mm: the window would hold one voxel")
    return radius


def _local_radius(fn: str, radius) -> Tuple[int, int, int]:
    try:
        r = tuple(-1 if isinstance(v, bool) else v.__index__() for v in radius)      # ints and numpy's, no floats
    except (TypeError, AttributeError):
        r = ()
    if len(r) != 3 or min(r) < 0:
        raise ValueError(f"{fn}: radius must be three integers >= 0 (rz, ry, rx), got {radius!r}")
    if max(r) > LOCAL_MAX_RADIUS:
        raise ValueError(f"{fn}: radius {r} exceeds the {LOCAL_MAX_RADIUS} the box count holds")
    return r


def local_fraction3d(image: Tensor, labels: Tensor, threshold: int = -950, radius=(1, 1, 1), out: Optional[Tensor] = None,
                     out_u8: Optional[Tensor] = None, want_counts: bool = False):
    """Local low-attenuation fraction (csrc/boxfrac.hip; definitions: INTEGRATION.md B13): at every lung voxel the share,
    in per mille, of the lung voxels in the box [z +- rz] x [y +- ry] x [x +- rx] around it (clipped to the volume) whose
    HU value is below ``threshold`` (strict, as in ``densitometry``).  Lung voxels of ANY label count, not only those of
    the voxel's own lobe.

    image [D,H,W] int16 HU, contiguous; labels [D,H,W] uint8 / int16 / bool, read in place like ``lobe_histogram``'s
    (lung = label > 0); threshold an integer in -32768..32768; radius (rz, ry, rx), integers in 0..16
    (``local_window`` gives them for a window in millimetres).  -> map [D,H,W] int16: q = (2000 num + den) // (2 den),
    0..1000, rounded half up, where the label is positive and -1 elsewhere; with ``want_counts`` (map, counts), counts
    [D,H,W] int32 = num << 16 | den at EVERY voxel (den: lung voxels in the box, num: those below the threshold; read
    num as ``(c >> 16) & 0xffff``: it passes 32 767 in the largest boxes).
    out: an int16 contiguous tensor of the image's shape (default: a new one).  out_u8: a uint8 [D,H,W] VIEW (x stride 1,
    rows and planes disjoint), e.g. the crop's window of a zero-filled volume of the scan's size: it receives
    (q * 255) // 1000, 0 where q = -1, and nothing outside the view is written.  Neither may share storage with an
    input.  Fewer than 2^31 voxels.  Two launches and a 32-bit intermediate from the shared workspace; integers only:
    bit-identical from call to call; the inputs are only read; never synchronises; every check runs before any launch."""
    fn = "local_fraction3d"
    rz, ry, rx = _local_radius(fn, radius)
    threshold = _hu_threshold(fn, threshold)
    D, H, W = _volume(fn, image, "image", (torch.int16,))
    apart = [image] + ([labels] if isinstance(labels, Tensor) else [])
    for name, t, dtype in (("out", out, torch.int16), ("out_u8", out_u8, torch.uint8)):
        if t is not None:
            _out(fn, name, t, (D, H, W), dtype, image.device, apart, of=None, rest="image, labels or the other output")
            apart.append(t)
    if out is not None and not out.is_contiguous():
        raise ValueError(f"{fn}: out must be contiguous")
    uz = uy = 0
    if out_u8 is not None:
        uz, uy, ux = (int(v) for v in out_u8.stride())
        if (W > 1 and ux != 1) or uz < 0 or uy < 0 or (H > 1 and uy < W) or (D > 1 and uz < (H - 1) * uy + W):
            raise ValueError(f"{fn}: out_u8 must be a view with x stride 1 whose rows and planes are disjoint, got strides "
                             f"{tuple(out_u8.stride())}")
    if not image.is_contiguous():
        raise ValueError(f"{fn}: image must be contiguous")
    labels, code, sz, sy = _label_view(fn, labels, "labels", image.shape)
    if labels.device != image.device:
        raise ValueError(f"{fn}: labels must live on the image's device")
    dev = image.device
    with launch_scope(dev):
        _req(image, f"{fn}: image", torch.int16)
        if out is None:
            out = torch.empty((D, H, W), device=dev, dtype=torch.int16)
        counts = torch.empty((D, H, W), device=dev, dtype=torch.int32) if want_counts else None
        nbytes = int(_L().dram_boxfrac3d_workspace(D, H, W))
        if nbytes < 0:
            raise RuntimeError("dram_boxfrac3d_workspace refused the volume")
        ws = _workspace(nbytes, dev)
        _chk(_L().dram_boxfrac3d(_p(image), _p(labels), code, sz, sy, threshold, rz, ry, rx, _p(counts), _p(out),
                                 _p(out_u8), uz, uy, _p(ws), ws.numel() * 4, D, H, W, _stream()), "dram_boxfrac3d")
    return (out, counts) if want_counts else out


EDT_FULL_UM = 1 << 26          # max_um from here on is the full transform (no distance in a supported volume reaches it)


def lung_zones_units(spacing, peel_mm, max_mm=None, fn: str = "lung_zones"):
    """(spacing in whole micrometres (z, y, x), peel_um, max_um) of ``lung_zones``: round(mm * 1000), ``max_mm=None``
    -> peel_mm, ``inf`` (or anything from 2^26 um on) -> ``EDT_FULL_UM``.  ValueError for a spacing or peel_mm that is
    not positive and finite, a spacing outside 1..20000 um, and max_mm < peel_mm, in the name of ``fn``.  Pure host code."""
    sp = [float(v) for v in spacing]
    if len(sp) != 3:
        raise ValueError(f"{fn}: spacing must have three entries (z, y, x)")
    if not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"{fn}: spacing must be positive and finite, got {tuple(sp)}")
    s_um = [int(round(v * 1000.0)) for v in sp]
    if not all(1 <= s <= 20000 for s in s_um):
        raise ValueError(f"{fn}: spacing must round to 1..20000 um per axis, got {tuple(sp)} mm")
    peel = float(peel_mm)
    if not (math.isfinite(peel) and peel > 0):
        raise ValueError(f"{fn}: peel_mm must be positive and finite, got {peel_mm}")
    peel_um = min(int(round(peel * 1000.0)), EDT_FULL_UM)
    if max_mm is None:
        max_um = peel_um
    else:
        mx = float(max_mm)
        if math.isnan(mx) or mx < peel:
            raise ValueError(f"{fn}: max_mm {max_mm} must be at least peel_mm {peel_mm}")
        max_um = EDT_FULL_UM if math.isinf(mx) else min(int(round(mx * 1000.0)), EDT_FULL_UM)
    return tuple(s_um), peel_um, max(max_um, peel_um)


def lung_zones(labels: Tensor, spacing, peel_mm: float, n_regions: Optional[int] = None, max_mm: Optional[float] = None,
               want_dist: bool = False):
    """Core / peel zones of the lung from the exact Euclidean distance transform of ``labels > 0`` at the scan's own
    anisotropic spacing (csrc/edt.hip; definitions: INTEGRATION.md B7).

    labels [D,H,W] uint8 / int16 / bool, read in place through their z / y strides when the x stride is 1
    (``prepare_case``'s 'lobe_labels' view; any other view is made contiguous first); spacing (z, y, x) and peel_mm in
    mm, taken in whole micrometres.  d2 = squared distance to the centre of the nearest background voxel OF THE VOLUME
    (nothing outside it is background), an integer in um^2; ``max_mm``: distances above it are +inf (None: peel_mm, the
    least work that decides the zones; inf: the full transform).  -> (zones, zone_labels | None, dist_mm | None):
      zones uint8: 0 not lung, 1 peel (d2 <= peel_um^2), 2 core;
      zone_labels uint8 (with ``n_regions`` = n in 1..7): label r in 1..n -> r + n * (zone - 1), a lung label above n ->
        255 -- the label volume of ``lobe_histogram`` / ``upproject_regions`` with 2 n regions;
      dist_mm float32 (``want_dist``): sqrt(d2) / 1000, 0 outside the lung, +inf where d2 is.
    Supported: fewer than 2^31 voxels, spacing 1..20000 um and (size - 1) * spacing < 2^25 um on every axis.  Exact
    integers: bit-identical from call to call; never synchronises; every check runs before any launch."""
    s_um, peel_um, max_um = lung_zones_units(spacing, peel_mm, max_mm)
    n = 0 if n_regions is None else _n_regions("lung_zones", n_regions, 7)
    if isinstance(labels, Tensor) and labels.dim() == 3:               # anything else: _label_view's refusal below
        for size, s, axis in zip(labels.shape, s_um, "zyx"):
            if (size - 1) * s >= 2 ** 25:
                raise ValueError(f"lung_zones: axis {axis}: (size - 1) * spacing = {(size - 1) * s} um must be below 2^25")
    labels, code, sz, sy = _label_view("lung_zones", labels, "labels")
    D, H, W = (int(v) for v in labels.shape)
    dev = labels.device
    with launch_scope(dev):
        nbytes = int(_L().dram_lung_zones_workspace(D, H, W, max_um))
        work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        zones = torch.empty((D, H, W), device=dev, dtype=torch.uint8)
        zlab = torch.empty((D, H, W), device=dev, dtype=torch.uint8) if n else None
        dist = torch.empty((D, H, W), device=dev, dtype=torch.float32) if want_dist else None
        _chk(_L().dram_lung_zones(_p(labels), code, sz, sy, _p(zones), _p(zlab), _p(dist), _p(work), D, H, W, *s_um,
                                  peel_um, max_um, n, _stream()), "dram_lung_zones")
    return zones, zlab, dist


def lobe_zones_units(spacing, peel_mm, fissure_mm, max_mm=None):
    """(spacing in whole micrometres (z, y, x), peel_um, fissure_um, max_um) of ``lobe_zones``: ``lung_zones_units``'
    rounding; ``max_mm=None`` -> max(peel_mm, fissure_mm), ``inf`` -> ``EDT_FULL_UM``.  ValueError for what
    ``lung_zones_units`` refuses, a fissure_mm that is not positive and finite, and max_mm below either width.  Pure
    host code."""
    s_um, peel_um, _ = lung_zones_units(spacing, peel_mm, fn="lobe_zones")
    fis = float(fissure_mm)
    if not (math.isfinite(fis) and fis > 0):
        raise ValueError(f"lobe_zones: fissure_mm must be positive and finite, got {fissure_mm}")
    fis_um = min(int(round(fis * 1000.0)), EDT_FULL_UM)
    widest = max(peel_um, fis_um)
    if max_mm is None:
        max_um = widest
    else:
        mx = float(max_mm)
        if math.isnan(mx) or mx < float(peel_mm) or mx < fis:
            raise ValueError(f"lobe_zones: max_mm {max_mm} must be at least peel_mm {peel_mm} and fissure_mm {fissure_mm}")
        max_um = EDT_FULL_UM if math.isinf(mx) else min(int(round(mx * 1000.0)), EDT_FULL_UM)
    return s_um, peel_um, fis_um, max(max_um, widest)


def lobe_zones(labels: Tensor, spacing, peel_mm: float, fissure_mm: float, n_regions: int = 5,
               max_mm: Optional[float] = None, want_dist: bool = False):
    """Peel / core / fissural rind of the lobes: ``lung_zones``' pleural distance d2 and, per lung voxel, the exact
    squared distance f2 to the nearest voxel of ANOTHER lobe (csrc/edt.hip; definitions: INTEGRATION.md B7).

    labels, spacing, peel_mm and the supported sizes as ``lung_zones``; ``n_regions`` = n in 1..5 (3 n <= 15).  A voxel's
    class is its label in 1..n, n + 1 for a lung label above n, 0 for a label <= 0; only classes 1..n are sites of f2 (a
    lung voxel that belongs to no region makes no fissure).  ``max_mm``: distances above it are +inf (None:
    max(peel_mm, fissure_mm), the least work that decides the zones; inf: the full transforms).  ->
    (zones, zone_labels, pleura_mm | None, fissure_mm | None):
      zones uint8: 0 not lung, 1 peel (d2 <= peel_um^2, ``lung_zones``' zone 1 bit for bit: the peel wins), 3 fissural
        rind (not peel and f2 <= fissure_um^2), 2 core (the rest);
      zone_labels uint8: class r in 1..n -> r + n * (zone - 1) (1..n peel, n+1..2n core, 2n+1..3n fissural rind), class
        n + 1 -> 255 -- the label volume of ``lobe_histogram`` / ``upproject_regions`` with 3 n regions;
      pleura_mm, fissure_mm float32 (``want_dist``): sqrt(d2 | f2) / 1000, 0 outside the lung, +inf where the squared
        distance is (no background / no foreign site, or none within max_mm).
    ``fissure_mm`` is the caller's choice.  Exact integers: bit-identical from call to call; never synchronises; every
    check runs before any launch."""
    s_um, peel_um, fis_um, max_um = lobe_zones_units(spacing, peel_mm, fissure_mm, max_mm)
    n = _n_regions("lobe_zones", n_regions, 5)
    if isinstance(labels, Tensor) and labels.dim() == 3:               # anything else: _label_view's refusal below
        for size, s, axis in zip(labels.shape, s_um, "zyx"):
            if (size - 1) * s >= 2 ** 25:
                raise ValueError(f"lobe_zones: axis {axis}: (size - 1) * spacing = {(size - 1) * s} um must be below 2^25")
    labels, code, sz, sy = _label_view("lobe_zones", labels, "labels")
    D, H, W = (int(v) for v in labels.shape)
    dev = labels.device
    with launch_scope(dev):
        nbytes = int(_L().dram_lobe_zones_workspace(D, H, W, max_um))
        work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        zones = torch.empty((D, H, W), device=dev, dtype=torch.uint8)
        zlab = torch.empty((D, H, W), device=dev, dtype=torch.uint8)
        pleura = torch.empty((D, H, W), device=dev, dtype=torch.float32) if want_dist else None
        fissure = torch.empty((D, H, W), device=dev, dtype=torch.float32) if want_dist else None
        _chk(_L().dram_lobe_zones(_p(labels), code, sz, sy, _p(zones), _p(zlab), _p(pleura), _p(fissure), _p(work), D, H, W,
                                  *s_um, peel_um, fis_um, max_um, n, _stream()), "dram_lobe_zones")
    return zones, zlab, pleura, fissure


CCL_TABLE_COLS = 35             # 32 size bins (2^k <= size < 2^(k+1)), components, foreground voxels, largest size


def _label_components(fn: str, name: str, labels: Tensor, image: Optional[Tensor], threshold: int, by_lobe: bool,
                      connectivity: int, n_regions: int, want_sizes: bool):
    conn = int(connectivity)
    if conn not in (6, 26):
        raise ValueError(f"{fn}: connectivity must be 6 or 26, got {connectivity}")
    n = _n_regions(fn, n_regions)
    labels, code, sz, sy = _label_view(fn, labels, name, None if image is None else image.shape)
    D, H, W = (int(v) for v in labels.shape)
    dev = labels.device
    with launch_scope(dev):
        if image is not None:
            _req(image, f"{fn}: image", torch.int16)
        nbytes = int(_L().dram_label_components_workspace(D, H, W))
        work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        comp = torch.empty((D, H, W), device=dev, dtype=torch.int32)
        sizes = torch.empty((D, H, W), device=dev, dtype=torch.int32) if want_sizes else None
        table = torch.empty((n + 1, CCL_TABLE_COLS), device=dev, dtype=torch.int64)
        _chk(_L().dram_label_components(_p(labels), code, sz, sy, _p(image), int(threshold), 1 if by_lobe else 0, conn, n,
                                        _p(comp), _p(sizes), _p(table), _p(work), D, H, W, _stream()),
             "dram_label_components")
    return comp, table, sizes


def label_components(key: Tensor, connectivity: int = 6, n_regions: int = 5, want_sizes: bool = False):
    """Connected components of a 3-D key volume (csrc/ccl.hip; definitions: INTEGRATION.md B8).

    key [D,H,W] uint8 / int16 / bool, read in place through its z / y strides when the x stride is 1 (any other view is
    made contiguous first): 0 (or below) is background, two voxels are connected when they are neighbours under
    ``connectivity`` (6 faces; 26 faces, edges, corners) and carry the same non-zero key.  -> (components, table,
    cluster_voxels | None):
      components int32 [D,H,W]: the linear index (z*H + y)*W + x of the component's smallest voxel, -1 on background;
      table int64 [n_regions + 1, 35]: a component counts in the row of its key (key r in 1..n_regions -> row r, a key
        above n_regions -> row 0); columns 0..31 the components with 2^k <= size < 2^(k+1), 32 the number of components,
        33 the foreground voxels, 34 the largest size;
      cluster_voxels int32 [D,H,W] (``want_sizes``): the size of the voxel's component, 0 on background.
    Fewer than 2^31 voxels.  Integer atomics only: bit-identical from call to call; never synchronises; every check runs
    before any launch."""
    return _label_components("label_components", "key", key, None, 0, True, connectivity, n_regions, want_sizes)


def laa_components(image: Tensor, labels: Tensor, threshold: int = -950, n_regions: int = 5, connectivity: int = 6,
                   by_lobe: bool = True, want_sizes: bool = False):
    """Low-attenuation clusters of a scan: ``label_components`` of the LAA key, formed inside the kernel.

    image [D,H,W] int16 HU, contiguous; labels [D,H,W] uint8 / int16 / bool of the same shape, read in place like
    ``lobe_histogram``'s.  The key is ``labels`` where ``labels > 0`` and ``image < threshold`` (strict, the comparison
    of ``densitometry``'s 'laa_counts'), else 0 -- clusters do not cross a fissure, each belongs to one lobe -- or, with
    ``by_lobe=False``, 1 there: whole-lung clusters, reported in row 1 of a table of two rows.  threshold: an integer HU
    in -32768..32768.  -> the triple of ``label_components``."""
    _volume("laa_components", image, "image", (torch.int16,), nonempty=False)
    t = _hu_threshold("laa_components", threshold, "an integer HU", bools=True)
    return _label_components("laa_components", "labels", labels, image, t, bool(by_lobe), connectivity,
                             n_regions if by_lobe else 1, want_sizes)


SHAPE_COLS = 18                 # columns of a ``component_shapes`` row
SHAPE_ROOT, SHAPE_CLASS, SHAPE_VOXELS = 0, 1, 2
SHAPE_Z0, SHAPE_Z1, SHAPE_Y0, SHAPE_Y1, SHAPE_X0, SHAPE_X1 = 3, 4, 5, 6, 7, 8     # bounding box, half-open
SHAPE_SUM_Z, SHAPE_SUM_Y, SHAPE_SUM_X = 9, 10, 11                                   # the centroid's numerators
SHAPE_FACES_Z, SHAPE_FACES_Y, SHAPE_FACES_X = 12, 13, 14                            # exposed faces normal to the axis
SHAPE_ZONE1, SHAPE_ZONE2, SHAPE_ZONE3 = 15, 16, 17                                  # voxels with zones == 1, 2, 3


def component_shapes(components: Tensor, labels: Optional[Tensor] = None, zones: Optional[Tensor] = None,
                     max_components: Optional[int] = None):
    """One row per connected component of a labelled volume (csrc/ccl_shapes.hip; definitions: INTEGRATION.md B8).

    components [D,H,W] int32, contiguous, only read: ``label_components``' first output, the linear index of the
    component's smallest voxel, -1 on background.  A voxel v with c = components[v] counts in component c only when
    0 <= c < D*H*W and components[c] == c; any other voxel is background.  labels (optional) [D,H,W] uint8 / int16 /
    bool, a view as ``label_components`` takes it; zones (optional) [D,H,W] uint8, contiguous: ``lung_zones`` /
    ``lobe_zones``' first output.  -> (rows, count):
      rows int64 [m, 18], row r the component whose root (``components[v] == v``) is the r-th in ascending linear index;
        columns (``SHAPE_*``): 0 root, 1 class (labels at the root, 0 without labels), 2 voxels, 3..8 z0, z1, y0, y1, x0,
        x1 (half-open box), 9..11 the sums of z, y, x over the voxels, 12..14 the exposed faces normal to z, y, x (the
        neighbour along the axis lies outside the volume or holds another value in ``components``; two components that
        touch each count the shared face), 15..17 the voxels with zones == 1, 2, 3 (0 without zones);
      count int64 [2]: the number of components, and the rows filled = min(that, m).
    ``max_components=None``: m is the number of components -- ``count[0]`` is read back between the ranking and the
    accumulation, the ONE synchronisation of this call; an empty volume gives zero rows.  ``max_components=k``: nothing
    is read back, rows is [k, 18], truncated to the first k components or zero-padded, and the caller reads ``count``.
    Fewer than 2^31 voxels.  Integer atomics only: bit-identical from call to call; every check runs before any
    launch."""
    fn = "component_shapes"
    D, H, W = _volume(fn, components, "components", (torch.int32,))
    if zones is not None:
        if not isinstance(zones, Tensor) or zones.dtype != torch.uint8:
            raise TypeError(f"{fn}: zones must be a uint8 tensor")
        if tuple(zones.shape) != (D, H, W):
            raise ValueError(f"{fn}: zones {tuple(zones.shape)} must have the shape of components {(D, H, W)}")
    cap = None
    if max_components is not None:
        cap = int(max_components)
        if cap != max_components or cap < 0:
            raise ValueError(f"{fn}: max_components must be a non-negative integer, got {max_components}")
    code, sz, sy = 1, 0, 0
    if labels is not None:
        labels, code, sz, sy = _label_view(fn, labels, "labels", (D, H, W))
    dev = components.device
    with launch_scope(dev):
        _req(components, f"{fn}: components", torch.int32)
        if zones is not None:
            _req(zones, f"{fn}: zones", torch.uint8)
        if labels is not None and labels.device != dev:
            raise RuntimeError(f"{fn}: labels must live on the device of components")
        work = torch.empty((int(_L().dram_component_shapes_workspace(D, H, W)),), device=dev, dtype=torch.uint8)
        count = torch.empty((2,), device=dev, dtype=torch.int64)
        _chk(_L().dram_component_rank(_p(components), _p(work), _p(count), D, H, W, _stream()), "dram_component_rank")
        if cap is None:
            cap = int(count[0].item())                                 # the one synchronisation
        rows = torch.empty((cap, SHAPE_COLS), device=dev, dtype=torch.int64)
        _chk(_L().dram_component_shapes(_p(components), _p(labels), code, sz, sy, _p(zones), _p(work),
                                        _p(rows) if cap else None, cap, _p(count), D, H, W, _stream()),
             "dram_component_shapes")
    return rows, count


def median_size(fn: str, size) -> Tuple[int, int, int]:
    """A median window ``size`` -- three entries in (z, y, x) order, each 1 or 3, at least one 3 -- as a tuple of ints;
    ValueError for anything else.  Pure host code."""
    try:
        s = tuple(size)
    except TypeError:
        s = ()
    if len(s) != 3 or any(isinstance(v, bool) or v not in (1, 3) for v in s) or max(s) != 3:
        raise ValueError(f"{fn}: size must have three entries (z, y, x), each 1 or 3 and at least one 3, got {size!r}")
    return tuple(int(v) for v in s)


def median_filter3d(image: Tensor, size=(3, 3, 3), out: Optional[Tensor] = None) -> Tensor:
    """Median filter of a scan (csrc/median.hip; definitions: INTEGRATION.md B9): every voxel becomes the median of the
    ``size`` window centred on it, indices clamped to the volume -- ``scipy.ndimage.median_filter(image, size,
    mode='nearest')``, exactly.

    image [D,H,W] int16 (made contiguous if it is not; never written); size (z, y, x), each entry 1 or 3 and at least
    one 3: (3,3,3) is the 27-sample filter, (1,3,3) the in-plane one for thick slices; out: an int16 contiguous tensor
    of the image's shape that shares no storage with it (default: a new one).  -> out.  Fewer than 2^31 voxels.  A
    min / max selection network on integers: bit-identical from call to call; never synchronises; every check runs
    before any launch."""
    rz, ry, rx = (v // 2 for v in median_size("median_filter3d", size))
    D, H, W = _volume("median_filter3d", image, "image", (torch.int16,))
    if out is not None:
        _out("median_filter3d", "out", out, (D, H, W), torch.int16, image.device, [image], a="an int16")
    image = image.contiguous()
    with launch_scope(image.device):
        _req(image, "median_filter3d: image", torch.int16)
        if out is None:
            out = torch.empty_like(image)
        _chk(_L().dram_median3d(_p(image), _p(out), D, H, W, rz, ry, rx, _stream()), "dram_median3d")
    return out


GAUSS_MAX_RADIUS = 16           # DramGaussTaps holds 17 weights per axis


def gaussian_radius(sigma: float, truncate: float = 4.0) -> int:
    """``int(truncate * sigma + 0.5)``, the radius of the reference's ``generate_gaussian_1d_kernel``
    (functional.py:46).  ValueError for a negative or non-finite sigma and for ``truncate`` <= 0.  Pure host code."""
    return _radius("gaussian_taps", sigma, truncate)


def gaussian_taps(sigma: float, truncate: float = 4.0) -> Tensor:
    """The reference's ``generate_gaussian_1d_kernel(sigma, truncate)`` (functional.py:44-51) as a CPU float32 tensor
    [2 r + 1]: r = ``gaussian_radius``, float32 ``exp(-0.5 / sigma^2 * k^2)`` over k = -r..r divided by its float32 sum.
    ``sigma == 0`` (and any sigma whose radius is 0) gives the single tap 1.0.  ValueError as ``gaussian_radius``, and
    for a radius above 16, which is what the kernel's tap table holds.  Pure host code."""
    r = gaussian_radius(sigma, truncate)
    if r > GAUSS_MAX_RADIUS:
        raise ValueError(f"gaussian_taps: sigma {float(sigma)!r} x truncate {float(truncate)!r} gives radius {r}; the "
                         f"filter holds radius <= {GAUSS_MAX_RADIUS}")
    if r == 0:
        return torch.ones(1, dtype=torch.float32)
    k = torch.arange(-r, r + 1)
    phi = torch.exp(-0.5 / float(sigma) ** 2 * k ** 2)
    return phi / phi.sum()


@functools.lru_cache(maxsize=256)
def _gauss_half(sigma: float, truncate: float) -> Tuple[float, ...]:
    """w[0..r] of ``gaussian_taps``: the half the C struct holds (cached: three axes usually share one sigma)"""
    w = gaussian_taps(sigma, truncate)
    return tuple(w[w.numel() // 2:].tolist())


def _gauss_box(box, shape):
    """``box`` -- None or [[z0,z1],[y0,y1],[x0,x1]] (a list or ``prepare_case``'s 'crop_slice' tensor) -- as three
    (lo, hi) pairs of ints inside ``shape``; ValueError otherwise.  The pairs size the output, so they are needed on the
    host: 'crop_slice' is a host tensor and costs nothing; a box given as a DEVICE tensor is read back here."""
    if box is None:
        return [(0, int(n)) for n in shape]
    try:
        pairs = [(int(lo), int(hi)) for lo, hi in (box.tolist() if isinstance(box, Tensor) else box)]
    except (TypeError, ValueError):
        pairs = []
    if len(pairs) != 3 or any(not 0 <= lo < hi <= n for (lo, hi), n in zip(pairs, shape)):
        raise ValueError(f"gaussian_filter3d: box must be [[z0,z1],[y0,y1],[x0,x1]] with 0 <= lo < hi <= size inside "
                         f"the image {tuple(shape)}, got {box!r}")
    return pairs


def gaussian_filter3d(image: Tensor, sigma, truncate: float = 4.0, mode: str = "nearest", box=None,
                      out: Optional[Tensor] = None, out_dtype=None) -> Tensor:
    """Separable Gaussian filter of a volume (csrc/gauss.hip; definitions: INTEGRATION.md B11): along each axis the
    taps of ``gaussian_taps(sigma_axis, truncate)``, x then y then z, in fp32.

    image [D,H,W] int16 or float32 (made contiguous if it is not; never written); sigma in VOXELS, a number or
    (z, y, x); an axis whose radius ``int(truncate * sigma + 0.5)`` is 0 is left untouched; mode: 'nearest' (indices
    clamped to the volume: ``scipy.ndimage.correlate1d(mode='nearest')``) or 'zero' (zeros outside: the reference's
    ``conv1d(padding='same')``); box: None, or [[z0,z1],[y0,y1],[x0,x1]] (``prepare_case``'s 'crop_slice' as it is):
    only that box of the filtered volume is computed, and it equals the crop of the whole result bit for bit (the
    border rule applies at the volume's faces, not the box's); out_dtype: the image's by default; float32 from either,
    int16 only from int16 (rint of the float32 result, clamped to the int16 range); out: a contiguous tensor of the
    box's shape and of out_dtype on the image's device that shares no storage with it (default: a new one).  -> out.
    Fewer than 2^31 voxels.  Two launches and an fp32 intermediate from the shared workspace; the order of the fp32
    operations of a voxel depends on the taps alone: bit-identical from call to call; never synchronises (give ``box``
    as a list or a host tensor: a device tensor would be read back first); every check runs before any launch."""
    if mode not in ("nearest", "zero"):
        raise ValueError(f"gaussian_filter3d: mode must be 'nearest' or 'zero', got {mode!r}")
    taps = _lib.DramGaussTaps()
    for a, s in enumerate(_sigma3("gaussian_filter3d", sigma)):
        half = _gauss_half(s, float(truncate))
        taps.radius[a] = len(half) - 1
        taps.w[a][:len(half)] = half
    D, H, W = _volume("gaussian_filter3d", image, "image", (torch.int16, torch.float32))
    out_dtype = image.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.int16, torch.float32) or (out_dtype == torch.int16 and image.dtype != torch.int16):
        raise TypeError(f"gaussian_filter3d: out_dtype must be float32, or int16 for an int16 image; got {out_dtype} "
                        f"for {image.dtype}")
    (z0, z1), (y0, y1), (x0, x1) = _gauss_box(box, image.shape)
    shape = (z1 - z0, y1 - y0, x1 - x0)
    if out is not None:
        _out("gaussian_filter3d", "out", out, shape, out_dtype, image.device, [image], of="the box's shape")
    image = image.contiguous()
    code = {torch.int16: 2, torch.float32: 4}
    with launch_scope(image.device):
        _req(image, "gaussian_filter3d: image", image.dtype)
        if out is None:
            out = torch.empty(shape, device=image.device, dtype=out_dtype)
        nbytes = int(_L().dram_gauss3d_workspace(D, z0, shape[0], shape[1], shape[2], int(taps.radius[0])))
        if nbytes < 0:
            raise RuntimeError("dram_gauss3d_workspace refused the box")
        ws = _workspace(nbytes, image.device)
        _chk(_L().dram_gauss3d(_p(image), code[image.dtype], _p(out), code[out_dtype], D, H, W, z0, y0, x0, *shape,
                               ctypes.byref(taps), 0 if mode == "nearest" else 1, _p(ws), ws.numel() * 4, _stream()),
             "dram_gauss3d")
    return out


BILAT_MAX_RADIUS = _lib.DRAM_BILAT_MAX_RADIUS       # DramBilateral holds 6 spatial entries per axis ...
BILAT_RANGE_LEN = _lib.DRAM_BILAT_RANGE_LEN         # ... and 1024 range entries


def bilateral_radius(sigma: float, truncate: float = 2.0) -> int:
    """``int(truncate * sigma + 0.5)``, the radius of one axis of ``bilateral_filter3d``.  ValueError for a negative or
    non-finite sigma and for ``truncate`` <= 0.  Pure host code."""
    return _radius("bilateral_tables", sigma, truncate)


@functools.lru_cache(maxsize=64)
def _bilateral_tables(sig: Tuple[float, float, float], sigma_hu: float, truncate: float):
    spatial = []
    for axis, s in zip("zyx", sig):
        r = bilateral_radius(s, truncate)
        if r > BILAT_MAX_RADIUS:
            raise ValueError(f"bilateral_tables: sigma {s!r} x truncate {truncate!r} on axis {axis} gives radius {r}; the "
                             f"filter holds radius <= {BILAT_MAX_RADIUS}")
        spatial.append(tuple(int(math.floor(256.0 * math.exp(-(k * k) / (2.0 * s * s)) + 0.5)) for k in range(r + 1))
                       if r else (256,))
    if not math.isfinite(sigma_hu) or not sigma_hu > 0:
        raise ValueError(f"bilateral_tables: sigma_hu must be finite and > 0, got {sigma_hu!r}")
    two_var = 2.0 * sigma_hu * sigma_hu
    rng = []
    while not rng or rng[-1] != 0:
        d = len(rng)
        if d > BILAT_RANGE_LEN:                         # the first zero lies beyond the table
            break
        rng.append(int(math.floor(256.0 * math.exp(-(d * d) / two_var) + 0.5)) if two_var > 0.0 else (256 if d == 0 else 0))
    if rng[-1] != 0 or len(rng) > BILAT_RANGE_LEN:
        raise ValueError(f"bilateral_tables: sigma_hu {sigma_hu!r} needs a range table of more than {BILAT_RANGE_LEN} "
                         "entries")
    return spatial[0], spatial[1], spatial[2], tuple(rng)


def bilateral_tables(sigma, sigma_hu: float, truncate: float = 2.0):
    """The integer tables of ``bilateral_filter3d`` -> (T_z, T_y, T_x, R), four lists of ints.
    sigma in VOXELS, a number or (z, y, x).  Per axis r = ``bilateral_radius`` and ``T[k] = floor(256 exp(-k^2 /
    (2 sigma^2)) + 0.5)`` for k = 0..r, [256] for r = 0; ``R[d] = floor(256 exp(-d^2 / (2 sigma_hu^2)) + 0.5)`` for
    d = 0, 1, ... up to and including the first d with R[d] = 0.  ValueError for a radius above 5 (naming the axis), a
    sigma_hu that is not finite and > 0, and a range table of more than 1024 entries.  Python floats; pure host code."""
    tz, ty, tx, rng = _bilateral_tables(_sigma3("bilateral_tables", sigma), float(sigma_hu), float(truncate))
    return list(tz), list(ty), list(tx), list(rng)


@functools.lru_cache(maxsize=64)
def _bilateral_struct(sig: Tuple[float, float, float], sigma_hu: float, truncate: float):
    """the tables as the C struct (cached; only read by the calls)"""
    *spatial, rng = _bilateral_tables(sig, sigma_hu, truncate)
    tab = _lib.DramBilateral()
    for a, t in enumerate(spatial):
        tab.radius[a] = len(t) - 1
        tab.spatial[a][:len(t)] = t
    tab.range_len = len(rng)
    tab.range[:len(rng)] = rng
    return tab


def bilateral_filter3d(image: Tensor, sigma, sigma_hu: float, truncate: float = 2.0, within: Optional[Tensor] = None,
                       out: Optional[Tensor] = None) -> Tensor:
    """Bilateral filter of a scan in exact integer fixed point (csrc/bilateral.hip; definitions: INTEGRATION.md B12).
    With (T_z, T_y, T_x, R) = ``bilateral_tables(sigma, sigma_hu, truncate)`` and L = len(R), a tap at (dz, dy, dx)
    weighs ``S = (T_z[|dz|] T_y[|dy|] T_x[|dx|] + 2^15) >> 16`` in space, and per centre c, over the taps inside the
    volume (and inside ``within``), ``d = v - v_c``, ``w = S R[min(|d|, L - 1)]``, ``num = sum w d``, ``den = sum w``,
    ``out_c = v_c + floor((2 num + den) / (2 den))``.

    image [D,H,W] int16 (made contiguous if it is not; never written); sigma in VOXELS, a number or (z, y, x), every
    radius ``int(truncate * sigma + 0.5)`` <= 5, an axis of radius 0 is left untouched; sigma_hu > 0 in the image's
    units, its range table at most 1024 long (sigma_hu <= 289); within: None, or a label volume [D,H,W] uint8 / int16 /
    bool read in place like ``lobe_histogram``'s labels: only voxels with ``within != 0`` are taps, and a voxel with
    ``within == 0`` keeps its value; out: an int16 contiguous tensor of the image's shape that shares no storage with
    it (default: a new one).  -> out.  Nothing outside the volume is read: no border rule.  Fewer than 2^31 voxels.
    One launch, integers only: bit-identical from call to call; never synchronises; every check runs before any launch."""
    tab = _bilateral_struct(_sigma3("bilateral_filter3d", sigma), float(sigma_hu), float(truncate))
    D, H, W = _volume("bilateral_filter3d", image, "image", (torch.int16,))
    if out is not None:
        _out("bilateral_filter3d", "out", out, (D, H, W), torch.int16, image.device, [image], a="an int16")
    code, sz, sy = 0, 0, 0
    if within is not None:
        within, code, sz, sy = _label_view("bilateral_filter3d", within, "within", (D, H, W))
        if within.device != image.device:
            raise RuntimeError("bilateral_filter3d: within must live on the image's device")
    image = image.contiguous()
    with launch_scope(image.device):
        _req(image, "bilateral_filter3d: image", torch.int16)
        if out is None:
            out = torch.empty_like(image)
        _chk(_L().dram_bilateral3d(_p(image), _p(out), _p(within), code, sz, sy, D, H, W, ctypes.byref(tab), _stream()),
             "dram_bilateral3d")
    return out


# --------------------------------------------------------------------------- heads / losses
def head_fwd(x: Tensor, w: Tensor, bias: Tensor, lungs: Optional[Tensor], sigmoid: bool):
    """x [B,D,H,W,32] (float32 or bfloat16); w [NO,32]; lungs None or [B,Dl,Hl,Wl] full-res mask.  The dense maps
    and the pooling partial sums are float32 on both storage paths."""
    sfx = _act(x, "x")
    B, D, H, W, C = x.shape
    if C != 32:
        raise ValueError("head_fwd: the head consumes the 32-channel us3 output")
    NO = w.shape[0]
    _req(w, "w", shape=(NO, 32))
    _req(bias, "bias", shape=(NO,))
    Dl = Hl = Wl = 0
    if lungs is not None:
        _req(lungs, "lungs")
        if lungs.dim() != 4 or lungs.shape[0] != B:
            raise ValueError("head_fwd: lungs must be [B,Dl,Hl,Wl]")
        _, Dl, Hl, Wl = lungs.shape
    nblk = _L().dram_head_nblk(D * H * W)
    dense = torch.empty((B, NO, D, H, W), device=x.device, dtype=torch.float32)
    partial = torch.empty((B, nblk, NO + 1), device=x.device, dtype=torch.float32)
    _chk(_fn("dram_head_fwd", sfx)(_p(x), _p(w), _p(bias), _p(lungs), Dl, Hl, Wl, _p(dense), _p(partial), B, D, H, W, NO,
                                   int(sigmoid), _stream()), "dram_head_fwd")
    return dense, partial


def head_bwd(x: Tensor, w: Tensor, dense: Optional[Tensor], gdense: Optional[Tensor], gpool: Tensor,
             lungs: Optional[Tensor], sigmoid: bool):
    sfx = _act(x, "x")
    B, D, H, W, C = x.shape
    NO = w.shape[0]
    _req(w, "w", shape=(NO, 32))
    _req(gpool, "gpool", shape=(B, NO))
    if dense is not None:
        _req(dense, "dense", shape=(B, NO, D, H, W))
    if gdense is not None:
        _req(gdense, "gdense", shape=(B, NO, D, H, W))
    Dl = Hl = Wl = 0
    if lungs is not None:
        _req(lungs, "lungs")
        _, Dl, Hl, Wl = lungs.shape
    nparts = _L().dram_head_bwd_nparts(D * H * W)
    dx = torch.empty_like(x)
    wpartial = torch.empty((B * nparts, NO, 33), device=x.device, dtype=torch.float32)
    _chk(_fn("dram_head_bwd", sfx)(_p(x), _p(w), _p(dense), _p(gdense), _p(gpool), _p(lungs), Dl, Hl, Wl, _p(dx),
                                   _p(wpartial), B, D, H, W, NO, int(sigmoid), _stream()), "dram_head_bwd")
    return dx, wpartial


CAM_METHODS = {"gradcam": _lib.DRAM_CAM_GRADCAM, "hirescam": _lib.DRAM_CAM_HIRESCAM, "layercam": _lib.DRAM_CAM_LAYERCAM}


def cam(x: Tensor, w: Tensor, bias: Tensor, gdense: Optional[Tensor], gpool: Tensor, lungs: Optional[Tensor],
        sigmoid: bool, method: str = "gradcam", relu: bool = True) -> Tensor:
    """Class-activation map at the target layer: x [B,D,H,W,32] (float32 or bfloat16) is the us3 output, w / bias the
    stacked heads, (gdense, gpool, lungs, sigmoid) the cotangents exactly as head_bwd takes them -> [B,D,H,W] float32.
    The layer gradient G = d score / d x is formed in registers from head_bwd's dpre and never stored.  hirescam /
    layercam: one pass over x; gradcam: the block sums of dpre, their fold in double (reduce_partials), the combine pass."""
    if method not in CAM_METHODS:
        raise ValueError(f"cam: unknown method {method!r} (one of {sorted(CAM_METHODS)})")
    sfx = _act(x, "x")
    if x.dim() != 5 or x.shape[-1] != 32:
        raise ValueError("cam: x must be the 32-channel us3 output [B,D,H,W,32]")
    B, D, H, W, _ = x.shape
    if min(B, D, H, W) < 1 or x.numel() >= 2 ** 31:
        raise ValueError("cam: x must be non-empty and hold fewer than 2^31 elements")
    NO = w.shape[0]
    _req(w, "w", shape=(NO, 32))
    _req(bias, "bias", shape=(NO,))
    _req(gpool, "gpool", shape=(B, NO))
    if gdense is not None:
        _req(gdense, "gdense", shape=(B, NO, D, H, W))
    Dl = Hl = Wl = 0
    if lungs is not None:
        _req(lungs, "lungs")
        if lungs.dim() != 4 or lungs.shape[0] != B:
            raise ValueError("cam: lungs must be [B,Dl,Hl,Wl]")
        _, Dl, Hl, Wl = lungs.shape
    out = torch.empty((B, D, H, W), device=x.device, dtype=torch.float32)
    head = (_p(x), _p(w), _p(bias), _p(gdense), _p(gpool), _p(lungs), Dl, Hl, Wl)
    if method != "gradcam":
        _chk(_fn("dram_cam_point", sfx)(*head, _p(out), B, D, H, W, NO, int(sigmoid), CAM_METHODS[method], int(relu),
                                        _stream()), "dram_cam_point")
        return out
    nblk = _L().dram_cam_nblk(D * H * W)
    partial = torch.empty((nblk, B, NO), device=x.device, dtype=torch.float32)
    _chk(_fn("dram_cam_sum", sfx)(*head, _p(partial), B, D, H, W, NO, int(sigmoid), _stream()), "dram_cam_sum")
    sums = reduce_partials(partial)                     # [B, NO] float64; nblk <= 1 024: one block, no ticket word
    _chk(_fn("dram_cam_combine", sfx)(_p(x), _p(w), _p(sums), _p(out), B, D, H, W, NO, int(relu), _stream()),
         "dram_cam_combine")
    return out


HEAT_MODES = {"classsum": _lib.DRAM_HEAT_CLASSSUM, "plain": _lib.DRAM_HEAT_PLAIN}


def _heat_dense(dense: Tensor, name: str):
    """One head's dense maps [B,C,d,h,w] float32, e.g. a channel view of the engine's one tensor: only the innermost
    three dimensions must be contiguous -> (B, C, d, h, w, batch stride, channel stride) in elements."""
    if not isinstance(dense, Tensor) or dense.dim() != 5 or min(dense.shape) < 1:
        raise ValueError(f"{name}: dense must be a non-empty [B,C,d,h,w] tensor")
    B, C, d, h, w = (int(s) for s in dense.shape)
    if w % 4:
        raise ValueError(f"{name}: the dense grid's w must be a multiple of 4 (the scan's W of 8), got {w}")
    if 8 * d * h * w >= 2 ** 31:
        raise ValueError(f"{name}: output grids of 2^31 voxels or more are not supported")
    try:
        _req(dense[0, 0], f"{name}: dense[b, c]")           # device, dtype, contiguous [d,h,w]
    except ValueError:
        raise ValueError(f"{name}: the innermost three dimensions of dense must be contiguous") from None
    sb, sc = (int(dense.stride(0)) if B > 1 else 0), (int(dense.stride(1)) if C > 1 else 0)
    if sb < 0 or sc < 0 or sb % 4 or sc % 4 or dense.data_ptr() % 16:
        raise ValueError(f"{name}: dense must be 16-byte aligned with non-negative batch / channel strides that are "
                         "multiples of 4 elements")
    return B, C, d, h, w, sb, sc


def heat_peak(dense: Tensor) -> Tensor:
    """peak [B] float32 = max over the whole x2 trilinear up-sampled volume (align_corners=False) of
    sum_{c>=1} relu(up_c), the normaliser of the classification maps (reference models.py:217-222), taken BEFORE the
    lung mask.  dense [B,C>=2,d,h,w] float32, batch / channel strides free (see heat_volume).  One reduction pass
    (per-block maxima) and an amax over [B,nblk] as glue; the up-sampled channels are never stored."""
    B, C, d, h, w, sb, sc = _heat_dense(dense, "heat_peak")
    if C < 2:
        raise ValueError("heat_peak: the class sum runs over the channels 1..C-1: C >= 2")
    nblk = _L().dram_heat_nblk(8 * d * h * w)
    partial = torch.empty((B, nblk), device=dense.device, dtype=torch.float32)
    _chk(_L().dram_heat_peak(_p(dense), sb, sc, C, _p(partial), B, d, h, w, 2 * d, 2 * h, 2 * w, _stream()),
         "dram_heat_peak")
    return partial.amax(1)


def heat_volume(dense: Tensor, lung: Tensor, mode: str, peak: Optional[Tensor] = None, zsel=None,
                want_f32: bool = False, want_u8: bool = True):
    """The heat volume the reference's _draw_predictions draws (models.py:201-229 / :464-488), fused into one pass:
    mode "classsum": sum_{c>=1} relu(up_c) / (peak + 1e-7) * lung, `peak` from heat_peak; "plain" (C == 1): up_0 * lung;
    up = F.interpolate(dense, size=(2d,2h,2w), mode='trilinear'), recomputed from dense and never stored.

    dense [B,C,d,h,w] float32 with free batch / channel strides (`dense_all[:, :n0]` works without a copy);
    lung [B,2d,2h,2w] bool / uint8, non-zero = lung.  zsel: [B,nz] output-grid z indices in [0, 2d) (per sample,
    repeats allowed; a host sequence, or a tensor -- a device tensor is read back for the range check): the result is
    [B,nz,2h,2w], those slices of the full [B,2d,2h,2w] result bit for bit.
    -> (f32 or None, u8 or None): v unclamped, and trunc(255 * clamp(v, 0, 1)).  Every check runs before any launch."""
    if mode not in HEAT_MODES:
        raise ValueError(f"heat_volume: unknown mode {mode!r} (one of {sorted(HEAT_MODES)})")
    if not (want_f32 or want_u8):
        raise ValueError("heat_volume: nothing to write (want_f32 and want_u8 are both off)")
    B, C, d, h, w, sb, sc = _heat_dense(dense, "heat_volume")
    D, H, W = 2 * d, 2 * h, 2 * w
    if mode == "classsum":
        if C < 2:
            raise ValueError("heat_volume: 'classsum' runs over the channels 1..C-1: C >= 2")
        if peak is None:
            raise ValueError("heat_volume: 'classsum' needs the peak (heat_peak(dense))")
        _req(peak, "peak", shape=(B,))
    elif C != 1:
        raise ValueError(f"heat_volume: 'plain' takes one channel, got {C}")
    if not isinstance(lung, Tensor) or lung.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"heat_volume: lung must be bool or uint8, got {getattr(lung, 'dtype', type(lung))}")
    if tuple(lung.shape) != (B, D, H, W):
        raise ValueError(f"heat_volume: lung must be {(B, D, H, W)} (twice the dense grid), got {tuple(lung.shape)}")
    if lung.dtype == torch.bool:
        lung = lung.contiguous().view(torch.uint8)
    _req(lung, "lung", torch.uint8)
    if lung.data_ptr() % 8:                     # the kernel reads 8 mask bytes per lane
        lung = lung.clone()
    zs, nz = None, 0
    if zsel is not None:
        zh = torch.as_tensor(zsel).cpu()
        if zh.dim() != 2 or zh.shape[0] != B or zh.shape[1] < 1 or zh.is_floating_point():
            raise ValueError(f"heat_volume: zsel must be [B={B}, nz >= 1] integers, got {tuple(zh.shape)} {zh.dtype}")
        if int(zh.min()) < 0 or int(zh.max()) >= D:
            raise ValueError(f"heat_volume: zsel entries must lie in [0, {D})")
        nz = int(zh.shape[1])
        if nz * H * W >= 2 ** 31:
            raise ValueError("heat_volume: zsel selects 2^31 voxels or more")
        zs = zh.to(torch.int32).contiguous().to(dense.device)
    shape = (B, nz if zs is not None else D, H, W)
    f32 = torch.empty(shape, device=dense.device, dtype=torch.float32) if want_f32 else None
    u8 = torch.empty(shape, device=dense.device, dtype=torch.uint8) if want_u8 else None
    _chk(_L().dram_heat_volume(_p(dense), sb, sc, C, _p(lung), _p(peak), _p(zs), nz, _p(f32), _p(u8), HEAT_MODES[mode],
                               B, d, h, w, D, H, W, _stream()), "dram_heat_volume")
    return f32, u8


def segloss_fwd(cle: Tensor, pse: Tensor, lungs: Tensor, ems: Tensor, binary: Tensor,
                smoothness: float = 0.85) -> Tensor:
    """cle/pse [B,D,H,W]; lungs/ems [B,Dl,Hl,Wl]; binary [B] -> partial [nblk,6].  smoothness: the in-mask
    weight of metrics.py:24 (0.85 at the models.py:529 call site)."""
    _req(cle, "cle")
    B, D, H, W = cle.shape
    _req(pse, "pse", shape=cle.shape)
    _req(lungs, "lungs")
    _req(ems, "ems", shape=lungs.shape)
    _req(binary, "binary", shape=(B,))
    _, Dl, Hl, Wl = lungs.shape
    nblk = _L().dram_segloss_nblk(B * D * H * W)
    partial = torch.empty((nblk, 6), device=cle.device, dtype=torch.float32)
    _chk(_L().dram_segloss_fwd(_p(cle), _p(pse), _p(lungs), _p(ems), _p(binary), Dl, Hl, Wl, _p(partial), B, D, H, W,
                               float(smoothness), _stream()), "dram_segloss_fwd")
    return partial


def segloss_bwd(cle: Tensor, pse: Tensor, lungs: Tensor, ems: Tensor, binary: Tensor, coef: Tensor,
                smoothness: float = 0.85):
    B, D, H, W = cle.shape
    _req(coef, "coef", shape=(8,))
    _, Dl, Hl, Wl = lungs.shape
    gcle = torch.empty_like(cle)
    gpse = torch.empty_like(pse)
    _chk(_L().dram_segloss_bwd(_p(cle), _p(pse), _p(lungs), _p(ems), _p(binary), Dl, Hl, Wl, _p(coef), _p(gcle),
                               _p(gpse), B, D, H, W, float(smoothness), _stream()), "dram_segloss_bwd")
    return gcle, gpse


def regloss_tail(partial: Tensor, reg_cle: Tensor, reg_pse: Tensor, cle_labels: Tensor, pse_labels: Tensor,
                 cle_w: Tensor, pse_w: Tensor, cle_bands: Tensor, pse_bands: Tensor, voxels_total: int,
                 smooth: float, beta: float, gamma: float):
    """The O(B) tail of models.py:549-574 in one launch (csrc/head_loss.hip regloss_tail_kernel) ->
    out [5] (loss, loss_cle, loss_pse, mul, seg), coef [8] for segloss_bwd, greg [2,B] = d loss / d reg_outs."""
    _req(partial, "partial")
    B = reg_cle.shape[0]
    for t, n in ((reg_cle, "reg_cle"), (reg_pse, "reg_pse"), (cle_w, "cle_w"), (pse_w, "pse_w")):
        _req(t, n, shape=(B,))
    for t, n in ((cle_labels, "cle_labels"), (pse_labels, "pse_labels")):
        _req(t, n, dtype=torch.int64, shape=(B,))
    _req(cle_bands, "cle_bands")
    _req(pse_bands, "pse_bands")
    dev = partial.device
    out = torch.empty(5, device=dev, dtype=torch.float32)
    coef = torch.empty(8, device=dev, dtype=torch.float32)
    greg = torch.empty((2, B), device=dev, dtype=torch.float32)
    _chk(_L().dram_regloss_tail(_p(partial), partial.shape[0], _p(reg_cle), _p(reg_pse), _p(cle_labels),
                                _p(pse_labels), _p(cle_w), _p(pse_w), _p(cle_bands), cle_bands.shape[0],
                                _p(pse_bands), pse_bands.shape[0], B, float(voxels_total), float(smooth), float(beta),
                                float(gamma), _p(out), _p(coef), _p(greg), _stream()), "dram_regloss_tail")
    return out, coef, greg


# --------------------------------------------------------------------------- optimizer
def adam_multi(table: Tensor, chunks: Tensor, nchunks: int, lr, b1, b2, eps, wd, bc1, bc2, grad_scale):
    _chk(_L().dram_adam_multi(_p(table), _p(chunks), nchunks, lr, b1, b2, eps, wd, bc1, bc2, grad_scale, _stream()),
         "dram_adam_multi")


def adam_multi_dev(table: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor):
    """hyper: float32[7] device tensor {lr, b1, b2, eps, wd, grad_scale, step} (graph-replayable form)."""
    _req(hyper, "hyper", shape=(7,))
    _chk(_L().dram_adam_multi_dev(_p(table), _p(chunks), nchunks, _p(hyper), _stream()), "dram_adam_multi_dev")


def sgd_multi(table: Tensor, chunks: Tensor, nchunks: int, lr, momentum, wd, first_step, grad_scale):
    _chk(_L().dram_sgd_multi(_p(table), _p(chunks), nchunks, lr, momentum, wd, int(first_step), grad_scale,
                             _stream()), "dram_sgd_multi")


def _clip_arr(clip: Tensor) -> Tensor:
    return _req(clip, "clip", shape=(4,))


def grad_norm_multi(table: Tensor, chunks: Tensor, nchunks: int, partials: Tensor, clip: Tensor, grad_scale: float,
                    hyper: Optional[Tensor] = None):
    """clip[2] = |grad_scale| * ||g||_2 over every gradient of the table, clip[3] = min(1, clip[0] / (clip[2] + 1e-6));
    partials: float64 scratch, one element per chunk; hyper given: grad_scale is read from hyper[5] on the device."""
    _req(partials, "partials", dtype=torch.float64)
    if partials.numel() < nchunks:
        raise ValueError(f"partials: {nchunks} chunks need {nchunks} doubles, got {partials.numel()}")
    if hyper is not None:
        _req(hyper, "hyper", shape=(7,))
    _chk(_L().dram_grad_norm_multi(_p(table), _p(chunks), nchunks, _p(partials), _p(_clip_arr(clip)), grad_scale,
                                   _p(hyper), _stream()), "dram_grad_norm_multi")


def grad_scale_multi(table: Tensor, chunks: Tensor, nchunks: int, clip: Tensor):
    """IN PLACE g = g * clip[3] (clip[1] < 0) or clamp(g, -clip[1], clip[1]): the table's gradients are written."""
    _chk(_L().dram_grad_scale_multi(_p(table), _p(chunks), nchunks, _p(_clip_arr(clip)), _stream()),
         "dram_grad_scale_multi")


def adam_multi_clip(table: Tensor, chunks: Tensor, nchunks: int, lr, b1, b2, eps, wd, bc1, bc2, grad_scale, clip: Tensor):
    _chk(_L().dram_adam_multi_clip(_p(table), _p(chunks), nchunks, lr, b1, b2, eps, wd, bc1, bc2, grad_scale,
                                   _p(_clip_arr(clip)), _stream()), "dram_adam_multi_clip")


def adam_multi_dev_clip(table: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, clip: Tensor):
    _req(hyper, "hyper", shape=(7,))
    _chk(_L().dram_adam_multi_dev_clip(_p(table), _p(chunks), nchunks, _p(hyper), _p(_clip_arr(clip)), _stream()),
         "dram_adam_multi_dev_clip")


def sgd_multi_clip(table: Tensor, chunks: Tensor, nchunks: int, lr, momentum, wd, first_step, grad_scale, clip: Tensor):
    _chk(_L().dram_sgd_multi_clip(_p(table), _p(chunks), nchunks, lr, momentum, wd, int(first_step), grad_scale,
                                  _p(_clip_arr(clip)), _stream()), "dram_sgd_multi_clip")
