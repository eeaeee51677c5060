"""GPU-side deterministic input pipeline of the reference's ``SubtypeDataModule._transform``
(reference models.py:55-63): IntensityWindow(from_span=(-1150,-300), to_span=(0,1)) ->
Standardize() -> Interpolate(target_size, align_corners=True, only_in_plane=True); masks take the
nearest-neighbour branch with the same depth indices.  Fused HIP kernels (csrc/prep.hip): one
reduction pass for the volume statistics, one fused window/standardize/resize pass.

The train-time random augmentations of models.py:66-74 (GaussianAddictive, BoxMaskOut, Flip, CropAndResize)
run as ONE fused gather kernel per volume (`dram_augment_image` / `dram_augment_mask`): ``TrainAugment`` draws
the parameters on the host with the reference's distributions (its ``get_params``), the kernels apply them;
with given parameters they reproduce the reference classes (tests/golden/augment.npz).
"""
from __future__ import annotations

if not __package__:          # imported top-level (this directory on sys.path): bind to the package, see _dropin.py
    import _dropin
    __package__ = _dropin.adopt(__name__)

import ctypes
import dataclasses
import math
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import torch

from . import ops
from .ops import _L, _chk, _p, _req, _stream

FROM_SPAN = (-1150.0, -300.0)      # models.py:60


def depth_indices(D: int, new_d: int, device) -> torch.Tensor:
    """spatial_transforms.py:66: torch.linspace(0, original_d - 1, new_d).long()"""
    return torch.linspace(0, D - 1, new_d).long().to(torch.int32).to(device)


def prepare_image(scan: torch.Tensor, target_size: Sequence[int], from_span=FROM_SPAN) -> torch.Tensor:
    """scan: raw HU volume [D,H,W] (any real dtype, device tensor) -> float32 [Do,Ho,Wo]."""
    scan = scan.float().contiguous()
    _req(scan, "scan")
    D, H, W = scan.shape
    Do, Ho, Wo = (int(v) for v in target_size)
    n = scan.numel()
    nblk = _L().dram_window_stats_nblk(n)
    partial = torch.empty((nblk, 2), device=scan.device, dtype=torch.float32)
    lo, hi = float(from_span[0]), float(from_span[1])
    _chk(_L().dram_window_stats(_p(scan), _p(partial), n, lo, hi, _stream()), "dram_window_stats")
    s = partial.double().sum(0)                                   # O(1) glue on [nblk,2]
    mean = s[0] / n
    var = (s[1] - n * mean * mean) / (n - 1)                       # torch.std(): unbiased
    mean_inv = torch.stack([mean, var.clamp_min(0).rsqrt()]).float().contiguous()
    zidx = depth_indices(D, Do, scan.device)
    out = torch.empty((Do, Ho, Wo), device=scan.device, dtype=torch.float32)
    _chk(_L().dram_prep_image(_p(scan), _p(zidx), _p(mean_inv), _p(out), D, H, W, Do, Ho, Wo, lo, hi, _stream()),
         "dram_prep_image")
    return out


def prepare_mask(mask: torch.Tensor, target_size: Sequence[int]) -> torch.Tensor:
    """mask [D,H,W] (bool / int / float) -> same dtype [Do,Ho,Wo], nearest in-plane + depth select."""
    dtype = mask.dtype
    m = mask.float().contiguous()
    _req(m, "mask")
    D, H, W = m.shape
    Do, Ho, Wo = (int(v) for v in target_size)
    zidx = depth_indices(D, Do, m.device)
    out = torch.empty((Do, Ho, Wo), device=m.device, dtype=torch.float32)
    _chk(_L().dram_prep_mask(_p(m), _p(zidx), _p(out), D, H, W, Do, Ho, Wo, _stream()), "dram_prep_mask")
    return out.to(dtype)


def prepare_labels(labels: torch.Tensor, target_size: Sequence[int]) -> torch.Tensor:
    """labels [D,H,W] uint8 / int16 / bool (a view with unit x stride is read in place, e.g. the lung crop of the lobe
    volume) -> uint8 [Do,Ho,Wo]: ``prepare_mask``'s nearest rule, values clamped to 0..255.  The source is neither
    copied nor converted to float; ``prepare_labels(l) > 0`` equals ``prepare_mask(l > 0)`` voxel for voxel."""
    labels, code, sz, sy = ops._label_view("prepare_labels", labels, "labels")
    D, H, W = (int(v) for v in labels.shape)
    Do, Ho, Wo = (int(v) for v in target_size)
    if min(Do, Ho, Wo) < 1:
        raise ValueError(f"prepare_labels: target_size {(Do, Ho, Wo)} must be positive")
    with ops.launch_scope(labels.device):
        zidx = depth_indices(D, Do, labels.device)
        out = torch.empty((Do, Ho, Wo), device=labels.device, dtype=torch.uint8)
        _chk(_L().dram_prep_labels(_p(labels), code, sz, sy, _p(zidx), _p(out), D, H, W, Do, Ho, Wo, _stream()),
             "dram_prep_labels")
    return out


def prepare_sample(sample: Dict[str, torch.Tensor], target_size: Sequence[int]) -> Dict[str, torch.Tensor]:
    """Dict transform with the reference's keys: 'image' + '*_mask' entries (base.py dict transforms); 'lobe_labels'
    (``prepare_case(want_lobes=True)``) goes through ``prepare_labels``."""
    out = dict(sample)
    for k, v in sample.items():
        if k == "image":
            out[k] = prepare_image(v, target_size)
        elif k.endswith("_mask"):
            out[k] = prepare_mask(v, target_size)
        elif k == "lobe_labels":
            out[k] = prepare_labels(v, target_size)
    return out


# --------------------------------------------------------------------------- archive case -> training sample
_SAMPLE_KEYS = ("image", "lung_mask", "em_mask")
_MAX_SPAN = 4095                   # sum c^2 over < 2^31 voxels stays inside int64 (dram_sample_stats_i16)


def _int_span(fn: str, from_span) -> Tuple[int, int]:
    """``from_span`` as the integer pair the int16 kernels take; ValueError for anything they cannot represent."""
    lo, hi = float(from_span[0]), float(from_span[1])
    if not (lo.is_integer() and hi.is_integer()):
        raise ValueError(f"{fn}: from_span {tuple(from_span)} is not integral, which the int16 path needs: pass the "
                         "image as float (image.float()) to window it with this span")
    if not (lo < hi and hi - lo <= _MAX_SPAN and -65536 <= lo and hi <= 65536):
        raise ValueError(f"{fn}: from_span {tuple(from_span)} must satisfy lo < hi, hi - lo <= {_MAX_SPAN} and lie in "
                         "-65536..65536 on the int16 path: pass the image as float for any other span")
    return int(lo), int(hi)


def sample_window_sums(scan: torch.Tensor, from_span=FROM_SPAN) -> torch.Tensor:
    """scan: int16 device tensor of n >= 2 elements (contiguous; the base may be 2-byte aligned only) -> int64
    [nblk, 2]: per-block ``{sum c, sum c^2}``, c = clamp(x, lo, hi) - lo.  Exact; the column sums do not depend on
    how the blocks are cut.  One launch, nothing read back."""
    fn = "sample_window_sums"
    if not isinstance(scan, torch.Tensor) or scan.dtype != torch.int16:
        raise TypeError(f"{fn}: expected an int16 tensor, got {getattr(scan, 'dtype', type(scan))}")
    lo, hi = _int_span(fn, from_span)
    n = scan.numel()
    if not 2 <= n < 2 ** 31:
        raise ValueError(f"{fn}: needs 2 <= n < 2^31 elements, got {n}")
    if not scan.is_cuda:
        raise TypeError(f"{fn}: expected a device tensor (libdram_hip has no CPU path)")
    with ops.launch_scope(scan.device):
        _req(scan, "scan", torch.int16)
        partial = torch.empty((_L().dram_sample_stats_nblk(n), 2), device=scan.device, dtype=torch.int64)
        _chk(_L().dram_sample_stats_i16(_p(scan), _p(partial), n, lo, hi, _stream()), "dram_sample_stats_i16")
    return partial


def _below(image: torch.Tensor, threshold) -> torch.Tensor:
    """image < threshold; for an integer image without torch's wrap of a scalar its dtype cannot hold"""
    if image.is_floating_point():
        return image < threshold
    info, t = torch.iinfo(image.dtype), int(math.ceil(threshold))         # x < t  <=>  x < ceil(t) for an integer x
    if t > info.max:
        return torch.ones_like(image, dtype=torch.bool)
    return image < max(t, info.min)


def _sample_out(fn: str, out, shape, device):
    """The three destinations of ``prepare_archive_sample`` as (image f32, lung uint8, em uint8, returned dict)."""
    if out is None:
        img = torch.empty(shape, device=device, dtype=torch.float32)
        lung = torch.empty(shape, device=device, dtype=torch.uint8)
        em = torch.empty(shape, device=device, dtype=torch.uint8)
        return img, lung, em, {"image": img, "lung_mask": lung.view(torch.bool), "em_mask": em.view(torch.bool)}
    if not isinstance(out, dict) or any(k not in out for k in _SAMPLE_KEYS):
        raise ValueError(f"{fn}: out must be a dict with the keys {_SAMPLE_KEYS}")
    views = []
    for k in _SAMPLE_KEYS:
        t = out[k]
        want = (torch.float32,) if k == "image" else (torch.bool, torch.uint8)
        if not isinstance(t, torch.Tensor) or t.dtype not in want:
            raise TypeError(f"{fn}: out[{k!r}] must be a {' / '.join(str(w) for w in want)} tensor")
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{fn}: out[{k!r}] must be a dense {tuple(shape)} block, got shape {tuple(t.shape)} "
                             f"strides {t.stride()}")
        if t.device != device:
            raise ValueError(f"{fn}: out[{k!r}] lives on {t.device}, the case on {device}")
        views.append(t.view(torch.uint8) if t.dtype == torch.bool else t)
    return views[0], views[1], views[2], {k: out[k] for k in _SAMPLE_KEYS}


def prepare_archive_sample(image: torch.Tensor, lung_mask: torch.Tensor, target_size: Sequence[int], out=None,
                           from_span=FROM_SPAN, em_threshold=-950) -> Dict[str, torch.Tensor]:
    """One case of the training archive (dataset.py:147-155: 'image' [D,H,W] raw HU, 'lung_mask') -> the sample the
    step trains on: {'image': float32 [Do,Ho,Wo] windowed, z-scored and resized, 'lung_mask': bool, 'em_mask': bool},
    em_mask = (image < em_threshold) & (lung_mask > 0) taken at full size (dataset.py:149), both masks resized nearest.

    ``out``: optional dict of the three destinations, dense [Do,Ho,Wo] views such as ``batch[k][b]`` (masks bool or
    uint8); they are written in place and returned.

    An int16 image with a uint8 / bool / int16 mask and an integral ``from_span`` takes the fused path of
    csrc/sample_prep.hip: one exact integer statistics pass and one output pass over the int16 data, two launches plus
    O(nblk) glue, nothing read back, no full-size temporary.  Any other dtype takes the composition ``prepare_image`` +
    ``prepare_mask`` (float32 copies of the full-size volumes).  Shapes, ``target_size``, host tensors and a span the
    int16 path cannot take are refused (ValueError / TypeError) before the device is touched."""
    fn = "prepare_archive_sample"
    for t, name in ((image, "image"), (lung_mask, "lung_mask")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{fn}: {name} must be a tensor, got {type(t)}")
    if image.dim() != 3 or min(image.shape) < 1 or tuple(image.shape) != tuple(lung_mask.shape):
        raise ValueError(f"{fn}: image {tuple(image.shape)} and lung_mask {tuple(lung_mask.shape)} must be one "
                         "non-empty [D,H,W] shape")
    try:
        target = tuple(int(v) for v in target_size)
        if any(t != v for t, v in zip(target, target_size)):
            target = ()
    except (TypeError, ValueError):
        target = ()
    if len(target) != 3 or min(target) < 1:
        raise ValueError(f"{fn}: target_size must be three positive integers, got {target_size!r}")
    if image.numel() >= 2 ** 31 or target[0] * target[1] * target[2] >= 2 ** 31:
        raise ValueError(f"{fn}: volumes of 2^31 voxels or more are not supported")
    if image.numel() < 2:
        raise ValueError(f"{fn}: the statistics need at least two voxels")
    fused = image.dtype == torch.int16 and lung_mask.dtype in (torch.uint8, torch.bool, torch.int16)
    if image.dtype == torch.int16:
        lo, hi = _int_span(fn, from_span)
    if not (image.is_cuda and lung_mask.is_cuda) or image.device != lung_mask.device:
        raise TypeError(f"{fn}: image and lung_mask must be tensors on one device (libdram_hip has no CPU path)")
    o_img, o_lung, o_em, ret = _sample_out(fn, out, target, image.device)
    if not fused:
        o_img.copy_(prepare_image(image, target, from_span))
        lung = lung_mask > 0
        o_lung.copy_(prepare_mask(lung, target))
        o_em.copy_(prepare_mask(_below(image, em_threshold) & lung, target))
        return ret
    D, H, W = (int(v) for v in image.shape)
    n = image.numel()
    thr = max(-32768, min(32768, int(math.ceil(em_threshold))))       # x < t  <=>  x < ceil(t) for an integer x
    with ops.launch_scope(image.device):
        scan = _req(image.contiguous(), "image", torch.int16)
        lung = lung_mask.contiguous()
        if lung.dtype == torch.bool:
            lung = lung.view(torch.uint8)
        _req(lung, "lung_mask", lung.dtype)
        s = sample_window_sums(scan, (lo, hi)).sum(0).double()        # exact int64 column sums -> float64 glue
        span = float(hi - lo)
        mean = s[0] / n / span
        var = (s[1] - s[0] * s[0] / n) / (n - 1) / (span * span)       # torch.std(): unbiased
        mean_inv = torch.stack([mean, var.clamp_min(0).rsqrt()]).float().contiguous()
        zidx = depth_indices(D, target[0], image.device)
        _chk(_L().dram_prep_sample_i16(_p(scan), _p(lung), 2 if lung.dtype == torch.int16 else 1, _p(zidx), _p(mean_inv),
                                       _p(o_img), _p(o_lung), _p(o_em), D, H, W, *target, lo, hi, thr, _stream()),
             "dram_prep_sample_i16")
    return ret


# --------------------------------------------------------------------------- scan + lobes -> prepared predict case
def _lobes_operand(lobes: torch.Tensor):
    """(tensor the kernels read, its lobe_dtype code): uint8 / bool and int16 volumes are read as they are, anything
    else is reduced to its `> 0` mask first (one torch pass)."""
    if lobes.dtype == torch.bool:
        lobes = lobes.contiguous().view(torch.uint8)
    elif lobes.dtype not in (torch.uint8, torch.int16):
        lobes = (lobes > 0).view(torch.uint8)
    lobes = lobes.contiguous()
    if lobes.data_ptr() % 16:                   # dram_lung_bbox reads 16-byte vectors
        lobes = lobes.clone()
    return lobes, (2 if lobes.dtype == torch.int16 else 1)


def prepare_case(scan: torch.Tensor, lobes: torch.Tensor, spacing: Sequence[float], crop_border: float = 5,
                 dilate_iterations: int = 2, fill_value: int = -2048, ess_threshold: int = -910,
                 want_original: bool = False, uid=None, want_lobes: bool = False) -> Dict[str, object]:
    """The reference's ``SubtypingInference.get_data`` (dataset.py:57-92) with ``utils.find_crops`` (utils.py:53-63) on
    the device: lung = lobes > 0; the scan outside ``dilate_iterations`` dilations of the lung (full 3x3x3 structure)
    is set to ``fill_value``; scan, lung and (``want_original``) the untouched scan are cropped to the lung's bounding
    box padded by ``ceil(crop_border / spacing)`` voxels per axis and clipped to the volume (``crop_border <= 0``: the
    tight box); ess_mask = (scan < ess_threshold) & lung.

    scan, lobes: device tensors [D,H,W]; spacing in array-axis order (z, y, x), as the reference's ``read_image``
    returns it.  A scan that is not int16 is converted with ``.to(torch.int16)`` first (the reference's
    ``astype(np.int16)``) and the threshold applies to the converted values.  Returns the reference's keys: 'image'
    int16, 'lung_mask' / 'ess_mask' bool, 'original_image' int16 (only when asked), 'crop_slice' int64 [3,2] and
    'original_size' int64 [3] (host tensors), 'uid'.  The dict feeds ``prepare_sample`` unchanged.  ``want_lobes`` adds
    'lobe_labels': the crop of the lobe volume itself, a VIEW (uint8 / int16 / bool lobes are not copied; any other
    integer type is clamped to 0..255 as uint8 first, floating-point lobes are refused), which ``prepare_sample`` resizes
    with ``prepare_labels`` -- so that ``lobe_labels > 0`` is the resized 'lung_mask' voxel for voxel.

    The bounding box is read back to the host once per case, because the sizes of the outputs depend on it: the call
    synchronises with the device and cannot be captured into a hipGraph.  Raises IndexError for an empty lung (as
    the reference's ``find_objects(...)[0]`` does) and ValueError when scan and lobes differ in shape."""
    for t, name in ((scan, "scan"), (lobes, "lobes")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"prepare_case: {name}: expected a device tensor (libdram_hip has no CPU path)")
    if scan.dim() != 3 or tuple(scan.shape) != tuple(lobes.shape):
        raise ValueError(f"prepare_case: scan {tuple(scan.shape)} and lobes {tuple(lobes.shape)} must be one [D,H,W] shape")
    if scan.numel() >= 2 ** 31:
        raise ValueError("prepare_case: volumes of 2^31 voxels or more are not supported")
    r = int(dilate_iterations)
    if not 0 <= r <= 3:
        raise ValueError("prepare_case: dilate_iterations must be 0..3")
    sp = [float(v) for v in spacing]
    if len(sp) != 3:
        raise ValueError("prepare_case: spacing must have three entries (z, y, x)")
    scan = scan.to(torch.int16).contiguous()
    _req(scan, "scan", torch.int16)
    if want_lobes and lobes.dtype not in (torch.bool, torch.uint8, torch.int16):
        if lobes.is_floating_point():
            raise TypeError("prepare_case: want_lobes needs integer lobe labels")
        lobes = lobes.clamp(0, 255).to(torch.uint8)
    lobes, code = _lobes_operand(lobes)
    _req(lobes, "lobes", lobes.dtype)
    D, H, W = (int(v) for v in scan.shape)
    dev = scan.device
    partial = torch.empty((_L().dram_lung_bbox_nblk(scan.numel()), 8), device=dev, dtype=torch.int32)
    box = torch.empty((8,), device=dev, dtype=torch.int32)
    _chk(_L().dram_lung_bbox(_p(lobes), code, _p(partial), _p(box), D, H, W, _stream()), "dram_lung_bbox")
    b = box.tolist()                                              # the one host read-back
    if b[6] == 0:
        raise IndexError("prepare_case: the lobe segmentation holds no lung voxel")
    sl = []
    for (lo, hi), size, s in zip((b[0:2], b[2:4], b[4:6]), (D, H, W), sp):
        pad = int(math.ceil(crop_border / s)) if crop_border > 0 else 0
        sl.append((max(0, lo - pad), min(size, hi + pad)))
    (z0, z1), (y0, y1), (x0, x1) = sl
    shape = (z1 - z0, y1 - y0, x1 - x0)
    image = torch.empty(shape, device=dev, dtype=torch.int16)
    lung = torch.empty(shape, device=dev, dtype=torch.uint8)
    ess = torch.empty(shape, device=dev, dtype=torch.uint8)
    orig = torch.empty(shape, device=dev, dtype=torch.int16) if want_original else None
    _chk(_L().dram_case_prepare(_p(scan), _p(lobes), code, _p(image), _p(lung), _p(ess), _p(orig), D, H, W, z0, y0, x0,
                                *shape, r, int(fill_value), int(math.ceil(ess_threshold)), _stream()), "dram_case_prepare")
    out = {"image": image, "lung_mask": lung.view(torch.bool), "ess_mask": ess.view(torch.bool),
           "crop_slice": torch.tensor(sl, dtype=torch.int64), "original_size": torch.tensor([D, H, W], dtype=torch.int64),
           "uid": uid}
    if want_original:
        out["original_image"] = orig
    if want_lobes:
        out["lobe_labels"] = lobes[z0:z1, y0:y1, x0:x1]
    return out


# --------------------------------------------------------------------------- train-time augmentations
def _frac_box(center, size, shape):
    """integer box of BoxMaskOut / CropAndResize (intensity_transforms.py:226-235, spatial_transforms.py:172-177)"""
    return [(max(0, int(mc * ds) - int(ms * ds) // 2), min(int(mc * ds) + (int(ms * ds) - int(ms * ds) // 2), ds))
            for mc, ds, ms in zip(center, shape, size)]


@dataclass
class AugmentParams:
    """One draw of the train-time transforms (None / empty = that transform is not applied).  ``smooth_sigma`` is no
    field of the C struct: ``augment_image`` runs GaussianSmooth as a call of its own between the boxes and the flip."""
    noise_sigma: Optional[float] = None                                   # GaussianAddictive
    box_centers: List[Tuple[float, float, float]] = field(default_factory=list)   # BoxMaskOut
    box_sizes: List[Tuple[float, float, float]] = field(default_factory=list)
    smooth_sigma: Optional[float] = None                                  # GaussianSmooth (voxels, isotropic)
    flip_dims: Tuple[int, ...] = ()                                       # Flip (axes of the [D,H,W] volume)
    crop_center: Optional[Tuple[float, float, float]] = None              # CropAndResize
    crop_size: Optional[Tuple[float, float, float]] = None

    def to_struct(self, shape) -> "ops._lib.DramAugment":
        a = ops._lib.DramAugment()
        flags = 0
        if self.noise_sigma is not None:
            flags |= 1
            a.sigma = float(self.noise_sigma)
        if self.box_centers:
            if len(self.box_centers) > 10:
                raise ValueError("BoxMaskOut: at most 10 boxes (reference n_masks=(1, 10))")
            flags |= 2
            a.n_boxes = len(self.box_centers)
            for b, (c, sz) in enumerate(zip(self.box_centers, self.box_sizes)):
                (z0, z1), (y0, y1), (x0, x1) = _frac_box(c, sz, shape)
                for k, v in enumerate((z0, z1, y0, y1, x0, x1)):
                    a.boxes[b][k] = v
        if self.flip_dims:
            flags |= 4
            a.flip_axes = sum(1 << int(d) for d in set(self.flip_dims))
        if self.crop_center is not None:
            flags |= 8
            for k, ((lo, hi), n) in enumerate(zip(_frac_box(self.crop_center, self.crop_size, shape), shape)):
                # torch: as_tensor(int box) / as_tensor(size) in float32
                a.box_lo[k] = float(np.float32(lo) / np.float32(n))
                a.box_hi[k] = float(np.float32(hi) / np.float32(n))
        a.flags = flags
        return a


def augment_image(image: torch.Tensor, params: AugmentParams, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """image [D,H,W] float32 device tensor -> augmented copy.  `noise` [D,H,W]: the N(0,1) draw of
    GaussianAddictive (drawn on the device when omitted).

    With ``params.smooth_sigma`` set the reference's order (models.py:66-74) takes three calls, each with its own
    transforms only: the fused kernel with noise + boxes, ``ops.gaussian_filter3d(mode='zero')`` (GaussianSmooth:
    functional.py:54-64), the fused kernel with flip + crop; a call whose transforms are all off is skipped.  The
    split is exact: noise and boxes act at the source voxel, flip and crop only move the gather, so without the
    smoothing the two fused calls compose to the single one that is issued then, as before."""
    if params.smooth_sigma is not None:
        head = dataclasses.replace(params, smooth_sigma=None, flip_dims=(), crop_center=None, crop_size=None)
        tail = dataclasses.replace(params, smooth_sigma=None, noise_sigma=None, box_centers=[], box_sizes=[])
        image = image.float().contiguous()
        _req(image, "image")
        if head.to_struct(image.shape).flags:
            image = augment_image(image, head, noise)
        image = ops.gaussian_filter3d(image, float(params.smooth_sigma), mode="zero")
        if tail.to_struct(image.shape).flags:
            image = augment_image(image, tail)
        return image
    image = image.float().contiguous()
    _req(image, "image")
    D, H, W = image.shape
    a = params.to_struct(image.shape)
    mm = None
    if a.flags & 1:
        if noise is None:
            noise = torch.randn(image.shape, device=image.device)
        _req(noise, "noise", shape=image.shape)
        nblk = _L().dram_minmax_nblk(image.numel())
        part = torch.empty((nblk, 2), device=image.device, dtype=torch.float32)
        _chk(_L().dram_minmax(_p(image), _p(part), image.numel(), _stream()), "dram_minmax")
        mm = torch.stack([part[:, 0].amin(), part[:, 1].amax()]).contiguous()     # O(nblk) glue
    out = torch.empty_like(image)
    _chk(_L().dram_augment_image(_p(image), _p(noise), _p(mm), _p(out), D, H, W, ctypes.byref(a), _stream()),
         "dram_augment_image")
    return out


def augment_mask(mask: torch.Tensor, params: AugmentParams) -> torch.Tensor:
    """mask [D,H,W] -> Flip + CropAndResize(nearest) with the same parameters (DualTransform semantics; the
    image-only transforms, ``smooth_sigma`` among them, leave a mask alone)."""
    dtype = mask.dtype
    m = mask.float().contiguous()
    _req(m, "mask")
    D, H, W = m.shape
    a = params.to_struct(m.shape)
    if not (a.flags & 12):
        return mask
    out = torch.empty_like(m)
    _chk(_L().dram_augment_mask(_p(m), _p(out), D, H, W, ctypes.byref(a), _stream()), "dram_augment_mask")
    return out.to(dtype)


class TrainAugment:
    """The augmentation list of models.py:66-74 with the reference's probabilities and parameter ranges:
    GaussianAddictive(p=.5, sigma (0.03, 0.06)), BoxMaskOut(p=.5, 1-10 boxes, centres (0.2, 0.8), sizes
    (0.01, 0.06)), Flip(p=.5, 1-2 of the 3 axes), CropAndResize(p=.5, centre (0.45, 0.55), size (0.95, 1.0)).
    Parameters are drawn on the host like the reference's get_params (same distributions; the streams of
    Python's / numpy's global generators are not reproduced).

    ``smooth_p`` > 0 switches on the list's commented-out GaussianSmooth (models.py:68) between BoxMaskOut and Flip:
    with probability ``smooth_p`` a sigma from ``smooth_sigma`` (voxels; the reference's (0.3, 0.6)).  Its two draws
    are made only then: at the default 0.0 the random stream is consumed exactly as without the argument, and
    ``smooth_sigma`` is neither drawn from nor checked (with ``smooth_p`` > 0: ValueError unless 0 <= lo <= hi and the
    radius of hi is at most 16)."""

    def __init__(self, p: float = 0.5, rng: Optional[random.Random] = None, smooth_p: float = 0.0,
                 smooth_sigma: Tuple[float, float] = (0.3, 0.6)):
        self.p = p
        self.rng = rng or random.Random()
        self.smooth_p = float(smooth_p)
        self.smooth_sigma = tuple(float(v) for v in smooth_sigma)
        if self.smooth_p > 0:                                          # off: the range is never drawn from, nor checked
            if len(self.smooth_sigma) != 2 or not 0 <= self.smooth_sigma[0] <= self.smooth_sigma[1]:
                raise ValueError(f"TrainAugment: smooth_sigma must be a range 0 <= lo <= hi, got {smooth_sigma!r}")
            ops.gaussian_taps(self.smooth_sigma[1])                    # the radius cap, before any draw

    def draw(self) -> AugmentParams:
        r, ap = self.rng, AugmentParams()
        if r.random() < self.p:
            ap.noise_sigma = r.uniform(0.03, 0.06)
        if r.random() < self.p:
            n = r.randint(1, 10)
            ap.box_centers = [tuple(r.uniform(0.2, 0.8) for _ in range(3)) for _ in range(n)]
            ap.box_sizes = [tuple(r.uniform(0.01, 0.06) for _ in range(3)) for _ in range(n)]
        if self.smooth_p > 0 and r.random() < self.smooth_p:
            ap.smooth_sigma = r.uniform(*self.smooth_sigma)
        if r.random() < self.p:
            ap.flip_dims = tuple(r.sample(range(3), r.randint(1, 2)))      # np.random.randint(1, 3) axes
        if r.random() < self.p:
            ap.crop_center = tuple(r.uniform(0.45, 0.55) for _ in range(3))
            ap.crop_size = tuple(r.uniform(0.95, 1.0) for _ in range(3))
        return ap

    def __call__(self, sample: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        ap = self.draw()
        out = dict(sample)
        for k, v in sample.items():
            if k == "image":
                out[k] = augment_image(v, ap)
            elif k.endswith("_mask"):
                out[k] = augment_mask(v, ap)
        return out
