"""Predict-path post-processing of the reference's ``processor.py`` (grand-challenge entrypoint) on the GPU.

reference processor.py:97-177: merge the ``predict_step`` outputs, resize every dRAM volume to its lung-crop
size (trilinear, align_corners=True), paste it into a zero volume of the original scan grid (:111-129),
derive the severity score from the lesion percentage (:34-38, :130-136) and write the json reports
(:160-177).  The resize + paste (+ the uint8 windowing of :143) is one gather kernel over the original grid
(``dram_resample_paste``); ``.mha`` writing (SimpleITK, :146-158) stays with the caller.
"""
from __future__ import annotations

if not __package__:          # imported top-level (this directory on sys.path): bind to the package, see _dropin.py
    import _dropin
    __package__ = _dropin.adopt(__name__)

import json
import math
import re
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import ops, transforms
from .models import CLE_RATIO_MAP, PSE_RATIO_MAP
from .ops import _L, _chk, _p, _req, _stream


def ratio_to_label(ratio: float, ratio_mapping: Dict[int, tuple]) -> int:
    """processor.py:34-38: the class whose [lo, hi) band holds the ratio."""
    for label, (lo, hi) in ratio_mapping.items():
        if lo <= ratio < hi:
            return label
    raise IndexError(f"ratio {ratio} is outside every band")       # the reference raises IndexError here too


def resample_paste(dense: torch.Tensor, crop_slice, original_size: Sequence[int], want_f32: bool = True,
                   want_u8: bool = False):
    """dense [D,H,W] (one sample of predict_step's *_dense_outs) -> (full f32 [Do,Ho,Wo] | None, full uint8 | None).
    crop_slice [[z0,z1],[y0,y1],[x0,x1]] (tensor or nested list); processor.py:111-129, :143."""
    dense = dense.float().contiguous()
    _req(dense, "dense")
    if dense.dim() != 3:
        raise ValueError("resample_paste: dense must be [D,H,W]")
    cs = [[int(v) for v in row] for row in (crop_slice.tolist() if torch.is_tensor(crop_slice) else crop_slice)]
    Do, Ho, Wo = (int(v) for v in (original_size.tolist() if torch.is_tensor(original_size) else original_size))
    (z0, z1), (y0, y1), (x0, x1) = cs
    if not (0 <= z0 < z1 <= Do and 0 <= y0 < y1 <= Ho and 0 <= x0 < x1 <= Wo):
        raise ValueError(f"crop_slice {cs} does not fit the original size {(Do, Ho, Wo)}")
    D, H, W = dense.shape
    of = torch.empty((Do, Ho, Wo), device=dense.device, dtype=torch.float32) if want_f32 else None
    ob = torch.empty((Do, Ho, Wo), device=dense.device, dtype=torch.uint8) if want_u8 else None
    _chk(_L().dram_resample_paste(_p(dense), _p(of), _p(ob), D, H, W, z1 - z0, y1 - y0, x1 - x0, z0, y0, x0, Do, Ho, Wo,
                                  _stream()), "dram_resample_paste")
    return of, ob


def _region_key(names, label: int) -> str:
    """``names[label]`` (a mapping or a sequence indexed by the label) or else the label as a string, the form json
    gives it: the key of one region in every per-region dict of the report."""
    try:
        return str(names[label]) if names is not None else str(label)
    except (KeyError, IndexError):
        return str(label)


def _fmt(v, spec: str, cast=float, unsigned_zero: bool = False) -> Optional[str]:
    """One number of the report: None (json null) for None or NaN, else ``spec.format(cast(v))``; ``unsigned_zero``: a
    value that prints as zero prints without a sign ("-0.000" reads "0.000")."""
    if v is None or (isinstance(v, float) and math.isnan(v)):
        return None
    s = spec.format(cast(v))
    return s.lstrip("-") if unsigned_zero and float(s) == 0 else s


def _lst(v):
    return v.tolist() if hasattr(v, "tolist") else v              # tensors, arrays and their scalars


def _column_metrics(caller: str, cols, names=None, unsigned_zero: bool = False) -> dict:
    """cols [(stem, values of the rows 0..n_regions, whole-lung value, spec, cast)] -> every '{stem}_per_region' dict
    (rows 1..n, keyed through ``names``), then every '{stem}_per_lung' value, all through ``_fmt``."""
    out = {}
    for stem, per_row, _, spec, cast in cols:
        if len(per_row) < 2:
            raise ValueError(f"{caller}: the result must hold rows 0..n_regions")
        out[f"{stem}_per_region"] = {_region_key(names, label): _fmt(per_row[label], spec, cast, unsigned_zero)
                                     for label in range(1, len(per_row))}
    for stem, _, whole, spec, cast in cols:
        out[f"{stem}_per_lung"] = _fmt(whole, spec, cast, unsigned_zero)
    return out


REGION_KEYS = ("cle_lesion_percentage_per_region", "cle_severity_score_per_region", "pse_lesion_percentage_per_region",
               "pse_severity_score_per_region", "region_voxels", "region_ess_fraction")


def region_metrics(table_row, names=None) -> dict:
    """One sample's region table [n+1, 4] (predict_step's 'region_table'[b]: rows 0..n of sum cle, sum pse, #ess,
    #voxels) -> the regional entries of the metrics dict, in the formats of the per-lung ones: per region the lesion
    percentage sum / #voxels ("{:.3f}"), its severity score (``ratio_to_label`` on the same bands, "{:d}"), the voxel
    count ("{:d}") and the share of the region below the ess threshold ("{:.3f}").  Each value is a dict keyed by
    ``names[label]`` (a mapping or a sequence indexed by the label) or else by the label as a string, the form json
    gives it.  A region without voxels has None (json null) for everything but its count.  Pure host code."""
    rows = table_row.tolist() if torch.is_tensor(table_row) else [list(r) for r in table_row]
    if len(rows) < 2 or any(len(r) != 4 for r in rows):
        raise ValueError("region_metrics: table_row must be [n_regions + 1, 4]")
    out = {k: {} for k in REGION_KEYS}
    for label in range(1, len(rows)):
        key = _region_key(names, label)
        s_cle, s_pse, n_ess, n_vox = (float(v) for v in rows[label])
        present = n_vox > 0
        for head, s, rmap in (("cle", s_cle, CLE_RATIO_MAP), ("pse", s_pse, PSE_RATIO_MAP)):
            pct = s / n_vox if present else None
            out[f"{head}_lesion_percentage_per_region"][key] = "{:.3f}".format(pct) if present else None
            out[f"{head}_severity_score_per_region"][key] = "{:d}".format(ratio_to_label(pct, rmap)) if present else None
        out["region_voxels"][key] = "{:d}".format(int(round(n_vox)))
        out["region_ess_fraction"][key] = "{:.3f}".format(n_ess / n_vox) if present else None
    return out


# --------------------------------------------------------------------------- per-lobe CT densitometry
_DENSITO_KEY = re.compile(r"(laa\d+_fraction|perc\d+_hu|mean_lung_density|volume_ml)_per_(region|lung)"
                          r"|local_laa\d+_(mean|sd|p\d+|above\d+)_per_(region|lung)|local_mm|local_window_voxels")


def densitometry_from_hist(hist: torch.Tensor, sums: torch.Tensor, spacing: Sequence[float],
                           thresholds: Sequence[int] = (-950, -910), percentiles: Sequence[int] = (15,),
                           hu_lo: int = -1024) -> dict:
    """The tensor math of ``densitometry``: ``ops.lobe_histogram``'s (hist [n+1, nbins], sums [n+1, 2]) int64 -> the
    result dict, O(rows * bins) torch operations on the tensors' own device (CPU tensors work), integer or float64
    arithmetic, nothing read back."""
    if hist.dim() != 2 or sums.dim() != 2 or hist.dtype != torch.int64 or sums.dtype != torch.int64 or \
            hist.shape[0] < 2 or tuple(sums.shape) != (hist.shape[0], 2):
        raise ValueError("densitometry: hist must be int64 [n_regions + 1, nbins] and sums int64 [n_regions + 1, 2]")
    sp = [float(v) for v in spacing]
    if len(sp) != 3:
        raise ValueError("densitometry: spacing must have three entries (z, y, x)")
    nbins, lo = int(hist.shape[1]), int(hu_lo)
    ts = [int(math.ceil(t)) for t in thresholds]           # #(hu < t) on integer HU = #(hu <= ceil(t) - 1)
    for t in ts:
        if not lo < t <= lo + nbins - 1:
            raise ValueError(f"densitometry: threshold {t} is outside ({lo}, {lo + nbins - 1}]: its count would not be exact")
    ps = list(percentiles)
    for p in ps:
        if int(p) != p or not 1 <= int(p) <= 99:
            raise ValueError(f"densitometry: percentiles are integers in 1..99, got {p}")
    ps = [int(p) for p in ps]
    h = torch.cat([hist, hist.sum(0, keepdim=True)])       # the last row: the whole lung
    s = torch.cat([sums, sums.sum(0, keepdim=True)])
    vox = s[:, 0]
    voxd = vox.double()
    cdf = h.cumsum(1)                                      # #(clamped hu <= hu_lo + bin)
    counts = torch.stack([cdf[:, t - 1 - lo] for t in ts]) if ts else h.new_zeros((0, h.shape[0]))
    perc = torch.full((len(ps), h.shape[0]), float("nan"), dtype=torch.float64, device=h.device)
    for i, p in enumerate(ps):
        k = ((vox * p + 99) // 100).clamp_min(1)           # nearest rank: max(1, ceil(p N / 100))
        idx = (cdf < k[:, None]).sum(1)                    # the first bin whose cumulative count reaches k
        ok = (vox > 0) & (idx > 0) & (idx < nbins - 1)     # an end bin holds a tail: the value is only a bound
        perc[i] = torch.where(ok, (idx + lo).double(), perc[i])
    full = {"voxels": vox, "volume_ml": voxd * (sp[0] * sp[1] * sp[2]) / 1000.0, "mean_density": s[:, 1].double() / voxd,
            "laa": counts.double() / voxd, "laa_counts": counts, "perc": perc}
    out = {k: v[..., :-1] for k, v in full.items()}
    out["whole_lung"] = {k: v[..., -1] for k, v in full.items()}
    out["thresholds"], out["percentiles"], out["hu_lo"], out["nbins"] = tuple(ts), tuple(ps), lo, nbins
    return out


def densitometry(image: torch.Tensor, labels: torch.Tensor, spacing: Sequence[float], n_regions: int = 5,
                 thresholds: Sequence[int] = (-950, -910), percentiles: Sequence[int] = (15,), hu_lo: int = -1024,
                 nbins: int = 1024) -> dict:
    """CT densitometry per lobe from ONE histogram pass (``ops.lobe_histogram``) over image [D,H,W] int16 HU and labels
    [D,H,W] (``prepare_case(want_lobes=True)``'s 'image' and 'lobe_labels', at the scan's own resolution); spacing in
    (z, y, x) mm.  Device tensors, rows 0..n_regions (row 0: lung voxels whose label is above n_regions; a label <= 0
    is not lung):
      'voxels' [n+1] int64; 'volume_ml' [n+1] float64 = voxels * sz*sy*sx / 1000; 'mean_density' [n+1] float64 (NaN for
      an empty row); 'laa' [len(thresholds), n+1] float64 = #(hu < t) / voxels and 'laa_counts' (int64), every t in
      (hu_lo, hu_lo + nbins - 1] so that the prefix sum is exact (else ValueError); 'perc' [len(percentiles), n+1]
      float64: the smallest integer HU h with #(hu <= h) >= max(1, ceil(p N / 100)) (inverted CDF, nearest rank; p an
      integer in 1..99), NaN for an empty row and where h falls in either end bin (the value is then only a bound);
      'whole_lung': the same quantities over the sum of all rows.
    Nothing is read back; ``densitometry_metrics`` formats the result on the host."""
    hist, sums = ops.lobe_histogram(image, labels, n_regions, hu_lo, nbins)
    return densitometry_from_hist(hist, sums, spacing, thresholds, percentiles, hu_lo)


def densitometry_metrics(result: dict, names=None) -> dict:
    """``densitometry``'s result -> entries of the metrics dict, beside ``region_metrics`` and keyed like it
    (``names[label]`` of a mapping or sequence, else the label as a string): 'laa{|t|}_fraction_per_region' per
    threshold and 'mean_lung_density_per_region' ("{:.3f}"), 'perc{p}_hu_per_region' ("{:d}"), 'volume_ml_per_region'
    ("{:.1f}"), and their whole-lung twins ending '_per_lung' (one value each).  None (json null) stands for NaN.
    Row 0 is not reported as a region.  Pure host code."""
    ts, ps = list(result["thresholds"]), list(result["percentiles"])
    lung = result["whole_lung"]
    laa, perc, lung_laa, lung_perc = (_lst(v) for v in (result["laa"], result["perc"], lung["laa"], lung["perc"]))
    cols = [(f"laa{abs(t)}_fraction", laa[i], lung_laa[i], "{:.3f}", float) for i, t in enumerate(ts)]
    cols += [(f"perc{p}_hu", perc[i], lung_perc[i], "{:d}", int) for i, p in enumerate(ps)]
    cols += [("mean_lung_density", _lst(result["mean_density"]), _lst(lung["mean_density"]), "{:.3f}", float),
             ("volume_ml", _lst(result["volume_ml"]), _lst(lung["volume_ml"]), "{:.1f}", float)]
    return _column_metrics("densitometry_metrics", cols, names)        # a mean of -0.0004 keeps its sign: "-0.000"


# --------------------------------------------------------------------------- local LAA map (rides the densitometry section)
LOCAL_NBINS = 1024                                   # the histogram of the per-mille map: bins 0..1000 hold every value
_LOCAL_KW = ("n_regions", "threshold", "cuts", "percentiles")


def local_laa_params(fn: str, threshold=-950, cuts: Sequence[float] = (0.10, 0.25, 0.50),
                     percentiles: Sequence[int] = (50, 90)) -> Tuple[int, Tuple[int, ...], Tuple[int, ...]]:
    """(threshold, cuts in whole per cent, percentiles) of ``local_laa`` as ints; ValueError for a threshold that is no
    integer in -32768..32768, a cut that is not a whole per cent in 1..100 (given as a fraction: 0.10, 0.25, ...) and a
    percentile that is no integer in 1..99.  Pure host code."""
    threshold = ops._hu_threshold(fn, threshold)
    cs = []
    for c in cuts:
        pct = round(float(c) * 100.0) if isinstance(c, (int, float)) and not isinstance(c, bool) and math.isfinite(c) else 0
        if not 1 <= pct <= 100 or abs(float(c) * 100.0 - pct) > 1e-9:
            raise ValueError(f"{fn}: cuts are fractions of a whole per cent in 0.01..1.00, got {c!r}")
        cs.append(int(pct))
    ps = []
    for p in percentiles:
        if isinstance(p, bool) or not isinstance(p, (int, float)) or int(p) != p or not 1 <= int(p) <= 99:
            raise ValueError(f"{fn}: percentiles are integers in 1..99, got {p!r}")
        ps.append(int(p))
    return threshold, tuple(cs), tuple(ps)


def local_laa_from_hist(hist: torch.Tensor, sums: torch.Tensor, cuts: Sequence[float] = (0.10, 0.25, 0.50),
                        percentiles: Sequence[int] = (50, 90)) -> dict:
    """The tensor math of ``local_laa``: ``ops.lobe_histogram(map, labels, n, hu_lo=0, nbins=1024)``'s (hist [n+1, nbins],
    sums [n+1, 2]) int64 of the per-mille map q -> per row 0..n, as fractions (q / 1000):
      'voxels' [n+1] int64; 'mean' float64 = sum q / (1000 N), both exact integers before the one division; 'sd' float64,
      the population standard deviation, from the int64 moments sum h_b (b - m) and sum h_b (b - m)^2 about the rounded
      mean bin m (no cancellation); 'perc' [len(percentiles), n+1] float64: the smallest value whose cumulative count
      reaches max(1, ceil(p N / 100)) -- the nearest-rank rule of ``densitometry_from_hist``, but bin 0 and bin 1000 are
      values here, not tails; 'above' [len(cuts), n+1] float64 = #(q >= round(cut * 1000)) / N and 'above_counts' (int64);
      NaN for a row without voxels; 'whole_lung': the same over the sum of all rows.
    O(rows * bins) torch operations on the tensors' own device (CPU tensors work), nothing read back."""
    if hist.dim() != 2 or sums.dim() != 2 or hist.dtype != torch.int64 or sums.dtype != torch.int64 or \
            hist.shape[0] < 2 or hist.shape[1] < 1001 or tuple(sums.shape) != (hist.shape[0], 2):
        raise ValueError("local_laa: hist must be int64 [n_regions + 1, nbins >= 1001] and sums int64 [n_regions + 1, 2]")
    _, cs, ps = local_laa_params("local_laa", -950, cuts, percentiles)
    h = torch.cat([hist, hist.sum(0, keepdim=True)])       # the last row: the whole lung
    s = torch.cat([sums, sums.sum(0, keepdim=True)])
    vox, tot = s[:, 0], s[:, 1]
    voxd = vox.double()
    nan = torch.full_like(voxd, float("nan"))
    some = vox > 0
    mean = tot.double() / (vox * 1000).double()            # 0 / 0 = NaN for an empty row
    b = torch.arange(h.shape[1], dtype=torch.int64, device=h.device)
    m = (2 * tot + vox) // (2 * vox.clamp_min(1))          # the mean bin, rounded
    d = b[None, :] - m[:, None]
    m1, m2 = (h * d).sum(1).double() / voxd, (h * d * d).sum(1).double() / voxd
    sd = torch.where(some, (m2 - m1 * m1).clamp_min(0.0).sqrt() / 1000.0, nan)
    cdf = h.cumsum(1)
    perc = torch.full((len(ps), h.shape[0]), float("nan"), dtype=torch.float64, device=h.device)
    # bin -> fraction, divided on the host: a percentile is then the same float64 on every device
    value = (torch.arange(h.shape[1], dtype=torch.float64) / 1000.0).to(h.device)
    for i, p in enumerate(ps):
        k = ((vox * p + 99) // 100).clamp_min(1)           # nearest rank: max(1, ceil(p N / 100))
        idx = (cdf < k[:, None]).sum(1)                    # the first bin whose cumulative count reaches k
        perc[i] = torch.where(some, value[idx.clamp_max(h.shape[1] - 1)], perc[i])
    counts = torch.stack([vox - cdf[:, 10 * c - 1] for c in cs]) if cs else h.new_zeros((0, h.shape[0]))
    full = {"voxels": vox, "mean": mean, "sd": sd, "perc": perc, "above": counts.double() / voxd, "above_counts": counts}
    out = {k: v[..., :-1] for k, v in full.items()}
    out["whole_lung"] = {k: v[..., -1] for k, v in full.items()}
    out["cuts"], out["percentiles"] = tuple(c / 100.0 for c in cs), ps
    return out


def local_laa(image: torch.Tensor, labels: torch.Tensor, spacing: Sequence[float], local_mm: float, n_regions: int = 5,
              threshold: int = -950, cuts: Sequence[float] = (0.10, 0.25, 0.50), percentiles: Sequence[int] = (50, 90),
              out_u8: Optional[torch.Tensor] = None) -> dict:
    """The local low-attenuation fraction and its spread per lobe.  image [D,H,W] int16 HU and labels
    [D,H,W] as ``densitometry`` takes them; spacing (z, y, x) in mm; ``local_mm`` the side of the window in millimetres
    (``ops.local_window``: a box of 2 r + 1 voxels per axis) -- the caller's choice, like ``cuts``; none is recommended.
    ``ops.local_fraction3d`` gives the per-mille map q (the share of the lung voxels in the window, of ANY lobe, below
    ``threshold``; -1 outside the lung), ONE ``ops.lobe_histogram(q, labels, n_regions, hu_lo=0, nbins=1024)`` its exact
    per-lobe histogram (0..1000 are never clamped; -1 sits only where the label is <= 0, which the histogram does not
    count), and ``local_laa_from_hist`` the statistics.  -> that function's dict plus 'map' (int16 [D,H,W]), 'radius'
    (rz, ry, rx), 'local_mm', 'threshold'.  ``out_u8``: ``ops.local_fraction3d``'s, the window of a zero-filled volume on
    the scan's grid.  ValueError for bad arguments before any device work; device tensors, nothing read back."""
    t, _, _ = local_laa_params("local_laa", threshold, cuts, percentiles)
    radius = ops.local_window(spacing, local_mm)
    n = ops._n_regions("local_laa", n_regions)
    q = ops.local_fraction3d(image, labels, t, radius, out_u8=out_u8)
    hist, sums = ops.lobe_histogram(q, labels, n, 0, LOCAL_NBINS)
    out = local_laa_from_hist(hist, sums, cuts, percentiles)
    out.update(map=q, radius=radius, local_mm=float(local_mm), threshold=t)
    return out


def local_laa_metrics(result: dict, names=None) -> dict:
    """``local_laa``'s result -> entries of the metrics dict, keyed like ``densitometry_metrics``: per region
    'local_laa{|t|}_mean_per_region', '..._sd_...', '..._p{p}_...' per percentile and '..._above{cut in per cent}_...' per
    cut, all fractions as "{:.3f}", then their whole-lung twins ending '_per_lung', then 'local_mm' ("{:.2f}") and
    'local_window_voxels' ('{z}x{y}x{x}', the box in voxels).  None (json null) stands for NaN.  Pure host code."""
    stem = f"local_laa{abs(int(result['threshold']))}"
    lung = result["whole_lung"]
    perc, above, lung_perc, lung_above = (_lst(v) for v in (result["perc"], result["above"], lung["perc"], lung["above"]))
    cols = [(f"{stem}_mean", _lst(result["mean"]), _lst(lung["mean"]), "{:.3f}", float),
            (f"{stem}_sd", _lst(result["sd"]), _lst(lung["sd"]), "{:.3f}", float)]
    cols += [(f"{stem}_p{p}", perc[i], lung_perc[i], "{:.3f}", float) for i, p in enumerate(result["percentiles"])]
    cols += [(f"{stem}_above{int(round(c * 100))}", above[i], lung_above[i], "{:.3f}", float)
             for i, c in enumerate(result["cuts"])]
    out = _column_metrics("local_laa_metrics", cols, names)
    out["local_mm"] = "{:.2f}".format(float(result["local_mm"]))
    out["local_window_voxels"] = "{}x{}x{}".format(*(2 * int(r) + 1 for r in result["radius"]))
    return out


# --------------------------------------------------------------------------- core / peel split of the per-lobe report
ZONES = ("peel", "core")
FISSURE_ZONES = ("peel", "core", "fissure")          # with ``fissure_mm``: 'core' is then neither rind
_CORE_PEEL_KEY = re.compile(r"((laa\d+_fraction|perc\d+_hu|mean_lung_density|volume_ml|(cle|pse)_lesion_percentage)"
                            r"_per_(region|lung)|region_voxels)_(peel|core|fissure)|peel_mm|fissure_mm")


def core_peel(image: torch.Tensor, labels: torch.Tensor, spacing: Sequence[float], peel_mm: float = 10.0,
              n_regions: int = 5, fissure_mm: Optional[float] = None, **densitometry_kw) -> dict:
    """``densitometry`` of every lobe split into its subpleural rind (the "peel": lung voxels within ``peel_mm`` of the
    nearest non-lung voxel of the crop, Euclidean, at the scan's own spacing) and the rest (the "core"):
    ``ops.lung_zones`` -> composite labels (1..n the peel, n+1..2n the core of lobe r) -> ONE ``ops.lobe_histogram``
    with 2n rows -> ``densitometry_from_hist`` on each zone's rows behind a zero row 0, so that each zone also has its
    'whole_lung'.  ``peel_mm`` is the caller's choice -- the 10 mm default is a common rind width, not a recommendation;
    ``n_regions`` 1..7; ``densitometry_kw``: thresholds, percentiles, hu_lo, nbins.  ->
      {'peel': <densitometry result>, 'core': <densitometry result>, 'outside_voxels': int64 0-dim (lung voxels whose
       label is above n_regions: row 0 of the composite histogram, in neither zone's rows), 'zones', 'zone_labels'
       (uint8 [D,H,W], ``ops.lung_zones``), 'peel_mm', 'n_regions'}.
    The field of view is no pleura: a lung cut by the crop has no peel there.  Device tensors, nothing read back.

    ``fissure_mm`` (None: off, everything above holds unchanged): a third zone, the fissural rind -- lung voxels outside
    the peel within ``fissure_mm`` of the nearest voxel of ANOTHER lobe (labels 1..n; the pleura folds into the
    interlobar fissures, which hold no non-lung voxel).  ``ops.lobe_zones`` -> composite labels (2n+1..3n the fissural
    rind of lobe r) -> ONE ``ops.lobe_histogram`` with 3n rows; ``n_regions`` 1..5.  The result also holds 'fissure' (a
    third densitometry result), 'fissure_mm' and 'zone_names' = ('peel', 'core', 'fissure'); 'peel' is what it is without
    the argument, and 'core' then means NEITHER rind: the lung outside the peel and outside the fissural rind.
    ``fissure_mm`` is the caller's choice as well."""
    n = int(n_regions)
    if not isinstance(image, torch.Tensor) or not isinstance(labels, torch.Tensor) or tuple(image.shape) != tuple(labels.shape):
        raise ValueError("core_peel: image and labels must be tensors of one [D,H,W] shape")
    kw = dict(densitometry_kw)
    hu_lo, nbins = int(kw.pop("hu_lo", -1024)), int(kw.pop("nbins", 1024))
    names = ZONES if fissure_mm is None else FISSURE_ZONES
    if fissure_mm is None:
        zones, zone_labels, _ = ops.lung_zones(labels, spacing, peel_mm, n_regions=n)
    else:
        zones, zone_labels, _, _ = ops.lobe_zones(labels, spacing, peel_mm, fissure_mm, n_regions=n)
    hist, sums = ops.lobe_histogram(image, zone_labels, len(names) * n, hu_lo, nbins)
    out = {}
    for i, zone in enumerate(names):
        rows = slice(1 + i * n, 1 + (i + 1) * n)
        out[zone] = densitometry_from_hist(torch.cat([torch.zeros_like(hist[:1]), hist[rows]]),
                                           torch.cat([torch.zeros_like(sums[:1]), sums[rows]]), spacing, hu_lo=hu_lo, **kw)
    out.update(outside_voxels=sums[0, 0], zones=zones, zone_labels=zone_labels, peel_mm=float(peel_mm), n_regions=n)
    if fissure_mm is not None:
        out.update(fissure_mm=float(fissure_mm), zone_names=FISSURE_ZONES)
    return out


def core_peel_metrics(result: dict, names=None) -> dict:
    """``core_peel``'s result -> entries of the metrics dict: ``densitometry_metrics`` of each zone with the zone's name
    appended to every key ('laa950_fraction_per_region_peel', 'volume_ml_per_lung_core', ...: the same formats, keyed
    through ``names`` the same way, None for NaN), and 'peel_mm' ("{:.3f}").  The zones are those the result names
    ('zone_names'; without it 'peel' and 'core'): a result of ``core_peel(fissure_mm=...)`` adds the keys ending
    '_fissure' and 'fissure_mm' ("{:.3f}").  Pure host code."""
    out = {}
    for zone in result.get("zone_names", ZONES):
        out.update({f"{k}_{zone}": v for k, v in densitometry_metrics(result[zone], names).items()})
    out["peel_mm"] = "{:.3f}".format(float(result["peel_mm"]))
    if "fissure_mm" in result:
        out["fissure_mm"] = "{:.3f}".format(float(result["fissure_mm"]))
    return out


def fold_zone_table(table_row, n_zones: int = 2) -> torch.Tensor:
    """The composite region table [2n+1, 4] (rows 1..n peel, n+1..2n core) -> the per-lobe one [n+1, 4] that
    ``region_metrics`` reads, in float64 on the host: row r = row r + row n+r, row 0 stays row 0.  ``n_zones`` = 3: the
    table is [3n+1, 4] (2n+1..3n the fissural rind) and row r = row r + row n+r + row 2n+r, added in that order."""
    t = torch.as_tensor(table_row).detach().cpu().double()
    z = int(n_zones)
    if z not in (2, 3):
        raise ValueError(f"fold_zone_table: n_zones must be 2 or 3, got {n_zones}")
    if t.dim() != 2 or t.shape[1] != 4 or t.shape[0] < z + 1 or t.shape[0] % z != 1:
        raise ValueError(f"fold_zone_table: table_row must be [{z} * n_regions + 1, 4]")
    n = (t.shape[0] - 1) // z
    rows = t[1:n + 1] + t[n + 1:2 * n + 1]
    if z == 3:
        rows = rows + t[2 * n + 1:]
    return torch.cat([t[:1], rows])


def zone_region_metrics(table_row, names=None, zones=ZONES) -> dict:
    """One sample's composite region table [2n+1, 4] (predict_step's 'region_table'[b] for ``core_peel``'s zone labels
    and 'n_regions' = 2n) -> for each zone Z in ('peel', 'core') 'cle_lesion_percentage_per_region_Z',
    'pse_lesion_percentage_per_region_Z' and 'region_voxels_Z' (keyed and formatted like ``region_metrics``; None for
    a lobe without voxels in that zone) and 'cle_lesion_percentage_per_lung_Z' / 'pse_lesion_percentage_per_lung_Z' =
    sum / voxels over the zone's rows (None for an empty zone).  No severity scores: the ratio bands are defined per
    lung.  ``zones``: the zone names in the order of the table's row blocks -- ``FISSURE_ZONES`` for the [3n+1, 4] table
    of ``core_peel(fissure_mm=...)``'s labels, which adds the keys ending '_fissure'; the row count alone does not tell
    (7 rows are 3 lobes in two zones or 2 lobes in three).  Pure host code, float64."""
    rows = table_row.tolist() if torch.is_tensor(table_row) else [list(r) for r in table_row]
    zones = tuple(zones)
    z = len(zones)
    if z not in (2, 3):
        raise ValueError(f"zone_region_metrics: zones must name 2 or 3 zones, got {zones}")
    if len(rows) < z + 1 or len(rows) % z != 1 or any(len(r) != 4 for r in rows):
        raise ValueError(f"zone_region_metrics: table_row must be [{z} * n_regions + 1, 4]")
    n = (len(rows) - 1) // z
    out = {}
    for i, zone in enumerate(zones):
        per = {f"{h}_lesion_percentage_per_region_{zone}": {} for h in ("cle", "pse")}
        per[f"region_voxels_{zone}"] = {}
        tot = [0.0, 0.0, 0.0]
        for label in range(1, n + 1):
            key = _region_key(names, label)
            s_cle, s_pse, _, n_vox = (float(v) for v in rows[i * n + label])
            for h, s in (("cle", s_cle), ("pse", s_pse)):
                per[f"{h}_lesion_percentage_per_region_{zone}"][key] = "{:.3f}".format(s / n_vox) if n_vox > 0 else None
            per[f"region_voxels_{zone}"][key] = "{:d}".format(int(round(n_vox)))
            tot = [tot[0] + s_cle, tot[1] + s_pse, tot[2] + n_vox]
        out.update(per)
        for h, s in (("cle", tot[0]), ("pse", tot[1])):
            out[f"{h}_lesion_percentage_per_lung_{zone}"] = "{:.3f}".format(s / tot[2]) if tot[2] > 0 else None
    return out


# --------------------------------------------------------------------------- LAA cluster analysis per lobe
_CLUSTER_KEY = re.compile(r"laa\d+_(clusters|largest_cluster_ml|cluster_d|bullae|bulla_ml|bulla_laa_share)_per_(region|lung)"
                          r"|laa\d+_(clusters|bullae)_per_(region|lung)_(peel|core|fissure)|laa\d+_largest_clusters"
                          r"|laa_cluster_connectivity|bulla_mm|bulla_min_voxels")


def clusters_from_table(table: torch.Tensor, spacing: Sequence[float]) -> dict:
    """The tensor math of ``laa_clusters``: ``ops.label_components``' table int64 [n+1, 35] -> per row 'clusters',
    'voxels', 'largest_voxels' (int64 [n+1]), 'largest_ml' = largest_voxels * sz*sy*sx / 1000 and 'mean_voxels' =
    voxels / clusters (float64, NaN for an empty row), 'size_hist' [n+1, 32] (clusters with 2^k <= size < 2^(k+1)) and
    'd' (float64 [n+1]): with kmax the highest non-empty bin and Y_k = sum_{j >= k} size_hist[j] (the clusters of at
    least 2^k voxels, exact) for k = 0..kmax, D = -slope of the least-squares line through (k ln 2, ln Y_k); NaN when
    kmax < 2 (fewer than three points).  O(rows * 32) torch operations on the table's own device (CPU tensors work),
    int64 / float64 arithmetic, nothing read back."""
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.int64 or \
            table.shape[0] < 2 or table.shape[1] != ops.CCL_TABLE_COLS:
        raise ValueError(f"clusters_from_table: table must be int64 [n_regions + 1, {ops.CCL_TABLE_COLS}]")
    sp = [float(v) for v in spacing]
    if len(sp) != 3:
        raise ValueError("clusters_from_table: spacing must have three entries (z, y, x)")
    nan = float("nan")
    hist = table[:, :32]
    count, vox, largest = table[:, 32], table[:, 33], table[:, 34]
    some = count > 0
    nan_row = torch.full_like(count, nan, dtype=torch.float64)
    largest_ml = torch.where(some, largest.double() * (sp[0] * sp[1] * sp[2]) / 1000.0, nan_row)
    mean_vox = torch.where(some, vox.double() / count.clamp_min(1).double(), nan_row)
    k = torch.arange(32, device=table.device)
    kmax = ((hist > 0) * k).amax(1)                                   # 0 for an empty row as well: NaN either way
    y = hist.flip(1).cumsum(1).flip(1)                                # Y_k, exact
    pts = (k[None, :] <= kmax[:, None]) & some[:, None]               # the points k = 0..kmax of a row
    w = pts.double()
    npts = w.sum(1)
    xs = k.double()[None, :] * math.log(2.0)
    ys = torch.where(pts, y.clamp_min(1).double().log(), torch.zeros_like(w))
    xm = (w * xs).sum(1) / npts.clamp_min(1.0)
    ym = (w * ys).sum(1) / npts.clamp_min(1.0)
    dx = (xs - xm[:, None]) * w
    sxx = (dx * dx).sum(1)
    sxy = (dx * (ys - ym[:, None])).sum(1)
    d = torch.where(npts >= 3, -sxy / sxx.clamp_min(1e-300), nan_row) + 0.0          # + 0.0: a flat line gives 0, not -0
    return {"clusters": count, "voxels": vox, "largest_voxels": largest, "largest_ml": largest_ml,
            "mean_voxels": mean_vox, "size_hist": hist, "d": d}


def bulla_min_voxels(spacing: Sequence[float], bulla_mm: float) -> int:
    """The smallest cluster, in voxels, whose equivalent-sphere diameter reaches ``bulla_mm``:
    max(1, ceil(pi/6 * bulla_mm^3 / (sz*sy*sx))), float64 on the host."""
    sp = [float(v) for v in spacing]
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError("bulla_min_voxels: spacing must have three positive, finite entries (z, y, x)")
    mm = float(bulla_mm)
    if not (math.isfinite(mm) and mm > 0):
        raise ValueError(f"bulla_min_voxels: bulla_mm must be positive and finite, got {bulla_mm}")
    return max(1, int(math.ceil(math.pi / 6.0 * mm ** 3 / (sp[0] * sp[1] * sp[2]))))


def shapes_from_rows(rows: torch.Tensor, spacing: Sequence[float], n_regions: int, bulla_mm: float = 10.0, top: int = 3,
                     origin: Sequence[int] = (0, 0, 0), n_zones: int = 0) -> dict:
    """The tensor math of the cluster shapes: ``ops.component_shapes``' rows int64 [m, 18] (m = 0 is valid) -> a dict.

    Scalars: 'bulla_mm' and 'bulla_min_voxels' (``bulla_min_voxels(spacing, bulla_mm)``, an int computed once on the
    host).  A cluster is a BULLA when its voxels >= bulla_min_voxels -- an integer comparison, hence exact; it says
    "equivalent-sphere diameter at least ``bulla_mm``".  The 10 mm default is the common definition; it is the caller's
    choice and no recommendation.
    Per row 0..n_regions (a cluster's class r in 1..n -> row r, any other class -> row 0): 'bullae', 'bulla_voxels',
    'cluster_voxels' (int64), 'bulla_ml' (float64) and 'bulla_laa_share' = bulla voxels / the row's cluster voxels
    (float64, NaN for a row without clusters).
    Per cluster, in the order of the rows: 'region' (its row, int64), 'voxels', 'is_bulla', 'volume_ml', 'diameter_mm' =
    (6 V / pi)^(1/3), 'extent_mm' [m, 3] = box * spacing, 'centroid' [m, 3] = sums / voxels + origin (voxels of the grid
    the origin is given in, (z, y, x)), 'surface_mm2' = fz sy sx + fy sz sx + fx sz sy, 'sphericity' = pi^(1/3)
    (6 V)^(2/3) / surface, and 'home_zone' (int64): the zone 1..3 that holds most of its voxels, the lower zone on a
    tie, 0 when the three counts are 0.  The surface is a sum of voxel faces, which overstates a smooth surface by a
    factor that depends on orientation: a cube has sphericity 0.806, a voxelised ball about 2/3 -- the number compares
    clusters of one report with each other and with nothing else.
    With ``n_zones`` = 2 or 3 (the rows were made with a zone volume): 'zone_clusters' and 'zone_bullae' int64
    [n_regions + 1, n_zones], the clusters / bullae of a row by home zone (a home zone of 0 or above n_zones counts in
    neither).
    'largest': the indices (int64 [min(top, m)]) of the ``top`` clusters by voxels descending, root ascending on ties.
    int64 / float64 torch operations on the rows' own device (CPU tensors work), nothing read back."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != torch.int64 or rows.shape[1] != ops.SHAPE_COLS:
        raise ValueError(f"shapes_from_rows: rows must be int64 [m, {ops.SHAPE_COLS}]")
    n, nz, k = int(n_regions), int(n_zones), int(top)
    if n < 1 or nz not in (0, 2, 3) or k < 0:
        raise ValueError("shapes_from_rows: n_regions >= 1, n_zones 0, 2 or 3 and top >= 0 are required")
    sp = [float(v) for v in spacing]
    org = [int(v) for v in origin]
    if len(org) != 3:
        raise ValueError("shapes_from_rows: origin must have three entries (z, y, x)")
    need = bulla_min_voxels(sp, bulla_mm)
    dev, f64 = rows.device, torch.float64
    voxel = sp[0] * sp[1] * sp[2]
    cls, vox = rows[:, ops.SHAPE_CLASS], rows[:, ops.SHAPE_VOXELS]
    region = torch.where((cls >= 1) & (cls <= n), cls, torch.zeros_like(cls))
    is_bulla = vox >= need
    zero = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    per_row = lambda w: zero.index_add(0, region, w)
    bullae, bulla_vox, cluster_vox = per_row(is_bulla.long()), per_row(vox * is_bulla.long()), per_row(vox)
    share = torch.where(cluster_vox > 0, bulla_vox.double() / cluster_vox.clamp_min(1).double(),
                        torch.full((n + 1,), float("nan"), dtype=f64, device=dev))
    v_mm3 = vox.double() * voxel
    box = rows[:, ops.SHAPE_Z0:ops.SHAPE_X1 + 1].reshape(-1, 3, 2)
    spt = torch.tensor(sp, dtype=f64, device=dev)
    extent = (box[:, :, 1] - box[:, :, 0]).double() * spt
    centroid = rows[:, ops.SHAPE_SUM_Z:ops.SHAPE_SUM_X + 1].double() / vox.clamp_min(1).double()[:, None] + \
        torch.tensor(org, dtype=f64, device=dev)
    faces = rows[:, ops.SHAPE_FACES_Z:ops.SHAPE_FACES_X + 1].double()
    surface = faces[:, 0] * (sp[1] * sp[2]) + faces[:, 1] * (sp[0] * sp[2]) + faces[:, 2] * (sp[0] * sp[1])
    sphericity = math.pi ** (1.0 / 3.0) * (6.0 * v_mm3) ** (2.0 / 3.0) / surface
    zc = rows[:, ops.SHAPE_ZONE1:ops.SHAPE_ZONE3 + 1]
    best = zc.amax(1)
    ties = (zc == best[:, None]).long()
    first = 2 - ties[:, 0] * 2 - (1 - ties[:, 0]) * ties[:, 1]                        # the lowest zone among the maxima
    home = torch.where(best > 0, first + 1, torch.zeros_like(best))
    out = {"bulla_mm": float(bulla_mm), "bulla_min_voxels": need, "bullae": bullae, "bulla_voxels": bulla_vox,
           "cluster_voxels": cluster_vox, "bulla_ml": bulla_vox.double() * voxel / 1000.0, "bulla_laa_share": share,
           "region": region, "voxels": vox, "is_bulla": is_bulla, "volume_ml": v_mm3 / 1000.0,
           "diameter_mm": (6.0 * v_mm3 / math.pi) ** (1.0 / 3.0), "extent_mm": extent, "centroid": centroid,
           "surface_mm2": surface, "sphericity": sphericity, "home_zone": home}
    if nz:
        flat = torch.zeros((n + 1) * nz, dtype=torch.int64, device=dev)
        zoned = ((home >= 1) & (home <= nz)).long()
        slot = region * nz + (home - 1).clamp(0, nz - 1)
        out["zone_clusters"] = flat.index_add(0, slot, zoned).reshape(n + 1, nz)
        out["zone_bullae"] = flat.index_add(0, slot, zoned * is_bulla.long()).reshape(n + 1, nz)
    out["largest"] = torch.sort(vox, descending=True, stable=True)[1][:k]
    return out


def laa_clusters(image: torch.Tensor, labels: torch.Tensor, spacing: Sequence[float], n_regions: int = 5,
                 threshold: int = -950, connectivity: int = 6, shapes: bool = False, bulla_mm: float = 10.0, top: int = 3,
                 zones: Optional[torch.Tensor] = None, zone_names: Optional[Sequence[str]] = None,
                 origin: Sequence[int] = (0, 0, 0)) -> dict:
    """How the low attenuation of every lobe is arranged: the connected clusters of ``image <
    threshold`` inside each lobe (``ops.laa_components(by_lobe=True)``: a cluster never crosses a fissure) ->
    ``clusters_from_table`` for the rows 0..n_regions (row 0: LAA voxels whose label is above n_regions), and once more
    over the whole lung (``by_lobe=False``: clusters may cross fissures), whose one row is 'whole_lung'.  Also
    'threshold', 'connectivity' and 'components', the per-lobe id volume (int32, -1 outside the clusters).  'd' is the
    exponent of the cumulative cluster-size distribution sampled at powers of two -- NOT Mishima's per-slice 2-D fit
    over every distinct size.  Device tensors, nothing read back; ``laa_cluster_metrics`` formats it on the host.

    ``shapes`` (off: the result is the above, key for key): the result gains 'shapes', ``shapes_from_rows(bulla_mm, top,
    origin)`` of ``ops.component_shapes`` on the per-lobe labelling, the class of a cluster read from ``labels`` at its
    root, plus 'whole_lung' (the same of the whole-lung labelling, every cluster in row 0 of two), 'rows' and
    'whole_lung_rows' (the raw int64 [m, 18] tables) and 'zone_names'.  No new labelling: two more kernel calls, each
    of which reads its number of clusters back (the two synchronisations of this function).  ``zones`` (uint8 [D,H,W],
    ``core_peel``'s 'zones') with ``zone_names`` (``ZONES`` / ``FISSURE_ZONES``, in the order of the zone values 1, 2,
    3) crosses the clusters with the zones: zone counts per cluster, a home zone, clusters and bullae per row and home
    zone.  ``origin``: the (z, y, x) offset of the volume in the grid the centroids are reported in."""
    comp, table, _ = ops.laa_components(image, labels, threshold, n_regions, connectivity, by_lobe=True)
    whole_comp, whole, _ = ops.laa_components(image, labels, threshold, 1, connectivity, by_lobe=False)
    out = clusters_from_table(table, spacing)
    out["whole_lung"] = {k: v[1] for k, v in clusters_from_table(whole, spacing).items()}
    out.update(threshold=int(threshold), connectivity=int(connectivity), components=comp)
    if shapes:
        if (zones is None) != (zone_names is None):
            raise ValueError("laa_clusters: zones and zone_names come together")
        names = () if zone_names is None else tuple(zone_names)
        if zones is not None and len(names) not in (2, 3):
            raise ValueError(f"laa_clusters: zone_names must name 2 or 3 zones, got {names}")
        kw = dict(bulla_mm=bulla_mm, top=top, origin=origin, n_zones=len(names))
        rows, _ = ops.component_shapes(comp, labels, zones)
        whole_rows, _ = ops.component_shapes(whole_comp, None, zones)
        sh = shapes_from_rows(rows, spacing, n_regions, **kw)
        sh.update(whole_lung=shapes_from_rows(whole_rows, spacing, 1, **kw), rows=rows, whole_lung_rows=whole_rows,
                  zone_names=names)
        out["shapes"] = sh
    return out


def _shape_metrics(t: int, sh: dict, names=None) -> dict:
    """the entries ``laa_cluster_metrics`` adds for a result with 'shapes'"""
    lung = sh["whole_lung"]
    cols = [(f"laa{t}_{stem}", _lst(sh[field]), _lst(lung[field])[0], spec, cast) for stem, field, spec, cast in
            (("bullae", "bullae", "{:d}", int), ("bulla_ml", "bulla_ml", "{:.3f}", float),
             ("bulla_laa_share", "bulla_laa_share", "{:.3f}", float))]
    out = _column_metrics("laa_cluster_metrics", cols, names)
    for i, zone in enumerate(sh["zone_names"]):
        for stem, field in (("clusters", "zone_clusters"), ("bullae", "zone_bullae")):
            per_row = _lst(sh[field])
            out[f"laa{t}_{stem}_per_region_{zone}"] = {_region_key(names, label): "{:d}".format(int(per_row[label][i]))
                                                       for label in range(1, len(per_row))}
            out[f"laa{t}_{stem}_per_lung_{zone}"] = "{:d}".format(int(_lst(lung[field])[0][i]))
    f3 = lambda v: _fmt(float(v), "{:.3f}")
    region, home = _lst(sh["region"]), _lst(sh["home_zone"])
    fields = {k: _lst(sh[k]) for k in ("volume_ml", "diameter_mm", "extent_mm", "centroid", "surface_mm2", "sphericity")}
    largest = []
    for i in _lst(sh["largest"]):
        zone = int(home[i])
        largest.append({"region": _region_key(names, int(region[i])) if int(region[i]) > 0 else None,
                        "volume_ml": f3(fields["volume_ml"][i]), "diameter_mm": f3(fields["diameter_mm"][i]),
                        "extent_mm": [f3(v) for v in fields["extent_mm"][i]],
                        "centroid": [_fmt(float(v), "{:.1f}") for v in fields["centroid"][i]],
                        "surface_mm2": f3(fields["surface_mm2"][i]), "sphericity": f3(fields["sphericity"][i]),
                        "zone": sh["zone_names"][zone - 1] if 1 <= zone <= len(sh["zone_names"]) else None})
    out[f"laa{t}_largest_clusters"] = largest
    out["bulla_mm"] = "{:.3f}".format(float(sh["bulla_mm"]))
    out["bulla_min_voxels"] = "{:d}".format(int(sh["bulla_min_voxels"]))
    return out


def laa_cluster_metrics(result: dict, names=None) -> dict:
    """``laa_clusters``' result -> entries of the metrics dict, keyed like ``densitometry_metrics`` (``names[label]`` of
    a mapping or sequence, else the label as a string), for t = |threshold|: 'laa{t}_clusters_per_region' ("{:d}"),
    'laa{t}_largest_cluster_ml_per_region' and 'laa{t}_cluster_d_per_region' ("{:.3f}", None -- json null -- for NaN),
    their whole-lung twins ending '_per_lung' (one value each) and 'laa_cluster_connectivity' ("{:d}").  Row 0 is not
    reported as a region.  Pure host code.

    A result of ``laa_clusters(shapes=True)`` adds 'laa{t}_bullae_per_region' ("{:d}"), 'laa{t}_bulla_ml_per_region' and
    'laa{t}_bulla_laa_share_per_region' ("{:.3f}", None for NaN) with their '_per_lung' twins; with zones, for each zone
    Z 'laa{t}_clusters_per_region_Z' and 'laa{t}_bullae_per_region_Z' ("{:d}", by home zone) with '_per_lung' twins;
    'laa{t}_largest_clusters', the ``top`` clusters of the per-lobe labelling, largest first, each a dict of 'region'
    (its key through ``names``, None for row 0), 'volume_ml', 'diameter_mm', 'extent_mm' [z, y, x], 'surface_mm2',
    'sphericity' ("{:.3f}"), 'centroid' [z, y, x] in voxels of the grid of ``origin`` ("{:.1f}") and 'zone' (the home
    zone's name or None); 'bulla_mm' ("{:.3f}") and 'bulla_min_voxels' ("{:d}")."""
    t = abs(int(result["threshold"]))
    lung = result["whole_lung"]
    cols = [(f"laa{t}_{stem}", _lst(result[field]), _lst(lung[field]), spec, cast) for stem, field, spec, cast in
            (("clusters", "clusters", "{:d}", int), ("largest_cluster_ml", "largest_ml", "{:.3f}", float),
             ("cluster_d", "d", "{:.3f}", float))]
    out = _column_metrics("laa_cluster_metrics", cols, names, unsigned_zero=True)   # a slope of +-1e-17 reads 0.000
    out["laa_cluster_connectivity"] = "{:d}".format(int(result["connectivity"]))
    if "shapes" in result:
        out.update(_shape_metrics(t, result["shapes"], names))
    return out


# --------------------------------------------------------------------------- the noise filter in front of the scan side
def filtered_image(case_image: torch.Tensor, size=(3, 3, 3)) -> torch.Tensor:
    """The scan-side input of ``densitometry`` / ``core_peel`` / ``laa_clusters`` with the noise filter in front:
    ``ops.median_filter3d`` of ``prepare_case``'s 'image' (int16 [D,H,W]; ``size``: (3, 3, 3), (1, 3, 3), ...), a new
    tensor.  At lung voxels it equals the crop of the filtered whole scan when the case was prepared with
    ``dilate_iterations`` >= 1 and ``crop_border`` > 0.  Device work only."""
    return ops.median_filter3d(case_image, size)


def _tagged_numbers(fn: str, scan_filter, tag: str, count: int, says: str) -> Optional[Tuple[float, ...]]:
    """the ``count`` numbers behind the string ``tag``; None without the tag; ValueError (``says``) for any other numbers"""
    if not isinstance(scan_filter, (tuple, list)) or len(scan_filter) < 1 or scan_filter[0] != tag:
        return None
    if len(scan_filter) != count + 1 or not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
                                                 and v > 0 for v in scan_filter[1:]):
        raise ValueError(f"{fn}: {says}, got {scan_filter!r}")
    return tuple(float(v) for v in scan_filter[1:])


def gaussian_sigma_mm(fn: str, scan_filter) -> Optional[float]:
    """The sigma in millimetres of a ``("gaussian", sigma_mm)`` scan filter; None for anything that does not start with
    the string 'gaussian' (a median window size).  ValueError unless sigma_mm is one finite number > 0.  Pure host code."""
    p = _tagged_numbers(fn, scan_filter, "gaussian", 1,
                        "a Gaussian scan filter is ('gaussian', sigma_mm) with a finite sigma_mm > 0")
    return None if p is None else p[0]


def sigma_voxels(fn: str, spacing, sigma_mm: float, radius_of: Callable, max_radius: int) -> Tuple[float, float, float]:
    """sigma_mm / spacing per axis (z, y, x) as Python floats.  ValueError, naming the axis and its spacing, when an axis'
    radius ``radius_of(sigma)`` exceeds ``max_radius``; radius 0 (slices much thicker than sigma): the axis is untouched."""
    sp = ops._spacing3(fn, spacing)
    if not (math.isfinite(sigma_mm) and sigma_mm > 0):
        raise ValueError(f"{fn}: sigma_mm must be finite and > 0, got {sigma_mm!r}")
    sig = tuple(float(sigma_mm) / v for v in sp)
    for axis, s, v in zip("zyx", sig, sp):
        r = radius_of(s)
        if r > max_radius:
            raise ValueError(f"{fn}: sigma {sigma_mm} mm on axis {axis} with spacing {v} mm is {s:.2f} voxels, radius "
                             f"{r}; the filter holds radius <= {max_radius}")
    return sig


def gaussian_sigma_voxels(fn: str, spacing: Sequence[float], sigma_mm: float) -> Tuple[float, float, float]:
    """``sigma_voxels`` under the Gaussian filter's cap: the radius ``int(4 sigma + 0.5)`` of an axis is at most 16."""
    return sigma_voxels(fn, spacing, sigma_mm, ops.gaussian_radius, ops.GAUSS_MAX_RADIUS)


def gaussian_image(scan: torch.Tensor, crop_slice, spacing: Sequence[float], sigma_mm: float) -> torch.Tensor:
    """The scan-side input of ``densitometry`` / ``core_peel`` / ``laa_clusters`` behind a Gaussian of ``sigma_mm``
    millimetres: ``ops.gaussian_filter3d`` of the SCAN itself (converted to int16 as
    ``prepare_case`` converts it), sigma_mm / spacing voxels per axis, edges replicated, evaluated on the box
    ``crop_slice`` only -> int16 of the crop's shape.  It is the crop of the filtered scan by construction: neither the
    fill value outside the dilated lung nor the crop's faces enter it.  Device work only: ``crop_slice`` is
    ``prepare_case``'s host tensor (or a list); a device tensor would be read back to size the output."""
    sig = gaussian_sigma_voxels("gaussian_image", spacing, float(sigma_mm))
    return ops.gaussian_filter3d(scan.to(torch.int16), sig, mode="nearest", box=crop_slice)


def bilateral_params(fn: str, scan_filter) -> Optional[Tuple[float, float]]:
    """(sigma_mm, sigma_hu) of a ``("bilateral", sigma_mm, sigma_hu)`` scan filter; None for anything that does not
    start with the string 'bilateral'.  ValueError unless both are finite numbers > 0 (no bools).  Pure host code."""
    return _tagged_numbers(fn, scan_filter, "bilateral", 2, "a bilateral scan filter is ('bilateral', sigma_mm, sigma_hu) "
                           "with finite sigma_mm > 0 and sigma_hu > 0")


def bilateral_sigma_voxels(fn: str, spacing: Sequence[float], sigma_mm: float) -> Tuple[float, float, float]:
    """``sigma_voxels`` under the bilateral filter's cap: the radius ``int(2 sigma + 0.5)`` of an axis is at most 5."""
    return sigma_voxels(fn, spacing, sigma_mm, ops.bilateral_radius, ops.BILAT_MAX_RADIUS)


def bilateral_image(case_image: torch.Tensor, lobe_labels: torch.Tensor, spacing: Sequence[float], sigma_mm: float,
                    sigma_hu: float) -> torch.Tensor:
    """The scan-side input of ``densitometry`` / ``core_peel`` / ``laa_clusters`` behind the bilateral filter
    (INTEGRATION.md B12): ``ops.bilateral_filter3d`` of ``prepare_case``'s 'image' (int16 [D,H,W]) with sigma_mm /
    spacing voxels per axis, truncated at 2 sigma, ``sigma_hu`` in HU and ``within=lobe_labels``, a new tensor.  Taps
    never leave the lung, so neither the fill value outside the dilated lung nor the crop's faces enter a lung voxel:
    there the result is the crop of the filtered whole scan (``within`` the whole lobe volume) under any
    ``dilate_iterations`` / ``crop_border``; a voxel outside the lung keeps the case's value.  Device work only."""
    sig = bilateral_sigma_voxels("bilateral_image", spacing, float(sigma_mm))
    return ops.bilateral_filter3d(case_image, sig, float(sigma_hu), within=lobe_labels)


class _ScanFilter(NamedTuple):
    """One kind of ``predict_case``'s ``scan_filter``.  A new filter is one record in ``_SCAN_FILTERS`` (plus its kernel)."""
    parse: Callable         # (fn, scan_filter) -> its parameters, or None: not this kind; ValueError for bad ones
    check: Callable         # (fn, params, spacing, prepare_kw): everything that is refused before device work
    image: Callable         # (params, scan, case, spacing) -> the filtered int16 image of the case; device work only
    name: Callable          # params -> the report's 'scan_filter' value


def _median_needs(fn: str, size, spacing, prepare_kw):
    if int(prepare_kw.get("dilate_iterations", 2)) < 1 or not prepare_kw.get("crop_border", 5) > 0:
        raise ValueError(f"{fn} needs dilate_iterations >= 1 and crop_border > 0: without them a window centred on a "
                         "lung voxel reaches the fill value or the crop's edge")


_SCAN_FILTERS = {       # asked in this order: the median, which takes whatever carries no name, comes last
    "bilateral": _ScanFilter(                               # its check: the radius cap per axis, the range table's cap
        bilateral_params, lambda fn, p, spacing, kw: ops.bilateral_tables(bilateral_sigma_voxels(fn, spacing, p[0]), p[1]),
        lambda p, scan, case, spacing: bilateral_image(case["image"], case["lobe_labels"], spacing, *p),
        lambda p: "bilateral{:.2f}mm{:.1f}hu".format(*p)),
    "gaussian": _ScanFilter(
        gaussian_sigma_mm, lambda fn, p, spacing, kw: gaussian_sigma_voxels(fn, spacing, p),      # the radius cap, per axis
        lambda p, scan, case, spacing: gaussian_image(scan, case["crop_slice"], spacing, p), "gaussian{:.2f}mm".format),
    "median": _ScanFilter(
        ops.median_size, _median_needs, lambda p, scan, case, spacing: filtered_image(case["image"], p),
        lambda p: "median{}x{}x{}".format(*p)),
}


def _scan_filter(fn: str, scan_filter) -> Tuple[_ScanFilter, object]:
    """(record, parameters) of a ``scan_filter`` value; ValueError in the name of ``fn`` for one that is no filter"""
    asked = ((record, record.parse(fn, scan_filter)) for record in _SCAN_FILTERS.values())
    return next((record, params) for record, params in asked if params is not None)


def filter_name(size) -> str:
    """The value of the report's 'scan_filter' key: 'median{z}x{y}x{x}' of a median window size, 'gaussian{:.2f}mm' of
    ``("gaussian", sigma_mm)``, 'bilateral{:.2f}mm{:.1f}hu' of ``("bilateral", sigma_mm, sigma_hu)``."""
    record, params = _scan_filter("filter_name", size)
    return record.name(params)


# --------------------------------------------------------------------------- the sections of the report
class _Section(NamedTuple):
    """One optional section of the predict report; ``_SECTIONS`` maps ``predict_case``'s switch to it.  Adding an analysis
    to the report is one record there (plus its switch and its json argument in the two signatures)."""
    json_arg: str                                   # write_reports' argument for the section's own file
    select: Union[Tuple[str, ...], re.Pattern]      # the section's metric keys: the names, or a pattern they match in full
    required: Tuple[str, ...]                       # patterns that selected keys must match, or the section is absent
    hint: str                                       # what write_reports says is missing
    # the scan side, run on the prepared case before the resize (None: the section comes from predict_step's table)
    run: Optional[Callable] = None                  # (image, lobe_labels, spacing, **kw) -> result; device work only
    metrics: Optional[Callable] = None              # (result, region_names) -> metrics entries
    outside: Optional[Callable] = None              # result -> (voxels outside 1..n, n); reads the device
    error: str = ""                                 # the error_messages line, .format(outside, n)


def _row0_voxels(result):
    return int(result["voxels"][0]), result["voxels"].shape[0] - 1


_SECTIONS = {          # in the order of the report: metric keys, error lines and files follow it
    "regions": _Section("regions_json", REGION_KEYS, REGION_KEYS, "regional metrics"),
    "densitometry": _Section(
        "densitometry_json", _DENSITO_KEY, ("mean_lung_density_per_region",), "densitometry metrics",
        densitometry, densitometry_metrics, _row0_voxels,
        "{:d} lung voxels carry a lobe label outside 1..{:d}: their density is in no region"),
    "core_peel": _Section(
        "core_peel_json", _CORE_PEEL_KEY, ("mean_lung_density_per_region_peel", "region_voxels_peel", "peel_mm"),
        "core / peel metrics", core_peel, lambda r, names: {**core_peel_metrics(r, names), **r["zone_metrics"]},
        lambda r: (int(r["outside_voxels"]), r["n_regions"]),
        "{:d} lung voxels carry a lobe label outside 1..{:d}: they are in no region's peel or core"),
    "clusters": _Section(
        "clusters_json", _CLUSTER_KEY, ("laa_cluster_connectivity", r"laa\d+_clusters_per_region"), "cluster metrics",
        laa_clusters, laa_cluster_metrics, _row0_voxels,
        "{:d} low-attenuation voxels carry a lobe label outside 1..{:d}: their clusters are in no region"),
}
_LAUNCH_ORDER = ("clusters", "densitometry", "core_peel")          # the order the scan-side kernels are issued in


def build_outputs(predictions: List[dict], want_u8: bool = True, region_names=None) -> List[dict]:
    """processor.py:102-145 for a list of predict_step outputs: per scan the pasted CLE / PSE volumes (uint8 like
    the written .mha, and/or float) and the metrics entry of the results json.  A prediction that carries a
    'region_table' adds ``region_metrics`` to its metrics, and a line in error_messages when row 0 of the table holds
    ess voxels: ess lies inside the lung, so those are lung voxels whose label is outside 1..n_regions."""
    results = []
    for out in predictions:
        B = out["cle_dense_outs"].shape[0]
        for b in range(B):
            vols = {}
            for name in ("cle", "pse"):
                d = out[f"{name}_dense_outs"][b]
                d = d.reshape(d.shape[-3:])
                f32, u8 = resample_paste(d, out["crop_slices"][b], out["original_size"][b], want_f32=not want_u8,
                                         want_u8=want_u8)
                vols[name] = u8 if want_u8 else f32
            cle_p, pse_p = float(out["cle_precentages"][b]), float(out["pse_precentages"][b])
            metrics = {"cle_severity_score": "{:d}".format(ratio_to_label(cle_p, CLE_RATIO_MAP)),
                       "cle_lesion_percentage_per_lung": "{:.3f}".format(cle_p),
                       "pse_severity_score": "{:d}".format(ratio_to_label(pse_p, PSE_RATIO_MAP)),
                       "pse_lesion_percentage_per_lung": "{:.3f}".format(pse_p)}
            errors = []
            if out.get("region_table") is not None:
                row = out["region_table"][b].cpu()
                metrics.update(region_metrics(row, region_names))
                if float(row[0, 2]) > 0:
                    errors.append("{:d} ess voxels carry a lobe label outside 1..{:d}: they are in no region".format(
                        int(round(float(row[0, 2]))), row.shape[0] - 1))
            uid = out["uids"][b] if out.get("uids") is not None else None
            results.append({"entity": uid, "metrics": metrics, "error_messages": errors, "full_cle": vols["cle"],
                            "full_pse": vols["pse"]})
    return results


def predict_case(module, scan: torch.Tensor, lobes: torch.Tensor, spacing: Sequence[float], target_size: Sequence[int],
                 uid=None, want_u8: bool = True, regions: bool = False, region_names=None, densitometry: bool = False,
                 densitometry_kw: Optional[dict] = None, core_peel: bool = False, peel_mm: float = 10.0,
                 fissure_mm: Optional[float] = None, clusters: bool = False, cluster_kw: Optional[dict] = None,
                 scan_filter=None,
                 scan_filter_sections: Sequence[str] = ("densitometry", "core_peel", "clusters"),
                 local_mm: Optional[float] = None, local_kw: Optional[dict] = None, **prepare_kw) -> dict:
    """One scan + its lobe segmentation -> its entry of ``build_outputs``: ``transforms.prepare_case`` (dataset.py:57-92)
    -> ``transforms.prepare_sample(target_size)`` -> a batch of one -> ``module.predict_step`` -> ``build_outputs``.
    The composition only; `prepare_kw` goes to ``prepare_case`` (crop_border, dilate_iterations, ...).  ``regions``:
    the lobe labels travel along (``prepare_case(want_lobes=True)``) and the entry carries the per-lobe metrics of
    ``region_metrics``, keyed through ``region_names``.  ``densitometry``: the entry also carries
    ``densitometry_metrics`` of the case's 'image' and 'lobe_labels' at the scan's own resolution (before the resize;
    ``densitometry_kw`` goes to ``densitometry``), keyed through ``region_names`` as well, and a line in error_messages
    when lung voxels carry a label above n_regions.  The two switches are independent: without ``regions`` the batch
    holds no 'lobe_labels'.

    ``core_peel`` (independent of both): every per-lobe number is split into the subpleural rind of ``peel_mm`` (the
    caller's choice) and the rest.  Scan side: ``core_peel_metrics`` of ``core_peel`` on the crop before the resize
    (n_regions = ``module.args.n_regions``, default 5; thresholds, percentiles, hu_lo, nbins from ``densitometry_kw``).
    Network side: the composite zone labels travel as the batch's 'lobe_labels' with 'n_regions' = 2n, the one fused
    tail gives a [2n+1, 4] table, and the entry carries ``zone_region_metrics`` of it; with ``regions`` the table
    ``region_metrics`` reads is that one folded on the host (``fold_zone_table``).  A line in error_messages when lung
    voxels carry a label above n_regions.

    ``fissure_mm`` (None: off; needs ``core_peel`` and the module's n_regions <= 5, else ValueError before any device
    work): the section gains a third zone, the fissural rind of ``core_peel(fissure_mm=...)`` -- voxels outside the peel
    within ``fissure_mm`` (the caller's choice) of another lobe.  The composite labels travel with 'n_regions' = 3n,
    the one fused tail gives a [3n+1, 4] table, every zone key gains a twin ending '_fissure', and the entry carries
    'fissure_mm'; the keys ending '_core' then describe the lung in neither rind.

    ``clusters`` (independent of the three): the entry also carries ``laa_cluster_metrics`` of ``laa_clusters`` on the
    case's 'image' and 'lobe_labels' before the resize (``cluster_kw``: n_regions, threshold, connectivity), keyed
    through ``region_names``, and a line in error_messages when LAA voxels carry a label above n_regions.
    ``cluster_kw={'shapes': True, 'bulla_mm': ..., 'top': ...}`` adds the cluster shapes of ``laa_clusters(shapes=True)``
    to the section (bullae per lobe, the largest clusters; the centroids in voxels of the scan's grid: ``origin`` is the
    crop's offset); only together with ``core_peel`` the clusters are crossed with that section's zones, which is then
    issued first.  With shapes off the launch order and the entry are what they are without the key.
    'full_cle' / 'full_pse' are the same bit for bit under every combination.

    ``scan_filter`` (None, or a window size of ``ops.median_filter3d``: (3, 3, 3) or (1, 3, 3), ...):
    the sections named in ``scan_filter_sections`` that are switched on read ``filtered_image`` of the case's 'image',
    filtered once, instead of the image itself; a section that is not named reads the raw one.  Only the scan side
    changes: the network's input, the masks, ``regions`` and the network side of ``core_peel`` (the zones depend on the
    labels alone) are those of the raw scan, bit for bit.  The metrics then end with 'scan_filter': 'median3x3x3' /
    'median1x3x3' (``filter_name``); with the filter off the key is absent and the entry is what it is without the
    argument.  It is an option for noisy scans, and no value of it is recommended.  ValueError, before any device work,
    for a bad size, a name in ``scan_filter_sections`` that is no scan-side section, and ``scan_filter`` together with
    ``dilate_iterations`` < 1 or ``crop_border`` <= 0: only with a dilation and a padded crop does every window centred
    on a lung voxel hold the scan's own values, so that the filtered crop equals the crop of the filtered scan there.

    ``scan_filter=("gaussian", sigma_mm)`` puts ``gaussian_image`` in the same place: a Gaussian
    of sigma_mm millimetres (sigma_mm / spacing voxels per axis, truncated at 4 sigma, edges replicated) of the scan
    ITSELF, evaluated on the crop, so the median's precondition does not apply; the key reads 'gaussian1.00mm'
    (two decimals).  ValueError, before any device work, for sigma_mm <= 0 and for an axis whose radius exceeds 16 (the
    message names the axis and its spacing).  No value of sigma_mm is recommended either.

    ``scan_filter=("bilateral", sigma_mm, sigma_hu)`` puts ``bilateral_image`` there: the exact
    fixed-point bilateral filter of the case's 'image' (sigma_mm / spacing voxels per axis, truncated at 2 sigma;
    sigma_hu in HU) whose taps are confined to the lobe labels, so the median's precondition does not apply either
    (``dilate_iterations=0`` is accepted); the key reads 'bilateral1.00mm60.0hu'.  ValueError, before any device work,
    unless both are finite numbers > 0, for an axis whose radius exceeds 5 (the message names the axis and its spacing)
    and for a sigma_hu whose range table exceeds 1024 entries (above 289).  No values are recommended.

    ``local_mm`` (None: off, and the launch sequence, the metrics and 'full_cle' / 'full_pse' are what they are without
    the argument): the densitometry section gains the local low-attenuation fraction in a window of
    ``local_mm`` millimetres -- ``local_laa`` on the image that section reads (the filtered one when ``scan_filter`` names
    'densitometry'), issued directly after the section's own launch; ``local_kw``: n_regions (default: the section's),
    threshold, cuts, percentiles.  ``local_laa_metrics`` follow the densitometry keys, and the entry gains
    'full_local_laa': uint8 on the scan's grid like 'full_cle' (255 = the whole window below the threshold), zero outside
    the lung.  It needs ``densitometry=True``; ValueError, before any device work, without it, for a bad ``local_mm`` or a
    radius outside 0..16 (the message names the axis and its spacing; all three 0 is refused too), and for an unknown key or
    a bad value in ``local_kw``.  The arguments never reach ``core_peel``.  No window size or cut is recommended."""
    local = None
    if local_mm is not None:
        if not densitometry:
            raise ValueError("predict_case: local_mm adds the local LAA map to the densitometry section: it needs "
                             "densitometry=True")
        local = dict(local_kw or {})
        unknown = sorted(set(local) - set(_LOCAL_KW))
        if unknown:
            raise ValueError(f"predict_case: local_kw: unknown keys {unknown}; it takes {_LOCAL_KW}")
        ops.local_window(spacing, local_mm)
        local_laa_params("predict_case: local_kw", **{k: v for k, v in local.items() if k != "n_regions"})
        local.setdefault("n_regions", (densitometry_kw or {}).get("n_regions", 5))
        ops._n_regions("predict_case: local_kw", local["n_regions"])
    elif local_kw:
        raise ValueError("predict_case: local_kw needs local_mm")
    named = tuple(scan_filter_sections)
    for name in named:
        if name not in _SECTIONS or _SECTIONS[name].run is None:
            raise ValueError(f"predict_case: scan_filter_sections: {name!r} is not a scan-side section "
                             f"{tuple(k for k, v in _SECTIONS.items() if v.run is not None)}")
    if scan_filter is not None:
        noise_filter, filter_params = _scan_filter("predict_case: scan_filter", scan_filter)
        noise_filter.check("predict_case: scan_filter", filter_params, spacing, prepare_kw)
    on = {"regions": bool(regions), "densitometry": bool(densitometry), "core_peel": bool(core_peel),
          "clusters": bool(clusters)}
    kw = {"densitometry": dict(densitometry_kw or {}), "clusters": dict(cluster_kw or {})}
    if fissure_mm is not None and not core_peel:
        raise ValueError("predict_case: fissure_mm adds the fissural rind to the core / peel section: it needs "
                         "core_peel=True")
    if core_peel:
        n = int(getattr(module.args, "n_regions", 5))
        kw["core_peel"] = dict(densitometry_kw or {}, peel_mm=peel_mm)
        if fissure_mm is not None:
            if not 1 <= n <= 5:
                raise ValueError(f"predict_case: fissure_mm splits every lobe in three (3 n <= 15 rows downstream): the "
                                 f"module's n_regions = {n} must be 1..5")
            kw["core_peel"]["fissure_mm"] = fissure_mm
        if int(kw["core_peel"].setdefault("n_regions", n)) != n:
            raise ValueError(f"predict_case: core_peel splits the module's n_regions = {n} lobes; densitometry_kw asks "
                             "for another count")
    case = transforms.prepare_case(scan, lobes, spacing, uid=uid, want_lobes=any(on.values()), **prepare_kw)
    filtered = scan_filter is not None and any(on[name] for name in named)
    smooth = noise_filter.image(filter_params, scan, case, spacing) if filtered else None
    order = _LAUNCH_ORDER
    shapes = on["clusters"] and bool(kw["clusters"].get("shapes"))
    if shapes:
        kw["clusters"]["origin"] = tuple(int(v) for v in case["crop_slice"][:, 0])
        if core_peel:                               # the clusters are crossed with the section's own zones: it runs first
            order = ("core_peel",) + tuple(name for name in _LAUNCH_ORDER if name != "core_peel")
    results = {}
    for name in order:
        if not on[name]:
            continue
        if name == "clusters" and shapes and core_peel:
            kw[name].update(zones=results["core_peel"]["zones"],
                            zone_names=results["core_peel"].get("zone_names", ZONES))
        source = smooth if filtered and name in named else case["image"]
        results[name] = _SECTIONS[name].run(source, case["lobe_labels"], spacing, **kw[name])
        if name == "densitometry" and local is not None:            # rides the section: its image, directly behind it
            (z0, z1), (y0, y1), (x0, x1) = case["crop_slice"].tolist()
            full_local = torch.zeros(tuple(case["original_size"].tolist()), dtype=torch.uint8, device=source.device)
            local_result = local_laa(source, case["lobe_labels"], spacing, local_mm,
                                     out_u8=full_local[z0:z1, y0:y1, x0:x1], **local)
    cp = results.get("core_peel")
    # core / peel rides the network side on the regions' tail: its zone labels are the batch's labels, with 2n regions
    # (3n with the fissural rind)
    zone_names = ZONES if cp is None else cp.get("zone_names", ZONES)
    if cp is not None:
        case = dict(case, lobe_labels=cp["zone_labels"])
    elif not regions:
        case = {k: v for k, v in case.items() if k != "lobe_labels"}
    sample = transforms.prepare_sample(case, target_size)
    labelled = bool(regions) or bool(core_peel)
    keys = ("image", "lung_mask", "ess_mask", "crop_slice", "original_size") + (("lobe_labels",) if labelled else ())
    batch = {k: sample[k].unsqueeze(0) for k in keys}
    batch["uid"] = [uid]
    if cp is not None:
        batch["n_regions"] = len(zone_names) * cp["n_regions"]
    pred = module.predict_step(batch, 0)
    if cp is not None:
        composite = pred["region_table"][0].cpu()
        results["core_peel"] = dict(cp, zone_metrics=zone_region_metrics(composite, region_names, zone_names))
        pred = {k: v for k, v in pred.items() if k != "region_table"}
        if regions:
            pred["region_table"] = fold_zone_table(composite, len(zone_names)).unsqueeze(0)
    entry = build_outputs([pred], want_u8=want_u8, region_names=region_names)[0]
    for name, section in _SECTIONS.items():
        if name in results:
            entry["metrics"].update(section.metrics(results[name], region_names))
            outside, n = section.outside(results[name])
            if outside > 0:
                entry["error_messages"].append(section.error.format(outside, n))
            if name == "densitometry" and local is not None:
                entry["metrics"].update(local_laa_metrics(local_result, region_names))
                entry["full_local_laa"] = full_local
    if filtered:
        entry["metrics"]["scan_filter"] = noise_filter.name(filter_params)
    return entry


def write_reports(results: List[dict], centrilobular_json: Optional[str] = None, paraseptal_json: Optional[str] = None,
                  output_json: Optional[str] = None, regions_json: Optional[str] = None,
                  densitometry_json: Optional[str] = None, core_peel_json: Optional[str] = None,
                  clusters_json: Optional[str] = None):
    """processor.py:160-177: the two single-scan score files and the results list; ``regions_json``: the regional
    entries (``REGION_KEYS``) of the first result, which must carry them; ``densitometry_json``: its densitometry
    entries (``densitometry_metrics``), likewise; ``core_peel_json``: its ``core_peel_metrics`` and
    ``zone_region_metrics`` entries, likewise; ``clusters_json``: its ``laa_cluster_metrics`` entries, likewise."""
    m = results[0]["metrics"]
    if centrilobular_json:
        with open(centrilobular_json, "w") as f:
            f.write(json.dumps({"score": int(float(m["cle_severity_score"])),
                                "percentage": float(m["cle_lesion_percentage_per_lung"])}))
    if paraseptal_json:
        with open(paraseptal_json, "w") as f:
            f.write(json.dumps({"score": int(float(m["pse_severity_score"])),
                                "percentage": float(m["pse_lesion_percentage_per_lung"])}))
    if output_json:
        with open(output_json, "w") as f:
            f.write(json.dumps([{k: r[k] for k in ("entity", "metrics", "error_messages")} for r in results]))
    paths = {"regions_json": regions_json, "densitometry_json": densitometry_json, "core_peel_json": core_peel_json,
             "clusters_json": clusters_json}
    for name, section in _SECTIONS.items():
        if not paths[section.json_arg]:
            continue
        sel = section.select
        keys = [k for k in sel if k in m] if isinstance(sel, tuple) else [k for k in m if sel.fullmatch(k)]
        if not all(any(re.fullmatch(need, k) for k in keys) for need in section.required):
            raise ValueError(f"write_reports: {section.json_arg} needs a result with {section.hint} "
                             f"(predict_case({name}=True))")
        with open(paths[section.json_arg], "w") as f:
            f.write(json.dumps({k: m[k] for k in keys}))
