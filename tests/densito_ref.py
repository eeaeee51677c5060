"""Yardstick of the per-lobe densitometry (tests only): numpy, int64, on the FLATTENED SELECTION scan[labels == r] --
the percentile by np.sort(v)[k - 1], the thresholds by comparison, the mean by an int64 sum.  ``densitometry`` builds no
histogram, so it shares no code path with csrc/densito.hip or processor.densitometry_from_hist; ``histogram`` (for the
kernel's own outputs) counts with np.bincount on the clamped values."""
import numpy as np


def rows_of(labels, n):
    """row per voxel: label r in 1..n -> r, a label above n -> 0, a label <= 0 -> -1 (not lung, counted nowhere)"""
    lab = np.asarray(labels).astype(np.int64)
    return np.where(lab <= 0, -1, np.where(lab > n, 0, lab))


def histogram(scan, labels, n, hu_lo=-1024, nbins=1024):
    """(hist [n+1, nbins] int64, sums [n+1, 2] int64 = voxel count, sum of the raw HU)"""
    hu = np.asarray(scan).astype(np.int64).ravel()
    row = rows_of(labels, n).ravel()
    keep = row >= 0
    row, hu = row[keep], hu[keep]
    key = row * nbins + (np.clip(hu, hu_lo, hu_lo + nbins - 1) - hu_lo)
    hist = np.bincount(key, minlength=(n + 1) * nbins).reshape(n + 1, nbins).astype(np.int64)
    order = np.argsort(row, kind="stable")                           # int64 sums per row: one sort, cumulative sums
    starts = np.searchsorted(row[order], np.arange(n + 1))
    csum = np.concatenate([[0], np.cumsum(hu[order], dtype=np.int64)])
    ends = np.append(starts[1:], row.size)
    sums = np.stack([ends - starts, csum[ends] - csum[starts]], axis=1).astype(np.int64)
    return hist, sums


def _one(v, voxel_ml, thresholds, percentiles, hu_lo, nbins):
    v = np.sort(v.astype(np.int64))
    N = int(v.size)
    counts = [int(np.count_nonzero(v < t)) for t in thresholds]
    perc = []
    for p in percentiles:
        h = float("nan")
        if N:
            k = max(1, -(-p * N // 100))
            h = int(v[k - 1])
            h = float(h) if hu_lo < h < hu_lo + nbins - 1 else float("nan")     # an end bin: only a bound
        perc.append(h)
    return {"voxels": N, "volume_ml": N * voxel_ml / 1000.0,
            "mean_density": (float(int(v.sum())) / float(N)) if N else float("nan"),
            "laa_counts": counts, "laa": [(float(c) / float(N)) if N else float("nan") for c in counts], "perc": perc}


def densitometry(scan, labels, spacing, n=5, thresholds=(-950, -910), percentiles=(15,), hu_lo=-1024, nbins=1024):
    """The layout of processor.densitometry's result, as numpy arrays: rows 0..n, and 'whole_lung' over labels > 0."""
    hu = np.asarray(scan).astype(np.int64).ravel()
    row = rows_of(labels, n).ravel()
    sz, sy, sx = (float(s) for s in spacing)
    voxel_ml = sz * sy * sx
    per = [_one(hu[row == r], voxel_ml, thresholds, percentiles, hu_lo, nbins) for r in range(n + 1)]
    whole = _one(hu[row >= 0], voxel_ml, thresholds, percentiles, hu_lo, nbins)

    def pack(items, scalar):
        out = {"voxels": np.array([i["voxels"] for i in items], dtype=np.int64),
               "volume_ml": np.array([i["volume_ml"] for i in items], dtype=np.float64),
               "mean_density": np.array([i["mean_density"] for i in items], dtype=np.float64),
               "laa_counts": np.array([i["laa_counts"] for i in items], dtype=np.int64).reshape(len(items), -1).T,
               "laa": np.array([i["laa"] for i in items], dtype=np.float64).reshape(len(items), -1).T,
               "perc": np.array([i["perc"] for i in items], dtype=np.float64).reshape(len(items), -1).T}
        return {k: v[..., 0] for k, v in out.items()} if scalar else out

    out = pack(per, False)
    out["whole_lung"] = pack([whole], True)
    out["thresholds"], out["percentiles"], out["hu_lo"], out["nbins"] = tuple(thresholds), tuple(percentiles), hu_lo, nbins
    return out


def assert_matches(got, want, what=""):
    """processor's result (tensors, any device) against the yardstick: counts and percentiles exactly (NaN in the same
    places), ratios within one float64 rounding of the yardstick's own division."""
    def cmp(g, w, where):
        for k in ("voxels", "laa_counts"):
            a = np.asarray(g[k].cpu())
            assert a.dtype == np.int64 and a.shape == w[k].shape and np.array_equal(a, w[k]), (what, where, k, a, w[k])
        a = np.asarray(g["perc"].cpu())
        assert a.dtype == np.float64 and a.shape == w["perc"].shape, (what, where, "perc")
        assert np.array_equal(a, w["perc"], equal_nan=True), (what, where, "perc", a, w["perc"])
        for k in ("volume_ml", "mean_density", "laa"):
            a = np.asarray(g[k].cpu())
            assert a.dtype == np.float64 and a.shape == w[k].shape, (what, where, k)
            assert np.array_equal(np.isnan(a), np.isnan(w[k])), (what, where, k, a, w[k])
            ok = np.abs(a - w[k]) <= np.spacing(np.abs(w[k]))
            assert bool(np.all(ok | np.isnan(w[k]))), (what, where, k, a, w[k])
    cmp(got, want, "regions")
    cmp(got["whole_lung"], want["whole_lung"], "whole lung")


def lung_like(shape, n, seed, hu_mean=-850.0, hu_sd=60.0):
    """(scan int16, labels uint8): HU peaked near -850 with a tail towards 0, labels in x-runs (slabs of lobes with a
    background margin), as a lobe map is"""
    rng = np.random.default_rng(seed)
    scan = np.clip(np.rint(rng.normal(hu_mean, hu_sd, size=shape) + rng.exponential(20.0, size=shape)), -32768, 32767)
    D, H, W = shape
    labels = np.zeros(shape, dtype=np.uint8)
    yy = (np.arange(H) * n // max(H, 1)) + 1
    labels[:] = yy[None, :, None]
    labels[:, :, : max(1, W // 10)] = 0
    labels[:, :, W - max(1, W // 12):] = 0
    return scan.astype(np.int16), labels
