"""Yardstick of the local LAA map (tests only): numpy, int64.  The box counts come from zero-padded cumulative sums along
each axis (a window sum is a difference of two prefix sums -- no running sum, no tile, no packed word, so it shares no
code path with csrc/boxfrac.hip), the map from the integer rounding rule, the per-lobe statistics from the FLATTENED
SELECTION q[labels == r] (no histogram: nothing shared with processor.local_laa_from_hist)."""
import numpy as np

from densito_ref import rows_of


def window_sum(a, radius):
    """sum of int64 ``a`` over the box [i - r, i + r] per axis, clipped to the array"""
    a = np.asarray(a, dtype=np.int64)
    for axis, r in enumerate(radius):
        n = a.shape[axis]
        c = np.concatenate([np.zeros_like(np.take(a, [0], axis=axis)), np.cumsum(a, axis=axis, dtype=np.int64)], axis=axis)
        i = np.arange(n)
        hi, lo = np.minimum(i + r + 1, n), np.maximum(i - r, 0)           # prefix sums: c[k] = sum of a[:k]
        a = np.take(c, hi, axis=axis) - np.take(c, lo, axis=axis)
    return a


def box_counts(image, labels, threshold, radius):
    """(num, den) int64 [D,H,W]: lung voxels of the clipped box below the threshold (strict), and lung voxels of the box"""
    lung = np.asarray(labels).astype(np.int64) > 0
    low = lung & (np.asarray(image).astype(np.int64) < int(threshold))
    return window_sum(low, radius), window_sum(lung, radius)


def fraction_map(image, labels, threshold, radius):
    """(map int16, counts int32, u8 uint8): q = (2000 num + den) // (2 den) where the label is positive, else -1;
    counts = num << 16 | den everywhere; u8 = (q * 255) // 1000, 0 where q = -1"""
    num, den = box_counts(image, labels, threshold, radius)
    lung = np.asarray(labels).astype(np.int64) > 0
    assert np.all(den[lung] >= 1) and num.max(initial=0) < 65536 and den.max(initial=0) < 65536
    q = np.where(lung, (2000 * num + den) // np.maximum(2 * den, 1), -1)
    u8 = np.where(q < 0, 0, q * 255 // 1000)
    return q.astype(np.int16), ((num << 16) | den).astype(np.int32), u8.astype(np.uint8)


def _one(v, cuts, percentiles):
    v = np.sort(v.astype(np.int64))
    N = int(v.size)
    if not N:
        nan = float("nan")
        return {"voxels": 0, "mean": nan, "sd": nan, "perc": [nan] * len(percentiles), "above": [nan] * len(cuts),
                "above_counts": [0] * len(cuts)}
    counts = [int(np.count_nonzero(v >= int(round(c * 1000)))) for c in cuts]
    return {"voxels": N, "mean": float(int(v.sum())) / float(1000 * N), "sd": float(np.std(v.astype(np.float64))) / 1000.0,
            "perc": [int(v[max(1, -(-p * N // 100)) - 1]) / 1000.0 for p in percentiles],      # nearest rank, ends included
            "above": [float(c) / float(N) for c in counts], "above_counts": counts}


def local_laa(q, labels, n=5, cuts=(0.10, 0.25, 0.50), percentiles=(50, 90)):
    """The layout of processor.local_laa_from_hist's result as numpy arrays: rows 0..n, 'whole_lung' over labels > 0"""
    q = np.asarray(q).astype(np.int64).ravel()
    row = rows_of(labels, n).ravel()
    per = [_one(q[row == r], cuts, percentiles) for r in range(n + 1)]
    whole = _one(q[row >= 0], cuts, percentiles)

    def pack(items, scalar):
        out = {"voxels": np.array([i["voxels"] for i in items], dtype=np.int64),
               "mean": np.array([i["mean"] for i in items], dtype=np.float64),
               "sd": np.array([i["sd"] for i in items], dtype=np.float64),
               "perc": np.array([i["perc"] for i in items], dtype=np.float64).reshape(len(items), -1).T,
               "above": np.array([i["above"] for i in items], dtype=np.float64).reshape(len(items), -1).T,
               "above_counts": np.array([i["above_counts"] for i in items], dtype=np.int64).reshape(len(items), -1).T}
        return {k: v[..., 0] for k, v in out.items()} if scalar else out

    out = pack(per, False)
    out["whole_lung"] = pack([whole], True)
    return out


SD_TOL = 1e-12     # fractions: both sides sum exact integers below 2^53; what differs is a handful of float64 roundings of
#                    numbers <= 1 (the yardstick: np.std, pairwise sums of squares <= 10^6 over < 2^20 voxels, relative 1e-14)


def assert_matches(got, want, what=""):
    """processor's result (tensors) against the yardstick: counts and percentiles exactly (NaN in the same places), ratios
    within one float64 rounding of the yardstick's own division, sd within SD_TOL."""
    def cmp(g, w, where):
        for k in ("voxels", "above_counts"):
            a = np.asarray(g[k].cpu())
            assert a.dtype == np.int64 and a.shape == w[k].shape and np.array_equal(a, w[k]), (what, where, k, a, w[k])
        a = np.asarray(g["perc"].cpu())
        assert a.dtype == np.float64 and a.shape == w["perc"].shape, (what, where, "perc")
        assert np.array_equal(a, w["perc"], equal_nan=True), (what, where, "perc", a, w["perc"])
        for k in ("mean", "above", "sd"):
            a = np.asarray(g[k].cpu())
            assert a.dtype == np.float64 and a.shape == w[k].shape, (what, where, k)
            assert np.array_equal(np.isnan(a), np.isnan(w[k])), (what, where, k, a, w[k])
            tol = SD_TOL if k == "sd" else np.spacing(np.abs(w[k]))
            assert bool(np.all((np.abs(a - w[k]) <= tol) | np.isnan(w[k]))), (what, where, k, a, w[k])
    cmp(got, want, "regions")
    cmp(got["whole_lung"], want["whole_lung"], "whole lung")


def lung_blob(shape, seed, pocket=True):
    """(image int16, labels uint8): an ellipsoid of five lobes (slabs along y) in a background of label 0, HU around -880
    with noise, and a pocket of low attenuation (-980) in one corner of the blob"""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    inside = ((z - (D - 1) / 2) / (D / 2 + 0.5)) ** 2 + ((y - (H - 1) / 2) / (H / 2 + 0.5)) ** 2 + \
        ((x - (W - 1) / 2) / (W / 2 + 0.5)) ** 2 <= 0.9
    labels = np.where(inside, y * 5 // max(H, 1) + 1, 0).astype(np.uint8)
    image = np.rint(rng.normal(-880.0, 40.0, size=shape)).astype(np.int16)
    image[~inside] = 40
    if pocket:
        image[: max(1, D // 2), : max(1, H // 2), : max(1, W // 3)][inside[: max(1, D // 2), : max(1, H // 2), : max(1, W // 3)]] = -980
    return image, labels
