"""The numpy yardstick of the fixed-point bilateral filter, in int64: one shifted view of the
sentinel-free padded volume per tap, the host tables of ``ops.bilateral_tables``.  tests/test_bilateral_host.py holds this
file to a triple loop over the definition and to a float64 bilateral filter."""
import itertools
import math

import numpy as np


def tables(sigma, sigma_hu, truncate=2.0):
    from bodyct_dram_emph_subtype_amd import ops
    return ops.bilateral_tables(sigma, sigma_hu, truncate)


def spatial_weight(tz, ty, tx, dz, dy, dx) -> int:
    return (tz[abs(dz)] * ty[abs(dy)] * tx[abs(dx)] + (1 << 15)) >> 16


def bilateral_filter(a: np.ndarray, sigma, sigma_hu, truncate=2.0, within=None) -> np.ndarray:
    """a [D,H,W] int16 -> the filter of the definition, int16; within: None or an array of a's shape, non-zero inside"""
    a = np.asarray(a)
    assert a.ndim == 3 and a.dtype == np.int16
    tz, ty, tx, R = tables(sigma, sigma_hu, truncate)
    R = np.asarray(R, dtype=np.int64)
    L = len(R)
    rz, ry, rx = len(tz) - 1, len(ty) - 1, len(tx) - 1
    D, H, W = a.shape
    mask = np.ones(a.shape, dtype=bool) if within is None else np.asarray(within) != 0
    assert mask.shape == a.shape
    v = a.astype(np.int64)
    pv = np.pad(v, [(rz, rz), (ry, ry), (rx, rx)])                   # the padding is masked out: its value is never used
    pm = np.pad(mask, [(rz, rz), (ry, ry), (rx, rx)])                # False outside the volume
    num = np.zeros(a.shape, dtype=np.int64)
    den = np.zeros(a.shape, dtype=np.int64)
    for dz, dy, dx in itertools.product(range(-rz, rz + 1), range(-ry, ry + 1), range(-rx, rx + 1)):
        S = spatial_weight(tz, ty, tx, dz, dy, dx)
        if S == 0:
            continue
        n = pv[rz + dz:rz + dz + D, ry + dy:ry + dy + H, rx + dx:rx + dx + W]
        m = pm[rz + dz:rz + dz + D, ry + dy:ry + dy + H, rx + dx:rx + dx + W]
        d = n - v
        w = S * R[np.minimum(np.abs(d), L - 1)] * m
        num += w * d
        den += w
    safe = np.where(mask, den, 1)                                    # a masked-out centre divides nothing
    out = np.where(mask, v + (2 * num + safe) // (2 * safe), v)
    assert out.min() >= -32768 and out.max() <= 32767
    return np.ascontiguousarray(out.astype(np.int16))


def brute_force(a: np.ndarray, sigma, sigma_hu, truncate=2.0, within=None) -> np.ndarray:
    """the definition, voxel by voxel, in Python integers"""
    tz, ty, tx, R = tables(sigma, sigma_hu, truncate)
    L = len(R)
    rz, ry, rx = len(tz) - 1, len(ty) - 1, len(tx) - 1
    D, H, W = a.shape
    out = np.empty_like(a)
    for z, y, x in itertools.product(range(D), range(H), range(W)):
        c = int(a[z, y, x])
        if within is not None and within[z, y, x] == 0:
            out[z, y, x] = c
            continue
        num = den = 0
        for dz, dy, dx in itertools.product(range(-rz, rz + 1), range(-ry, ry + 1), range(-rx, rx + 1)):
            zz, yy, xx = z + dz, y + dy, x + dx
            if not (0 <= zz < D and 0 <= yy < H and 0 <= xx < W) or (within is not None and within[zz, yy, xx] == 0):
                continue
            S = spatial_weight(tz, ty, tx, dz, dy, dx)
            d = int(a[zz, yy, xx]) - c
            w = S * R[min(abs(d), L - 1)]
            num += w * d
            den += w
        out[z, y, x] = c + (2 * num + den) // (2 * den)
    return out


def float_bilateral(a: np.ndarray, sigma, sigma_hu, truncate=2.0) -> np.ndarray:
    """a float64 bilateral filter on the same support (the box of the radii, taps outside the volume left out), not
    rounded: exp(-k^2 / (2 sigma^2)) per axis, exp(-d^2 / (2 sigma_hu^2)) in range"""
    sig = [float(s) for s in sigma]
    r = [int(truncate * s + 0.5) for s in sig]
    D, H, W = a.shape
    v = a.astype(np.float64)
    pv = np.pad(v, [(k, k) for k in r])
    pm = np.pad(np.ones(a.shape), [(k, k) for k in r])
    g = [[math.exp(-(k * k) / (2.0 * s * s)) if rr else 1.0 for k in range(rr + 1)] for s, rr in zip(sig, r)]
    num = np.zeros(a.shape)
    den = np.zeros(a.shape)
    for dz, dy, dx in itertools.product(*(range(-k, k + 1) for k in r)):
        n = pv[r[0] + dz:r[0] + dz + D, r[1] + dy:r[1] + dy + H, r[2] + dx:r[2] + dx + W]
        m = pm[r[0] + dz:r[0] + dz + D, r[1] + dy:r[1] + dy + H, r[2] + dx:r[2] + dx + W]
        d = n - v
        w = g[0][abs(dz)] * g[1][abs(dy)] * g[2][abs(dx)] * np.exp(-(d * d) / (2.0 * sigma_hu * sigma_hu)) * m
        num += w * d
        den += w
    return v + num / den
