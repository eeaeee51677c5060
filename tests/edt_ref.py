"""Yardstick of the lung distance transform and the core / peel split (tests only): numpy, int64.

``dist2`` is a separable min-plus over the 0 / +inf indicator of the background, one axis after the other, with the
offsets k = 1 .. K applied as whole-array shifts -- no scans, no ballots, no early exit, no capping between the axes --
so it shares no code path with csrc/edt.hip.  ``brute`` is the definition itself (a minimum over all background
voxels) for tiny shapes.  Units as in INTEGRATION.md B7: spacing and distances in whole micrometres, d2 in um^2, INF
for "no background (within max_um)"."""
import numpy as np

import densito_ref as DR

INF = np.iinfo(np.int64).max
_BIG = np.int64(1) << 62                    # working infinity: _BIG + (s k)^2 stays inside int64


def units(spacing_mm, peel_mm=None, max_mm=None):
    """(s_um (z, y, x), peel_um, max_um): round(mm * 1000); max_mm None -> peel, inf -> None (the full transform)"""
    s = tuple(int(round(float(v) * 1000.0)) for v in spacing_mm)
    peel = None if peel_mm is None else int(round(float(peel_mm) * 1000.0))
    if max_mm is None:
        mx = peel
    else:
        mx = None if np.isinf(max_mm) else int(round(float(max_mm) * 1000.0))
    return s, peel, mx


def dist2(lung, s_um, max_um=None):
    """lung bool [D,H,W], s_um three ints -> int64 [D,H,W]: 0 for background, else the squared distance in um^2 to the
    nearest background voxel of the volume, INF when there is none or (max_um given) none within max_um."""
    lung = np.asarray(lung, dtype=bool)
    f = np.where(lung, _BIG, np.int64(0)).astype(np.int64)
    for axis, s in enumerate(int(v) for v in s_um):
        n = f.shape[axis]
        K = n - 1 if max_um is None else min(n - 1, int(max_um) // s)
        g = np.moveaxis(f, axis, 0)
        out = g.copy()
        for k in range(1, K + 1):
            c = np.int64((s * k) ** 2)
            np.minimum(out[k:], g[:-k] + c, out=out[k:])
            np.minimum(out[:-k], g[k:] + c, out=out[:-k])
        f = np.moveaxis(out, 0, axis)
    f = np.ascontiguousarray(f)
    far = f >= _BIG
    if max_um is not None:
        far |= f > np.int64(int(max_um) ** 2)
    return np.where(far, INF, f)


def brute(lung, s_um, max_um=None):
    """the definition: min over background voxels u of sum_a (s_a (v_a - u_a))^2 (tiny shapes only)"""
    lung = np.asarray(lung, dtype=bool)
    s = np.array([int(v) for v in s_um], dtype=np.int64)
    bg = np.argwhere(~lung).astype(np.int64)
    out = np.zeros(lung.shape, dtype=np.int64)
    for v in np.argwhere(lung):
        if bg.shape[0] == 0:
            out[tuple(v)] = INF
            continue
        d = int((((bg - v[None, :].astype(np.int64)) * s[None, :]) ** 2).sum(1).min())
        out[tuple(v)] = INF if (max_um is not None and d > int(max_um) ** 2) else d
    return out


def zones(d2, lung, peel_um):
    """uint8: 0 not lung, 1 peel (d2 <= peel_um^2), 2 core (INF included)"""
    lung = np.asarray(lung, dtype=bool)
    return np.where(~lung, 0, np.where(d2 <= np.int64(int(peel_um) ** 2), 1, 2)).astype(np.uint8)


def zone_labels(labels, z, n):
    """uint8: 0 not lung; lung label r in 1..n -> r + n (zone - 1); a lung label above n -> 255"""
    lab = np.asarray(labels).astype(np.int64)
    comp = np.where(lab > n, 255, lab + n * (z.astype(np.int64) - 1))
    return np.where(lab > 0, comp, 0).astype(np.uint8)


def dist_mm(d2, lung):
    """float32(sqrt(float64(d2)) / 1000.0): two IEEE operations in double, one rounding to float"""
    lung = np.asarray(lung, dtype=bool)
    fin = np.where(d2 == INF, 0, d2).astype(np.float64)
    out = (np.sqrt(fin) / 1000.0).astype(np.float32)
    out[d2 == INF] = np.inf
    out[~lung] = 0.0
    return out


def lung_zones(labels, spacing_mm, peel_mm, n=None, max_mm=None):
    """(d2, zones, zone_labels | None) of a label volume, as ops.lung_zones defines them"""
    s, peel, mx = units(spacing_mm, peel_mm, max_mm)
    lung = np.asarray(labels).astype(np.int64) > 0
    d2 = dist2(lung, s, mx)
    z = zones(d2, lung, peel)
    return d2, z, (None if n is None else zone_labels(labels, z, n))


def core_peel(scan, labels, spacing_mm, peel_mm, n=5, **densito_kw):
    """{'peel', 'core'}: densito_ref.densitometry on the voxels of each zone (labels above n and the other zone set to
    0, so row 0 is empty), 'outside_voxels', 'zones', 'zone_labels'"""
    _, z, zl = lung_zones(labels, spacing_mm, peel_mm, n)
    lab = np.asarray(labels).astype(np.int64)
    out = {"zones": z, "zone_labels": zl, "outside_voxels": int((lab > n).sum())}
    for code, name in ((1, "peel"), (2, "core")):
        sel = np.where((z == code) & (lab <= n), lab, 0).astype(np.int16)
        out[name] = DR.densitometry(scan, sel, spacing_mm, n, **densito_kw)
    return out
