"""Yardstick of the lobe-to-lobe distance map and the three-zone split (tests only): numpy, int64.

``f2`` runs one BINARY transform per class -- ``edt_ref.dist2`` of the mask "not class c" gives every voxel its squared
distance to the nearest voxel of class c -- and takes, per voxel, the minimum over the classes that are not its own.  No
pairs, no packing, no reduction to two candidates, no early exit: it shares no code path with the multi-label passes of
csrc/edt.hip.  ``brute`` is the definition itself (a minimum over all sites of another class) for tiny shapes.  Units as
in INTEGRATION.md B7: spacing and distances in whole micrometres, squared distances in um^2, INF for "no such voxel
(within max_um)".  Classes: a label in 1..n -> the label, a lung label above n -> n + 1, a label <= 0 -> 0; only classes
1..n are sites."""
import numpy as np

import densito_ref as DR
import edt_ref as ER

INF = ER.INF
ZONE_NAMES = ("peel", "core", "fissure")


def units(spacing_mm, peel_mm, fissure_mm, max_mm=None):
    """(s_um (z, y, x), peel_um, fissure_um, max_um): round(mm * 1000); max_mm None -> the wider of the two widths, inf
    -> None (the full transform)"""
    s, peel, _ = ER.units(spacing_mm, peel_mm)
    fis = int(round(float(fissure_mm) * 1000.0))
    if max_mm is None:
        mx = max(peel, fis)
    else:
        mx = None if np.isinf(max_mm) else int(round(float(max_mm) * 1000.0))
    return s, peel, fis, mx


def classes(labels, n):
    lab = np.asarray(labels).astype(np.int64)
    return np.where(lab <= 0, 0, np.where(lab > n, n + 1, lab))


def f2(labels, s_um, n, max_um=None):
    """int64 [D,H,W]: 0 outside the lung, else the squared distance to the nearest site of another class, INF when there
    is none or (max_um given) none within max_um"""
    cls = classes(labels, n)
    out = np.full(cls.shape, INF, dtype=np.int64)
    for c in range(1, n + 1):
        to_c = ER.dist2(cls != c, s_um, max_um)                 # 0 on class c itself: excluded below
        out = np.where(cls != c, np.minimum(out, to_c), out)
    return np.where(cls > 0, out, 0)


def brute(labels, s_um, n, max_um=None):
    """the definition: min over sites u with class(u) != class(v) of sum_a (s_a (v_a - u_a))^2 (tiny shapes only)"""
    cls = classes(labels, n)
    s = np.array([int(v) for v in s_um], dtype=np.int64)
    sites = np.argwhere((cls >= 1) & (cls <= n)).astype(np.int64)
    site_cls = cls[tuple(sites.T)] if sites.shape[0] else np.zeros((0,), dtype=np.int64)
    out = np.zeros(cls.shape, dtype=np.int64)
    for v in np.argwhere(cls > 0):
        other = sites[site_cls != cls[tuple(v)]]
        if other.shape[0] == 0:
            out[tuple(v)] = INF
            continue
        d = int((((other - v[None, :].astype(np.int64)) * s[None, :]) ** 2).sum(1).min())
        out[tuple(v)] = INF if (max_um is not None and d > int(max_um) ** 2) else d
    return out


def zones(d2, f, lung, peel_um, fissure_um):
    """uint8: 0 not lung, 1 peel (d2 <= peel_um^2; the peel wins), 3 fissural rind (f2 <= fissure_um^2), 2 core"""
    lung = np.asarray(lung, dtype=bool)
    inner = np.where(f <= np.int64(int(fissure_um) ** 2), 3, 2)
    return np.where(~lung, 0, np.where(d2 <= np.int64(int(peel_um) ** 2), 1, inner)).astype(np.uint8)


def lobe_zones(labels, spacing_mm, peel_mm, fissure_mm, n=5, max_mm=None):
    """{'d2', 'f2' (int64), 'zones', 'zone_labels' (uint8), 'pleura_mm', 'fissure_mm' (float32)} as ops.lobe_zones
    defines them; zone_labels is edt_ref's rule, r + n (zone - 1), so zone 3 lands in 2n+1..3n"""
    s, peel, fis, mx = units(spacing_mm, peel_mm, fissure_mm, max_mm)
    lung = np.asarray(labels).astype(np.int64) > 0
    d2 = ER.dist2(lung, s, mx)
    f = f2(labels, s, n, mx)
    z = zones(d2, f, lung, peel, fis)
    return {"d2": d2, "f2": f, "zones": z, "zone_labels": ER.zone_labels(labels, z, n),
            "pleura_mm": ER.dist_mm(d2, lung), "fissure_mm": ER.dist_mm(f, lung)}


def core_peel(scan, labels, spacing_mm, peel_mm, fissure_mm, n=5, **densito_kw):
    """processor.core_peel(fissure_mm=...)'s layout: 'peel', 'core', 'fissure' (densito_ref.densitometry on the voxels of
    each zone; labels above n and the other zones set to 0, so row 0 is empty), 'outside_voxels', 'zones',
    'zone_labels', 'peel_mm', 'fissure_mm', 'n_regions', 'zone_names'"""
    r = lobe_zones(labels, spacing_mm, peel_mm, fissure_mm, n)
    lab = np.asarray(labels).astype(np.int64)
    out = {"zones": r["zones"], "zone_labels": r["zone_labels"], "outside_voxels": int((lab > n).sum()),
           "peel_mm": float(peel_mm), "fissure_mm": float(fissure_mm), "n_regions": n, "zone_names": ZONE_NAMES}
    for code, name in ((1, "peel"), (2, "core"), (3, "fissure")):
        sel = np.where((r["zones"] == code) & (lab <= n), lab, 0).astype(np.int16)
        out[name] = DR.densitometry(scan, sel, spacing_mm, n, **densito_kw)
    return out
