"""Yardstick of the per-component table and of the cluster shapes built on it (tests only): numpy, int64.  The rows come
from np.unique / np.bincount / np.minimum.at over the voxels that count, the faces from whole-array shifted
comparisons: no waves, no runs, no atomics -- it shares no code path with csrc/ccl_shapes.hip.  ``from_rows`` restates
processor.shapes_from_rows with python loops over the clusters."""
import math

import numpy as np

COLS = 18
ROOT, CLASS, VOXELS, Z0, Z1, Y0, Y1, X0, X1, SUM_Z, SUM_Y, SUM_X, FACES_Z, FACES_Y, FACES_X, ZONE1, ZONE2, ZONE3 = range(18)


def counted(comp):
    """bool [D,H,W]: the voxels that count -- c = comp[v] with 0 <= c < size and comp.flat[c] == c"""
    comp = np.asarray(comp).astype(np.int64)
    flat = comp.ravel()
    inside = (comp >= 0) & (comp < flat.size)
    return inside & (flat[np.where(inside, comp, 0)] == comp)


def exposed(comp):
    """int64 [3, D,H,W]: per axis the exposed faces (0, 1 or 2) of every voxel -- the neighbour along the axis lies
    outside the volume or holds another value in comp"""
    comp = np.asarray(comp).astype(np.int64)
    out = np.zeros((3,) + comp.shape, dtype=np.int64)
    for a in range(3):
        n = comp.shape[a]
        lo = np.ones(comp.shape, dtype=bool)                    # the face towards index - 1
        hi = np.ones(comp.shape, dtype=bool)
        cur = [slice(None)] * 3
        nxt = [slice(None)] * 3
        cur[a], nxt[a] = slice(1, n), slice(0, n - 1)
        lo[tuple(cur)] = comp[tuple(cur)] != comp[tuple(nxt)]
        hi[tuple(nxt)] = comp[tuple(nxt)] != comp[tuple(cur)]
        out[a] = lo.astype(np.int64) + hi.astype(np.int64)
    return out


def rows(comp, labels=None, zones=None):
    """int64 [m, 18]: one row per component in ascending root order, the columns of dram_component_shapes"""
    comp = np.asarray(comp).astype(np.int64)
    ok = counted(comp)
    roots, inv = np.unique(comp[ok], return_inverse=True)
    m = roots.size
    out = np.zeros((m, COLS), dtype=np.int64)
    if m == 0:
        return out
    z, y, x = (g[ok] for g in np.indices(comp.shape))
    out[:, ROOT] = roots
    if labels is not None:
        out[:, CLASS] = np.asarray(labels).astype(np.int64).ravel()[roots]
    out[:, VOXELS] = np.bincount(inv, minlength=m)
    for c0, g in ((Z0, z), (Y0, y), (X0, x)):
        lo = np.full(m, np.iinfo(np.int64).max)
        hi = np.full(m, -1)
        np.minimum.at(lo, inv, g)
        np.maximum.at(hi, inv, g)
        out[:, c0], out[:, c0 + 1] = lo, hi + 1
    for c, g in ((SUM_Z, z), (SUM_Y, y), (SUM_X, x)):
        np.add.at(out[:, c], inv, g.astype(np.int64))
    faces = exposed(comp)
    for a in range(3):
        np.add.at(out[:, FACES_Z + a], inv, faces[a][ok])
    if zones is not None:
        zn = np.asarray(zones).astype(np.int64)[ok]
        for k in (1, 2, 3):
            np.add.at(out[:, ZONE1 + k - 1], inv, (zn == k).astype(np.int64))
    return out


def with_capacity(full, capacity):
    """(rows [capacity, 18], count [2]) of a call with max_components = capacity"""
    m = full.shape[0]
    out = np.zeros((capacity, COLS), dtype=np.int64)
    k = min(m, capacity)
    out[:k] = full[:k]
    return out, np.array([m, k], dtype=np.int64)


def bulla_min_voxels(spacing, bulla_mm):
    return max(1, int(math.ceil(math.pi / 6.0 * float(bulla_mm) ** 3 / (float(spacing[0]) * float(spacing[1]) * float(spacing[2])))))


def from_rows(r, spacing, n_regions, bulla_mm=10.0, top=3, origin=(0, 0, 0), n_zones=0):
    """the layout of processor.shapes_from_rows' result, as numpy arrays, cluster by cluster"""
    r = np.asarray(r, dtype=np.int64).reshape(-1, COLS)
    sz, sy, sx = (float(v) for v in spacing)
    need = bulla_min_voxels(spacing, bulla_mm)
    n, m, nan = int(n_regions), r.shape[0], float("nan")
    per = {k: np.zeros(n + 1, dtype=np.int64) for k in ("bullae", "bulla_voxels", "cluster_voxels")}
    zone_clusters = np.zeros((n + 1, max(n_zones, 1)), dtype=np.int64)
    zone_bullae = np.zeros_like(zone_clusters)
    cl = {k: [] for k in ("region", "voxels", "is_bulla", "volume_ml", "diameter_mm", "extent_mm", "centroid", "surface_mm2",
                          "sphericity", "home_zone")}
    for row in r:
        c, v = int(row[CLASS]), int(row[VOXELS])
        reg = c if 1 <= c <= n else 0
        bulla = v >= need
        per["cluster_voxels"][reg] += v
        per["bullae"][reg] += int(bulla)
        per["bulla_voxels"][reg] += v if bulla else 0
        vol = v * (sz * sy * sx)
        surf = float(row[FACES_Z]) * (sy * sx) + float(row[FACES_Y]) * (sz * sx) + float(row[FACES_X]) * (sz * sy)
        zc = [int(row[ZONE1]), int(row[ZONE2]), int(row[ZONE3])]
        home = 0 if max(zc) == 0 else zc.index(max(zc)) + 1
        if 1 <= home <= n_zones:
            zone_clusters[reg, home - 1] += 1
            zone_bullae[reg, home - 1] += int(bulla)
        cl["region"].append(reg)
        cl["voxels"].append(v)
        cl["is_bulla"].append(bulla)
        cl["volume_ml"].append(vol / 1000.0)
        cl["diameter_mm"].append((6.0 * vol / math.pi) ** (1.0 / 3.0))
        cl["extent_mm"].append([(int(row[Z1]) - int(row[Z0])) * sz, (int(row[Y1]) - int(row[Y0])) * sy,
                                (int(row[X1]) - int(row[X0])) * sx])
        cl["centroid"].append([float(row[SUM_Z]) / v + origin[0], float(row[SUM_Y]) / v + origin[1],
                               float(row[SUM_X]) / v + origin[2]])
        cl["surface_mm2"].append(surf)
        cl["sphericity"].append(math.pi ** (1.0 / 3.0) * (6.0 * vol) ** (2.0 / 3.0) / surf)
        cl["home_zone"].append(home)
    out = {"bulla_mm": float(bulla_mm), "bulla_min_voxels": need, **per,
           "bulla_ml": per["bulla_voxels"].astype(np.float64) * (sz * sy * sx) / 1000.0,
           "bulla_laa_share": np.array([float(b) / float(c) if c else nan
                                        for b, c in zip(per["bulla_voxels"], per["cluster_voxels"])])}
    for k, v in cl.items():
        dt = {"region": np.int64, "voxels": np.int64, "home_zone": np.int64, "is_bulla": bool}.get(k, np.float64)
        a = np.array(v, dtype=dt)
        out[k] = a.reshape(m, 3) if k in ("extent_mm", "centroid") else a.reshape(m)
    if n_zones:
        out["zone_clusters"], out["zone_bullae"] = zone_clusters, zone_bullae
    order = sorted(range(m), key=lambda i: (-int(r[i, VOXELS]), int(r[i, ROOT])))
    out["largest"] = np.array(order[:int(top)], dtype=np.int64)
    return out


INT_KEYS = ("bullae", "bulla_voxels", "cluster_voxels", "region", "voxels", "home_zone", "largest", "zone_clusters",
            "zone_bullae")
FLOAT_KEYS = ("bulla_ml", "bulla_laa_share", "volume_ml", "diameter_mm", "extent_mm", "centroid", "surface_mm2", "sphericity")


def assert_shapes(got, want, what):
    """integers exactly, float64 fields to 1e-12 relative, NaN where the yardstick has NaN"""
    arr = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    assert got["bulla_min_voxels"] == want["bulla_min_voxels"] and got["bulla_mm"] == want["bulla_mm"], what
    for k in INT_KEYS:
        assert (k in got) == (k in want), (what, k)
        if k in want:
            a = arr(got[k])
            assert a.dtype == np.int64 and a.shape == want[k].shape and np.array_equal(a, want[k]), (what, k, a, want[k])
    assert np.array_equal(arr(got["is_bulla"]), want["is_bulla"]), what
    for k in FLOAT_KEYS:
        a, w = arr(got[k]), want[k]
        assert a.dtype == np.float64 and a.shape == w.shape, (what, k, a.shape, w.shape)
        assert np.array_equal(np.isnan(a), np.isnan(w)), (what, k, a, w)
        assert bool(np.all((np.abs(a - w) <= 1e-12 * np.abs(w)) | np.isnan(w))), (what, k, a, w)
