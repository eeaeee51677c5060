"""Yardstick of the connected-component labelling and the LAA cluster analysis (tests only): numpy, int64, by
MIN-PROPAGATION -- every foreground voxel starts at its own linear index and repeatedly takes the minimum over its
same-key neighbours through whole-array shifts, one per neighbour offset, until nothing changes.  No union-find, no
parent array, no runs: it shares no code path with csrc/ccl.hip.  The table is built by np.bincount, D by np.polyfit."""
import itertools

import numpy as np

COLS = 35
BIG = np.iinfo(np.int64).max


def offsets(connectivity):
    """the neighbour offsets (dz, dy, dx) of one half-space; the sweep applies each one in both directions"""
    if connectivity == 6:
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    if connectivity == 26:
        return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]
    raise ValueError(connectivity)


def _shifted(a, off, fill):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that lies outside the volume"""
    out = np.full_like(a, fill)
    src, dst = [], []
    for n, d in zip(a.shape, off):
        src.append(slice(max(d, 0), n + min(d, 0)))
        dst.append(slice(max(-d, 0), n + min(-d, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def components(key, connectivity=6):
    """key [D,H,W] (any integer or bool type; <= 0 is background) -> (components int64 [D,H,W]: the linear index of the
    smallest voxel of the voxel's component, -1 on background; the number of sweeps)"""
    key = np.asarray(key).astype(np.int64)
    key = np.where(key > 0, key, 0)
    fg = key > 0
    lab = np.where(fg, np.arange(key.size, dtype=np.int64).reshape(key.shape), BIG)
    both = [o for off in offsets(connectivity) for o in (off, tuple(-v for v in off))]
    same = [fg & (_shifted(key, o, 0) == key) for o in both]
    sweeps = 0
    while True:
        sweeps += 1
        new = lab
        for o, s in zip(both, same):
            new = np.where(s, np.minimum(new, _shifted(new, o, BIG)), new)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(fg, lab, -1), sweeps


def laa_key(image, labels, threshold, n_regions=5, by_lobe=True):
    """the LAA key: labels where labels > 0 and image < threshold (strict), else 0; 1 there with by_lobe=False"""
    lab = np.asarray(labels).astype(np.int64)
    low = (lab > 0) & (np.asarray(image).astype(np.int64) < int(threshold))
    return np.where(low, lab if by_lobe else 1, 0)


def sizes(comp):
    """cluster_voxels: per voxel the size of its component, 0 on background"""
    flat = comp.ravel()
    cnt = np.bincount(flat[flat >= 0], minlength=flat.size)
    return np.where(comp >= 0, cnt[np.maximum(comp, 0)], 0).astype(np.int64)


def table(key, comp, n_regions):
    """int64 [n + 1, 35]: per row the components per size bin 2^k <= s < 2^(k+1) (0..31), their number (32), the
    foreground voxels (33), the largest size (34); key r in 1..n -> row r, a key above n -> row 0"""
    key = np.asarray(key).astype(np.int64).ravel()
    flat = comp.ravel()
    cnt = np.bincount(flat[flat >= 0], minlength=flat.size)
    roots = np.nonzero(cnt)[0]
    s = cnt[roots]
    row = np.where(key[roots] > n_regions, 0, key[roots])
    rows = n_regions + 1
    t = np.zeros((rows, COLS), dtype=np.int64)
    bins = np.floor(np.log2(s.astype(np.float64))).astype(np.int64) if s.size else s       # s < 2^31: exact in double
    assert bool(np.all((1 << bins) <= s)) and bool(np.all(s < (2 << bins)))
    t[:, :32] = np.bincount(row * 32 + bins, minlength=rows * 32).reshape(rows, 32)
    t[:, 32] = np.bincount(row, minlength=rows)
    t[:, 33] = np.array([int(s[row == r].sum()) for r in range(rows)], dtype=np.int64)
    t[:, 34] = np.array([int(s[row == r].max()) if np.any(row == r) else 0 for r in range(rows)], dtype=np.int64)
    return t


def label(key, connectivity=6, n_regions=5):
    """(components int64, table int64, cluster_voxels int64) of a key volume"""
    comp, _ = components(key, connectivity)
    return comp, table(key, comp, n_regions), sizes(comp)


def d_exponent(hist):
    """D of one row's size histogram [32]: -slope of np.polyfit through (k ln 2, ln Y_k), k = 0..kmax, Y_k the number
    of clusters of at least 2^k voxels; NaN when kmax < 2"""
    hist = np.asarray(hist, dtype=np.int64)
    nz = np.nonzero(hist)[0]
    if nz.size == 0 or nz[-1] < 2:
        return float("nan")
    kmax = int(nz[-1])
    y = np.array([int(hist[k:].sum()) for k in range(kmax + 1)], dtype=np.float64)
    x = np.arange(kmax + 1, dtype=np.float64) * np.log(2.0)
    return float(-np.polyfit(x, np.log(y), 1)[0])


def from_table(t, spacing):
    """the layout of processor.clusters_from_table's result, as numpy arrays"""
    t = np.asarray(t, dtype=np.int64)
    voxel_ml = float(spacing[0]) * float(spacing[1]) * float(spacing[2])
    n = t[:, 32]
    nan = float("nan")
    return {"clusters": n.copy(), "voxels": t[:, 33].copy(), "largest_voxels": t[:, 34].copy(),
            "largest_ml": np.array([float(v) * voxel_ml / 1000.0 if c else nan for v, c in zip(t[:, 34], n)]),
            "mean_voxels": np.array([float(v) / float(c) if c else nan for v, c in zip(t[:, 33], n)]),
            "size_hist": t[:, :32].copy(), "d": np.array([d_exponent(r[:32]) for r in t])}


def laa_clusters(image, labels, spacing, n_regions=5, threshold=-950, connectivity=6):
    """the layout of processor.laa_clusters' result: rows 0..n by lobe, 'whole_lung' from the by_lobe=False key"""
    key = laa_key(image, labels, threshold, n_regions, True)
    comp, t, _ = label(key, connectivity, n_regions)
    out = from_table(t, spacing)
    one = laa_key(image, labels, threshold, 1, False)
    _, tw, _ = label(one, connectivity, 1)
    out["whole_lung"] = {k: v[1] for k, v in from_table(tw, spacing).items()}
    out.update(threshold=int(threshold), connectivity=int(connectivity), components=comp)
    return out


def slab_lobes(shape, n=5):
    """n slab "lobes" along y, labels 1..n (uint8)"""
    D, H, W = shape
    lab = np.zeros(shape, dtype=np.uint8)
    lab[:] = ((np.arange(H) * n // H) + 1)[None, :, None]
    return lab


def bernoulli_key(shape, p, seed, n=5):
    """a Bernoulli(p) mask carrying the slab lobes' labels"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < p, slab_lobes(shape, n), 0).astype(np.uint8)


CLUSTER_KEYS = {f"laa950_{s}_per_{w}" for s in ("clusters", "largest_cluster_ml", "cluster_d") for w in ("region", "lung")} | \
    {"laa_cluster_connectivity"}


def assert_clusters(got, want, what):
    for k in ("clusters", "voxels", "largest_voxels", "size_hist"):
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        assert a.dtype == np.int64 and np.array_equal(a, want[k]), (what, k, a, want[k])
    for k in ("largest_ml", "mean_voxels", "d"):
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = np.asarray(want[k])
        assert a.dtype == np.float64 and a.shape == w.shape, (what, k)
        assert np.array_equal(np.isnan(a), np.isnan(w)), (what, k, a, w)
        ok = np.abs(a - w) <= 1e-12 * np.abs(w)
        assert bool(np.all(ok | np.isnan(w))), (what, k, a, w)
