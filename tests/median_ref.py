"""The numpy yardstick of the median noise filter: pad by the radii with edge replication, stack the
shifted views of the window, sort, take the middle one.  The count is odd, so the result is one of the inputs and every
comparison with it is exact.  tests/test_median_host.py holds this file to scipy.ndimage.median_filter(mode='nearest')
and to a triple loop over the definition."""
import itertools

import numpy as np

SIZES = [s for s in itertools.product((1, 3), repeat=3) if max(s) == 3]          # the seven windows, (z, y, x)


def median_filter(a: np.ndarray, size=(3, 3, 3)) -> np.ndarray:
    """a [D,H,W] of any integer type -> the median over the ``size`` window, indices clamped to the volume"""
    a = np.asarray(a)
    assert a.ndim == 3 and len(size) == 3 and all(s in (1, 3) for s in size)
    r = [s // 2 for s in size]
    p = np.pad(a, [(v, v) for v in r], mode="edge")
    D, H, W = a.shape
    views = [p[dz:dz + D, dy:dy + H, dx:dx + W] for dz in range(size[0]) for dy in range(size[1]) for dx in range(size[2])]
    n = len(views)
    return np.ascontiguousarray(np.sort(np.stack(views), axis=0)[n // 2])


def brute_force(a: np.ndarray, size) -> np.ndarray:
    """the definition, voxel by voxel"""
    D, H, W = a.shape
    r = [s // 2 for s in size]
    out = np.empty_like(a)
    for z, y, x in itertools.product(range(D), range(H), range(W)):
        vals = [a[min(max(z + dz, 0), D - 1), min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
                for dz in range(-r[0], r[0] + 1) for dy in range(-r[1], r[1] + 1) for dx in range(-r[2], r[2] + 1)]
        out[z, y, x] = sorted(vals)[len(vals) // 2]
    return out


def full_range(shape, seed) -> np.ndarray:
    """uniform over the whole int16 range, with -32768 and 32767 planted at the corners and in the interior"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, size=shape, dtype=np.int64).astype(np.int16)
    D, H, W = shape
    for k, c in enumerate(itertools.product((0, D - 1), (0, H - 1), (0, W - 1))):
        a[c] = -32768 if k % 2 == 0 else 32767
    mid = (D // 2, H // 2, W // 2)
    a[mid] = 32767
    a[mid[0], mid[1], max(mid[2] - 1, 0)] = -32768
    a[mid[0], max(mid[1] - 1, 0), mid[2]] = -32768
    a[max(mid[0] - 1, 0), mid[1], mid[2]] = 32767
    return a


def three_values(shape, seed) -> np.ndarray:
    """ties everywhere"""
    return np.random.default_rng(seed).choice(np.array([-32768, -950, 32767], dtype=np.int16), size=shape)


def hu_noise(shape, seed) -> np.ndarray:
    """noise around -900 HU with a block of the fill value -2048"""
    rng = np.random.default_rng(seed)
    a = np.clip(np.rint(rng.normal(-900.0, 40.0, size=shape)), -1100, -700).astype(np.int16)
    D, H, W = shape
    a[: (D + 1) // 2, : (H + 1) // 2, : (W + 1) // 2] = -2048
    return a


CONTENTS = {"full_range": full_range, "three_values": three_values, "hu_noise": hu_noise,
            "constant": lambda shape, seed: np.full(shape, -1000 + seed, dtype=np.int16)}
