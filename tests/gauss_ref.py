"""numpy float64 yardstick of the separable Gaussian filter (csrc/gauss.hip), and the bound the
tests grant.

gaussian_filter(volume, taps_zyx, mode, box=None): out[z,y,x] = sum_k wz[k] sum_j wy[j] sum_i wx[i] in[z+k, y+j, x+i] in
float64, each w the full odd-length tap array of its axis (length 1: the axis is untouched), indices outside the volume
clamped ('nearest') or read as 0 ('zero'); ``box`` [[z0,z1],[y0,y1],[x0,x1]] crops the result.

bound(taps_zyx, max_abs): B = 2 (nz + ny + nx + 3) 2^-24 max|src|.  An fp32 evaluation of positive taps that sum to 1
differs from the exact result by at most about (nz + ny + nx + 3) u max|src| (n_a - 1 additions and one rounding of
each product per axis, and the taps' own rounding of their sum); the factor 2 leaves the summation order free."""
import numpy as np

MODES = ("nearest", "zero")


def _along(a, w, axis, mode):
    w = np.asarray(w, dtype=np.float64)
    assert w.ndim == 1 and w.size % 2 == 1
    r = w.size // 2
    if r == 0:
        return a * w[0]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="edge") if mode == "nearest" else np.pad(a, pad, mode="constant", constant_values=0.0)
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(w.size):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(k, k + n)
        out += w[k] * p[tuple(sl)]
    return out


def gaussian_filter(volume, taps_zyx, mode, box=None):
    assert mode in MODES
    a = np.asarray(volume, dtype=np.float64)
    assert a.ndim == 3 and len(taps_zyx) == 3
    for axis in (2, 1, 0):
        a = _along(a, taps_zyx[axis], axis, mode)
    if box is not None:
        (z0, z1), (y0, y1), (x0, x1) = [(int(lo), int(hi)) for lo, hi in box]
        a = a[z0:z1, y0:y1, x0:x1]
    return np.ascontiguousarray(a)


def brute_force(volume, taps_zyx, mode):
    """the definition, voxel by voxel (tiny volumes only)"""
    a = np.asarray(volume, dtype=np.float64)
    D, H, W = a.shape
    rz, ry, rx = (len(w) // 2 for w in taps_zyx)

    def at(z, y, x):
        if mode == "nearest":
            return a[min(max(z, 0), D - 1), min(max(y, 0), H - 1), min(max(x, 0), W - 1)]
        return a[z, y, x] if 0 <= z < D and 0 <= y < H and 0 <= x < W else 0.0

    out = np.zeros_like(a)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                s = 0.0
                for k in range(-rz, rz + 1):
                    for j in range(-ry, ry + 1):
                        for i in range(-rx, rx + 1):
                            s += taps_zyx[0][k + rz] * taps_zyx[1][j + ry] * taps_zyx[2][i + rx] * at(z + k, y + j, x + i)
                out[z, y, x] = s
    return out


def bound(taps_zyx, max_abs):
    return 2.0 * (sum(len(w) for w in taps_zyx) + 3) * 2.0 ** -24 * float(max_abs)


def rint_i16(a):
    """the int16 output rule applied to a float array: round half to even, clamp to the int16 range"""
    return np.clip(np.rint(a), -32768, 32767).astype(np.int16)
