"""Cost of the fixed-point bilateral filter (csrc/bilateral.hip) on a scan, beside the two other scan filters.

  int16 [320,320,400] seeded noise (-900 +- 40 HU), sigma_hu = 60
  radii (2,3,3), (3,4,4), (5,5,5)   sigma = (1.0, 1.4, 1.4), (1.4, 1.9, 1.9), (2.5, 2.5, 2.5) voxels at truncate 2; 1 mm on
                       a (1.0, 0.7, 0.7) mm grid is the first of them
  within               None, and a uint8 label volume 1..5 that is non-zero in the central box holding half of the voxels
                       (the lung's share of a chest scan, roughly): a centre outside it is copied, a tap outside weighs 0
  taps/s               centres filtered (all of them, or those inside `within`) x taps with S > 0 / time
  median 3x3x3, gaussian 1 mm @ 0.7 mm   ops.median_filter3d and ops.gaussian_filter3d (radii 6, 6, 6) on the same scan

Each call between device events, 3 unrecorded warm-up rounds, all calls interleaved round by round, medians.  The
kernel's result is checked first, at every radius and with the mask, against the same integer arithmetic written with
torch int64 tensors on a [24,40,72] corner of the scan.

  python tools/bilateral_bench.py [--reps 21] [--out FILE]
"""
import argparse
import itertools
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCAN = (320, 320, 400)
SIGMA_HU = 60.0
CASES = [((1.0, 1.4, 1.4), (2, 3, 3)), ((1.4, 1.9, 1.9), (3, 4, 4)), ((2.5, 2.5, 2.5), (5, 5, 5))]
N = 5


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def taps_of(tables):
    tz, ty, tx, _ = tables
    return [(dz, dy, dx, (tz[abs(dz)] * ty[abs(dy)] * tx[abs(dx)] + (1 << 15)) >> 16)
            for dz, dy, dx in itertools.product(*(range(-(len(t) - 1), len(t)) for t in (tz, ty, tx)))]


def torch_reference(img, tables, within=None):
    """the definition in torch int64 on the device: one padded shifted view per tap"""
    R = torch.tensor(tables[3], device=img.device, dtype=torch.int64)
    r = [len(t) - 1 for t in tables[:3]]
    D, H, W = img.shape
    v = img.to(torch.int64)
    mask = torch.ones_like(v, dtype=torch.bool) if within is None else within != 0
    pad = (r[2], r[2], r[1], r[1], r[0], r[0])
    pv, pm = F.pad(v, pad), F.pad(mask.to(torch.int64), pad)
    num, den = torch.zeros_like(v), torch.zeros_like(v)
    for dz, dy, dx, S in taps_of(tables):
        if S == 0:
            continue
        box = (slice(r[0] + dz, r[0] + dz + D), slice(r[1] + dy, r[1] + dy + H), slice(r[2] + dx, r[2] + dx + W))
        d = pv[box] - v
        w = S * R[d.abs().clamp(max=len(tables[3]) - 1)] * pm[box]
        num += w * d
        den += w
    den = torch.where(mask, den, torch.ones_like(den))
    return torch.where(mask, v + torch.div(2 * num + den, 2 * den, rounding_mode="floor"), v).to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops, processor
    dram.load_library()
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(0)
    scan = (torch.randn(*SCAN, device=dev, generator=g) * 40.0 - 900.0).round().to(torch.int16).contiguous()
    D, H, W = SCAN
    lobes = torch.zeros(SCAN, dtype=torch.uint8, device=dev)
    zs, ys, xs = (slice(int(n * 0.103), n - int(n * 0.103)) for n in SCAN)        # 0.794^3 = 0.50 of the voxels
    lobes[zs, ys, xs] = ((torch.arange(D, device=dev) * N // D + 1).to(torch.uint8)[:, None, None].expand(*SCAN))[zs, ys, xs]
    inside = int((lobes != 0).sum())
    out = torch.empty_like(scan)

    runs, count = {}, {}
    for sig, radii in CASES:
        tables = ops.bilateral_tables(sig, SIGMA_HU)
        if tuple(len(t) - 1 for t in tables[:3]) != radii:
            raise SystemExit(f"sigma {sig} gives radii {[len(t) - 1 for t in tables[:3]]}, not {radii}")
        ntaps = sum(1 for t in taps_of(tables) if t[3] > 0)
        small, small_lobes = scan[:24, :40, :72].contiguous(), lobes[20:44, 20:60, 30:102]
        for within in (None, small_lobes):
            if not torch.equal(ops.bilateral_filter3d(small, sig, SIGMA_HU, within=within), torch_reference(small, tables, within)):
                raise SystemExit(f"radii {radii}: bilateral_filter3d differs from the torch int64 composition")
        k = f"radii {radii}"
        runs[k] = lambda sig=sig: ops.bilateral_filter3d(scan, sig, SIGMA_HU, out=out)
        runs[k + " within"] = lambda sig=sig: ops.bilateral_filter3d(scan, sig, SIGMA_HU, within=lobes, out=out)
        count[k], count[k + " within"] = (scan.numel(), ntaps), (inside, ntaps)
    gsig = processor.gaussian_sigma_voxels("bilateral_bench", (0.7, 0.7, 0.7), 1.0)
    runs["median 3x3x3"] = lambda: ops.median_filter3d(scan, (3, 3, 3), out=out)
    runs["gaussian 1 mm @ 0.7 mm"] = lambda: ops.gaussian_filter3d(scan, gsig, mode="nearest", out=out)

    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        for k, fn in runs.items():
            t, res = events(fn)
            del res
            if r >= 3:
                ms[k].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}

    say(f"int16 {list(SCAN)} seeded noise (-900 +- 40 HU), sigma_hu = {SIGMA_HU:g}; within: uint8 labels, non-zero at "
        f"{100.0 * inside / scan.numel():.1f} % of the voxels; medians of {args.reps} (3 warm-up rounds), device events, "
        f"interleaved; {torch.cuda.get_device_name(0)}")
    for k, (centres, ntaps) in count.items():
        say(f"  bilateral {k:24s} {ntaps:5d} taps  {med[k]:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  "
            f"{scan.numel() / (med[k] * 1e-3) / 1e9:6.2f} Gvoxel/s  {centres * ntaps / (med[k] * 1e-3) / 1e12:.3f} Ttaps/s")
    for k in ("median 3x3x3", "gaussian 1 mm @ 0.7 mm"):
        say(f"  {k:34s} {med[k]:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f}) on the same scan")
    for k in count:
        say(f"  bilateral {k} / median 3x3x3 = {med[k] / med['median 3x3x3']:.1f}, / gaussian = "
            f"{med[k] / med['gaussian 1 mm @ 0.7 mm']:.1f}")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
