"""Cost of the median noise filter (csrc/median.hip) beside the two existing scan-side kernels it stands in front of, on one
volume: int16 [320,320,400] of seeded noise (normal, -900 +- 40 HU, about a tenth of it below -950 HU) and uint8 lobe
labels 1..5 in z-slabs over the whole volume.

  median 3x3x3, 1x3x3   ops.median_filter3d into a preallocated `out` (the other five window sizes follow as context: with
                        3 samples the time is staging and stores, the rest is what the selection network adds)
  lobe_histogram        ops.lobe_histogram: the existing one-pass, memory-bound kernel (3 B per voxel)
  laa_components        ops.laa_components at -950 HU, 6-connectivity: the heaviest existing scan-side kernel
  floor                 the filter must read and write every voxel once: 4 B per voxel at the achievable HBM rate of
                        DESIGN.md section 6; the achieved rate is 4 B * voxels / time

Each call between device events, 3 unrecorded warm-up rounds, all calls interleaved round by round, medians.  The filter's
result is checked against a torch restatement of the definition on a sub-volume first.

  python tools/median_bench.py [--reps 21] [--size D H W] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
N, THRESHOLD = 5, -950


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def torch_median(a, size):
    """the definition on the device: replicate-pad, stack the shifted views, the middle of the sorted stack"""
    r = [s // 2 for s in size]
    p = F.pad(a[None, None].float(), (r[2], r[2], r[1], r[1], r[0], r[0]), mode="replicate")[0, 0].to(torch.int16)
    D, H, W = a.shape
    views = [p[dz:dz + D, dy:dy + H, dx:dx + W] for dz in range(size[0]) for dy in range(size[1]) for dx in range(size[2])]
    return torch.stack(views).sort(0).values[len(views) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--size", type=int, nargs=3, default=[320, 320, 400])
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops
    dram.load_library()
    dev = "cuda:0"
    D, H, W = args.size
    vox = D * H * W
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(0)
    scan = (torch.randn(D, H, W, device=dev, generator=g) * 40.0 - 900.0).round().to(torch.int16).contiguous()
    labels = (torch.arange(D, device=dev) * N // D + 1).to(torch.uint8)[:, None, None].expand(D, H, W).contiguous()
    out = torch.empty_like(scan)

    sub = scan[: min(D, 48), : min(H, 56), :].contiguous()
    for size in ((3, 3, 3), (1, 3, 3)):
        if not torch.equal(ops.median_filter3d(sub, size), torch_median(sub, size)):
            raise SystemExit(f"median_filter3d {size} differs from the definition")

    others = [(3, 3, 1), (3, 1, 3), (3, 1, 1), (1, 3, 1), (1, 1, 3)]     # context: 9 and 3 samples, staging and stores alike
    runs = {"median 3x3x3": lambda: ops.median_filter3d(scan, (3, 3, 3), out=out),
            "median 1x3x3": lambda: ops.median_filter3d(scan, (1, 3, 3), out=out),
            "lobe_histogram": lambda: ops.lobe_histogram(scan, labels, N),
            "laa_components": lambda: ops.laa_components(scan, labels, THRESHOLD, N, 6)}
    for size in others:
        runs["median {}x{}x{}".format(*size)] = lambda size=size: ops.median_filter3d(scan, size, out=out)
    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        for k, fn in runs.items():
            t, res = events(fn)
            del res
            if r >= 3:
                ms[k].append(t)
    low = int((scan < THRESHOLD).sum())
    say(f"int16 [{D},{H},{W}] seeded noise (-900 +- 40 HU, {100 * low / vox:.1f} % below {THRESHOLD}), uint8 labels 1..{N}; "
        f"medians of {args.reps} (3 warm-up rounds), device events, interleaved; {torch.cuda.get_device_name(0)}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    floor = 4.0 * vox / HBM_ACHIEVABLE * 1e3
    for k in runs:
        line = f"  {k:15s} {med[k]:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  {vox / (med[k] * 1e-3) / 1e9:6.1f} Gvoxel/s"
        if k.startswith("median"):
            line += (f"  {4.0 * vox / (med[k] * 1e-3) / 1e12:.2f} TB/s of the 4 B per voxel it must move "
                     f"(floor {floor:.3f} ms at {HBM_ACHIEVABLE / 1e12:.1f} TB/s: {100 * floor / med[k]:.0f} % of the time)")
        say(line)
    for k in ("median 3x3x3", "median 1x3x3"):
        say(f"  {k} / lobe_histogram = {med[k] / med['lobe_histogram']:.2f}, / laa_components = "
            f"{med[k] / med['laa_components']:.2f}")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
