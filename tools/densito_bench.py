"""Cost of the per-lobe densitometry (csrc/densito.hip) at a realistic lung crop: int16 scan [350,300,400] with a
lung-like HU distribution (peak near -850, a tail towards 0), uint8 labels of 5 lobes in slabs of a centred ellipsoid:

  hist      ops.lobe_histogram: the histogram pass + the fold (3 B per voxel + the workgroups' partial images)
  densito   processor.densitometry: hist + the O(rows x bins) torch glue (cumsum, ratios, percentile search)
  torch     the composition a caller writes without it: per lobe scan[labels == r] (a mask and a compaction), a
            comparison + sum per threshold, the mean, and a sort for the 15th percentile (torch.quantile refuses more
            than 16 777 216 elements)
  roof      bytes by shape / the achievable HBM rate of DESIGN.md section 6

  python tools/densito_bench.py [--reps 15] [--out FILE]    device events, warm (3 unrecorded rounds), interleaved
  python tools/densito_bench.py --kernels-only              a few rounds of `hist` alone, for a kernel trace
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
THRESHOLDS, PERCENTILE = (-950, -910), 15


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--size", type=int, nargs=3, default=[350, 300, 400])
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops, processor
    dram.load_library()
    dev, n = "cuda:0", 5
    D, H, W = args.size
    vox = D * H * W
    spacing = (0.7, 0.65, 0.65)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(0)
    hu = torch.randn(D, H, W, device=dev, generator=g) * 60.0 - 850.0
    hu = hu - 20.0 * torch.log(torch.rand(D, H, W, device=dev, generator=g).clamp_min(1e-6))       # + Exp(20)
    scan = hu.round().clamp(-1024, 3000).to(torch.int16)
    del hu
    z, y, x = ((torch.arange(m, device=dev).float() - (m - 1) / 2) / (0.45 * m) for m in (D, H, W))
    lung = ((z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2) <= 1.0)
    slab = (torch.arange(D, device=dev) * n // D + 1).to(torch.uint8)[:, None, None]
    labels = (lung * slab).contiguous()
    scan = torch.where(lung, scan, torch.full_like(scan, -2048))          # prepare_case's fill outside the lung
    del lung

    def composed():
        out = []
        for r in range(1, n + 1):
            v = scan[labels == r]
            cnt = v.numel()
            below = [(v < t).sum() for t in THRESHOLDS]
            k = max(1, -(-PERCENTILE * cnt // 100))
            out.append((cnt, v.sum(dtype=torch.int64) / cnt, below, [b / cnt for b in below], torch.sort(v).values[k - 1]))
        return out

    runs = {"hist": lambda: ops.lobe_histogram(scan, labels, n),
            "densito": lambda: processor.densitometry(scan, labels, spacing, n, THRESHOLDS, (PERCENTILE,))}
    if args.kernels_only:
        for _ in range(5):
            runs["hist"]()
        torch.cuda.synchronize()
        return
    runs["torch"] = composed
    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        outs = {}
        for k, fn in runs.items():
            t, outs[k] = events(fn)
            if r >= 3:
                ms[k].append(t)
    d, c = outs["densito"], outs["torch"]
    same = all(int(d["voxels"][r]) == c[r - 1][0] and float(d["perc"][0, r]) == float(c[r - 1][4])
               and int(d["laa_counts"][0, r]) == int(c[r - 1][2][0]) for r in range(1, n + 1))
    nblk = ops._L().dram_lobe_hist_nblk(vox)
    scratch = nblk * ((n + 1) * 1024 * 4 + (n + 1) * 16)
    traffic = 3.0 * vox + 2.0 * scratch + (n + 1) * (1024 + 2) * 8
    say(f"scan int16 [{D},{H},{W}] + uint8 labels, n_regions {n}, {int(d['whole_lung']['voxels'])} lung voxels, bins -1024..-1; "
        f"medians of {args.reps} (3 warm-up rounds), device events, interleaved")
    say(f"  voxel counts, LAA-950 counts and Perc15 equal to the torch composition's: {same}; "
        f"Perc15 {[int(v) for v in d['perc'][0, 1:].tolist()]}, LAA-950 {[round(v, 4) for v in d['laa'][0, 1:].tolist()]}")
    say(f"  {nblk} workgroups, partial images {scratch / 1e6:.1f} MB written and read once; bytes by shape {traffic / 1e6:.1f} MB "
        f"-> roof {traffic / HBM_ACHIEVABLE * 1e3:.3f} ms at {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
    for k in runs:
        m = statistics.median(ms[k])
        s = f"  {k:8s} {m:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})"
        if k == "hist":
            bw = traffic / (m * 1e-3)
            s += (f"  {bw / 1e12:.2f} TB/s = {100 * bw / HBM_ACHIEVABLE:.0f} % of {HBM_ACHIEVABLE / 1e12:.1f}; "
                  f"{vox / (m * 1e-3) / 1e9:.1f} Gvoxel/s")
        else:
            s += f"  x{m / statistics.median(ms['hist']):.1f} the histogram call"
        say(s)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
