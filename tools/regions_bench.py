"""Cost of the regional predict tail (csrc/regions.hip) at the sizes a user runs, dense [B,2,64,128,128] of both
regression heads, n_regions = 5, lobes five slabs of a centred ellipsoid:

  fused     ops.upproject_regions: both heads' volumes and the region table, one pass + the fold
  table     the same with want_volumes=False (2 B per voxel of traffic: what the arithmetic alone costs)
  parent    the composition the predict step ran before, extended to regions with torch: ess.float(), lungs.float(),
            lungs.sum(), ops.upproject per head (+ .contiguous() of the head view), and per head five masked sums

  python tools/regions_bench.py [--reps 15] [--out FILE]    device events, warm (3 unrecorded rounds), interleaved
  python tools/regions_bench.py --kernels-only              a few rounds of `fused` alone, for a kernel trace
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("batch of two", 2, (128, 256, 256)), ("one scan", 1, (151, 512, 512))]
HBM_ACHIEVABLE = 6.3e12


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
    ap.add_argument("--grid", type=int, nargs=3, default=[64, 128, 128])
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops
    dram.load_library()
    dev, n = "cuda:0", 5
    d, h, w = args.grid
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for title, B, size in CASES:
        D, H, W = size
        vps = D * H * W
        g = torch.Generator(device=dev).manual_seed(0)
        dense = torch.rand(B, 2, d, h, w, device=dev, generator=g)
        heads = [dense[:, 0], dense[:, 1]]
        z, y, x = ((torch.arange(m, device=dev).float() - (m - 1) / 2) / (0.4 * m) for m in (D, H, W))
        lung = ((z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2) <= 1.0)
        slab = (torch.arange(D, device=dev) * n // D + 1).to(torch.uint8)[:, None, None]
        labels = (lung * slab)[None].expand(B, D, H, W).contiguous()
        lung = lung[None].expand(B, D, H, W).contiguous()
        ess = lung & (torch.rand(B, D, H, W, device=dev, generator=g) < 0.3)
        ess_u8 = ess.view(torch.uint8)

        def parent():
            lf, ef = lung.float(), ess.float()
            lung_sum = lf.sum()
            out = []
            for hd in heads:
                up, part = ops.upproject(hd.contiguous(), ef, size)
                sums = torch.stack([(up * (labels == r)).sum((1, 2, 3)) for r in range(1, n + 1)], 1)
                out.append((up, part.sum(1) / lung_sum, sums))
            return out

        runs = {"fused": lambda: ops.upproject_regions(heads[0], heads[1], ess_u8, labels, size, n),
                "table": lambda: ops.upproject_regions(heads[0], heads[1], ess_u8, labels, size, n, want_volumes=False)}
        if args.kernels_only:
            for _ in range(5):
                runs["fused"]()
            torch.cuda.synchronize()
            continue
        runs["parent"] = parent
        ms = {k: [] for k in runs}
        for r in range(3 + args.reps):
            outs = {}
            for k, fn in runs.items():
                t, outs[k] = events(fn)
                if r >= 3:
                    ms[k].append(t)
        same = all(torch.equal(outs["fused"][i], outs["parent"][i][0]) for i in (0, 1)) and torch.equal(outs["fused"][2], outs["table"][2])
        rel = max(float(((outs["fused"][2][:, 1:, i] - outs["parent"][i][2].double()).abs()
                         / outs["parent"][i][2].double().abs().clamp_min(1e-30)).max()) for i in (0, 1))
        say(f"{title}: dense [{B},2,{d},{h},{w}] -> [{B},{D},{H},{W}], n_regions {n}; medians of {args.reps} "
            f"(3 warm-up rounds), device events, interleaved")
        say(f"  volumes bit-identical to the two upproject calls and table-only table identical: {same}; "
            f"region sums vs torch masked sums: rel {rel:.2e}")
        traffic = {"fused": B * (10.0 * vps + 8.0 * d * h * w), "table": B * (2.0 * vps + 8.0 * d * h * w)}
        for k in runs:
            m = statistics.median(ms[k])
            s = f"  {k:7s} {m:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})"
            if k in traffic:
                bw = traffic[k] / (m * 1e-3)
                s += (f"  {traffic[k] / 1e6:7.1f} MB by shape -> {bw / 1e12:.2f} TB/s = {100 * bw / HBM_ACHIEVABLE:.0f} % of "
                      f"{HBM_ACHIEVABLE / 1e12:.1f}; {vps * B / (m * 1e-3) / 1e9:.1f} Gvoxel/s")
            else:
                s += f"  x{m / statistics.median(ms['fused']):.1f} the fused call"
            say(s)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
