"""Cost of the per-component table (csrc/ccl_shapes.hip) next to the labelling it reads, on the synthetic lung crop of
tools/ccl_bench.py (int16 HU and uint8 lobe labels [300,350,450]), for four fills of the key volume:

  realistic  the LAA key of the crop at -950 HU: isolated noise voxels and blobs of radius 1..24
  lungs      the two solid lungs as two components: every x-row crosses both giants
  box        the whole box as ONE component: every segment of the chip lands on one row
  bernoulli  12 % of the lung voxels at random: more than a million clusters of one or two voxels

  label      ops.label_components(key, 6, 1) of the fill
  shapes     ops.component_shapes(components, key, max_components=<the count>): rank + init + accumulate, nothing read
             back; `+zones` with a zone volume as well
  rank       the ranking and the row init alone (max_components=0)

  python tools/shapes_bench.py [--reps 10] [--out FILE]    device events, warm (3 unrecorded rounds), interleaved; the
rows of every fill are checked against the labelling's table (count, voxels) before anything is timed
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ccl_bench  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=3, default=[300, 350, 450])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as pkg
    from bodyct_dram_emph_subtype_amd import ops
    pkg.load_library()
    dev = "cuda:0"
    D, H, W = args.size
    scan, _, lung = ccl_bench.synthetic_case(D, H, W, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    fills = {"realistic": ((scan < -950) & lung).to(torch.uint8), "lungs": lung.to(torch.uint8),
             "box": torch.ones(D, H, W, dtype=torch.uint8, device=dev),
             "bernoulli": ((torch.rand(D, H, W, device=dev, generator=g) < 0.12) & lung).to(torch.uint8)}
    zones = (lung.to(torch.uint8) * (1 + (torch.arange(W, device=dev) % 3).to(torch.uint8))[None, None, :]).contiguous()
    lines = [f"component_shapes next to label_components, {D} x {H} x {W}, medians of {args.reps} (min, max), ms"]
    result = {}
    for name, key in fills.items():
        comp, table, _ = ops.label_components(key, 6, 1)
        n, fg = int(table[:, 32].sum()), int(table[:, 33].sum())
        rows, count = ops.component_shapes(comp, key, zones)
        assert rows.shape[0] == n == int(count[0]) and int(rows[:, 2].sum()) == fg, name
        assert int(rows[:, 15:].sum()) == int((zones[key > 0] > 0).sum()), name
        runs = {"label": lambda: ops.label_components(key, 6, 1),
                "shapes": lambda: ops.component_shapes(comp, key, None, max_components=n),
                "shapes+zones": lambda: ops.component_shapes(comp, key, zones, max_components=n),
                "rank": lambda: ops.component_shapes(comp, None, None, max_components=0)}
        t = {k: [] for k in runs}
        for rep in range(args.reps + 3):
            for k, fn in runs.items():
                ms, _ = events(fn)
                if rep >= 3:
                    t[k].append(ms)
        result[name] = {"components": n, "foreground": fg,
                        **{k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}}
        lines.append(f"  {name:10s} {n:9d} components {fg:10d} voxels  " + "  ".join(
            f"{k} {statistics.median(v):.3f} ({min(v):.3f}, {max(v):.3f})" for k, v in t.items()))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
