"""Cost of the local LAA map (csrc/boxfrac.hip) on a crop of realistic size, its two launches apart, beside its traffic
model and the two-launch Gaussian at the same volume and radius.

  int16 [320,288,384], 5 lobes as slabs along z with a background margin, HU noise around -900
  windows              10 mm on spacing (0.7, 0.7, 0.7) (radii 7, 7, 7) and the largest box (radii 16, 16, 16)
  traffic model        in-plane pass: 2 B image + 1 B labels in, 4 B intermediate out = 7 B per voxel; z pass: the
                       intermediate re-read 2 + (2 rz + 1) / 64 times (the entering and the leaving plane, and the first
                       window of each 64-plane segment), 1 B labels, 2 B map (+ 1 B u8, + 4 B counts) out
  in-plane / z pass    from the library's own kernel timeline (a run of its own: the events around every launch are not
                       in the timed calls); GB/s = the model's bytes over that time
  gaussian             ops.gaussian_filter3d of the same scan with taps of the same radius, int16 -> int16, and its split
  lobe_histogram       the pass that follows the map in processor.local_laa, on the map

Each call between device events, 3 unrecorded warm-up rounds, all calls interleaved round by round, medians.  The map is
checked against a torch composition of the box count (cumulative sums) first.

  python tools/local_laa_bench.py [--reps 21] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCAN = (320, 288, 384)
N = 5
ZSEG = 64                        # csrc/boxfrac.hip


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def torch_box(a, radius):
    """clipped box sums of an int32 volume by cumulative sums, axis by axis"""
    for axis, r in enumerate(radius):
        n = a.shape[axis]
        c = torch.cat([torch.zeros_like(a.narrow(axis, 0, 1)), a.cumsum(axis, dtype=torch.int32)], dim=axis)
        i = torch.arange(n, device=a.device)
        a = c.index_select(axis, (i + r + 1).clamp(max=n)) - c.index_select(axis, (i - r).clamp(min=0))
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import ops
    dram.load_library()
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(0)
    scan = (torch.randn(*SCAN, device=dev, generator=g) * 40.0 - 900.0).round().to(torch.int16).contiguous()
    D, H, W = SCAN
    labels = (torch.arange(D, device=dev) * N // D + 1).to(torch.uint8)[:, None, None].expand(*SCAN).contiguous()
    labels[:, :24] = 0
    labels[:, :, -30:] = 0
    vox = scan.numel()
    cases = [("10 mm @ 0.7 mm", ops.local_window((0.7, 0.7, 0.7), 10.0)), ("largest box", (16, 16, 16))]
    out_q, out_i = torch.empty_like(scan), torch.empty_like(scan)
    full = torch.zeros((D + 40, H + 60, W + 80), dtype=torch.uint8, device=dev)
    window = full[20:20 + D, 30:30 + H, 40:40 + W]

    runs, model = {}, {}
    for name, radius in cases:
        lung = labels > 0
        den = torch_box(lung.to(torch.int32), radius)
        num = torch_box((lung & (scan < -950)).to(torch.int32), radius)
        want = torch.where(lung, (2000 * num + den) // (2 * den).clamp(min=1), torch.full_like(den, -1)).to(torch.int16)
        got = ops.local_fraction3d(scan, labels, -950, radius)
        if not torch.equal(got, want):
            raise SystemExit(f"{name}: local_fraction3d differs from the torch composition")
        del den, num, want, lung
        reads = 2.0 + (2 * radius[0] + 1) / ZSEG
        runs[f"map {name}"] = lambda radius=radius: ops.local_fraction3d(scan, labels, -950, radius, out=out_q)
        runs[f"map + u8 {name}"] = lambda radius=radius: ops.local_fraction3d(scan, labels, -950, radius, out=out_q, out_u8=window)
        model[f"map {name}"] = (radius, 7.0 * vox, (4.0 * reads + 1.0 + 2.0) * vox)
        model[f"map + u8 {name}"] = (radius, 7.0 * vox, (4.0 * reads + 1.0 + 3.0) * vox)
        sig = tuple((r + 0.25) / 4.0 for r in radius)                 # int(4 sigma + 0.5) = r
        assert tuple(ops.gaussian_radius(s) for s in sig) == tuple(radius)
        runs[f"gaussian {name}"] = lambda sig=sig: ops.gaussian_filter3d(scan, sig, mode="nearest", out=out_i)
    qmap = ops.local_fraction3d(scan, labels, -950, cases[0][1])
    runs["lobe_histogram of the map"] = lambda: ops.lobe_histogram(qmap, labels, N, 0, 1024)

    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        for k, fn in runs.items():
            t, res = events(fn)
            del res
            if r >= 3:
                ms[k].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}

    # the two launches apart: the library's timeline, a pass of its own
    split = {}
    for k in runs:
        if k.startswith("lobe"):
            continue
        a, b = (26, 27) if k.startswith("gaussian") else (29, 30)
        tl = ops.KernelTimeline()
        tl.start()
        for _ in range(5):
            runs[k]()
        v = tl.families()["prep"]["variants"]
        tl.stop()
        split[k] = (v[a][1] / v[a][0], v[b][1] / v[b][0])

    say(f"int16 {list(SCAN)} seeded noise (-900 +- 40 HU), {100.0 * float((labels > 0).float().mean()):.0f} % lung; medians of "
        f"{args.reps} (3 warm-up rounds), device events, interleaved; {torch.cuda.get_device_name(0)}")
    for k, (radius, b1, b2) in model.items():
        p, z = split[k]
        say(f"  {k:28s} radii {list(radius)}  {med[k]:7.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  "
            f"{vox / (med[k] * 1e-3) / 1e9:6.1f} Gvoxel/s")
        say(f"  {'':28s} in-plane pass {p:.3f} ms = {b1 / (p * 1e-3) / 1e9:.0f} GB/s of {b1 / vox:.0f} B per voxel; "
            f"z pass {z:.3f} ms = {b2 / (z * 1e-3) / 1e9:.0f} GB/s of {b2 / vox:.1f} B per voxel (kernel timeline, separate run)")
    for name, _ in cases:
        k = f"gaussian {name}"
        say(f"  {k:28s} {med[k]:7.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f}); in-plane pass {split[k][0]:.3f} ms, "
            f"z pass {split[k][1]:.3f} ms; map / gaussian = {med['map ' + name] / med[k]:.2f}")
    k = "lobe_histogram of the map"
    say(f"  {k:28s} {med[k]:7.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
