"""Cost of the separable Gaussian filter (csrc/gauss.hip) at the two sizes it is used at, beside its byte floor, the
existing scan-side kernels it stands in front of and a plain torch composition of the same filter.

  fp32 [128,224,288], zero border      the GaussianSmooth augmentation of a training volume: radius 1, 2 (sigma 0.3-0.6
                                       voxels, the reference's range) and 8 (sigma 2.0), float32 -> float32
  int16 [320,320,400], edges replicated  the scan filter at sigma = 1 mm on spacings (0.7, 0.7, 0.7) (radii 6, 6, 6) and
                                       (2.5, 0.7, 0.7) (radii 2, 6, 6), int16 -> int16
  floor                the two-launch form reads the source, writes and re-reads the fp32 intermediate and writes the
                       result: 16 B per voxel fp32 -> fp32, 12 B int16 -> int16, at the achievable HBM rate of DESIGN.md
                       section 6 (a single-launch form that never writes the intermediate would move 8 and 4 B)
  in-plane / z pass    the two launches apart, from the library's own kernel timeline (a run of its own: the events
                       around every launch are not in the timed calls)
  torch conv1d x 3     the reference's method (functional.py:54-64) written out here on the device: conv1d(padding=
                       'same') along the last axis, permute, three times; for the int16 scan behind a replicate pad,
                       with the float conversion and the rounding back in the timed call
  median 3x3x3, lobe_histogram   ops.median_filter3d and ops.lobe_histogram on the same scan

Each call between device events, 3 unrecorded warm-up rounds, all calls interleaved round by round, medians.  The
kernel's result is checked against the torch composition first (fp32: within 1e-5 of max|src|; int16: within 1).

  python tools/gauss_bench.py [--reps 21] [--out FILE]
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
TRAIN, SCAN = (128, 224, 288), (320, 320, 400)
N = 5


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def torch_smooth(img, taps, replicate=False):
    """the reference's gaussian_smooth on the device: taps (z, y, x) device tensors; x first, then y, then z"""
    for w in (taps[2], taps[1], taps[0]):
        r = w.numel() // 2
        rows = img.reshape(-1, 1, img.shape[-1])
        if replicate:
            rows = F.conv1d(F.pad(rows, (r, r), mode="replicate"), w.view(1, 1, -1))
        else:
            rows = F.conv1d(rows, w.view(1, 1, -1), padding="same")
        img = rows.view(*img.shape).permute(2, 0, 1).contiguous()
    return img


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
    vol = torch.randn(*TRAIN, device=dev, generator=g)
    scan = (torch.randn(*SCAN, device=dev, generator=g) * 40.0 - 900.0).round().to(torch.int16).contiguous()
    D = SCAN[0]
    labels = (torch.arange(D, device=dev) * N // D + 1).to(torch.uint8)[:, None, None].expand(*SCAN).contiguous()
    out_f, out_i = torch.empty_like(vol), torch.empty_like(scan)

    def dev_taps(sig):
        return [ops.gaussian_taps(s).to(dev) for s in sig]

    train_cases = [("r=1 (sigma 0.30)", (0.3,) * 3), ("r=2 (sigma 0.60)", (0.6,) * 3), ("r=8 (sigma 2.00)", (2.0,) * 3)]
    scan_cases = [(f"1 mm @ {sp}", processor.gaussian_sigma_voxels("gauss_bench", sp, 1.0))
                  for sp in ((0.7, 0.7, 0.7), (2.5, 0.7, 0.7))]
    runs, floors, radii = {}, {}, {}
    for name, sig in train_cases:
        k = f"fp32 {name}"
        t = dev_taps(sig)
        ref = torch_smooth(vol, t)
        err = float((ops.gaussian_filter3d(vol, sig, mode="zero") - ref).abs().max() / vol.abs().max())
        if not err < 1e-5:
            raise SystemExit(f"{k}: gaussian_filter3d differs from the torch composition by {err:.2e} max|src|")
        runs[k] = lambda sig=sig: ops.gaussian_filter3d(vol, sig, mode="zero", out=out_f)
        runs[k + " torch"] = lambda t=t: torch_smooth(vol, t)
        floors[k], radii[k] = 16.0 * vol.numel(), [w.numel() // 2 for w in t]
        del ref
    for name, sig in scan_cases:
        k = f"int16 {name}"
        t = dev_taps(sig)
        ref = torch_smooth(scan.float(), t, replicate=True)
        err = float((ops.gaussian_filter3d(scan, sig, mode="nearest").float() - ref).abs().max())
        if not err <= 1.0:
            raise SystemExit(f"{k}: gaussian_filter3d differs from the torch composition by {err:.3f} HU")
        runs[k] = lambda sig=sig: ops.gaussian_filter3d(scan, sig, mode="nearest", out=out_i)
        runs[k + " torch"] = lambda t=t: torch_smooth(scan.float(), t, replicate=True).round().clamp(-32768, 32767).to(torch.int16)
        floors[k], radii[k] = 12.0 * scan.numel(), [w.numel() // 2 for w in t]
        del ref
    runs["median 3x3x3"] = lambda: ops.median_filter3d(scan, (3, 3, 3), out=out_i)
    runs["lobe_histogram"] = lambda: ops.lobe_histogram(scan, labels, N)

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
    for k in floors:
        tl = ops.KernelTimeline()
        tl.start()
        for _ in range(5):
            runs[k]()
        v = tl.families()["prep"]["variants"]
        tl.stop()
        split[k] = (v[26][1] / v[26][0], v[27][1] / v[27][0])

    say(f"fp32 {list(TRAIN)} seeded N(0,1), zero border; int16 {list(SCAN)} seeded noise (-900 +- 40 HU), edges replicated; "
        f"medians of {args.reps} (3 warm-up rounds), device events, interleaved; {torch.cuda.get_device_name(0)}")
    for k in floors:
        vox = vol.numel() if k.startswith("fp32") else scan.numel()
        floor = floors[k] / HBM_ACHIEVABLE * 1e3
        say(f"  {k:34s} radii {radii[k]}  {med[k]:7.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  "
            f"{vox / (med[k] * 1e-3) / 1e9:6.1f} Gvoxel/s  {floors[k] / (med[k] * 1e-3) / 1e12:.2f} TB/s of the "
            f"{floors[k] / vox:.0f} B per voxel of the two-launch form (floor {floor:.3f} ms at "
            f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s: {100 * floor / med[k]:.0f} % of the time)")
        say(f"  {'':34s} in-plane pass {split[k][0]:.3f} ms, z pass {split[k][1]:.3f} ms (kernel timeline, separate run)")
        t = med[k + " torch"]
        say(f"  {'':34s} torch conv1d x 3 {t:7.3f} ms (min {min(ms[k + ' torch']):.3f}, max {max(ms[k + ' torch']):.3f}): "
            f"kernel / torch = {med[k] / t:.2f}")
    for k in ("median 3x3x3", "lobe_histogram"):
        say(f"  {k:34s} {med[k]:7.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f}) on the int16 scan")
    for k in floors:
        if k.startswith("int16"):
            say(f"  {k} / median 3x3x3 = {med[k] / med['median 3x3x3']:.2f}, / lobe_histogram = "
                f"{med[k] / med['lobe_histogram']:.2f}")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
