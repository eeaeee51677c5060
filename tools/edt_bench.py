"""Cost of the lung distance transform (csrc/edt.hip) and of the core / peel split at a realistic lung crop: uint8 lobe
labels [300,350,450] at spacing (1.0, 0.7, 0.7) mm, the lung a pair of ellipsoids (5 lobes in z-slabs), 15 voxels of
background margin on every face:

  capped    ops.lung_zones(n_regions=5) at max_mm = peel_mm = 10: what the report runs
  full      the same at max_mm = inf (uint64 work volumes, windows of the whole axis)
  +dist     capped, with dist_mm written as well
  roof      the passes' algorithmic bytes / the achievable HBM rate of DESIGN.md section 6: per voxel and element size e
            (4 capped, 8 full): x pass 2 label reads + e written, e read, e written; y pass e + e; z pass e + 1 label
            + zones + zone_labels (+ 4 with dist_mm)
  scipy     scipy.ndimage.distance_transform_edt on the same mask on the host (context only; skipped when absent)
  predict   processor.predict_case(regions=True, densitometry=True) with and without core_peel=True on the volume as a
            scan (med3ddram18, random weights, --target): the added time of the switch

  python tools/edt_bench.py [--reps 15] [--out FILE]    device events, warm (3 unrecorded rounds), interleaved
  python tools/edt_bench.py --kernels-only              a few rounds of `capped` and `full`, for a kernel trace
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
SPACING, PEEL_MM, N = (1.0, 0.7, 0.7), 10.0, 5


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def algorithmic_bytes(vox, elem, dist):
    return vox * (2.0 + 3.0 * elem + 2.0 * elem + elem + 1.0 + 2.0 + (4.0 if dist else 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--size", type=int, nargs=3, default=[300, 350, 450])
    ap.add_argument("--target", type=int, nargs=3, default=[64, 112, 144])
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import bodyct_dram_emph_subtype_amd as dram
    from bodyct_dram_emph_subtype_amd import models, ops, processor
    dram.load_library()
    dev = "cuda:0"
    D, H, W = args.size
    vox = D * H * W
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = 15
    z = (torch.arange(D, device=dev).float() - (D - 1) / 2) / ((D - 2 * m) / 2)
    y = (torch.arange(H, device=dev).float() - (H - 1) / 2) / ((H - 2 * m) / 2)
    xl = (torch.arange(W, device=dev).float() - (W - 1) / 4 - m / 2) / ((W - 3 * m) / 4)
    xr = (torch.arange(W, device=dev).float() - 3 * (W - 1) / 4 + m / 2) / ((W - 3 * m) / 4)
    body = z[:, None, None] ** 2 + y[None, :, None] ** 2
    lung = ((body + xl[None, None, :] ** 2) < 1.0) | ((body + xr[None, None, :] ** 2) < 1.0)
    slab = (torch.arange(D, device=dev) * N // D + 1).to(torch.uint8)[:, None, None]
    labels = (lung * slab).contiguous()
    n_lung = int(lung.sum())

    runs = {"capped": lambda: ops.lung_zones(labels, SPACING, PEEL_MM, n_regions=N),
            "full": lambda: ops.lung_zones(labels, SPACING, PEEL_MM, n_regions=N, max_mm=math.inf),
            "+dist": lambda: ops.lung_zones(labels, SPACING, PEEL_MM, n_regions=N, want_dist=True)}
    if args.kernels_only:
        for _ in range(3):
            runs["capped"]()
            runs["full"]()
        torch.cuda.synchronize()
        return
    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        outs = {}
        for k, fn in runs.items():
            t, outs[k] = events(fn)
            if r >= 3:
                ms[k].append(t)
    zc, zf = outs["capped"][0], outs["full"][0]
    say(f"uint8 labels [{D},{H},{W}] at {SPACING} mm, {n_lung} lung voxels ({100 * n_lung / vox:.0f} %), peel {PEEL_MM} mm: "
        f"peel {int((zc == 1).sum())}, core {int((zc == 2).sum())}; zones of capped and full equal: {torch.equal(zc, zf)}; "
        f"medians of {args.reps} (3 warm-up rounds), device events, interleaved")
    for k, elem, dist in (("capped", 4, False), ("full", 8, False), ("+dist", 4, True)):
        med = statistics.median(ms[k])
        traffic = algorithmic_bytes(vox, elem, dist)
        roof = traffic / HBM_ACHIEVABLE * 1e3
        say(f"  {k:8s} {med:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  bytes by shape {traffic / 1e6:.0f} MB -> roof "
            f"{roof:.3f} ms at {HBM_ACHIEVABLE / 1e12:.1f} TB/s: the roof is {100 * roof / med:.0f} % of the time; "
            f"{vox / (med * 1e-3) / 1e9:.1f} Gvoxel/s")
    del outs, zc, zf
    torch.cuda.empty_cache()

    try:
        from scipy import ndimage
        host = lung.cpu().numpy()
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(host, sampling=SPACING)
        say(f"  scipy    {1e3 * (time.perf_counter() - t0):8.0f} ms  distance_transform_edt on the host, one run "
            f"({os.cpu_count()} CPUs visible, {torch.get_num_threads()} threads allowed)")
    except ImportError:
        say("  scipy    not installed")

    if not args.no_predict:
        torch.manual_seed(0)
        mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(dev).eval()
        g = torch.Generator(device=dev).manual_seed(0)
        scan = (torch.randn(D, H, W, device=dev, generator=g) * 60.0 - 850.0).round().to(torch.int16)
        target = tuple(args.target)
        kinds = {"regions+densitometry": dict(regions=True, densitometry=True),
                 "... +core_peel": dict(regions=True, densitometry=True, core_peel=True, peel_mm=PEEL_MM)}
        pm = {k: [] for k in kinds}
        for r in range(2 + max(3, args.reps // 3)):
            for k, sw in kinds.items():
                t, _ = events(lambda: processor.predict_case(mod, scan, labels, SPACING, target, uid="bench", **sw))
                if r >= 2:
                    pm[k].append(t)
        a, b = (statistics.median(pm[k]) for k in kinds)
        say(f"  predict_case, med3ddram18 at {target}, medians of {len(pm['... +core_peel'])}: regions + densitometry "
            f"{a:.2f} ms, with core_peel {b:.2f} ms: +{b - a:.2f} ms")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
