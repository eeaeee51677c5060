"""Cost of the lobe-to-lobe distance map (dram_lobe_zones, csrc/edt.hip) and of the fissural rind in the report, on the
crop of tools/edt_bench.py: uint8 lobe labels [300,350,450] at spacing (1.0, 0.7, 0.7) mm, the lung a pair of
ellipsoids (5 lobes in z-slabs), 15 voxels of background margin on every face; peel 10 mm, fissural rind 10 mm:

  lobe capped   ops.lobe_zones(n_regions=5) at max_mm = max(peel_mm, fissure_mm) = 10: what the report runs
  lobe full     the same at max_mm = inf (uint64 pleural volumes, windows of the whole axis)
  lobe +dist    capped, with pleura_mm and fissure_mm written as well
  lung capped   ops.lung_zones(n_regions=5) on the same input in the same interleaved rounds, and the ratio of the two
  lung full
  roof          the passes' algorithmic bytes / the achievable HBM rate of DESIGN.md section 6: per voxel, with e the
                pleural element size (4 capped, 8 full): pleural x pass 2 label reads + e written, e read, e written;
                pleural y pass e + e; pair x pass 1 label + 16; pair y pass 16 + 16; z pass e + 16 + 1 label + zones +
                zone_labels (+ 8 with both distance volumes)
  predict       processor.predict_case(regions=True, densitometry=True, core_peel=True) with and without fissure_mm on the
                volume as a scan (med3ddram18, random weights, --target): the added time of the argument

  python tools/lobe_zones_bench.py [--reps 9] [--out FILE]    device events, warm (2 unrecorded rounds), interleaved
  python tools/lobe_zones_bench.py --kernels-only             a few rounds of `lobe capped` and `lobe full`, for a kernel trace
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
SPACING, PEEL_MM, FISSURE_MM, N = (1.0, 0.7, 0.7), 10.0, 10.0, 5
WARM = 2


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def lung_bytes(vox, elem):
    return vox * (2.0 + 3.0 * elem + 2.0 * elem + elem + 1.0 + 2.0)


def lobe_bytes(vox, elem, dist):
    return vox * (2.0 + 3.0 * elem + 2.0 * elem + (1.0 + 16.0) + 32.0 + (elem + 16.0 + 1.0 + 2.0) + (8.0 if dist else 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
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

    lobe = lambda **kw: ops.lobe_zones(labels, SPACING, PEEL_MM, FISSURE_MM, n_regions=N, **kw)
    lungz = lambda **kw: ops.lung_zones(labels, SPACING, PEEL_MM, n_regions=N, **kw)
    runs = {"lobe capped": lambda: lobe(), "lobe full": lambda: lobe(max_mm=math.inf), "lobe +dist": lambda: lobe(want_dist=True),
            "lung capped": lambda: lungz(), "lung full": lambda: lungz(max_mm=math.inf)}
    if args.kernels_only:
        for _ in range(3):
            runs["lobe capped"]()
            runs["lobe full"]()
        torch.cuda.synchronize()
        return
    ms = {k: [] for k in runs}
    for r in range(WARM + args.reps):
        outs = {}
        for k, fn in runs.items():
            t, out = events(fn)
            outs[k] = out[0]
            del out
            if r >= WARM:
                ms[k].append(t)
    zc, zf, lc = outs["lobe capped"], outs["lobe full"], outs["lung capped"]
    say(f"uint8 labels [{D},{H},{W}] at {SPACING} mm, {n_lung} lung voxels ({100 * n_lung / vox:.0f} %), peel {PEEL_MM} mm, "
        f"fissural rind {FISSURE_MM} mm: peel {int((zc == 1).sum())}, core {int((zc == 2).sum())}, rind {int((zc == 3).sum())}; "
        f"zones of capped and full equal: {torch.equal(zc, zf)}; the peel is lung_zones' peel: {torch.equal(zc == 1, lc == 1)}; "
        f"medians of {args.reps} ({WARM} warm-up rounds), device events, interleaved")
    med = {k: statistics.median(v) for k, v in ms.items()}
    rows = (("lobe capped", lobe_bytes(vox, 4, False)), ("lobe full", lobe_bytes(vox, 8, False)),
            ("lobe +dist", lobe_bytes(vox, 4, True)), ("lung capped", lung_bytes(vox, 4)), ("lung full", lung_bytes(vox, 8)))
    for k, traffic in rows:
        roof = traffic / HBM_ACHIEVABLE * 1e3
        say(f"  {k:12s} {med[k]:9.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  bytes by shape {traffic / 1e6:.0f} MB -> roof "
            f"{roof:.3f} ms at {HBM_ACHIEVABLE / 1e12:.1f} TB/s: the roof is {100 * roof / med[k]:.0f} % of the time; "
            f"{vox / (med[k] * 1e-3) / 1e9:.1f} Gvoxel/s")
    say(f"  lobe_zones / lung_zones: capped {med['lobe capped'] / med['lung capped']:.2f} x, "
        f"full {med['lobe full'] / med['lung full']:.2f} x")
    del outs, zc, zf, lc
    torch.cuda.empty_cache()

    if not args.no_predict:
        torch.manual_seed(0)
        mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(dev).eval()
        g = torch.Generator(device=dev).manual_seed(0)
        scan = (torch.randn(D, H, W, device=dev, generator=g) * 60.0 - 850.0).round().to(torch.int16)
        target = tuple(args.target)
        base = dict(regions=True, densitometry=True, core_peel=True, peel_mm=PEEL_MM)
        kinds = {"core_peel": base, "... +fissure_mm": dict(base, fissure_mm=FISSURE_MM)}
        pm = {k: [] for k in kinds}
        for r in range(2 + max(3, args.reps // 2)):
            for k, sw in kinds.items():
                t, _ = events(lambda: processor.predict_case(mod, scan, labels, SPACING, target, uid="bench", **sw))
                if r >= 2:
                    pm[k].append(t)
        a, b = (statistics.median(pm[k]) for k in kinds)
        say(f"  predict_case, med3ddram18 at {target}, medians of {len(pm['core_peel'])}: regions + densitometry + core_peel "
            f"{a:.2f} ms (min {min(pm['core_peel']):.2f}, max {max(pm['core_peel']):.2f}), with fissure_mm {b:.2f} ms "
            f"(min {min(pm['... +fissure_mm']):.2f}, max {max(pm['... +fissure_mm']):.2f}): +{b - a:.2f} ms")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
