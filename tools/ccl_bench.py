"""Cost of the connected-component labelling (csrc/ccl.hip) and of the LAA cluster analysis at a realistic lung crop:
int16 HU and uint8 lobe labels [300,350,450], the lung a pair of ellipsoids (5 lobes in z-slabs) with 15 voxels of
background margin, parenchyma noise around -870 HU (a few isolated voxels below -950) and low-attenuation blobs of
mixed sizes (radii 1..24 voxels, many small ones and a few large) at -985 HU:

  c6, c26   ops.laa_components(by_lobe=True) at the threshold -950 for both connectivities: the whole call between device
            events, and each of its launches (init, merge, compress, table) from the library's kernel timeline in a
            separate recorded round
  +sizes    the same with cluster_voxels written as well (a fifth launch)
  mask      ops.label_components of the lobe labels themselves (39 % of the crop in five solid components): the union
            chains of large solid objects, the hard case of the merge
  roof      the least the four phases must move / the achievable HBM rate of DESIGN.md section 6: per voxel, init reads
            label + image (3 B) and writes parent + size counter + key (10 B); merge reads key + parent (6 B); compress
            reads key + parent and writes the id (10 B); table reads the id (4 B)
  scipy     scipy.ndimage.label on the whole-lung mask on the host (context only; skipped when absent)
  predict   processor.predict_case(regions=True, densitometry=True) with and without clusters=True on the volume as a
            scan (med3ddram18, random weights, --target): the added time of the switch

  python tools/ccl_bench.py [--reps 15] [--out FILE]    device events, warm (3 unrecorded rounds), interleaved
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
SPACING, N, THRESHOLD = (1.0, 0.7, 0.7), 5, -950
PHASES = {16: "init", 17: "merge", 18: "compress", 19: "table", 20: "sizes"}
PHASE_BYTES = {16: 13.0, 17: 6.0, 18: 10.0, 19: 4.0, 20: 12.0}     # init of a key volume without an image: 2 B less


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def synthetic_case(D, H, W, dev):
    m = 15
    z = (torch.arange(D, device=dev).float() - (D - 1) / 2) / ((D - 2 * m) / 2)
    y = (torch.arange(H, device=dev).float() - (H - 1) / 2) / ((H - 2 * m) / 2)
    xl = (torch.arange(W, device=dev).float() - (W - 1) / 4 - m / 2) / ((W - 3 * m) / 4)
    xr = (torch.arange(W, device=dev).float() - 3 * (W - 1) / 4 + m / 2) / ((W - 3 * m) / 4)
    body = z[:, None, None] ** 2 + y[None, :, None] ** 2
    lung = ((body + xl[None, None, :] ** 2) < 1.0) | ((body + xr[None, None, :] ** 2) < 1.0)
    slab = (torch.arange(D, device=dev) * N // D + 1).to(torch.uint8)[:, None, None]
    labels = (lung * slab).contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    scan = torch.randn(D, H, W, device=dev, generator=g) * 35.0 - 870.0
    cpu = torch.Generator().manual_seed(1)
    zz, yy, xx = (torch.arange(n, device=dev) for n in (D, H, W))
    for radius, count in ((1, 3000), (2, 1500), (3, 600), (5, 200), (8, 60), (12, 20), (24, 6)):
        cz = torch.randint(0, D, (count,), generator=cpu).tolist()
        cy = torch.randint(0, H, (count,), generator=cpu).tolist()
        cx = torch.randint(0, W, (count,), generator=cpu).tolist()
        for a, b, c in zip(cz, cy, cx):
            z0, z1, y0, y1, x0, x1 = (max(0, a - radius), a + radius + 1, max(0, b - radius), b + radius + 1,
                                      max(0, c - radius), c + radius + 1)
            d2 = ((zz[z0:z1] - a) ** 2)[:, None, None] + ((yy[y0:y1] - b) ** 2)[None, :, None] + \
                ((xx[x0:x1] - c) ** 2)[None, None, :]
            scan[z0:z1, y0:y1, x0:x1][d2 <= radius * radius] = -985.0
    return scan.round().to(torch.int16).contiguous(), labels, lung


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--size", type=int, nargs=3, default=[300, 350, 450])
    ap.add_argument("--target", type=int, nargs=3, default=[64, 112, 144])
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

    scan, labels, lung = synthetic_case(D, H, W, dev)
    n_lung = int(lung.sum())
    low = (scan < THRESHOLD) & lung
    runs = {"c6": lambda: ops.laa_components(scan, labels, THRESHOLD, N, 6),
            "c26": lambda: ops.laa_components(scan, labels, THRESHOLD, N, 26),
            "c6+sizes": lambda: ops.laa_components(scan, labels, THRESHOLD, N, 6, want_sizes=True),
            "mask c6": lambda: ops.label_components(labels, 6, N),
            "mask c26": lambda: ops.label_components(labels, 26, N)}
    ms = {k: [] for k in runs}
    for r in range(3 + args.reps):
        outs = {}
        for k, fn in runs.items():
            t, outs[k] = events(fn)
            if r >= 3:
                ms[k].append(t)
    say(f"int16 HU + uint8 labels [{D},{H},{W}], {n_lung} lung voxels ({100 * n_lung / vox:.0f} %), {int(low.sum())} below "
        f"{THRESHOLD} HU ({100 * int(low.sum()) / max(n_lung, 1):.1f} % of the lung); medians of {args.reps} (3 warm-up rounds), "
        f"device events, interleaved")
    for k in ("c6", "c26", "mask c6"):
        t = outs[k][1]
        res = processor.clusters_from_table(t, SPACING)
        say(f"  {k:9s} clusters per row {t[:, 32].tolist()}, largest {t[:, 34].tolist()} voxels, "
            f"D {[round(v, 3) for v in res['d'].tolist()]}")
    phase_ms = {}
    for k in runs:                                       # one recorded round each: the launches of the call, one by one
        tl = ops.KernelTimeline(64)
        tl.start()
        runs[k]()
        tl.stop()
        fam = tl.families()
        phase_ms[k] = {v: t[1] for d in fam.values() for v, t in d["variants"].items() if v in PHASES}
    for k in runs:
        med = statistics.median(ms[k])
        phases = [16, 17, 18, 19] + ([20] if k.endswith("sizes") else [])
        nbytes = dict(PHASE_BYTES)
        if k.startswith("mask"):
            nbytes[16] -= 2.0
        traffic = vox * sum(nbytes[p] for p in phases)
        roof = traffic / HBM_ACHIEVABLE * 1e3
        say(f"  {k:9s} {med:8.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  least bytes {traffic / 1e6:.0f} MB -> roof "
            f"{roof:.3f} ms at {HBM_ACHIEVABLE / 1e12:.1f} TB/s: the roof is {100 * roof / med:.0f} % of the time; "
            f"{vox / (med * 1e-3) / 1e9:.1f} Gvoxel/s")
        parts = ", ".join(f"{PHASES[p]} {phase_ms[k].get(p, float('nan')):.3f} ms (roof "
                          f"{vox * nbytes[p] / HBM_ACHIEVABLE * 1e3:.3f})" for p in phases)
        worst = max(phases, key=lambda p: phase_ms[k].get(p, 0.0))
        say(f"           launches, one recorded round: {parts}; the longest is {PHASES[worst]}")
    del outs
    torch.cuda.empty_cache()

    try:
        from scipy import ndimage
        host = low.cpu().numpy()
        for name, rank in (("6", 1), ("26", 3)):
            t0 = time.perf_counter()
            _, n = ndimage.label(host, structure=ndimage.generate_binary_structure(3, rank))
            say(f"  scipy    {1e3 * (time.perf_counter() - t0):8.0f} ms  ndimage.label, connectivity {name}, whole-lung mask on "
                f"the host, one run: {n} components ({os.cpu_count()} CPUs visible, {torch.get_num_threads()} threads allowed)")
    except ImportError:
        say("  scipy    not installed")

    if not args.no_predict:
        torch.manual_seed(0)
        mod = models.ScanRegLightningModule(models.make_args("med3ddram18")).to(dev).eval()
        target = tuple(args.target)
        kinds = {"regions+densitometry": dict(regions=True, densitometry=True),
                 "... +clusters": dict(regions=True, densitometry=True, clusters=True)}
        pm = {k: [] for k in kinds}
        for r in range(2 + max(3, args.reps // 3)):
            for k, sw in kinds.items():
                t, _ = events(lambda: processor.predict_case(mod, scan, labels, SPACING, target, uid="bench", **sw))
                if r >= 2:
                    pm[k].append(t)
        a, b = (statistics.median(pm[k]) for k in kinds)
        say(f"  predict_case, med3ddram18 at {target}, medians of {len(pm['... +clusters'])}: regions + densitometry "
            f"{a:.2f} ms, with clusters {b:.2f} ms: +{b - a:.2f} ms")
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
